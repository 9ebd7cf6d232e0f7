// unipeak_amd/host/gzio.hpp -- the reference's stream filters by file-name
// suffix (misc/filterstream.cpp:30-50, 86-104; GZIP_SUFFIX / BZIP2_SUFFIX,
// misc/defaults.hpp:26-27): a name ending in ".gz" is read through a gzip
// decompressor and written through a gzip compressor (zlib, default level,
// like boost::iostreams' gzip filters).  ".bz2" takes bzip2 filters there.
// Here a ".bz2" input is read through the project's own bzip2 decoder
// (its host twin by default, csrc/bzip2.hip on the device on request; concatenated
// streams included, anything that is not a valid stream is an "error:" line
// and exit 1, never read as plain bytes).  A ".bz2" output is still refused
// with an "error:" line and exit 1: there is no bzip2 encoder yet.
#pragma once

#include <cstdio>
#include <string>

namespace unipeak {

bool is_gz(const std::string &fname);
bool is_bz2(const std::string &fname);

// fopen(fname, "rb") through the suffix's filter (".bz2": a FILE over the
// decoded bytes; a corrupt stream is fatal).  nullptr when the file cannot
// be opened.
FILE *open_input(const std::string &fname);

// fopen(fname, "wb") through the suffix's filter (".bz2": fatal); fclose()
// finishes the gzip stream.  nullptr when the file cannot be created.
FILE *open_output(const std::string &fname);

// the whole decompressed content of a ".gz" file into out; false when the
// file cannot be opened; a corrupt stream is fatal
bool inflate_file(const std::string &fname, std::string &out);

// the same for a ".bz2" file: through the decoder's host twin (no device is
// opened), or through the device decoder with UNIPEAK_BZ_DEVICE=1 (behind the
// switch until it beats the twin).  UNIPEAK_TIMING=1
// prints a "[timing] bz2" line.
bool bunzip_file(const std::string &fname, std::string &out);

}  // namespace unipeak
