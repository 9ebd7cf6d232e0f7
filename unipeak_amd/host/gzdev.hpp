// unipeak_amd/host/gzdev.hpp -- the batching gzip writer behind open_output
// for ".gz" names.  Writes are gathered into batches;
// every full batch is compressed by a GzCompressor (the device's DEFLATE
// encoder, up_dfl_stream) and appended to the file as one gzip member:
// header, raw deflate bytes, an empty final block (03 00), CRC-32, ISIZE.
// gzip readers, zlib's gzread among them, read the members as one stream.
//
// A file that closes before its first batch fills and holds less than
// kGzSmall bytes is written by zlib exactly as gzopen/gzwrite/gzclose would:
// region tables and shift reports keep their bytes and never open a device.
//
// The writer knows nothing of HIP: the compressor is made by a factory at the
// first batch, so the framing can be driven by a stub in a host-only program.
#pragma once

#include <cstdint>
#include <cstdio>
#include <functional>
#include <memory>
#include <string>
#include <vector>

namespace unipeak {

constexpr size_t kGzSmall = 1u << 20;       // below this an unbatched file goes through zlib
constexpr size_t kGzBatchDefault = 32u << 20;

struct GzCompressor {
    virtual ~GzCompressor() = default;
    // raw deflate of src[0, n), byte-aligned at the end, no final block;
    // *out stays valid until the next call.  false on failure (error() says why)
    virtual bool stream(const void *src, uint64_t n, const void **out, uint64_t *n_out, uint32_t *crc32) = 0;
    virtual double device_ms() const = 0;
    virtual std::string error() const = 0;
};
using GzCompressorFactory = std::function<std::unique_ptr<GzCompressor>(std::string *err)>;

class GzBatchWriter {
public:
    // batch: bytes per member (at least min_batch, the compressor's block)
    GzBatchWriter(std::string name, size_t batch, GzCompressorFactory make, bool timing);
    ~GzBatchWriter();
    bool open();                             // creates the file
    bool write(const char *buf, size_t n);   // false: see error()
    bool close();                            // writes what is left and the timing line
    const std::string &error() const { return err_; }

private:
    bool flush_member(const char *p, size_t n);
    bool finish_zlib();
    std::string name_, err_;
    size_t batch_;
    GzCompressorFactory make_;
    bool timing_;
    FILE *raw_ = nullptr;
    std::unique_ptr<GzCompressor> comp_;
    std::vector<char> buf_;
    uint64_t in_ = 0, out_ = 0, members_ = 0;
};

}  // namespace unipeak
