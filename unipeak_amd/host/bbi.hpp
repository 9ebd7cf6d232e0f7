// unipeak_amd/host/bbi.hpp -- the pieces of a BBI (bigWig, version 4) file that
// bin/wigs2bigwigs and regions -W both write: little-endian put helpers, the
// header with its zoom headers, the total summary, the chromosome B+ tree, the
// R-tree (cirTree) over compressed blocks, and a zoom level (record count,
// zlib blocks of up to 1,024 summary records of one chromosome, their R-tree).
// Everything is appended to a std::string; `base` is the file offset of that
// string's first byte, for a writer that does not hold the whole file.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace unipeak {
namespace bbi {

void put16(std::string &b, uint16_t v);
void put32(std::string &b, uint32_t v);
void put64(std::string &b, uint64_t v);
void putf(std::string &b, float v);
void putd(std::string &b, double v);
void set64(std::string &b, size_t at, uint64_t v);

constexpr uint32_t kItemsPerSection = 1024;  // items of a data section, records of a zoom block
constexpr uint32_t kRtreeBlock = 256;        // children per R-tree node
constexpr size_t kHeaderBytes = 64, kZoomHeaderBytes = 24, kSummaryBytes = 40, kSectionHeaderBytes = 24;

struct Block {  // one compressed section and its extent
    uint32_t chrom, start, end;
    uint64_t offset, size;
};

// R-tree over the blocks, bottom-up, block_size children per node
void write_rtree(std::string &f, const std::vector<Block> &blocks, uint32_t block_size, uint32_t items_per_slot,
                 uint64_t base = 0);

// one zoom-level record (bbiSummaryOnDisk) as it is on disk
struct ZoomRecord {
    uint32_t chrom, start, end, valid;
    float vmin, vmax, sum, sumsq;
};
static_assert(sizeof(ZoomRecord) == 32, "bbiSummaryOnDisk");

// zlib (compress2, level 6) of raw; false when zlib fails
bool deflate6(const char *raw, size_t n, std::string &out);

// The device's DEFLATE encoder (up_dfl_segments) in deflate6's place: many
// sections in one call, each an independent zlib stream.  Opt-in
// (UNIPEAK_BIGWIG_DEFLATE=device); the handle is opened
// at the first call.
class DeviceDeflater {
public:
    DeviceDeflater() = default;
    DeviceDeflater(const DeviceDeflater &) = delete;
    DeviceDeflater &operator=(const DeviceDeflater &) = delete;
    ~DeviceDeflater();
    static bool wanted();  // the environment asks for it
    // raw[off[i], off[i + 1]) -> out[i], each at most 65,536 bytes; false on failure
    bool segments(const char *raw, const std::vector<uint64_t> &off, std::vector<std::string> &out);
    double device_ms() const;

private:
    void *h_ = nullptr;  // up_dfl
};

// the chromosome B+ tree in one leaf: names in key order, ids 0 .. n - 1
// (at most 65,535 names: the caller checks)
void write_chrom_tree(std::string &f, const std::vector<std::string> &names, const std::vector<uint32_t> &sizes);
// the bytes write_chrom_tree appends for n names of at most key_size bytes
size_t chrom_tree_bytes(size_t n, size_t key_size);

// the header of a varStep section of span 1 .. (24 bytes, items follow)
void put_section_header(std::string &raw, uint32_t chrom, uint32_t start, uint32_t end, uint32_t span, uint16_t n);

// a zoom level at file offset base + f.size(), its blocks compressed on
// `threads` threads (the bytes do not depend on it), or by dev in one call
// when it is given: false when the compression fails
struct ZoomPlace {
    uint32_t reduction;
    uint64_t data, index;
};
bool write_zoom_level(std::string &f, const ZoomRecord *rec, size_t n, uint32_t reduction, uint32_t &max_raw,
                      ZoomPlace &place, uint64_t base = 0, unsigned threads = 1, DeviceDeflater *dev = nullptr);

// header + zoom headers (kHeaderBytes + kZoomHeaderBytes per level)
std::string header_bytes(uint64_t tree_off, uint64_t data_off, uint64_t index_off, uint64_t summary_off,
                         uint32_t max_raw, const std::vector<ZoomPlace> &zooms);
// the total summary (kSummaryBytes)
std::string summary_bytes(uint64_t valid, double vmin, double vmax, double sum, double sumsq);

constexpr uint32_t kMagic = 0x888FFC26u;

}  // namespace bbi
}  // namespace unipeak
