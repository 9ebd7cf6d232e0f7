// unipeak_amd/host/bbi.cpp -- see bbi.hpp.
#include "bbi.hpp"

#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <utility>

#include "../../include/unipeak_hip.h"
#include "cli.hpp"

namespace unipeak {
namespace bbi {

void put32(std::string &b, uint32_t v) { b.append((const char *)&v, 4); }
void put64(std::string &b, uint64_t v) { b.append((const char *)&v, 8); }
void put16(std::string &b, uint16_t v) { b.append((const char *)&v, 2); }
void putf(std::string &b, float v) { b.append((const char *)&v, 4); }
void putd(std::string &b, double v) { b.append((const char *)&v, 8); }
void set64(std::string &b, size_t at, uint64_t v) { std::memcpy(&b[at], &v, 8); }

void write_rtree(std::string &f, const std::vector<Block> &blocks, uint32_t block_size, uint32_t items_per_slot,
                 uint64_t base) {
    const uint64_t data_end = base + f.size();
    put32(f, 0x2468ACE0u);
    put32(f, block_size);
    put64(f, blocks.size());
    put32(f, blocks.empty() ? 0 : blocks.front().chrom);
    put32(f, blocks.empty() ? 0 : blocks.front().start);
    put32(f, blocks.empty() ? 0 : blocks.back().chrom);
    uint32_t end_base = 0;
    for (const Block &b : blocks)
        if (b.chrom == blocks.back().chrom) end_base = std::max(end_base, b.end);
    put32(f, end_base);
    put64(f, data_end);
    put32(f, items_per_slot);
    put32(f, 0);
    // levels: level 0 = leaves over the blocks; each parent level groups
    // block_size nodes.  Nodes are written root first.
    struct Node {
        uint32_t c0, s0, c1, s1;
        size_t first, count;  // children in the level below
    };
    std::vector<std::vector<Node>> levels;
    {
        std::vector<Node> leaves;
        for (size_t i = 0; i < blocks.size(); i += block_size) {
            const size_t n = std::min<size_t>(block_size, blocks.size() - i);
            Node nd{blocks[i].chrom, blocks[i].start, blocks[i + n - 1].chrom, 0, i, n};
            for (size_t k = i; k < i + n; ++k)
                if (blocks[k].chrom == nd.c1) nd.s1 = std::max(nd.s1, blocks[k].end);
            leaves.push_back(nd);
        }
        if (leaves.empty()) leaves.push_back(Node{0, 0, 0, 0, 0, 0});
        levels.push_back(leaves);
    }
    while (levels.back().size() > 1) {
        const std::vector<Node> &below = levels.back();
        std::vector<Node> up;
        for (size_t i = 0; i < below.size(); i += block_size) {
            const size_t n = std::min<size_t>(block_size, below.size() - i);
            Node nd{below[i].c0, below[i].s0, below[i + n - 1].c1, 0, i, n};
            for (size_t k = i; k < i + n; ++k)
                if (below[k].c1 == nd.c1) nd.s1 = std::max(nd.s1, below[k].s1);
            up.push_back(nd);
        }
        levels.push_back(up);
    }
    // offsets: root level first, then downwards
    const size_t L = levels.size();
    std::vector<std::vector<uint64_t>> off(L);
    uint64_t at = base + f.size();
    for (size_t l = L; l-- > 0;) {
        const bool leaf = l == 0;
        for (const Node &nd : levels[l]) {
            off[l].push_back(at);
            at += 4 + nd.count * (leaf ? 32 : 24);
        }
    }
    for (size_t l = L; l-- > 0;) {
        const bool leaf = l == 0;
        for (const Node &nd : levels[l]) {
            f.push_back(leaf ? 1 : 0);
            f.push_back(0);
            put16(f, (uint16_t)nd.count);
            for (size_t k = nd.first; k < nd.first + nd.count; ++k) {
                if (leaf) {
                    const Block &b = blocks[k];
                    put32(f, b.chrom);
                    put32(f, b.start);
                    put32(f, b.chrom);
                    put32(f, b.end);
                    put64(f, b.offset);
                    put64(f, b.size);
                } else {
                    const Node &c = levels[l - 1][k];
                    put32(f, c.c0);
                    put32(f, c.s0);
                    put32(f, c.c1);
                    put32(f, c.s1);
                    put64(f, off[l - 1][k]);
                }
            }
        }
    }
}

bool deflate6(const char *raw, size_t n, std::string &out) {
    uLongf clen = compressBound(n);
    out.resize(clen);
    if (compress2((Bytef *)&out[0], &clen, (const Bytef *)raw, n, 6) != Z_OK) return false;
    out.resize(clen);
    return true;
}

DeviceDeflater::~DeviceDeflater() { up_dfl_close((up_dfl *)h_); }

bool DeviceDeflater::wanted() {
    const char *e = std::getenv("UNIPEAK_BIGWIG_DEFLATE");
    return e && std::strcmp(e, "device") == 0;
}

bool DeviceDeflater::segments(const char *raw, const std::vector<uint64_t> &off, std::vector<std::string> &out) {
    if (off.size() < 2) return true;
    if (!h_) {
        up_dfl *h = nullptr;
        if (up_dfl_open(cli_physical_device(0), &h) != UP_OK) return false;
        h_ = h;
    }
    const uint32_t n = (uint32_t)(off.size() - 1);
    std::vector<uint64_t> oo(off.size());
    const void *p = nullptr;
    if (up_dfl_segments((up_dfl *)h_, raw, off.data(), n, &p, oo.data()) != UP_OK) return false;
    out.resize(n);
    for (uint32_t i = 0; i < n; ++i) out[i].assign((const char *)p + oo[i], (size_t)(oo[i + 1] - oo[i]));
    return true;
}

double DeviceDeflater::device_ms() const {
    double v[1] = {0};
    if (h_) up_dfl_timings((up_dfl *)h_, v, 1);
    return v[0];
}

size_t chrom_tree_bytes(size_t n, size_t key_size) { return 32 + 4 + n * (key_size + 8); }

void write_chrom_tree(std::string &f, const std::vector<std::string> &names, const std::vector<uint32_t> &sizes) {
    size_t key_size = 1;
    for (const std::string &n : names) key_size = std::max(key_size, n.size());
    const uint32_t nchrom = (uint32_t)names.size();
    put32(f, 0x78CA8C91u);
    put32(f, std::max<uint32_t>(nchrom, 1));
    put32(f, (uint32_t)key_size);
    put32(f, 8);
    put64(f, nchrom);
    put64(f, 0);
    f.push_back(1);
    f.push_back(0);
    put16(f, (uint16_t)nchrom);
    for (uint32_t i = 0; i < nchrom; ++i) {
        std::string k = names[i];
        k.resize(key_size, '\0');
        f += k;
        put32(f, i);
        put32(f, sizes[i]);
    }
}

void put_section_header(std::string &raw, uint32_t chrom, uint32_t start, uint32_t end, uint32_t span, uint16_t n) {
    put32(raw, chrom);
    put32(raw, start);
    put32(raw, end);
    put32(raw, 0);
    put32(raw, span);
    raw.push_back(2);  // varStep
    raw.push_back(0);
    put16(raw, n);
}

bool write_zoom_level(std::string &f, const ZoomRecord *sm, size_t n, uint32_t reduction, uint32_t &max_raw,
                      ZoomPlace &place, uint64_t base, unsigned threads, DeviceDeflater *dev) {
    place.reduction = reduction;
    place.data = base + f.size();
    put32(f, (uint32_t)n);
    // blocks of up to kItemsPerSection records of one chromosome; each block's
    // bytes depend on its records alone, so the threads only share the work
    std::vector<std::pair<size_t, size_t>> cut;
    for (size_t i = 0; i < n;) {
        size_t j = i;
        while (j < n && j - i < kItemsPerSection && sm[j].chrom == sm[i].chrom) ++j;
        cut.emplace_back(i, j);
        max_raw = std::max<uint32_t>(max_raw, (uint32_t)((j - i) * sizeof(ZoomRecord)));
        i = j;
    }
    std::vector<std::string> comp(cut.size());
    std::atomic<size_t> next{0};
    std::atomic<bool> failed{false};
    auto work = [&] {
        for (size_t k; (k = next.fetch_add(1)) < cut.size();)
            if (!deflate6((const char *)(sm + cut[k].first), (cut[k].second - cut[k].first) * sizeof(ZoomRecord),
                          comp[k]))
                failed = true;
    };
    const unsigned nt = (unsigned)std::min<size_t>(std::max(1u, threads), cut.size());
    if (dev) {  // the records are contiguous: the blocks are segments of them
        std::vector<uint64_t> off;
        for (const auto &c : cut) off.push_back(c.first * sizeof(ZoomRecord));
        off.push_back(n * sizeof(ZoomRecord));
        if (!dev->segments((const char *)sm, off, comp)) failed = true;
    } else if (nt <= 1) {
        work();
    } else {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < nt; ++t) pool.emplace_back(work);
        for (auto &th : pool) th.join();
    }
    if (failed) return false;
    std::vector<Block> zb;
    zb.reserve(cut.size());
    for (size_t k = 0; k < cut.size(); ++k) {
        zb.push_back(Block{sm[cut[k].first].chrom, sm[cut[k].first].start, sm[cut[k].second - 1].end,
                           base + f.size(), comp[k].size()});
        f += comp[k];
        std::string().swap(comp[k]);
    }
    place.index = base + f.size();
    write_rtree(f, zb, kRtreeBlock, kItemsPerSection, base);
    return true;
}

std::string header_bytes(uint64_t tree_off, uint64_t data_off, uint64_t index_off, uint64_t summary_off,
                         uint32_t max_raw, const std::vector<ZoomPlace> &zooms) {
    std::string h;
    put32(h, kMagic);
    put16(h, 4);
    put16(h, (uint16_t)zooms.size());
    put64(h, tree_off);
    put64(h, data_off);
    put64(h, index_off);
    put16(h, 0);
    put16(h, 0);
    put64(h, 0);
    put64(h, summary_off);
    put32(h, max_raw);
    put64(h, 0);
    for (const ZoomPlace &z : zooms) {
        put32(h, z.reduction);
        put32(h, 0);
        put64(h, z.data);
        put64(h, z.index);
    }
    return h;
}

std::string summary_bytes(uint64_t valid, double vmin, double vmax, double sum, double sumsq) {
    std::string s;
    put64(s, valid);
    putd(s, valid ? vmin : 0);
    putd(s, valid ? vmax : 0);
    putd(s, sum);
    putd(s, sumsq);
    return s;
}

}  // namespace bbi
}  // namespace unipeak
