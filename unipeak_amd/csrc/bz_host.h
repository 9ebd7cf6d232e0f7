// unipeak_amd/csrc/bz_host.h -- the host side of the bzip2 decoder: the twin
// that decodes a file serially along its chain (up_bz_decode_host), and the
// chain logic that the device path runs over its scan candidates.  Plain C++
// over bz_block.h, no HIP: bzip2.hip includes it, and so does the stand-alone
// sanitizer check (tools/bz_check.cpp).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "bz_block.h"

namespace upk {

struct BzCand {
    uint64_t bit;
    uint8_t kind;  // 0 block magic, 1 end-of-stream magic
};

struct BzChainBlock {
    uint32_t cand;    // index into the candidate list
    uint32_t stream;  // index into BzChain::streams
};
struct BzChainStream {
    uint32_t first_block, n_blocks;
    uint32_t stored_crc;  // the stream's combined CRC as the file states it
    uint64_t bit;         // of its "BZh"
};
struct BzChain {
    std::vector<BzChainBlock> blocks;
    std::vector<BzChainStream> streams;
};

inline const uint32_t *bz_crc_table() {
    static const std::vector<uint32_t> tab = [] {
        std::vector<uint32_t> t(256);
        for (uint32_t i = 0; i < 256; ++i) t[i] = bz_crc_entry(i);
        return t;
    }();
    return tab.data();
}

// bits [bit, bit + k) of src, k <= 48; the caller has checked the range
inline uint64_t bz_bits_at(const uint8_t *src, uint64_t bit, uint32_t k) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < k; ++i, ++bit) v = (v << 1) | ((src[bit >> 3] >> (7 - (bit & 7))) & 1u);
    return v;
}

// "BZh" + level at byte pos: the level 1..9, or 0 with *reason set.  first:
// the file's first stream (anything else there is not bzip2; later it is
// trailing data).
inline uint32_t bz_stream_level(const uint8_t *src, uint64_t n, uint64_t pos, bool first, int *reason) {
    const uint64_t left = n - pos;
    if (left < 4) {
        const bool prefix = left > 0 && std::memcmp(src + pos, "BZh", std::min<uint64_t>(left, 3)) == 0;
        *reason = !first ? UP_BZ_TRAILING : (left == 0 || prefix) ? UP_BZ_TRUNCATED : UP_BZ_NOT_BZIP2;
        return 0;
    }
    if (std::memcmp(src + pos, "BZh", 3) != 0) {
        *reason = first ? UP_BZ_NOT_BZIP2 : UP_BZ_TRAILING;
        return 0;
    }
    const uint8_t l = src[pos + 3];
    if (l < '1' || l > '9') {
        *reason = UP_BZ_BAD_LEVEL;
        return 0;
    }
    return (uint32_t)(l - '0');
}

// every bit offset where one of the two magics stands, ascending (the scan
// kernel's result, computed serially)
inline std::vector<BzCand> bz_scan_host(const uint8_t *src, uint64_t n) {
    std::vector<BzCand> out;
    if (n < 6) return out;
    uint64_t w = 0;
    const uint64_t mask = (1ull << 48) - 1;
    for (uint64_t bit = 0; bit < n * 8; ++bit) {
        w = ((w << 1) | ((src[bit >> 3] >> (7 - (bit & 7))) & 1u)) & mask;
        if (bit >= 47 && (w == kBzBlockMagic || w == kBzEndMagic))
            out.push_back({bit - 47, (uint8_t)(w == kBzEndMagic)});
    }
    return out;
}

// the entropy stage of the block whose magic stands at `bit`: what the device
// kernel does per candidate
inline void bz_entropy_host(const uint8_t *src, uint64_t n, uint64_t bit, uint32_t cap, BzTables &T, uint8_t *tt,
                            uint32_t *hist, BzRec &R) {
    BzBits br;
    br.init(src, n, bit + 48);
    BzBlockHdr H{};
    R = BzRec{0, 0, 0, 0, UP_BZ_OK};
    R.err = bz_read_header(br, cap, T, H);
    if (R.err) return;
    for (uint32_t t = 0; t < H.n_groups; ++t) bz_build_table(T, t, H.n_in_use + 2);
    R.err = bz_decode_symbols(br, H, T, cap, tt, hist, &R.n_block);
    if (R.err) return;
    R.orig_ptr = H.orig_ptr;
    R.stored_crc = H.stored_crc;
    R.end_bit = br.pos();
    if (H.orig_ptr >= R.n_block) R.err = UP_BZ_ORIGPTR;
}

// Links the candidates into the exact chain.  From bit 32 of a stream, a
// block that decoded without error and ends at another candidate links to it;
// an end magic closes the stream, and another "BZh" may follow at the next
// byte.  Candidates that nothing links to are false positives of the 48-bit
// pattern and stay out; a position on the chain that is no candidate, or a
// block with an error, is a corrupt file.  cands ascending; recs[i] belongs to
// cands[i] (unused for end magics).  CRCs are compared later (bz_check_crcs).
inline int bz_chain(const uint8_t *src, uint64_t n, const std::vector<BzCand> &cands,
                    const std::vector<BzRec> &recs, BzChain &C, up_bz_info_t &info) {
    C.blocks.clear();
    C.streams.clear();
    info = up_bz_info_t{0, 0, 0, UP_BZ_OK, 0};
    auto fail = [&](int reason, uint64_t bit) {
        info.reason = reason;
        info.fail_bit = bit;
        return reason;
    };
    uint64_t pos = 0;
    for (;;) {
        int reason = 0;
        const uint32_t level = bz_stream_level(src, n, pos, pos == 0, &reason);
        if (!level) return fail(reason, pos * 8);
        const uint32_t cap = level * 100000;
        C.streams.push_back({(uint32_t)C.blocks.size(), 0, 0, pos * 8});
        uint64_t bit = pos * 8 + 32;
        for (;;) {
            if (bit + 48 > n * 8) return fail(UP_BZ_TRUNCATED, bit);
            auto it = std::lower_bound(cands.begin(), cands.end(), bit,
                                       [](const BzCand &c, uint64_t b) { return c.bit < b; });
            if (it == cands.end() || it->bit != bit) return fail(UP_BZ_BAD_MAGIC, bit);
            const size_t ci = (size_t)(it - cands.begin());
            if (it->kind == 1) {
                if (bit + 80 > n * 8) return fail(UP_BZ_TRUNCATED, bit);
                C.streams.back().stored_crc = (uint32_t)bz_bits_at(src, bit + 48, 32);
                pos = (bit + 80 + 7) / 8;
                break;
            }
            const BzRec &R = recs[ci];
            if (R.err) return fail(R.err, bit);
            if (R.n_block > cap) return fail(UP_BZ_OVERFLOW, bit);
            if (R.end_bit <= bit) return fail(UP_BZ_BAD_MAGIC, bit);  // cannot happen: a block has a header
            C.blocks.push_back({(uint32_t)ci, (uint32_t)C.streams.size() - 1});
            C.streams.back().n_blocks++;
            bit = R.end_bit;
        }
        info.streams++;
        if (pos == n) break;
    }
    info.blocks = (uint32_t)C.blocks.size();
    info.dropped = (uint32_t)(cands.size() - C.blocks.size() - C.streams.size());
    return UP_BZ_OK;
}

// block CRCs against the stored ones, then each stream's combined CRC, in
// file order.  crc[i] = computed CRC of chain block i.
inline int bz_check_crcs(const BzChain &C, const std::vector<BzCand> &cands, const std::vector<BzRec> &recs,
                         const uint32_t *crc, up_bz_info_t &info) {
    for (const BzChainStream &s : C.streams) {
        uint32_t comb = 0;
        for (uint32_t b = s.first_block; b < s.first_block + s.n_blocks; ++b) {
            const uint32_t ci = C.blocks[b].cand;
            if (crc[b] != recs[ci].stored_crc) {
                info.reason = UP_BZ_BLOCK_CRC;
                info.fail_bit = cands[ci].bit;
                return UP_BZ_BLOCK_CRC;
            }
            comb = ((comb << 1) | (comb >> 31)) ^ crc[b];
        }
        if (comb != s.stored_crc) {
            info.reason = UP_BZ_STREAM_CRC;
            info.fail_bit = s.bit;
            return UP_BZ_STREAM_CRC;
        }
    }
    return UP_BZ_OK;
}

// inverse BWT of one block on the host: tt[0, n) with its histogram into
// txt[0, n).  Position p of the sorted column holds byte F[p] and the index
// succ[p] of the BWT byte it came from (stable within equal bytes); the text
// is F[p] for p = origPtr, succ[origPtr], ...
inline void bz_unbwt_host(const uint8_t *tt, uint32_t n, const uint32_t *hist, uint32_t orig_ptr,
                          std::vector<uint32_t> &work, uint8_t *txt) {
    uint32_t cf[256], at = 0;
    for (uint32_t i = 0; i < 256; ++i) {
        cf[i] = at;
        at += hist[i];
    }
    work.resize(n);
    for (uint32_t i = 0; i < n; ++i) work[cf[tt[i]]++] = (i << 8) | tt[i];
    uint32_t p = orig_ptr;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t w = work[p];
        txt[i] = (uint8_t)w;
        p = w >> 8;
    }
}

// The host twin: serial along the chain, no scan.  Writes at most cap bytes
// to dst and returns the full size in *n_out; UP_BZ_* as the result.
inline int bz_decode_host(const uint8_t *src, uint64_t n, uint8_t *dst, uint64_t cap_out, uint64_t *n_out,
                          up_bz_info_t &info) {
    info = up_bz_info_t{0, 0, 0, UP_BZ_OK, 0};
    *n_out = 0;
    auto fail = [&](int reason, uint64_t bit) {
        info.reason = reason;
        info.fail_bit = bit;
        return reason;
    };
    std::unique_ptr<BzTables> T(new BzTables);
    std::vector<uint8_t> tt(kBzMaxCap), txt(kBzMaxCap);
    std::vector<uint32_t> work;
    uint32_t hist[256];
    uint64_t pos = 0, out = 0;
    for (;;) {
        int reason = 0;
        const uint32_t level = bz_stream_level(src, n, pos, pos == 0, &reason);
        if (!level) return fail(reason, pos * 8);
        const uint32_t cap = level * 100000;
        uint64_t bit = pos * 8 + 32;
        uint32_t comb = 0;
        for (;;) {
            if (bit + 48 > n * 8) return fail(UP_BZ_TRUNCATED, bit);
            const uint64_t magic = bz_bits_at(src, bit, 48);
            if (magic == kBzEndMagic) {
                if (bit + 80 > n * 8) return fail(UP_BZ_TRUNCATED, bit);
                if ((uint32_t)bz_bits_at(src, bit + 48, 32) != comb) return fail(UP_BZ_STREAM_CRC, pos * 8);
                pos = (bit + 80 + 7) / 8;
                break;
            }
            if (magic != kBzBlockMagic) return fail(UP_BZ_BAD_MAGIC, bit);
            BzRec R;
            bz_entropy_host(src, n, bit, cap, *T, tt.data(), hist, R);
            if (R.err) return fail(R.err, bit);
            bz_unbwt_host(tt.data(), R.n_block, hist, R.orig_ptr, work, txt.data());
            uint32_t crc = 0;
            const uint64_t room = out < cap_out ? cap_out - out : 0;
            out += bz_rle_expand(txt.data(), R.n_block, room ? dst + out : nullptr, room, bz_crc_table(), &crc);
            if (crc != R.stored_crc) return fail(UP_BZ_BLOCK_CRC, bit);
            comb = ((comb << 1) | (comb >> 31)) ^ crc;
            info.blocks++;
            bit = R.end_bit;
        }
        info.streams++;
        if (pos == n) break;
    }
    *n_out = out;
    if (out > cap_out) return fail(UP_BZ_NOSPACE, 0);
    return UP_BZ_OK;
}

// the body of the C entry up_bz_decode_host (bzip2.hip forwards to it; the
// sanitizer check compiles it a second time)
inline int bz_decode_host_capi(const void *src, uint64_t n, void *dst, uint64_t cap, uint64_t *n_out,
                               up_bz_info_t *info) {
    up_bz_info_t local;
    if (!info) info = &local;
    *info = up_bz_info_t{0, 0, 0, UP_BZ_OK, 0};
    if (!n_out || (n && !src) || (cap && !dst)) return UP_E_ARG;
    const int r = bz_decode_host((const uint8_t *)src, n, (uint8_t *)dst, cap, n_out, *info);
    if (r != UP_BZ_OK && r != UP_BZ_NOSPACE) *n_out = 0;
    return r == UP_BZ_OK ? UP_OK : UP_E_ARG;
}

inline const char *bz_reason_text(int r) {
    switch (r) {
    case UP_BZ_OK: return "ok";
    case UP_BZ_NOT_BZIP2: return "not in bzip2 format";
    case UP_BZ_BAD_LEVEL: return "bzip2 level byte outside 1..9";
    case UP_BZ_TRUNCATED: return "bzip2 stream ends early";
    case UP_BZ_BAD_MAGIC: return "bzip2 block or end marker missing";
    case UP_BZ_RANDOMISED: return "randomised bzip2 block (pre-0.9.5) not supported";
    case UP_BZ_ORIGPTR: return "bzip2 block start pointer out of range";
    case UP_BZ_SYMMAP: return "bzip2 block uses no symbol";
    case UP_BZ_NGROUPS: return "bzip2 coding table count outside 2..6";
    case UP_BZ_NSELECTORS: return "bzip2 block has no selector";
    case UP_BZ_SELECTOR: return "bzip2 selector out of range";
    case UP_BZ_CODELEN: return "bzip2 code length outside 1..20";
    case UP_BZ_BAD_CODE: return "invalid bzip2 code";
    case UP_BZ_OVERFLOW: return "bzip2 block larger than its capacity";
    case UP_BZ_BLOCK_CRC: return "bzip2 block CRC mismatch";
    case UP_BZ_STREAM_CRC: return "bzip2 stream CRC mismatch";
    case UP_BZ_TRAILING: return "trailing bytes after the bzip2 stream";
    case UP_BZ_NOSPACE: return "output buffer too small";
    }
    return "unknown bzip2 error";
}

}  // namespace upk
