// unipeak_amd/csrc/bz_block.h -- one bzip2 block from bits to checked fields,
// the same routines on the host (bz_host.h: up_bz_decode_host) and on the
// device (bzip2.hip).  The format is the one libbz2 1.0.x reads and writes
// (DESIGN.md section 17).
//
// Every quantity that comes from the file is range-checked before it indexes
// anything; a failed check returns a UP_BZ_* code and touches no memory.  The
// caller owns all storage:
//   BzBits     MSB-first bit reader over src[0, n), never reads past n
//   BzTables   selectors, code lengths, decode tables and the MTF list of one
//              block (24 KiB: LDS on the device)
//   tt / hist  the block's BWT bytes (at most cap) and their byte histogram
// A block goes through bz_read_header (after its 48-bit magic), bz_build_table
// once per coding table (independent of each other: one lane each on the
// device), bz_decode_symbols, and -- after the inverse BWT, which is the
// caller's -- bz_rle_expand, the run-length stage 1 with the block CRC.
#pragma once

#include <stdint.h>

#include "../../include/unipeak_hip.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UPK_BZ_HD __host__ __device__
#else
#define UPK_BZ_HD
#endif

namespace upk {

constexpr uint64_t kBzBlockMagic = 0x314159265359ull;
constexpr uint64_t kBzEndMagic = 0x177245385090ull;
constexpr uint32_t kBzMaxCap = 900000;      // level 9
constexpr uint32_t kBzMaxSelectors = 18002;  // 2 + 900000 / 50
constexpr uint32_t kBzMaxAlpha = 258;
constexpr uint32_t kBzMaxLen = 20;
constexpr uint32_t kBzGroup = 50;

struct BzBits {
    const uint8_t *p;
    uint64_t n;     // bytes in p
    uint64_t next;  // next byte to load
    uint64_t acc;   // cnt valid bits, left-aligned
    uint32_t cnt;

    UPK_BZ_HD void init(const uint8_t *src, uint64_t bytes, uint64_t bit) {
        p = src;
        n = bytes;
        next = bit >> 3;
        if (next > n) next = n;
        acc = 0;
        cnt = 0;
        const uint32_t skip = (uint32_t)(bit & 7);
        if (skip) {
            fill();
            if (cnt >= skip) {
                acc <<= skip;
                cnt -= skip;
            } else {
                cnt = 0;
            }
        }
    }
    UPK_BZ_HD void fill() {
        while (cnt <= 56 && next < n) {
            acc |= (uint64_t)p[next++] << (56 - cnt);
            cnt += 8;
        }
    }
    // position of the next unread bit
    UPK_BZ_HD uint64_t pos() const { return next * 8 - cnt; }
    // k <= 32 bits; false when the data ends first (nothing is consumed then)
    UPK_BZ_HD bool get(uint32_t k, uint32_t *v) {
        if (cnt < k) {
            fill();
            if (cnt < k) return false;
        }
        *v = k ? (uint32_t)(acc >> (64 - k)) : 0;
        acc = k < 64 ? acc << k : 0;
        cnt -= k;
        return true;
    }
    // the next 20 bits, zero-padded where the data ends; *have = bits there
    UPK_BZ_HD uint32_t peek20(uint32_t *have) {
        if (cnt < 20) fill();
        *have = cnt;
        return (uint32_t)(acc >> 44);
    }
    UPK_BZ_HD void drop(uint32_t k) {  // k <= cnt
        acc <<= k;
        cnt -= k;
    }
};

struct BzTables {
    uint8_t sel[kBzMaxSelectors];
    uint8_t len[6][kBzMaxAlpha];
    int32_t limit[6][kBzMaxLen + 3];
    int32_t base[6][kBzMaxLen + 3];
    uint16_t perm[6][kBzMaxAlpha];
    uint8_t min_len[6], max_len[6];
    uint8_t mtf[256];
    uint8_t seq2unseq[256];
};

// what the entropy stage leaves per block (one per scan candidate on the device)
struct BzRec {
    uint64_t end_bit;  // first bit after EOB
    uint32_t n_block;  // BWT bytes
    uint32_t orig_ptr;
    uint32_t stored_crc;
    int32_t err;  // UP_BZ_*
};

struct BzBlockHdr {
    uint32_t stored_crc;
    uint32_t orig_ptr;
    uint32_t n_in_use;
    uint32_t n_groups;
    uint32_t n_selectors;  // after the cut to kBzMaxSelectors
};

#define UPK_BZ_GET(k, v)                              \
    do {                                              \
        if (!br.get((k), &(v))) return UP_BZ_TRUNCATED; \
    } while (0)

// the block header after its magic: CRC .. code lengths.  cap = the stream's
// block capacity (level * 100,000).
UPK_BZ_HD inline int bz_read_header(BzBits &br, uint32_t cap, BzTables &T, BzBlockHdr &H) {
    uint32_t v = 0;
    UPK_BZ_GET(32, H.stored_crc);
    UPK_BZ_GET(1, v);
    if (v) return UP_BZ_RANDOMISED;
    UPK_BZ_GET(24, H.orig_ptr);
    if (H.orig_ptr >= cap) return UP_BZ_ORIGPTR;
    uint32_t used16 = 0;
    UPK_BZ_GET(16, used16);
    uint32_t n_in_use = 0;
    for (uint32_t i = 0; i < 16; ++i) {
        if (!(used16 & (0x8000u >> i))) continue;
        uint32_t m = 0;
        UPK_BZ_GET(16, m);
        for (uint32_t j = 0; j < 16; ++j)
            if (m & (0x8000u >> j)) T.seq2unseq[n_in_use++] = (uint8_t)(i * 16 + j);  // n_in_use <= 255 here
    }
    if (n_in_use == 0) return UP_BZ_SYMMAP;
    H.n_in_use = n_in_use;
    const uint32_t alpha = n_in_use + 2;  // <= 258
    UPK_BZ_GET(3, H.n_groups);
    if (H.n_groups < 2 || H.n_groups > 6) return UP_BZ_NGROUPS;
    uint32_t n_sel = 0;
    UPK_BZ_GET(15, n_sel);
    if (n_sel < 1) return UP_BZ_NSELECTORS;
    uint32_t order = 0x543210;  // the selectors' MTF list, four bits per entry (registers, not an array)
    for (uint32_t i = 0; i < n_sel; ++i) {
        uint32_t j = 0;
        for (;;) {
            UPK_BZ_GET(1, v);
            if (!v) break;
            if (++j >= H.n_groups) return UP_BZ_SELECTOR;
        }
        const uint32_t g = (order >> (4 * j)) & 15u;  // j < n_groups <= 6
        const uint32_t below = order & ((1u << (4 * j)) - 1u);
        order = (order & ~((1u << (4 * (j + 1))) - 1u)) | (below << 4) | g;
        if (i < kBzMaxSelectors) T.sel[i] = (uint8_t)g;  // the rest is read and dropped (libbz2 1.0.8)
    }
    H.n_selectors = n_sel < kBzMaxSelectors ? n_sel : kBzMaxSelectors;
    for (uint32_t t = 0; t < H.n_groups; ++t) {
        uint32_t curr = 0;
        UPK_BZ_GET(5, curr);
        for (uint32_t i = 0; i < alpha; ++i) {
            for (;;) {
                if (curr < 1 || curr > kBzMaxLen) return UP_BZ_CODELEN;
                UPK_BZ_GET(1, v);
                if (!v) break;
                UPK_BZ_GET(1, v);
                curr = v ? curr - 1 : curr + 1;
            }
            T.len[t][i] = (uint8_t)curr;
        }
    }
    return UP_BZ_OK;
}

// limit / base / perm of coding table t (libbz2's BZ2_hbCreateDecodeTables);
// every length is 1..20 here
UPK_BZ_HD inline void bz_build_table(BzTables &T, uint32_t t, uint32_t alpha) {
    const uint8_t *len = T.len[t];
    int32_t *limit = T.limit[t], *base = T.base[t];
    uint32_t lo = 32, hi = 0;
    for (uint32_t i = 0; i < alpha; ++i) {
        if (len[i] > hi) hi = len[i];
        if (len[i] < lo) lo = len[i];
    }
    T.min_len[t] = (uint8_t)lo;
    T.max_len[t] = (uint8_t)hi;
    uint32_t pp = 0;
    for (uint32_t l = lo; l <= hi; ++l)
        for (uint32_t i = 0; i < alpha; ++i)
            if (len[i] == l) T.perm[t][pp++] = (uint16_t)i;
    for (uint32_t i = 0; i < kBzMaxLen + 3; ++i) base[i] = limit[i] = 0;
    for (uint32_t i = 0; i < alpha; ++i) base[len[i] + 1]++;
    for (uint32_t i = 1; i < kBzMaxLen + 3; ++i) base[i] += base[i - 1];
    int64_t vec = 0;  // an over-subscribed set of lengths runs past 2^31 in 32 bits
    for (uint32_t l = lo; l <= hi; ++l) {
        vec += base[l + 1] - base[l];
        limit[l] = (int32_t)(vec - 1 > 0x3fffffff ? 0x3fffffff : vec - 1);
        vec <<= 1;
        if (vec > 0x40000000) vec = 0x40000000;
    }
    for (uint32_t l = lo + 1; l <= hi; ++l) base[l] = ((limit[l - 1] + 1) << 1) - base[l];
}

// the symbol stream up to EOB: the block's BWT bytes into tt[0, *n_block) and
// their counts into hist[0, 256) (zeroed here).  cap <= the size of tt.
UPK_BZ_HD inline int bz_decode_symbols(BzBits &br, const BzBlockHdr &H, BzTables &T, uint32_t cap, uint8_t *tt,
                                       uint32_t *hist, uint32_t *n_block) {
    const uint32_t alpha = H.n_in_use + 2, eob = H.n_in_use + 1;
    for (uint32_t i = 0; i < 256; ++i) {
        hist[i] = 0;
        T.mtf[i] = (uint8_t)i;
    }
    uint32_t nb = 0, group = 0, left = 0, g = 0;
    uint32_t run = 0, run_n = 1;
    *n_block = 0;
    for (;;) {
        if (left == 0) {
            if (group >= H.n_selectors) return UP_BZ_SELECTOR;
            g = T.sel[group++];  // < n_groups
            left = kBzGroup;
        }
        --left;
        uint32_t have = 0;
        const uint32_t peek = br.peek20(&have);
        const uint32_t hi = T.max_len[g];
        uint32_t zn = T.min_len[g];
        while (zn <= hi && (int32_t)(peek >> (20 - zn)) > T.limit[g][zn]) ++zn;
        if (zn > hi) return have < hi ? UP_BZ_TRUNCATED : UP_BZ_BAD_CODE;
        if (zn > have) return UP_BZ_TRUNCATED;
        const int32_t idx = (int32_t)(peek >> (20 - zn)) - T.base[g][zn];
        if (idx < 0 || idx >= (int32_t)alpha) return UP_BZ_BAD_CODE;
        br.drop(zn);
        const uint32_t sym = T.perm[g][idx];
        if (sym <= 1) {  // RUNA / RUNB: bijective base 2
            if (run_n > (1u << 21)) return UP_BZ_OVERFLOW;
            run += run_n << sym;
            run_n <<= 1;
            continue;
        }
        if (run) {
            if (run > cap - nb) return UP_BZ_OVERFLOW;
            const uint8_t uc = T.seq2unseq[T.mtf[0]];
            hist[uc] += run;
            for (uint32_t k = 0; k < run; ++k) tt[nb + k] = uc;
            nb += run;
            run = 0;
            run_n = 1;
        }
        if (sym == eob) break;
        if (nb >= cap) return UP_BZ_OVERFLOW;
        const uint32_t nn = sym - 1;  // 1 .. n_in_use - 1
        const uint8_t m = T.mtf[nn];
        for (uint32_t k = nn; k > 0; --k) T.mtf[k] = T.mtf[k - 1];
        T.mtf[0] = m;
        const uint8_t uc = T.seq2unseq[m];
        hist[uc]++;
        tt[nb++] = uc;
    }
    *n_block = nb;
    return UP_BZ_OK;
}

#undef UPK_BZ_GET

// entry i of the MSB-first CRC-32 table (polynomial 0x04c11db7)
UPK_BZ_HD inline uint32_t bz_crc_entry(uint32_t i) {
    uint32_t c = i << 24;
    for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ 0x04c11db7u : c << 1;
    return c;
}

// run-length stage 1 over a block's bytes after the inverse BWT: four equal
// bytes are followed by a count byte.  Returns the expanded size; writes the
// bytes to dst while they fit dst_cap (dst may be null with dst_cap 0: sizing
// only) and leaves the block CRC in *crc when crc_tab is given.  The run state
// starts fresh: it does not cross blocks.  Count bytes 252..255, which no
// encoder writes, are taken as libbz2 takes them.
UPK_BZ_HD inline uint64_t bz_rle_expand(const uint8_t *txt, uint32_t n, uint8_t *dst, uint64_t dst_cap,
                                        const uint32_t *crc_tab, uint32_t *crc) {
    uint64_t o = 0;
    uint32_t c = 0xffffffffu;
    int32_t prev = -1;
    uint32_t run = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t b = txt[i];
        if (o < dst_cap) dst[o] = b;
        ++o;
        if (crc_tab) c = (c << 8) ^ crc_tab[(c >> 24) ^ b];
        run = (int32_t)b == prev ? run + 1 : 1;
        prev = b;
        if (run == 4 && i + 1 < n) {
            const uint32_t k = txt[++i];
            for (uint32_t j = 0; j < k; ++j) {
                if (o < dst_cap) dst[o] = b;
                ++o;
                if (crc_tab) c = (c << 8) ^ crc_tab[(c >> 24) ^ b];
            }
            prev = -1;
            run = 0;
        }
    }
    if (crc) *crc = ~c;
    return o;
}

}  // namespace upk
