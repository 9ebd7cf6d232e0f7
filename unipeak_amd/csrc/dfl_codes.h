// unipeak_amd/csrc/dfl_codes.h -- length-limited Huffman code lengths for the
// DEFLATE encoder, the same routine on the host (up_dfl_code_lengths) and on
// the device (deflate.hip), plus the symbol arithmetic of RFC 1951 3.2.5.
//
// dfl_lengths_sorted() takes the used symbols in ascending (freq, symbol)
// order -- the host sorts, the device ranks in parallel; the keys are unique,
// so both give the same order -- and
//  1. builds the Huffman tree with the two-queue method (leaves in sorted
//     order, internal nodes in creation order: both queues are ascending, a
//     leaf wins a tie), which is O(m) and needs no heap;
//  2. counts the leaves per depth, every depth above max_len clamped to it;
//  3. repairs the Kraft sum K = sum 2^(max_len - len) to exactly 2^max_len:
//     while K is above it, the deepest leaf that is still above max_len moves
//     one level down (K drops by 2^(max_len - d - 1)); if the last such move
//     overshoots, leaves move one level up, largest gain that fits first (a
//     leaf at max_len gains 1, and that level is populated whenever a clamp
//     happened, so the deficit always closes);
//  4. hands the lengths out in sorted order, longest to the least frequent,
//     so a more frequent symbol never has a longer code.  That costs nothing:
//     for a fixed multiset of lengths it is the cheapest assignment.
// Where no depth exceeds max_len, steps 2-4 leave the Huffman cost as it is.
// m <= 2^max_len is the caller's check (no prefix code exists otherwise).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UPK_DFL_HD __host__ __device__
#else
#define UPK_DFL_HD
#endif

namespace upk {

constexpr int kDflMaxSyms = 288;  // literal/length alphabet (286 used)
constexpr int kDflMaxBits = 15;

// scratch of one dfl_lengths_sorted call
struct DflScratch {
    uint32_t node_freq[kDflMaxSyms];   // internal nodes in creation order
    uint16_t leaf_parent[kDflMaxSyms];
    uint16_t node_parent[kDflMaxSyms];
    uint16_t node_depth[kDflMaxSyms];
    uint32_t bl_count[kDflMaxBits + 1];
};

// len[order[j]] for j < m; len of other symbols is not touched.  bl_count of
// the result is left in s->bl_count[1..max_len].
UPK_DFL_HD inline void dfl_lengths_sorted(const uint32_t *freq, const uint16_t *order, uint32_t m,
                                          uint32_t max_len, uint8_t *len, DflScratch *s) {
    for (uint32_t d = 0; d <= (uint32_t)kDflMaxBits; ++d) s->bl_count[d] = 0;
    if (m == 0) return;
    if (m == 1) {
        len[order[0]] = 1;
        s->bl_count[1] = 1;
        return;
    }
    uint32_t li = 0, ni = 0;  // heads of the leaf queue and the internal-node queue
    for (uint32_t k = 0; k + 1 < m; ++k) {
        uint32_t sum = 0;
        for (int pick = 0; pick < 2; ++pick) {
            const bool leaf = li < m && (ni >= k || freq[order[li]] <= s->node_freq[ni]);
            if (leaf) {
                sum += freq[order[li]];
                s->leaf_parent[li++] = (uint16_t)k;
            } else {
                sum += s->node_freq[ni];
                s->node_parent[ni++] = (uint16_t)k;
            }
        }
        s->node_freq[k] = sum;
    }
    s->node_depth[m - 2] = 0;
    for (uint32_t k = m - 2; k-- > 0;) s->node_depth[k] = (uint16_t)(s->node_depth[s->node_parent[k]] + 1);
    for (uint32_t j = 0; j < m; ++j) {
        uint32_t d = (uint32_t)s->node_depth[s->leaf_parent[j]] + 1;
        if (d > max_len) d = max_len;
        s->bl_count[d]++;
    }
    const uint32_t target = 1u << max_len;
    uint32_t kraft = 0;
    for (uint32_t d = 1; d <= max_len; ++d) kraft += s->bl_count[d] << (max_len - d);
    while (kraft > target) {
        uint32_t d = max_len - 1;
        while (s->bl_count[d] == 0) --d;
        s->bl_count[d]--;
        s->bl_count[d + 1]++;
        kraft -= 1u << (max_len - d - 1);
    }
    while (kraft < target) {
        for (uint32_t d = 2; d <= max_len; ++d) {
            const uint32_t gain = 1u << (max_len - d);
            if (s->bl_count[d] && gain <= target - kraft) {
                s->bl_count[d]--;
                s->bl_count[d - 1]++;
                kraft += gain;
                break;
            }
        }
    }
    uint32_t j = 0;  // ascending frequency takes the longest codes first
    for (uint32_t d = max_len; d >= 1; --d)
        for (uint32_t c = s->bl_count[d]; c > 0; --c) len[order[j++]] = (uint8_t)d;
}

// The whole routine on the host (up_dfl_code_lengths): sorts the used symbols
// by (freq, symbol), then dfl_lengths_sorted.  false where no such code
// exists or an argument is out of range.
inline bool dfl_code_lengths_host(const uint32_t *freq, uint32_t n, uint32_t max_len, uint8_t *len) {
    if (!freq || !len || n > (uint32_t)kDflMaxSyms || max_len < 1 || max_len > (uint32_t)kDflMaxBits) return false;
    uint16_t order[kDflMaxSyms];
    uint32_t m = 0;
    uint64_t total = 0;
    for (uint32_t s = 0; s < n; ++s) {
        len[s] = 0;
        total += freq[s];
        if (freq[s]) order[m++] = (uint16_t)s;
    }
    if (total > 0xFFFFFFFFull || m > (1u << max_len)) return false;  // the weights would wrap; too many symbols
    for (uint32_t i = 1; i < m; ++i) {  // insertion sort: at most 288 keys
        const uint16_t v = order[i];
        uint32_t j = i;
        while (j > 0 && (freq[order[j - 1]] > freq[v] || (freq[order[j - 1]] == freq[v] && order[j - 1] > v))) {
            order[j] = order[j - 1];
            --j;
        }
        order[j] = v;
    }
    DflScratch sc;
    dfl_lengths_sorted(freq, order, m, max_len, len, &sc);
    return true;
}

// literal/length symbol of a match length 3..258, its extra-bit count and value
UPK_DFL_HD inline uint32_t dfl_len_sym(uint32_t mlen, uint32_t *ebits, uint32_t *eval) {
    const uint32_t l = mlen - 3;
    if (l < 8) {
        *ebits = 0;
        *eval = 0;
        return 257 + l;
    }
    if (l == 255) {
        *ebits = 0;
        *eval = 0;
        return 285;
    }
    const uint32_t e = (31u - (uint32_t)__builtin_clz(l)) - 2;
    *ebits = e;
    *eval = l & ((1u << e) - 1);
    return 261 + 4 * e + ((l >> e) & 3);
}

// distance symbol of a distance 1..32768
UPK_DFL_HD inline uint32_t dfl_dist_sym(uint32_t dist, uint32_t *ebits, uint32_t *eval) {
    const uint32_t d = dist - 1;
    if (d < 4) {
        *ebits = 0;
        *eval = 0;
        return d;
    }
    const uint32_t e = (31u - (uint32_t)__builtin_clz(d)) - 1;
    *ebits = e;
    *eval = d & ((1u << e) - 1);
    return 2 * e + 2 + ((d >> e) & 1);
}

// extra bits of a literal/length symbol and of a distance symbol
UPK_DFL_HD inline uint32_t dfl_ll_extra(uint32_t sym) {
    return (sym < 265 || sym >= 285) ? 0 : (sym - 261) >> 2;
}
UPK_DFL_HD inline uint32_t dfl_d_extra(uint32_t sym) { return sym < 4 ? 0 : (sym >> 1) - 1; }

// CRC-32 (reflected, polynomial 0xEDB88320) arithmetic on remainders:
// x^0 is 0x80000000.  a * b mod P.
UPK_DFL_HD inline uint32_t dfl_crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
    }
    return p;
}
// x^(8 * nbytes) mod P: feeding nbytes zero bytes multiplies the register by it
UPK_DFL_HD inline uint32_t dfl_crc_xpow8(uint64_t nbytes) {
    uint32_t r = 0x80000000u, b = 0x00800000u;  // 1, x^8
    for (; nbytes; nbytes >>= 1) {
        if (nbytes & 1) r = dfl_crc_mul(r, b);
        b = dfl_crc_mul(b, b);
    }
    return r;
}

}  // namespace upk
