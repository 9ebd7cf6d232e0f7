// unipeak_amd/csrc/proftext.hip -- the -w wiggle lines formatted on the device
// (up_unit_profile_text).  #included by api.hip.
//
// Input: the dense f and r of a position range [first, first + count), as the
// fused K1 profile path or wide_profile_kernel leave them.  Output: the lines
// "<pos> <%g of f + r>\n" of every position whose f + r is not 0, ascending
// and contiguous, their byte and line counts, and the byte offsets of
// caller-given cut positions.  The digits come from fmt_g6.h, the routine
// up_format_g6 runs on the host.
//
// A workgroup of 256 threads owns 1,024 consecutive positions, four per thread,
// in all three kernels, so that a line's offset is the sum of the lengths in
// front of it in position order and nothing depends on timing (no atomics):
//
//   proftext_len_kernel    f + r of every position (one IEEE add), its six
//                          digits and exponent packed into one code word (0: no
//                          line), and per workgroup the bytes and lines of its
//                          1,024 positions; a score the digit routine does not
//                          format (or |score| >= limit) raises the range's flag
//   proftext_scan_kernel   one workgroup: the exclusive prefix of the
//                          workgroups' bytes, the totals and the flag in
//                          totals[0..2]
//   proftext_write_kernel  lengths again from the code words, a workgroup scan,
//                          every thread's lines into LDS as bytes, then the
//                          workgroup's text out as aligned dwords with a byte
//                          head and tail (the text sits in LDS at the global
//                          offset's residue mod 4, so both sides are aligned)
//   proftext_cut_kernel    one wave per cut: the workgroup's prefix plus the
//                          lengths of its positions below the cut
//
// The code array is padded to whole workgroups and f, r to whole groups of
// four positions (zero-filled), so every vector access is in bounds.

#include "fmt_g6.h"

namespace upk {

constexpr int kPtThreads = 256;
constexpr int kPtPer = 4;                            // positions per thread
constexpr uint32_t kPtBlock = kPtThreads * kPtPer;   // positions per workgroup
constexpr int kPtPosMax = 10;                        // digits of a position (checked by the caller)
constexpr int kPtLineMax = kPtPosMax + 1 + 1 + kG6Max + 1;  // pos, ' ', '-', score, '\n'
constexpr uint32_t kPtLdsWords = (kPtBlock * kPtLineMax + 3) / 4 + 1;  // + the residue shift

// code word of a line: the six digits, the exponent + 64, the sign, "a line"
constexpr uint32_t kPtLine = 1u << 31;

__device__ inline uint32_t pt_code(double f, double r, double limit, bool &bad) {
    const double s = f + r;
    if (s == 0) return 0;  // (a NaN is not 0: the digit routine refuses it)
    uint32_t D;
    int X;
    bool neg;
    bool ok = g6_digits((uint64_t)__double_as_longlong(s), &D, &X, &neg);
    if (ok && !(__builtin_fabs(s) < limit)) ok = false;
    if (!ok) {
        bad = true;
        return 0;
    }
    return kPtLine | D | ((uint32_t)(X + 64) << 20) | (neg ? 1u << 27 : 0u);
}

__device__ inline int pt_posdig(uint64_t p) {  // p < 10^10
    return 1 + (p >= 10ull) + (p >= 100ull) + (p >= 1000ull) + (p >= 10000ull) + (p >= 100000ull) +
           (p >= 1000000ull) + (p >= 10000000ull) + (p >= 100000000ull) + (p >= 1000000000ull);
}

__device__ inline uint32_t pt_linelen(uint32_t code, uint64_t pos, int negate) {
    if (!code) return 0;
    return (uint32_t)(pt_posdig(pos) + 1 + (negate ? 1 : 0) +
                      g6_len(code & 0xfffffu, (int)((code >> 20) & 0x7fu) - 64, (code >> 27) & 1u) + 1);
}

// sum over the workgroup (kPtThreads threads); every thread gets it
__device__ inline uint32_t pt_block_sum(uint32_t v, uint32_t *sh /* [4] */) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

// exclusive prefix of v over the workgroup in thread order; *total: the sum
template <typename T>
__device__ inline T pt_block_excl(T v, T *sh /* [4] */, T *total) {
    T inc = v;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) {
        const T t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();
    if (lane == 63) sh[w] = inc;
    __syncthreads();
    T base = 0;
    for (int i = 0; i < w; ++i) base += sh[i];
    *total = sh[0] + sh[1] + sh[2] + sh[3];
    return base + inc - v;
}

__global__ __launch_bounds__(kPtThreads) void proftext_len_kernel(
    const double *__restrict__ f, const double *__restrict__ r, uint64_t first, uint32_t count, int negate,
    double limit, uint32_t *__restrict__ code, uint32_t *__restrict__ blk_bytes,
    uint32_t *__restrict__ blk_lines, uint32_t *__restrict__ flag) {
    __shared__ uint32_t sh[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kPtBlock + (uint64_t)threadIdx.x * kPtPer;
    uint32_t c[kPtPer] = {0, 0, 0, 0};
    uint32_t bytes = 0, lines = 0;
    bool bad = false;
    if (i0 < count) {  // (f and r are padded to a multiple of four positions)
        const double2 fa = *(const double2 *)(f + i0), fb = *(const double2 *)(f + i0 + 2);
        const double2 ra = *(const double2 *)(r + i0), rb = *(const double2 *)(r + i0 + 2);
        const double fv[kPtPer] = {fa.x, fa.y, fb.x, fb.y}, rv[kPtPer] = {ra.x, ra.y, rb.x, rb.y};
#pragma unroll
        for (int j = 0; j < kPtPer; ++j) {
            if (i0 + j >= count) continue;
            c[j] = pt_code(fv[j], rv[j], limit, bad);
            if (c[j]) {
                bytes += pt_linelen(c[j], first + i0 + j, negate);
                ++lines;
            }
        }
    }
    *(uint4 *)(code + i0) = make_uint4(c[0], c[1], c[2], c[3]);
    if (bad) *flag = 1u;  // (every writer stores the same word)
    const uint32_t tb = pt_block_sum(bytes, sh);
    const uint32_t tl = pt_block_sum(lines, sh);
    if (threadIdx.x == 0) {
        blk_bytes[blockIdx.x] = tb;
        blk_lines[blockIdx.x] = tl;
    }
}

// blk_off[0 .. nblk]: bytes in front of each workgroup ([nblk]: all of them);
// totals: bytes, lines, flag
__global__ __launch_bounds__(kPtThreads) void proftext_scan_kernel(
    const uint32_t *__restrict__ blk_bytes, const uint32_t *__restrict__ blk_lines, uint32_t nblk,
    const uint32_t *__restrict__ flag, uint64_t *__restrict__ blk_off, uint64_t *__restrict__ totals) {
    __shared__ uint64_t sh[4];
    uint64_t carry = 0, lines = 0;
    for (uint32_t b0 = 0; b0 < nblk; b0 += kPtThreads) {  // (uniform trip count)
        const uint32_t b = b0 + threadIdx.x;
        const uint64_t v = b < nblk ? blk_bytes[b] : 0, l = b < nblk ? blk_lines[b] : 0;
        uint64_t tot, ltot;
        const uint64_t ex = pt_block_excl<uint64_t>(v, sh, &tot);
        (void)pt_block_excl<uint64_t>(l, sh, &ltot);
        if (b < nblk) blk_off[b] = carry + ex;
        carry += tot;
        lines += ltot;
    }
    if (threadIdx.x == 0) {
        blk_off[nblk] = carry;
        totals[0] = carry;
        totals[1] = lines;
        totals[2] = *flag;
    }
}

__global__ __launch_bounds__(kPtThreads) void proftext_write_kernel(
    const uint32_t *__restrict__ code, const uint64_t *__restrict__ blk_off, uint64_t first, int negate,
    uint8_t *__restrict__ text) {
    __shared__ uint32_t lw[kPtLdsWords];
    __shared__ uint32_t sh[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kPtBlock + (uint64_t)threadIdx.x * kPtPer;
    const uint4 cv = *(const uint4 *)(code + i0);
    const uint32_t c[kPtPer] = {cv.x, cv.y, cv.z, cv.w};
    uint32_t len[kPtPer], mine = 0;
#pragma unroll
    for (int j = 0; j < kPtPer; ++j) {
        len[j] = pt_linelen(c[j], first + i0 + j, negate);
        mine += len[j];
    }
    uint32_t total;
    uint32_t o = pt_block_excl<uint32_t>(mine, sh, &total);
    const uint64_t G = blk_off[blockIdx.x];
    const uint32_t shift = (uint32_t)(G & 3u);
    uint8_t *l8 = (uint8_t *)lw + shift;  // l8[x] is the byte for text[G + x]
#pragma unroll
    for (int j = 0; j < kPtPer; ++j) {
        if (!len[j]) continue;
        uint64_t p = first + i0 + j;
        const int nd = pt_posdig(p);
        for (int k = nd - 1; k >= 0; --k) {
            const uint64_t q = p / 10ull;
            l8[o + k] = (uint8_t)('0' + (uint32_t)(p - q * 10ull));
            p = q;
        }
        uint32_t w = o + nd;
        l8[w++] = ' ';
        if (negate) l8[w++] = '-';
        w += g6_put(l8 + w, c[j] & 0xfffffu, (int)((c[j] >> 20) & 0x7fu) - 64, (c[j] >> 27) & 1u);
        l8[w++] = '\n';
        o += len[j];
    }
    __syncthreads();
    // bytes until the global address is a multiple of 4, dwords, bytes
    const uint32_t head = min(total, (4u - shift) & 3u);
    const uint32_t nw = (total - head) / 4u;
    const uint32_t tail0 = head + nw * 4u;
    if (threadIdx.x < head) text[G + threadIdx.x] = l8[threadIdx.x];
    uint32_t *gw = (uint32_t *)(text + G + head);
    const uint32_t *sw = lw + (shift + head) / 4u;
    for (uint32_t w = threadIdx.x; w < nw; w += kPtThreads) gw[w] = sw[w];
    if (threadIdx.x < total - tail0) text[G + tail0 + threadIdx.x] = l8[tail0 + threadIdx.x];
}

// cut_off[i] = bytes of the lines at positions < cut_pos[i]; one wave per cut
__global__ __launch_bounds__(64) void proftext_cut_kernel(
    const uint32_t *__restrict__ code, const uint64_t *__restrict__ blk_off, uint32_t nblk, uint64_t first,
    uint32_t count, int negate, const uint64_t *__restrict__ cut_pos, uint32_t n_cuts, uint64_t *__restrict__ cut_off) {
    const uint32_t ci = blockIdx.x;
    if (ci >= n_cuts) return;
    const uint64_t p = cut_pos[ci] - first;  // (first <= cut_pos <= first + count: the caller)
    if (p >= count) {
        if (threadIdx.x == 0) cut_off[ci] = blk_off[nblk];
        return;
    }
    const uint32_t b = (uint32_t)(p / kPtBlock);
    uint32_t v = 0;
    for (uint64_t i = (uint64_t)b * kPtBlock + threadIdx.x; i < p; i += 64) v += pt_linelen(code[i], first + i, negate);
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if (threadIdx.x == 0) cut_off[ci] = blk_off[b] + v;
}

}  // namespace upk
