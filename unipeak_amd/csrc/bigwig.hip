// unipeak_amd/csrc/bigwig.hip -- the -w profile as bigWig items, section
// statistics and zoom summaries on the device (up_unit_profile_bigwig).
// #included by api.hip, after proftext.hip (its workgroup helpers and scan).
//
// Input: the dense f and r of a position range [first, first + count), as for
// proftext.hip.  An item's value is the float a reader of the -w line gets,
// (float)strtod("<%g of f + r>"), made from the six digits without any text
// (fmt_g6.h: g6_digits_to_float).  Nothing depends on timing: no atomics, every
// offset is a prefix sum in position order, every sum has a fixed order.
//
//   bigwig_value_kernel     a workgroup of 256 threads owns 1,024 positions, four
//                           per thread: f + r (one IEEE add), its digits, the
//                           float's bits into a dense array (0: no item; positions
//                           above clip_end are 0 as well), the workgroup's item
//                           count; a score the routine refuses (or |score| >=
//                           limit) raises the range's flag
//   proftext_scan_kernel    (proftext.hip) the exclusive prefix of the counts
//   bigwig_items_kernel     the (start = pos - 1, value) pairs compacted through
//                           LDS, written out as consecutive 8-byte words
//   bigwig_sections_kernel  one wave per 1,024 consecutive items: extent, min,
//                           max, and the sums of v and v * v in FP64 (lane l adds
//                           items l, l + 64, ... in order, then a fixed tree)
//   bigwig_zoom0_kernel     level 0 bins [j * R, (j + 1) * R) of 0-based starts
//                           from the dense array, one thread per bin, in order
//   bigwig_zoomup_kernel    level z + 1 from level z: four children in ascending
//                           order, the doubles added before any rounding
//   bigwig_zcount_kernel    non-empty bins per workgroup of 256 bins, all levels
//                           in one launch (a level's bins are padded to whole
//                           workgroups, so its records are a range of the prefix)
//   bigwig_zwrite_kernel    the 32-byte on-disk records of the non-empty bins
//
// The dense array is padded to whole workgroups (zeros), f and r to whole
// groups of four positions, the level arrays to whole workgroups of bins.

namespace upk {

constexpr int kBwMaxLevels = 10;
constexpr uint32_t kBwSection = 1024;  // items per section
constexpr uint32_t kBwZBlock = 256;    // bins per workgroup of the zoom compaction

struct BwBin {  // one bin of one level, 32 bytes
    double sum, sumsq;
    float vmin, vmax;
    uint32_t valid, pad;
};

struct BwSection {  // up_bw_section
    uint32_t start, end, count, pad;
    float vmin, vmax;
    double sum, sumsq;
};

struct BwLevels {  // where each level's bins sit in the bin array, in workgroups of kBwZBlock
    uint32_t n;
    uint32_t blk0[kBwMaxLevels + 1];
    uint32_t nbins[kBwMaxLevels];
    uint32_t red[kBwMaxLevels];
};

__global__ __launch_bounds__(kPtThreads) void bigwig_value_kernel(
    const double *__restrict__ f, const double *__restrict__ r, uint64_t first, uint32_t count, int negate,
    uint64_t clip_end, double limit, uint32_t *__restrict__ val, uint32_t *__restrict__ blk_cnt,
    uint32_t *__restrict__ flag) {
    __shared__ uint32_t sh[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kPtBlock + (uint64_t)threadIdx.x * kPtPer;
    uint32_t v[kPtPer] = {0, 0, 0, 0};
    uint32_t items = 0;
    bool bad = false;
    if (i0 < count) {  // (f and r are padded to a multiple of four positions)
        const double2 fa = *(const double2 *)(f + i0), fb = *(const double2 *)(f + i0 + 2);
        const double2 ra = *(const double2 *)(r + i0), rb = *(const double2 *)(r + i0 + 2);
        const double fv[kPtPer] = {fa.x, fa.y, fb.x, fb.y}, rv[kPtPer] = {ra.x, ra.y, rb.x, rb.y};
#pragma unroll
        for (int j = 0; j < kPtPer; ++j) {
            if (i0 + j >= count || first + i0 + j > clip_end) continue;
            const double s = fv[j] + rv[j];
            if (s == 0) continue;  // (a NaN is not 0: the digit routine refuses it)
            uint32_t D, fb32 = 0;
            int X;
            bool neg;
            bool ok = g6_digits((uint64_t)__double_as_longlong(s), &D, &X, &neg);
            if (ok && !(__builtin_fabs(s) < limit)) ok = false;
            if (ok) ok = g6_digits_to_float(D, X, neg != (negate != 0), &fb32);
            if (!ok) {
                bad = true;
                continue;
            }
            v[j] = fb32;  // (not 0: |s| >= 2^-67 is a normal float)
            ++items;
        }
    }
    *(uint4 *)(val + i0) = make_uint4(v[0], v[1], v[2], v[3]);
    if (bad) *flag = 1u;  // (every writer stores the same word)
    const uint32_t t = pt_block_sum(items, sh);
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = t;
}

__global__ __launch_bounds__(kPtThreads) void bigwig_items_kernel(
    const uint32_t *__restrict__ val, const uint64_t *__restrict__ blk_off, uint64_t first,
    uint2 *__restrict__ items) {
    __shared__ uint2 st[kPtBlock];
    __shared__ uint32_t sh[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kPtBlock + (uint64_t)threadIdx.x * kPtPer;
    const uint4 cv = *(const uint4 *)(val + i0);
    const uint32_t v[kPtPer] = {cv.x, cv.y, cv.z, cv.w};
    const uint32_t mine = (v[0] != 0) + (v[1] != 0) + (v[2] != 0) + (v[3] != 0);
    uint32_t total;
    uint32_t o = pt_block_excl<uint32_t>(mine, sh, &total);
#pragma unroll
    for (int j = 0; j < kPtPer; ++j)
        if (v[j]) st[o++] = make_uint2((uint32_t)(first + i0 + j - 1), v[j]);
    __syncthreads();
    uint2 *out = items + blk_off[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < total; i += kPtThreads) out[i] = st[i];
}

__global__ __launch_bounds__(64) void bigwig_sections_kernel(const uint2 *__restrict__ items, uint64_t n_items,
                                                             BwSection *__restrict__ sec) {
    const uint64_t b = (uint64_t)blockIdx.x * kBwSection;
    if (b >= n_items) return;
    const uint32_t n = (uint32_t)(n_items - b < kBwSection ? n_items - b : kBwSection);
    const uint2 *it = items + b;
    double sum = 0, sumsq = 0;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (uint32_t i = threadIdx.x; i < n; i += 64) {
        const float v = __uint_as_float(it[i].y);
        const double d = (double)v;
        sum += d;
        sumsq += d * d;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_down(sum, o, 64);
        sumsq += __shfl_down(sumsq, o, 64);
        lo = fminf(lo, __shfl_down(lo, o, 64));
        hi = fmaxf(hi, __shfl_down(hi, o, 64));
    }
    if (threadIdx.x == 0) {
        BwSection s;
        s.start = it[0].x;
        s.end = it[n - 1].x + 1u;
        s.count = n;
        s.pad = 0;
        s.vmin = lo;
        s.vmax = hi;
        s.sum = sum;
        s.sumsq = sumsq;
        sec[blockIdx.x] = s;
    }
}

// level 0: bin j holds the positions first + j * red .. first + (j + 1) * red - 1 of the call
__global__ __launch_bounds__(256) void bigwig_zoom0_kernel(const uint32_t *__restrict__ val, uint32_t count,
                                                           uint32_t red, uint32_t nbins, BwBin *__restrict__ bins) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= nbins) return;
    const uint64_t a = (uint64_t)j * red;
    const uint64_t e = a + red < count ? a + red : count;
    BwBin b;
    b.sum = b.sumsq = 0;
    b.vmin = __builtin_inff();
    b.vmax = -__builtin_inff();
    b.valid = 0;
    b.pad = 0;
    for (uint64_t i = a; i < e; ++i) {
        const uint32_t w = val[i];
        if (!w) continue;
        const float v = __uint_as_float(w);
        const double d = (double)v;
        b.sum += d;
        b.sumsq += d * d;
        b.vmin = fminf(b.vmin, v);
        b.vmax = fmaxf(b.vmax, v);
        ++b.valid;
    }
    bins[j] = b;
}

__global__ __launch_bounds__(256) void bigwig_zoomup_kernel(const BwBin *__restrict__ below, uint32_t nbelow,
                                                            uint32_t nbins, BwBin *__restrict__ bins) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= nbins) return;
    BwBin b;
    b.sum = b.sumsq = 0;
    b.vmin = __builtin_inff();
    b.vmax = -__builtin_inff();
    b.valid = 0;
    b.pad = 0;
    for (uint32_t k = 0; k < 4u; ++k) {
        const uint64_t c = (uint64_t)j * 4u + k;
        if (c >= nbelow) break;
        const BwBin x = below[c];
        if (!x.valid) continue;
        b.sum += x.sum;
        b.sumsq += x.sumsq;
        b.vmin = fminf(b.vmin, x.vmin);
        b.vmax = fmaxf(b.vmax, x.vmax);
        b.valid += x.valid;
    }
    bins[j] = b;
}

__device__ inline uint32_t bw_level_of(const BwLevels &L, uint32_t blk) {
    uint32_t z = 0;
    while (z + 1 < L.n && blk >= L.blk0[z + 1]) ++z;
    return z;
}

__global__ __launch_bounds__(kBwZBlock) void bigwig_zcount_kernel(const BwBin *__restrict__ bins, BwLevels L,
                                                                  uint32_t *__restrict__ blk_cnt) {
    __shared__ uint32_t sh[4];
    const uint32_t z = bw_level_of(L, blockIdx.x);
    const uint32_t j = (blockIdx.x - L.blk0[z]) * kBwZBlock + threadIdx.x;
    const uint32_t have = j < L.nbins[z] && bins[(uint64_t)blockIdx.x * kBwZBlock + threadIdx.x].valid != 0;
    const uint32_t t = pt_block_sum(have, sh);
    if (threadIdx.x == 0) blk_cnt[blockIdx.x] = t;
}

__global__ __launch_bounds__(kBwZBlock) void bigwig_zwrite_kernel(const BwBin *__restrict__ bins, BwLevels L,
                                                                  const uint64_t *__restrict__ blk_off, uint32_t chrom,
                                                                  uint64_t first, uint64_t clip_end,
                                                                  uint4 *__restrict__ rec) {
    __shared__ uint32_t sh[4];
    const uint32_t z = bw_level_of(L, blockIdx.x);
    const uint32_t j = (blockIdx.x - L.blk0[z]) * kBwZBlock + threadIdx.x;
    BwBin b;
    b.valid = 0;
    if (j < L.nbins[z]) b = bins[(uint64_t)blockIdx.x * kBwZBlock + threadIdx.x];
    uint32_t total;
    const uint32_t o = pt_block_excl<uint32_t>(b.valid != 0, sh, &total);
    if (!b.valid) return;
    const uint64_t start = first - 1 + (uint64_t)j * L.red[z];
    const uint64_t end = start + L.red[z] < clip_end ? start + L.red[z] : clip_end;
    uint4 *out = rec + 2 * (blk_off[blockIdx.x] + o);
    out[0] = make_uint4(chrom, (uint32_t)start, (uint32_t)end, b.valid);
    out[1] = make_uint4(__float_as_uint(b.vmin), __float_as_uint(b.vmax), __float_as_uint((float)b.sum),
                        __float_as_uint((float)b.sumsq));
}

}  // namespace upk
