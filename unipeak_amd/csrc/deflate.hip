// unipeak_amd/csrc/deflate.hip -- a DEFLATE (RFC 1951) encoder on the GPU
// (include/unipeak_hip.h "deflate").
//
// One workgroup of 256 threads encodes one independent block of up to 65,536
// input bytes: a 64 KiB piece of a stream (up_dfl_stream) or one segment
// (up_dfl_segments, each a complete zlib stream).  The phases, separated by
// workgroup barriers:
//   1. checksum: every thread runs CRC-32 (stream) or Adler-32 (segment) over
//      its own 256 bytes; the partial values are shifted to the block's end
//      (x^(8 * bytes after) mod P, resp. the Adler sums' closed form) and
//      combined with LDS xor / add, which are order-independent.
//   2. match: in stripes of 256 positions, one per thread.  A position takes
//      two candidates: the most recent position of an earlier stripe with the
//      same hash of its next four bytes (an LDS table filled with atomicMax
//      after every stripe's lookups, so its content does not depend on the
//      order the threads arrive in), and the nearest earlier position inside
//      its own wave with the same next three bytes (63 wave shuffles).  Both
//      are verified byte by byte; the longer one wins, the nearer on a tie.
//      A match never leaves its 512-byte sub-range, so the parse below needs
//      nothing from its neighbour.
//   3. parse: 128 threads walk one sub-range each, greedy with one step of
//      lazy evaluation, write its tokens compactly over the match records and
//      count the symbols (LDS adds).
//   4. codes: the used symbols are ranked by (frequency, symbol) in parallel,
//      one thread per alphabet runs dfl_lengths_sorted (dfl_codes.h), and the
//      canonical codes are derived per symbol.
//   5. emit: per-sub-range bit counts, their prefix sum, then every sub-range
//      writes its bits at its offset.  A 32-bit word that two writers share
//      is ORed in with atomicOr into memory zeroed beforehand; a word that
//      lies inside one writer's range is stored plainly.
// A block whose dynamic-Huffman form is not smaller than stored goes out
// stored.  Nothing depends on timing: a block's bytes are a function of its
// input bytes alone.  A second kernel compacts the blocks' outputs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/unipeak_hip.h"
#include "devmem.h"
#include "dfl_codes.h"

namespace {

constexpr uint32_t kBlock = 65536;   // input bytes per workgroup, at most
constexpr uint32_t kThreads = 256;
constexpr uint32_t kSub = 512;       // bytes per parse sub-range
constexpr uint32_t kSubs = kBlock / kSub;  // 128
constexpr uint32_t kHashBits = 13;
constexpr uint32_t kStoredMax = 65535;
constexpr uint32_t kSlotExtra = 32;  // >= 2 (zlib header) + 10 (two stored headers) + 4 (Adler-32)
constexpr uint32_t kFar3 = 4096;     // a 3-byte match further back than this costs more than literals
constexpr uint64_t kMaxLaunchBlocks = 1024;  // stream mode: 64 MiB per launch

enum { kStream = 0, kZlib = 1 };

struct Shared {
    uint32_t head[1u << kHashBits];  // position + 1 of the latest earlier-stripe occurrence, 0 = none
    uint32_t ll_freq[upk::kDflMaxSyms];
    uint32_t d_freq[32];
    uint16_t ll_order[upk::kDflMaxSyms];
    uint16_t d_order[32];
    uint16_t ll_code[upk::kDflMaxSyms];
    uint16_t d_code[32];
    uint8_t ll_len[upk::kDflMaxSyms];
    uint8_t d_len[32];
    upk::DflScratch sc[2];
    uint32_t crc_tab[256];
    uint32_t sub_cnt[kSubs];
    uint32_t sub_bits[kSubs];
    uint32_t next_ll[16], next_d[16];
    uint32_t ll_used, d_used, ll_top, d_top, body_bits, sum_a, sum_b, crc;
};

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint64_t ld64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// bytes that a[0, cap) and b[0, cap) have in common from the start
__device__ __forceinline__ uint32_t match_len(const uint8_t *a, const uint8_t *b, uint32_t cap) {
    uint32_t k = 0;
    while (k + 8 <= cap) {
        const uint64_t x = ld64(a + k) ^ ld64(b + k);
        if (x) return k + (uint32_t)(__builtin_ctzll(x) >> 3);
        k += 8;
    }
    while (k < cap && a[k] == b[k]) ++k;
    return k;
}

__device__ __forceinline__ uint32_t bit_reverse(uint32_t code, uint32_t len) {
    return __brev(code) >> (32 - len);
}

// LSB-first bit writer into 32-bit words of zeroed global memory.  The first
// word it touches and the last partial one may be shared with a neighbour:
// those are ORed in atomically; every word in between is its own.
struct BitWriter {
    uint32_t *w;
    uint64_t acc = 0;
    uint32_t cnt;
    uint32_t pos;  // absolute bit position (for align)
    bool first = true;
    __device__ BitWriter(uint32_t *base, uint32_t bit) : w(base + (bit >> 5)), cnt(bit & 31), pos(bit) {}
    __device__ void put(uint32_t v, uint32_t nb) {  // nb <= 32, v < 2^nb
        acc |= (uint64_t)v << cnt;
        cnt += nb;
        pos += nb;
        if (cnt >= 32) {
            if (first) atomicOr(w, (uint32_t)acc);
            else *w = (uint32_t)acc;
            first = false;
            ++w;
            acc >>= 32;
            cnt -= 32;
        }
    }
    __device__ void align() { put(0, (0u - pos) & 7); }
    __device__ void finish() {
        if (cnt) atomicOr(w, (uint32_t)acc);
    }
};

template <int MODE>
__global__ void __launch_bounds__(kThreads) dfl_encode(const uint8_t *__restrict__ src_all,
                                                        const uint64_t *__restrict__ seg_off, uint64_t n_total,
                                                        uint32_t *__restrict__ tok_all,
                                                        uint8_t *__restrict__ slots, uint32_t slot_stride,
                                                        uint32_t *__restrict__ sizes,
                                                        uint32_t *__restrict__ sums) {
    __shared__ Shared S;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint64_t blk = blockIdx.x;
    uint64_t base;
    uint32_t n;
    if (MODE == kStream) {
        base = blk * kBlock;
        n = (uint32_t)(n_total - base < kBlock ? n_total - base : kBlock);
    } else {
        base = seg_off[blk];
        n = (uint32_t)(seg_off[blk + 1] - base);
    }
    const uint8_t *src = src_all + base;
    uint32_t *tok = tok_all + base;
    uint8_t *dst = slots + blk * slot_stride;
    const uint32_t pre = MODE == kZlib ? 2 : 0;  // zlib header bytes

    if (MODE == kZlib && n == 0) {  // header, an empty final fixed block, Adler-32 of nothing
        if (tid == 0) {
            const uint8_t e[8] = {0x78, 0x9C, 0x03, 0x00, 0x00, 0x00, 0x00, 0x01};
            for (int i = 0; i < 8; ++i) dst[i] = e[i];
            sizes[blk] = 8;
            sums[blk] = 1;
        }
        return;
    }

    // ---- 0. LDS ----
    for (uint32_t i = tid; i < (1u << kHashBits); i += kThreads) S.head[i] = 0;
    for (uint32_t i = tid; i < (uint32_t)upk::kDflMaxSyms; i += kThreads) {
        S.ll_freq[i] = i == 256 ? 1u : 0u;  // end-of-block
        S.ll_len[i] = 0;
    }
    if (tid < 32) {
        S.d_freq[tid] = 0;
        S.d_len[tid] = 0;
    }
    if (tid < kSubs) S.sub_cnt[tid] = 0;
    {
        uint32_t c = tid;
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        S.crc_tab[tid] = c;
    }
    if (tid == 0) {
        S.ll_used = S.d_used = S.ll_top = S.d_top = S.body_bits = S.sum_a = S.sum_b = S.crc = 0;
    }
    __syncthreads();

    // ---- 1. checksum of src[0, n): thread t owns bytes [256 t, 256 t + 256) ----
    {
        const uint32_t lo = tid * 256 < n ? tid * 256 : n;
        const uint32_t hi = lo + 256 < n ? lo + 256 : n;
        const uint32_t after = n - hi;
        if (MODE == kStream) {
            uint32_t r = tid == 0 ? 0xFFFFFFFFu : 0u;
            uint32_t i = lo;
            for (; i + 4 <= hi; i += 4) {
                uint32_t v = ld32(src + i);
                for (int k = 0; k < 4; ++k, v >>= 8) r = S.crc_tab[(r ^ v) & 0xFF] ^ (r >> 8);
            }
            for (; i < hi; ++i) r = S.crc_tab[(r ^ src[i]) & 0xFF] ^ (r >> 8);
            if (r) atomicXor(&S.crc, upk::dfl_crc_mul(r, upk::dfl_crc_xpow8(after)));
        } else {
            uint32_t a = 0, b = 0;  // b = sum (hi - i) * byte_i <= 255 * 256 * 257 / 2
            for (uint32_t i = lo; i < hi; ++i) {
                a += src[i];
                b += a;
            }
            if (a) {
                atomicAdd(&S.sum_a, a);
                atomicAdd(&S.sum_b, (uint32_t)(((uint64_t)b + (uint64_t)a * after) % 65521u));
            }
        }
    }

    // ---- 2. match candidates, stripe by stripe ----
    for (uint32_t sb = 0; sb < n; sb += kThreads) {
        const uint32_t i = sb + tid;
        const bool in = i < n;
        const uint32_t w = in ? ld32(src + i) : 0u;  // may read up to 3 bytes past n: the buffer is padded
        const uint32_t w3 = w & 0xFFFFFFu;
        const uint32_t h = (w * 2654435761u) >> (32 - kHashBits);
        const bool can4 = in && i + 4 <= n;
        const uint32_t c1 = can4 ? S.head[h] : 0u;
        uint32_t d2 = 0;
#pragma unroll 7
        for (uint32_t d = 1; d < 64; ++d) {
            const uint32_t o = (uint32_t)__shfl_up((int)w3, d, 64);
            if (lane >= d && o == w3 && d2 == 0) d2 = d;
        }
        __syncthreads();  // every lookup of this stripe is done
        if (can4) atomicMax(&S.head[h], i + 1);
        uint32_t best = 0, bdist = 0;
        if (in) {
            uint32_t cap = n - i;
            if (cap > 258) cap = 258;
            const uint32_t room = kSub - (i & (kSub - 1));
            if (cap > room) cap = room;
            if (cap >= 3) {
                if (d2) {
                    best = match_len(src + i, src + i - d2, cap);
                    bdist = d2;
                }
                if (c1 && i - (c1 - 1) <= 32768u) {
                    const uint32_t l1 = match_len(src + i, src + (c1 - 1), cap);
                    if (l1 > best) {
                        best = l1;
                        bdist = i - (c1 - 1);
                    }
                }
                if (best < 3 || (best == 3 && bdist > kFar3)) best = 0;
            }
        }
        if (in) tok[i] = best ? (best << 16) | (bdist - 1) : 0u;
        __syncthreads();  // the inserts are in before the next stripe looks up
    }
    __syncthreads();

    // ---- 3. parse: thread s < 128 owns [512 s, 512 s + 512) ----
    if (tid < kSubs) {
        const uint32_t lo = tid * kSub;
        const uint32_t hi = lo + kSub < n ? lo + kSub : n;
        uint32_t i = lo, k = 0;
        while (i < hi) {
            uint32_t t = tok[i];
            uint32_t len = t >> 16;
            if (len >= 3 && i + 1 < hi && (tok[i + 1] >> 16) > len) len = 0;  // lazy: the next one is longer
            if (len >= 3) {
                uint32_t eb, ev;
                atomicAdd(&S.ll_freq[upk::dfl_len_sym(len, &eb, &ev)], 1u);
                atomicAdd(&S.d_freq[upk::dfl_dist_sym((t & 0xFFFFu) + 1, &eb, &ev)], 1u);
                i += len;
            } else {
                t = src[i];
                atomicAdd(&S.ll_freq[t], 1u);
                i += 1;
            }
            tok[lo + k++] = t;  // k <= i - lo: behind every record still to be read
        }
        S.sub_cnt[tid] = k;
    }
    __syncthreads();

    // ---- 4. code lengths and canonical codes ----
    for (uint32_t s = tid; s < 286; s += kThreads) {
        const uint32_t f = S.ll_freq[s];
        if (!f) continue;
        uint32_t rank = 0;
        for (uint32_t o = 0; o < 286; ++o) {
            const uint32_t g = S.ll_freq[o];
            rank += (g && (g < f || (g == f && o < s))) ? 1u : 0u;
        }
        S.ll_order[rank] = (uint16_t)s;
        atomicAdd(&S.ll_used, 1u);
        atomicMax(&S.ll_top, s + 1);
    }
    if (tid < 30) {
        const uint32_t s = tid, f = S.d_freq[s];
        if (f) {
            uint32_t rank = 0;
            for (uint32_t o = 0; o < 30; ++o) {
                const uint32_t g = S.d_freq[o];
                rank += (g && (g < f || (g == f && o < s))) ? 1u : 0u;
            }
            S.d_order[rank] = (uint16_t)s;
            atomicAdd(&S.d_used, 1u);
            atomicMax(&S.d_top, s + 1);
        }
    }
    __syncthreads();
    if (tid == 0 || tid == 64) {
        const int which = tid == 0 ? 0 : 1;
        upk::DflScratch *sc = &S.sc[which];
        if (which == 0) {
            upk::dfl_lengths_sorted(S.ll_freq, S.ll_order, S.ll_used, 15, S.ll_len, sc);
        } else {
            upk::dfl_lengths_sorted(S.d_freq, S.d_order, S.d_used, 15, S.d_len, sc);
            if (S.d_used == 0) {  // no match at all: one distance code of length 1 is still declared
                S.d_len[0] = 1;
                sc->bl_count[1] = 1;
            }
        }
        uint32_t *next = which == 0 ? S.next_ll : S.next_d;
        uint32_t code = 0;
        next[0] = 0;
        for (uint32_t b = 1; b <= 15; ++b) {
            code = (code + (b > 1 ? sc->bl_count[b - 1] : 0u)) << 1;
            next[b] = code;
        }
    }
    __syncthreads();
    for (uint32_t s = tid; s < 286; s += kThreads) {
        const uint32_t L = S.ll_len[s];
        if (!L) continue;
        uint32_t c = S.next_ll[L];
        for (uint32_t o = 0; o < s; ++o) c += S.ll_len[o] == L ? 1u : 0u;
        S.ll_code[s] = (uint16_t)bit_reverse(c, L);
        atomicAdd(&S.body_bits, S.ll_freq[s] * (L + upk::dfl_ll_extra(s)));
    }
    if (tid < 30) {
        const uint32_t s = tid, L = S.d_len[s];
        if (L) {
            uint32_t c = S.next_d[L];
            for (uint32_t o = 0; o < s; ++o) c += S.d_len[o] == L ? 1u : 0u;
            S.d_code[s] = (uint16_t)bit_reverse(c, L);
            atomicAdd(&S.body_bits, S.d_freq[s] * (L + upk::dfl_d_extra(s)));
        }
    }
    __syncthreads();

    // ---- 5. sizes; stored or dynamic ----
    const uint32_t hlit = S.ll_top > 257 ? S.ll_top : 257;
    const uint32_t hdist = S.d_top > 1 ? S.d_top : 1;
    const uint32_t hdr_bits = 3 + 5 + 5 + 4 + 19 * 3 + 4 * (hlit + hdist);
    const uint32_t end_bits = pre * 8 + hdr_bits + S.body_bits;  // after the end-of-block code
    const uint32_t n_stored = (n + kStoredMax - 1) / kStoredMax;
    uint32_t dyn_bytes, stored_bytes, sum;
    if (MODE == kStream) {
        dyn_bytes = ((end_bits + 3 + 7) >> 3) + 4;  // + the empty stored block of a sync flush
        stored_bytes = n + 5 * n_stored;
        sum = S.crc ^ 0xFFFFFFFFu;
    } else {
        dyn_bytes = ((end_bits + 7) >> 3) + 4;
        stored_bytes = 2 + n + 5 * n_stored + 4;
        sum = (((n + S.sum_b) % 65521u) << 16) | ((1u + S.sum_a) % 65521u);
    }
    if (dyn_bytes >= stored_bytes) {
        if (tid < n_stored) {
            const uint32_t at = tid * kStoredMax;
            const uint32_t len = n - at < kStoredMax ? n - at : kStoredMax;
            uint8_t *p = dst + pre + at + 5 * tid;
            p[0] = (MODE == kZlib && tid + 1 == n_stored) ? 1 : 0;
            p[1] = (uint8_t)len;
            p[2] = (uint8_t)(len >> 8);
            p[3] = (uint8_t)~len;
            p[4] = (uint8_t)(~len >> 8);
        }
        for (uint32_t i = tid; i < n; i += kThreads) dst[pre + 5 * (i / kStoredMax + 1) + i] = src[i];
        if (MODE == kZlib && tid == 0) {
            dst[0] = 0x78;
            dst[1] = 0x9C;
            uint8_t *p = dst + stored_bytes - 4;
            p[0] = (uint8_t)(sum >> 24);
            p[1] = (uint8_t)(sum >> 16);
            p[2] = (uint8_t)(sum >> 8);
            p[3] = (uint8_t)sum;
        }
        if (tid == 0) {
            sizes[blk] = stored_bytes;
            sums[blk] = sum;
        }
        return;
    }

    if (tid < kSubs) {
        const uint32_t lo = tid * kSub, cnt = S.sub_cnt[tid];
        uint32_t bits = 0;
        for (uint32_t k = 0; k < cnt; ++k) {
            const uint32_t t = tok[lo + k];
            if (t >> 16) {
                uint32_t eb, ev, db, dv;
                const uint32_t ls = upk::dfl_len_sym(t >> 16, &eb, &ev);
                const uint32_t ds = upk::dfl_dist_sym((t & 0xFFFFu) + 1, &db, &dv);
                bits += S.ll_len[ls] + eb + S.d_len[ds] + db;
            } else {
                bits += S.ll_len[t];
            }
        }
        S.sub_bits[tid] = bits;
    }
    __syncthreads();
    uint32_t *out32 = reinterpret_cast<uint32_t *>(dst);
    if (tid < kSubs) {
        const uint32_t lo = tid * kSub, cnt = S.sub_cnt[tid];
        if (cnt) {
            uint32_t at = pre * 8 + hdr_bits;
            for (uint32_t s = 0; s < tid; ++s) at += S.sub_bits[s];
            BitWriter bw(out32, at);
            for (uint32_t k = 0; k < cnt; ++k) {
                const uint32_t t = tok[lo + k];
                if (t >> 16) {
                    uint32_t eb, ev, db, dv;
                    const uint32_t ls = upk::dfl_len_sym(t >> 16, &eb, &ev);
                    const uint32_t ds = upk::dfl_dist_sym((t & 0xFFFFu) + 1, &db, &dv);
                    bw.put(S.ll_code[ls] | (ev << S.ll_len[ls]), S.ll_len[ls] + eb);  // <= 20 bits
                    bw.put(S.d_code[ds] | (dv << S.d_len[ds]), S.d_len[ds] + db);     // <= 28 bits
                } else {
                    bw.put(S.ll_code[t], S.ll_len[t]);
                }
            }
            bw.finish();
        }
    } else if (tid == kSubs) {  // the block header
        BitWriter bw(out32, 0);
        if (MODE == kZlib) bw.put(0x9C78u, 16);
        bw.put(MODE == kZlib ? 1u : 0u, 1);  // BFINAL
        bw.put(2, 2);                        // BTYPE: dynamic Huffman
        bw.put(hlit - 257, 5);
        bw.put(hdist - 1, 5);
        bw.put(19 - 4, 4);
        // the code-length code: symbols 0..15 with 4 bits each (complete), 16..18 unused;
        // sent in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
        for (int k = 0; k < 19; ++k) bw.put(k < 3 ? 0u : 4u, 3);
        for (uint32_t s = 0; s < hlit; ++s) bw.put(bit_reverse(S.ll_len[s], 4), 4);
        for (uint32_t s = 0; s < hdist; ++s) bw.put(bit_reverse(S.d_len[s], 4), 4);
        bw.finish();
    } else if (tid == kSubs + 1) {  // end of block and what follows it
        BitWriter bw(out32, end_bits - S.ll_len[256]);
        bw.put(S.ll_code[256], S.ll_len[256]);
        if (MODE == kStream) {
            bw.put(0, 3);  // an empty stored block, not final
            bw.align();
            bw.put(0x0000u, 16);
            bw.put(0xFFFFu, 16);
        } else {
            bw.align();
            bw.put(((sum >> 24) & 0xFF) | ((sum >> 8) & 0xFF00), 16);
            bw.put(((sum >> 8) & 0xFF) | ((sum << 8) & 0xFF00), 16);
        }
        bw.finish();
    }
    if (tid == 0) {
        sizes[blk] = dyn_bytes;
        sums[blk] = sum;
    }
}

// block b's sizes[b] bytes from its slot to out + off[b]; aligned 32-bit
// stores once the destination is aligned
__global__ void __launch_bounds__(kThreads) dfl_compact(const uint8_t *__restrict__ slots, uint32_t slot_stride,
                                                         const uint32_t *__restrict__ sizes,
                                                         const uint64_t *__restrict__ off,
                                                         uint8_t *__restrict__ out) {
    const uint64_t blk = blockIdx.x;
    const uint8_t *s = slots + blk * slot_stride;
    uint8_t *d = out + off[blk];
    const uint32_t n = sizes[blk];
    uint32_t a = (uint32_t)((0 - (uintptr_t)d) & 3);
    if (a > n) a = n;
    if (threadIdx.x < a) d[threadIdx.x] = s[threadIdx.x];
    const uint32_t words = (n - a) >> 2;
    uint32_t *d32 = reinterpret_cast<uint32_t *>(d + a);
    for (uint32_t w = threadIdx.x; w < words; w += kThreads) d32[w] = ld32(s + a + 4 * w);
    const uint32_t done = a + 4 * words;
    if (threadIdx.x < n - done) d[done + threadIdx.x] = s[done + threadIdx.x];
}

}  // namespace

struct up_dfl {
    int dev = 0;
    upk::Stream stream;
    upk::Event ev[2];
    upk::DevBuf<uint8_t> src, slots, out;
    upk::DevBuf<uint32_t> tok, sizes, sums;
    upk::DevBuf<uint64_t> off, seg;
    upk::HostBuf<uint8_t> h_out;
    double ms_kernels = 0;
    uint64_t bytes_in = 0, bytes_out = 0, calls = 0;
};

#define DFCHK(x)                                                                        \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) return e_ == hipErrorOutOfMemory ? UP_E_NOMEM : UP_E_HIP; \
    } while (0)

namespace {

// encode n_blk blocks that are already on the device (h->src, h->seg for
// segments), compact them and append the result to h->h_out at *pos;
// sizes/sums of the blocks come back in the two vectors
template <int MODE>
int run_blocks(up_dfl *h, uint64_t n_blk, uint64_t n_bytes, uint32_t stride, uint64_t *pos,
               std::vector<uint32_t> &sizes, std::vector<uint32_t> &sums, std::vector<uint64_t> &off) {
    hipStream_t st = h->stream;
    DFCHK(h->tok.ensure_exact(n_bytes + 16));
    DFCHK(h->slots.ensure_exact(n_blk * stride));
    DFCHK(h->sizes.ensure_exact(n_blk));
    DFCHK(h->sums.ensure_exact(n_blk));
    DFCHK(h->off.ensure_exact(n_blk + 1));
    DFCHK(hipMemsetAsync(h->slots.p, 0, n_blk * stride, st));
    DFCHK(hipEventRecord(h->ev[0], st));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(dfl_encode<MODE>), dim3((uint32_t)n_blk), dim3(kThreads), 0, st, h->src.p,
                       h->seg.p, n_bytes, h->tok.p, h->slots.p, stride, h->sizes.p, h->sums.p);
    DFCHK(hipGetLastError());
    sizes.resize(n_blk);
    sums.resize(n_blk);
    off.assign(n_blk + 1, 0);
    DFCHK(hipMemcpyAsync(sizes.data(), h->sizes.p, n_blk * 4, hipMemcpyDeviceToHost, st));
    DFCHK(hipMemcpyAsync(sums.data(), h->sums.p, n_blk * 4, hipMemcpyDeviceToHost, st));
    DFCHK(hipStreamSynchronize(st));
    for (uint64_t b = 0; b < n_blk; ++b) {
        if (sizes[b] > stride) return UP_E_INTERNAL;
        off[b + 1] = off[b] + sizes[b];
    }
    const uint64_t total = off[n_blk];
    if (*pos + total > h->h_out.n) return UP_E_INTERNAL;
    DFCHK(h->out.ensure_exact(total + 16));
    DFCHK(hipMemcpyAsync(h->off.p, off.data(), (n_blk + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(dfl_compact, dim3((uint32_t)n_blk), dim3(kThreads), 0, st, h->slots.p, stride,
                       h->sizes.p, h->off.p, h->out.p);
    DFCHK(hipGetLastError());
    DFCHK(hipEventRecord(h->ev[1], st));
    if (total) DFCHK(hipMemcpyAsync(h->h_out.p + *pos, h->out.p, total, hipMemcpyDeviceToHost, st));
    DFCHK(hipStreamSynchronize(st));
    float ms = 0;
    DFCHK(hipEventElapsedTime(&ms, h->ev[0], h->ev[1]));
    h->ms_kernels += ms;
    *pos += total;
    return UP_OK;
}

}  // namespace

extern "C" {

int up_dfl_open(int device, up_dfl **out) {
    if (!out) return UP_E_ARG;
    *out = nullptr;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) return UP_E_NODEV;
    if (device < 0 || device >= nd) return UP_E_ARG;
    up_dfl *h = new up_dfl;
    h->dev = device;
    auto fail = [&](int code) {
        up_dfl_close(h);
        return code;
    };
    if (hipSetDevice(device) != hipSuccess) return fail(UP_E_HIP);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail(UP_E_HIP);
    for (auto &e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(UP_E_HIP);
    *out = h;
    return UP_OK;
}

void up_dfl_close(up_dfl *h) {
    if (!h) return;
    (void)hipSetDevice(h->dev);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
}

uint32_t up_dfl_block(void) { return kBlock; }

uint64_t up_dfl_bound(uint64_t n) {
    // a stored block holds 65,535 bytes: a full 65,536-byte block that goes
    // out stored is two of them, 10 bytes of headers
    return n + 10 * ((n + kBlock - 1) / kBlock);
}

int up_dfl_stream(up_dfl *h, const void *src, uint64_t n, const void **out, uint64_t *n_out, uint32_t *crc32) {
    if (!h || !out || !n_out || (n && !src)) return UP_E_ARG;
    DFCHK(hipSetDevice(h->dev));
    DFCHK(h->h_out.ensure(up_dfl_bound(n) + 16));
    *out = h->h_out.p;
    *n_out = 0;
    if (crc32) *crc32 = 0;
    if (n == 0) return UP_OK;
    hipStream_t st = h->stream;
    uint64_t pos = 0;
    uint32_t crc = 0;
    std::vector<uint32_t> sizes, sums;
    std::vector<uint64_t> off;
    for (uint64_t at = 0; at < n; at += kMaxLaunchBlocks * kBlock) {
        const uint64_t len = std::min<uint64_t>(n - at, kMaxLaunchBlocks * kBlock);
        const uint64_t n_blk = (len + kBlock - 1) / kBlock;
        DFCHK(h->src.ensure_exact(len + 16));
        DFCHK(hipMemcpyAsync(h->src.p, (const uint8_t *)src + at, len, hipMemcpyHostToDevice, st));
        const int rc = run_blocks<kStream>(h, n_blk, len, kBlock + kSlotExtra, &pos, sizes, sums, off);
        if (rc != UP_OK) return rc;
        for (uint64_t b = 0; b < n_blk; ++b) {  // crc(A || B) = crc(A) * x^(8 |B|) + crc(B)
            const uint64_t bl = std::min<uint64_t>(kBlock, len - b * kBlock);
            crc = upk::dfl_crc_mul(crc, upk::dfl_crc_xpow8(bl)) ^ sums[b];
        }
    }
    h->bytes_in += n;
    h->bytes_out += pos;
    h->calls++;
    *n_out = pos;
    if (crc32) *crc32 = crc;
    return UP_OK;
}

int up_dfl_segments(up_dfl *h, const void *src, const uint64_t *seg_off, uint32_t n_seg, const void **out,
                    uint64_t *out_off) {
    if (!h || !out || !out_off || !seg_off) return UP_E_ARG;
    uint64_t longest = 0;
    for (uint32_t i = 0; i < n_seg; ++i) {
        if (seg_off[i + 1] < seg_off[i]) return UP_E_ARG;
        longest = std::max(longest, seg_off[i + 1] - seg_off[i]);
    }
    if (longest > kBlock) return UP_E_ARG;
    const uint64_t lo = seg_off[0], n = seg_off[n_seg] - lo;
    if (n && !src) return UP_E_ARG;
    DFCHK(hipSetDevice(h->dev));
    const uint32_t stride = (uint32_t)((longest + kSlotExtra + 31) & ~(uint64_t)31);
    DFCHK(h->h_out.ensure((uint64_t)n_seg * 16 + n + 10 * (uint64_t)n_seg + 16));
    *out = h->h_out.p;
    out_off[0] = 0;
    if (n_seg == 0) return UP_OK;
    hipStream_t st = h->stream;
    std::vector<uint64_t> rel(n_seg + 1);
    for (uint32_t i = 0; i <= n_seg; ++i) rel[i] = seg_off[i] - lo;
    DFCHK(h->src.ensure_exact(n + 16));
    DFCHK(h->seg.ensure_exact(n_seg + 1));
    if (n) DFCHK(hipMemcpyAsync(h->src.p, (const uint8_t *)src + lo, n, hipMemcpyHostToDevice, st));
    DFCHK(hipMemcpyAsync(h->seg.p, rel.data(), (n_seg + 1) * 8, hipMemcpyHostToDevice, st));
    uint64_t pos = 0;
    std::vector<uint32_t> sizes, sums;
    std::vector<uint64_t> off;
    const int rc = run_blocks<kZlib>(h, n_seg, n, stride, &pos, sizes, sums, off);
    if (rc != UP_OK) return rc;
    for (uint32_t i = 0; i <= n_seg; ++i) out_off[i] = off[i];
    h->bytes_in += n;
    h->bytes_out += pos;
    h->calls++;
    return UP_OK;
}

int up_dfl_timings(up_dfl *h, double *v, int n) {
    if (!h || !v || n < 0) return UP_E_ARG;
    if (n > 0) v[0] = h->ms_kernels;
    if (n > 1) v[1] = (double)h->bytes_in;
    if (n > 2) v[2] = (double)h->bytes_out;
    if (n > 3) v[3] = (double)h->calls;
    return UP_OK;
}

int up_dfl_code_lengths(const uint32_t *freq, uint32_t n, uint32_t max_len, uint8_t *len) {
    return upk::dfl_code_lengths_host(freq, n, max_len, len) ? UP_OK : UP_E_ARG;
}

}  // extern "C"
