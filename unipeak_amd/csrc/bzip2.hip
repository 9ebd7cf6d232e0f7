// unipeak_amd/csrc/bzip2.hip -- a bzip2 decoder on the GPU, parallel over the
// file's blocks (include/unipeak_hip.h "bunzip").
//
// A .bz2 file is a chain of independent blocks that start at any bit.  The
// stages, each one kernel over all blocks (or all candidates) at once:
//   1. bz_scan      every bit offset against the two 48-bit magics; the host
//                   sorts the few hundred hits.
//   2. bz_entropy   one wave per block candidate: header, coding tables (one
//                   lane per table, in LDS), then the Huffman / MTF / run
//                   decode, which is a serial bit chain and runs on one lane.
//                   Leaves the block's BWT bytes, their histogram and a BzRec.
//   3. (host)       bz_chain links the candidates into the exact chain and
//                   drops the false positives of the pattern (bz_host.h).
//   4. bz_rank      one wave per block: stable counting sort into the word
//                   vector w[p] = F[p] | succ[p] << 8, 64 bytes per step (the
//                   rank among equal bytes of a step comes from eight wave
//                   ballots), then marks the walk's starts in bit 31.
//      bz_walk<0>   one lane per start walks succ until the next marked
//                   position and counts its steps;
//      bz_order     follows the segments from origPtr and prefix-sums their
//                   lengths; a permutation that falls into several cycles
//                   (periodic content) does not reach the block length and
//                   is flagged for the serial walk;
//      bz_walk<1>   the same walk again, writing F[p] at the segment's offset
//                   over the block's BWT bytes, which nobody reads any more.
//   5. bz_rle<0/1>  run-length stage 1, one lane per block: sizes first, then,
//                   after the host's prefix sum, bytes to their offsets with
//                   the block CRC on the way.
// Every index that comes from the file was range-checked in bz_block.h; the
// kernels check the derived ones (positions, offsets) once more before a
// store, so a wrong table gives a wrong CRC and never a wild write.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/unipeak_hip.h"
#include "bz_block.h"
#include "bz_host.h"
#include "devmem.h"

namespace {

constexpr uint32_t kSlot = 900096;     // bytes per block slot: kBzMaxCap rounded up to 128
constexpr uint32_t kMaxStarts = 4096;  // walk starts per block, at most
constexpr uint32_t kBatch = 256;       // blocks per inverse-BWT batch (3.6 MB of words each)
constexpr uint32_t kMark = 0x80000000u;
constexpr uint32_t kSuccMask = 0xFFFFFu;  // 20 bits: positions below 900,000

__global__ void __launch_bounds__(256) bz_scan(const uint8_t *__restrict__ src, uint64_t n,
                                               uint64_t *__restrict__ bit_off, uint8_t *__restrict__ kind,
                                               uint64_t cap, unsigned long long *__restrict__ count) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;  // byte
    if (i + 6 > n) return;
    uint64_t w = 0;
    for (uint32_t k = 0; k < 8; ++k) w = (w << 8) | (i + k < n ? src[i + k] : 0u);
    for (uint32_t s = 0; s < 8; ++s) {
        if (i * 8 + s + 48 > n * 8) break;
        const uint64_t v = (w << s) >> 16;
        if (v == upk::kBzBlockMagic || v == upk::kBzEndMagic) {
            const unsigned long long at = atomicAdd(count, 1ull);
            if (at < cap) {
                bit_off[at] = i * 8 + s;
                kind[at] = (uint8_t)(v == upk::kBzEndMagic);
            }
        }
    }
}

struct EntropyShared {
    upk::BzTables T;
    upk::BzBlockHdr H;
    uint32_t hist[256];
    int32_t err;
};

__global__ void __launch_bounds__(64) bz_entropy(const uint8_t *__restrict__ src, uint64_t n,
                                                 const uint64_t *__restrict__ bit, uint8_t *__restrict__ slots,
                                                 uint32_t *__restrict__ hists, upk::BzRec *__restrict__ recs) {
    __shared__ EntropyShared S;
    const uint32_t c = blockIdx.x, tid = threadIdx.x;
    upk::BzBits br;
    br.init(src, n, bit[c] + 48);
    if (tid == 0) S.err = upk::bz_read_header(br, upk::kBzMaxCap, S.T, S.H);
    __syncthreads();
    if (S.err == UP_BZ_OK && tid < S.H.n_groups) upk::bz_build_table(S.T, tid, S.H.n_in_use + 2);
    __syncthreads();
    if (tid == 0) {
        upk::BzRec R{0, 0, 0, 0, S.err};
        if (R.err == UP_BZ_OK) {
            R.err = upk::bz_decode_symbols(br, S.H, S.T, upk::kBzMaxCap, slots + (uint64_t)c * kSlot, S.hist,
                                           &R.n_block);
            R.orig_ptr = S.H.orig_ptr;
            R.stored_crc = S.H.stored_crc;
            R.end_bit = br.pos();
            if (R.err == UP_BZ_OK && R.orig_ptr >= R.n_block) R.err = UP_BZ_ORIGPTR;
        }
        S.err = R.err;
        recs[c] = R;
    }
    __syncthreads();
    if (S.err == UP_BZ_OK)
        for (uint32_t k = tid; k < 256; k += 64) hists[(uint64_t)c * 256 + k] = S.hist[k];
}

__device__ __forceinline__ uint32_t start_stride(uint32_t n, uint32_t n_starts) {
    return (n + n_starts - 1) / n_starts;  // n >= 1
}

// start s of a block: s < n_starts at s * stride, s == n_starts at origPtr
// unless that is one of the others
__device__ __forceinline__ bool start_pos(uint32_t s, uint32_t n_starts, uint32_t n, uint32_t orig, uint32_t *p) {
    const uint32_t stride = start_stride(n, n_starts);
    if (s < n_starts) {
        *p = s * stride;
        return *p < n;
    }
    *p = orig;
    return s == n_starts && orig % stride != 0;
}

__device__ __forceinline__ uint32_t start_id(uint32_t p, uint32_t n_starts, uint32_t n) {
    const uint32_t stride = start_stride(n, n_starts);
    return p % stride == 0 ? p / stride : n_starts;
}

__global__ void __launch_bounds__(64) bz_rank(const uint8_t *__restrict__ slots,
                                              const uint32_t *__restrict__ hists,
                                              const upk::BzRec *__restrict__ recs,
                                              const uint32_t *__restrict__ blk_slot, uint32_t first,
                                              uint32_t *__restrict__ words, uint32_t n_starts) {
    __shared__ uint32_t cnt[256];
    const uint32_t lane = threadIdx.x;
    const uint32_t c = blk_slot[first + blockIdx.x];
    const uint32_t n = min(recs[c].n_block, upk::kBzMaxCap), orig = recs[c].orig_ptr;
    const uint8_t *tt = slots + (uint64_t)c * kSlot;
    uint32_t *w = words + (uint64_t)blockIdx.x * kSlot;
    for (uint32_t k = lane; k < 256; k += 64) cnt[k] = hists[(uint64_t)c * 256 + k];
    __syncthreads();
    if (lane == 0) {
        uint32_t at = 0;
        for (uint32_t k = 0; k < 256; ++k) {
            const uint32_t h = cnt[k];
            cnt[k] = at;
            at += h;
        }
    }
    __syncthreads();
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint32_t lo = 0; lo < n; lo += 64) {
        const uint32_t i = lo + lane;
        const bool valid = i < n;
        const uint32_t v = valid ? tt[i] : 0u;
        uint64_t same = __ballot(valid);
        for (uint32_t k = 0; k < 8; ++k) {
            const uint64_t b = __ballot((v >> k) & 1u);
            same &= ((v >> k) & 1u) ? b : ~b;
        }
        const uint32_t rank = (uint32_t)__popcll(same & below), total = (uint32_t)__popcll(same);
        const uint32_t base = valid ? cnt[v] : 0u;
        __syncthreads();
        if (valid) {
            const uint32_t p = base + rank;
            if (p < n) w[p] = v | (i << 8);
            if (rank + 1 == total) cnt[v] = base + total;
        }
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    const uint32_t stride = start_stride(n, n_starts);
    for (uint32_t s = lane; s < n_starts; s += 64)
        if ((uint64_t)s * stride < n) atomicOr(&w[s * stride], kMark);
    if (lane == 0 && orig < n) atomicOr(&w[orig], kMark);
}

// WRITE = 0: start s walks to the next marked position, leaves its step count
// and where it arrived.  WRITE = 1: the same steps again, F[p] to txt at the
// segment's offset; a block flagged serial is walked by its start 0 alone,
// n steps from origPtr.
template <int WRITE>
__global__ void __launch_bounds__(256) bz_walk(const upk::BzRec *__restrict__ recs,
                                               const uint32_t *__restrict__ blk_slot, uint32_t first,
                                               const uint32_t *__restrict__ words, uint32_t n_starts,
                                               uint32_t *__restrict__ seg_len, uint32_t *__restrict__ seg_next,
                                               const uint32_t *__restrict__ seg_off,
                                               const uint32_t *__restrict__ serial, uint8_t *__restrict__ slots) {
    const uint32_t s = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (s > n_starts) return;
    const uint32_t c = blk_slot[first + b];
    const uint32_t n = min(recs[c].n_block, upk::kBzMaxCap), orig = recs[c].orig_ptr;
    const uint32_t *w = words + (uint64_t)b * kSlot;
    const uint64_t at = (uint64_t)b * (kMaxStarts + 1) + s;
    uint32_t p = 0;
    const bool active = start_pos(s, n_starts, n, orig, &p) && orig < n;
    if (!WRITE) {
        uint32_t len = 0, nxt = 0;
        if (active) {
            uint32_t x = w[p];
            for (;;) {
                nxt = (x >> 8) & kSuccMask;
                ++len;
                if (nxt >= n || len >= n) break;  // nxt >= n: not a permutation, the order kernel sees a short chain
                x = w[nxt];
                if (x & kMark) break;
            }
            if (nxt >= n) nxt = 0, len = 0;
        }
        seg_len[at] = len;
        seg_next[at] = nxt;
    } else {
        uint8_t *txt = slots + (uint64_t)c * kSlot;
        if (serial[b]) {
            if (s != 0 || orig >= n) return;
            p = orig;
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t x = w[p];
                txt[i] = (uint8_t)x;
                p = (x >> 8) & kSuccMask;
                if (p >= n) return;
            }
            return;
        }
        if (!active) return;
        const uint32_t len = seg_len[at];
        uint32_t o = seg_off[at];
        if ((uint64_t)o + len > n) return;
        for (uint32_t i = 0; i < len; ++i) {
            const uint32_t x = w[p];
            txt[o++] = (uint8_t)x;
            p = (x >> 8) & kSuccMask;
            if (p >= n) return;
        }
    }
}

__global__ void __launch_bounds__(256) bz_order(const upk::BzRec *__restrict__ recs,
                                                const uint32_t *__restrict__ blk_slot, uint32_t first,
                                                uint32_t n_starts, const uint32_t *__restrict__ seg_len,
                                                const uint32_t *__restrict__ seg_next,
                                                uint32_t *__restrict__ seg_off, uint32_t *__restrict__ serial) {
    __shared__ uint32_t len[kMaxStarts + 1];
    __shared__ uint32_t nxt[kMaxStarts + 1];
    const uint32_t b = blockIdx.x, c = blk_slot[first + b];
    const uint32_t n = min(recs[c].n_block, upk::kBzMaxCap), orig = recs[c].orig_ptr;
    const uint64_t at = (uint64_t)b * (kMaxStarts + 1);
    for (uint32_t s = threadIdx.x; s <= n_starts; s += 256) {
        len[s] = seg_len[at + s];
        nxt[s] = seg_next[at + s];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t head = orig < n ? start_id(orig, n_starts, n) : 0;
        uint32_t cur = head, off = 0, steps = 0;
        do {
            const uint32_t l = len[cur];
            const uint32_t to = start_id(nxt[cur], n_starts, n);  // <= n_starts
            len[cur] = off;
            off += l;
            cur = to;
            ++steps;
        } while (cur != head && steps <= n_starts && off <= n && off > 0);
        serial[b] = !(cur == head && off == n);
    }
    __syncthreads();
    for (uint32_t s = threadIdx.x; s <= n_starts; s += 256) seg_off[at + s] = len[s];
}

template <int WRITE>
__global__ void __launch_bounds__(64) bz_rle(const upk::BzRec *__restrict__ recs,
                                             const uint32_t *__restrict__ blk_slot,
                                             const uint8_t *__restrict__ slots, uint64_t *__restrict__ sizes,
                                             const uint64_t *__restrict__ off, uint8_t *__restrict__ out,
                                             uint32_t *__restrict__ crcs) {
    __shared__ uint32_t tab[256];
    const uint32_t b = blockIdx.x, c = blk_slot[b];
    const uint32_t n = min(recs[c].n_block, upk::kBzMaxCap);
    const uint8_t *txt = slots + (uint64_t)c * kSlot;
    if (WRITE) {
        for (uint32_t k = threadIdx.x; k < 256; k += 64) tab[k] = upk::bz_crc_entry(k);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    if (!WRITE) {
        sizes[b] = upk::bz_rle_expand(txt, n, nullptr, 0, nullptr, nullptr);
    } else {
        uint32_t crc = 0;
        upk::bz_rle_expand(txt, n, out + off[b], sizes[b], tab, &crc);  // stops writing at the size pass's count
        crcs[b] = crc;
    }
}

}  // namespace

struct up_bz {
    int dev = 0;
    uint32_t n_starts = kMaxStarts;
    upk::Stream stream;
    upk::Event ev[2];
    upk::DevBuf<uint8_t> src, kind, slots, out;
    upk::DevBuf<uint64_t> bit, sizes, off;
    upk::DevBuf<unsigned long long> count;
    upk::DevBuf<uint32_t> hists, words, blk_slot, seg_len, seg_next, seg_off, serial, crcs;
    upk::DevBuf<upk::BzRec> recs;
    upk::HostBuf<uint8_t> h_out;
    double ms[5] = {0, 0, 0, 0, 0};
    uint64_t bytes_in = 0, bytes_out = 0, calls = 0;
};

#define BZCHK(x)                                                                        \
    do {                                                                                \
        hipError_t e_ = (x);                                                            \
        if (e_ != hipSuccess) return e_ == hipErrorOutOfMemory ? UP_E_NOMEM : UP_E_HIP; \
    } while (0)

namespace {

// stage timing: begin() before the launches, end(k) after them (waits for them)
struct StageTimer {
    up_bz *h;
    hipError_t begin() { return hipEventRecord(h->ev[0], h->stream); }
    hipError_t end(int k) {
        hipError_t e = hipEventRecord(h->ev[1], h->stream);
        if (e != hipSuccess) return e;
        e = hipEventSynchronize(h->ev[1]);
        if (e != hipSuccess) return e;
        float ms = 0;
        e = hipEventElapsedTime(&ms, h->ev[0], h->ev[1]);
        if (e == hipSuccess) h->ms[k] += ms;
        return e;
    }
};

// the file onto the device and stage 1: the sorted candidates
int scan_file(up_bz *h, const void *src, uint64_t n, std::vector<upk::BzCand> &cands) {
    hipStream_t st = h->stream;
    StageTimer tm{h};
    cands.clear();
    const uint64_t cap = n / 4 + 16;  // a magic cannot stand again within 32 bits of itself
    BZCHK(h->src.ensure_exact(n + 16));
    BZCHK(h->bit.ensure_exact(cap));
    BZCHK(h->kind.ensure_exact(cap));
    BZCHK(h->count.ensure_exact(1));
    BZCHK(hipMemsetAsync(h->src.p + n, 0, 16, st));
    if (n) BZCHK(hipMemcpyAsync(h->src.p, src, n, hipMemcpyHostToDevice, st));
    BZCHK(hipMemsetAsync(h->count.p, 0, sizeof(unsigned long long), st));
    unsigned long long count = 0;
    if (n >= 6) {
        BZCHK(tm.begin());
        hipLaunchKernelGGL(bz_scan, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, h->src.p, n, h->bit.p,
                           h->kind.p, cap, h->count.p);
        BZCHK(hipGetLastError());
        BZCHK(tm.end(0));
        BZCHK(hipMemcpyAsync(&count, h->count.p, sizeof count, hipMemcpyDeviceToHost, st));
        BZCHK(hipStreamSynchronize(st));
    }
    if (count > cap) return UP_E_INTERNAL;
    std::vector<uint64_t> bits(count);
    std::vector<uint8_t> kinds(count);
    if (count) {
        BZCHK(hipMemcpyAsync(bits.data(), h->bit.p, count * 8, hipMemcpyDeviceToHost, st));
        BZCHK(hipMemcpyAsync(kinds.data(), h->kind.p, count, hipMemcpyDeviceToHost, st));
        BZCHK(hipStreamSynchronize(st));
    }
    cands.resize(count);
    for (uint64_t i = 0; i < count; ++i) cands[i] = {bits[i], kinds[i]};
    std::sort(cands.begin(), cands.end(), [](const upk::BzCand &a, const upk::BzCand &b) { return a.bit < b.bit; });
    return UP_OK;
}

}  // namespace

extern "C" {

int up_bz_open(int device, up_bz **out) {
    if (!out) return UP_E_ARG;
    *out = nullptr;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd < 1) return UP_E_NODEV;
    if (device < 0 || device >= nd) return UP_E_ARG;
    up_bz *h = new up_bz;
    h->dev = device;
    if (const char *e = std::getenv("UNIPEAK_BZ_STARTS"))  // measurements: one start against many
        h->n_starts = (uint32_t)std::min<long>(std::max<long>(std::atol(e), 1), kMaxStarts);
    auto fail = [&](int code) {
        up_bz_close(h);
        return code;
    };
    if (hipSetDevice(device) != hipSuccess) return fail(UP_E_HIP);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail(UP_E_HIP);
    for (auto &e : h->ev)
        if (hipEventCreate(&e) != hipSuccess) return fail(UP_E_HIP);
    *out = h;
    return UP_OK;
}

void up_bz_close(up_bz *h) {
    if (!h) return;
    (void)hipSetDevice(h->dev);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
}

int up_bz_scan(up_bz *h, const void *src, uint64_t n, uint64_t *bit_off, uint8_t *kind, uint64_t cap,
               uint64_t *n_cand) {
    if (!h || !n_cand || (n && !src) || (cap && (!bit_off || !kind))) return UP_E_ARG;
    BZCHK(hipSetDevice(h->dev));
    std::vector<upk::BzCand> cands;
    const int rc = scan_file(h, src, n, cands);
    if (rc != UP_OK) return rc;
    *n_cand = cands.size();
    for (uint64_t i = 0; i < cands.size() && i < cap; ++i) {
        bit_off[i] = cands[i].bit;
        kind[i] = cands[i].kind;
    }
    return UP_OK;
}

int up_bz_decode(up_bz *h, const void *src, uint64_t n, const void **out, uint64_t *n_out, up_bz_info_t *info) {
    up_bz_info_t local;
    if (!info) info = &local;
    *info = up_bz_info_t{0, 0, 0, UP_BZ_OK, 0};
    if (!h || !out || !n_out || (n && !src)) return UP_E_ARG;
    *out = nullptr;
    *n_out = 0;
    BZCHK(hipSetDevice(h->dev));
    hipStream_t st = h->stream;
    StageTimer tm{h};
    const uint8_t *s8 = (const uint8_t *)src;

    std::vector<upk::BzCand> cands;
    int rc = scan_file(h, src, n, cands);
    if (rc != UP_OK) return rc;

    // stage 2: every block candidate's entropy stage
    std::vector<uint32_t> slot_of(cands.size(), 0);
    std::vector<uint64_t> bbit;
    for (size_t i = 0; i < cands.size(); ++i)
        if (cands[i].kind == 0) {
            slot_of[i] = (uint32_t)bbit.size();
            bbit.push_back(cands[i].bit);
        }
    const size_t n_bc = bbit.size();
    std::vector<upk::BzRec> recs(cands.size(), upk::BzRec{0, 0, 0, 0, UP_BZ_OK});
    if (n_bc) {
        BZCHK(h->slots.ensure_exact(n_bc * (uint64_t)kSlot));
        BZCHK(h->hists.ensure_exact(n_bc * 256));
        BZCHK(h->recs.ensure_exact(n_bc));
        BZCHK(hipMemcpyAsync(h->bit.p, bbit.data(), n_bc * 8, hipMemcpyHostToDevice, st));  // n_bc <= the scan's cap
        BZCHK(tm.begin());
        hipLaunchKernelGGL(bz_entropy, dim3((uint32_t)n_bc), dim3(64), 0, st, h->src.p, n, h->bit.p, h->slots.p,
                           h->hists.p, h->recs.p);
        BZCHK(hipGetLastError());
        BZCHK(tm.end(1));
        std::vector<upk::BzRec> got(n_bc);
        BZCHK(hipMemcpyAsync(got.data(), h->recs.p, n_bc * sizeof(upk::BzRec), hipMemcpyDeviceToHost, st));
        BZCHK(hipStreamSynchronize(st));
        for (size_t i = 0; i < cands.size(); ++i)
            if (cands[i].kind == 0) recs[i] = got[slot_of[i]];
    }

    // stage 3: the chain
    upk::BzChain chain;
    if (upk::bz_chain(s8, n, cands, recs, chain, *info) != UP_BZ_OK) return UP_E_ARG;
    const uint32_t nb = (uint32_t)chain.blocks.size();
    std::vector<uint32_t> blk_slot(nb);
    for (uint32_t b = 0; b < nb; ++b) blk_slot[b] = slot_of[chain.blocks[b].cand];

    std::vector<uint64_t> sizes(nb), off(nb + 1, 0);
    std::vector<uint32_t> crcs(nb);
    if (nb) {
        // stage 4: inverse BWT in batches
        const uint32_t batch = std::min(nb, kBatch), S = h->n_starts;
        BZCHK(h->blk_slot.ensure_exact(nb));
        BZCHK(h->words.ensure_exact((uint64_t)batch * kSlot));
        BZCHK(h->seg_len.ensure_exact((uint64_t)batch * (kMaxStarts + 1)));
        BZCHK(h->seg_next.ensure_exact((uint64_t)batch * (kMaxStarts + 1)));
        BZCHK(h->seg_off.ensure_exact((uint64_t)batch * (kMaxStarts + 1)));
        BZCHK(h->serial.ensure_exact(batch));
        BZCHK(hipMemcpyAsync(h->blk_slot.p, blk_slot.data(), nb * 4, hipMemcpyHostToDevice, st));
        for (uint32_t first = 0; first < nb; first += batch) {
            const uint32_t k = std::min(batch, nb - first);
            const dim3 wgrid((S + 1 + 255) / 256, k);
            BZCHK(tm.begin());
            hipLaunchKernelGGL(bz_rank, dim3(k), dim3(64), 0, st, h->slots.p, h->hists.p, h->recs.p, h->blk_slot.p,
                               first, h->words.p, S);
            BZCHK(hipGetLastError());
            BZCHK(tm.end(2));
            BZCHK(tm.begin());
            hipLaunchKernelGGL(HIP_KERNEL_NAME(bz_walk<0>), wgrid, dim3(256), 0, st, h->recs.p, h->blk_slot.p, first,
                               h->words.p, S, h->seg_len.p, h->seg_next.p, h->seg_off.p, h->serial.p, h->slots.p);
            hipLaunchKernelGGL(bz_order, dim3(k), dim3(256), 0, st, h->recs.p, h->blk_slot.p, first, S,
                               h->seg_len.p, h->seg_next.p, h->seg_off.p, h->serial.p);
            hipLaunchKernelGGL(HIP_KERNEL_NAME(bz_walk<1>), wgrid, dim3(256), 0, st, h->recs.p, h->blk_slot.p, first,
                               h->words.p, S, h->seg_len.p, h->seg_next.p, h->seg_off.p, h->serial.p, h->slots.p);
            BZCHK(hipGetLastError());
            BZCHK(tm.end(3));
        }
        // stage 5: sizes, the prefix sum, then the bytes and the CRCs
        BZCHK(h->sizes.ensure_exact(nb));
        BZCHK(h->off.ensure_exact(nb + 1));
        BZCHK(h->crcs.ensure_exact(nb));
        BZCHK(tm.begin());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(bz_rle<0>), dim3(nb), dim3(64), 0, st, h->recs.p, h->blk_slot.p,
                           h->slots.p, h->sizes.p, h->off.p, h->out.p, h->crcs.p);
        BZCHK(hipGetLastError());
        BZCHK(tm.end(4));
        BZCHK(hipMemcpyAsync(sizes.data(), h->sizes.p, nb * 8, hipMemcpyDeviceToHost, st));
        BZCHK(hipStreamSynchronize(st));
        for (uint32_t b = 0; b < nb; ++b) {
            if (sizes[b] > 52ull * upk::kBzMaxCap) return UP_E_INTERNAL;  // 255 / 5 of the capacity, at most
            off[b + 1] = off[b] + sizes[b];
        }
        BZCHK(h->out.ensure_exact(off[nb] + 16));
        BZCHK(hipMemcpyAsync(h->off.p, off.data(), (nb + 1) * 8, hipMemcpyHostToDevice, st));
        BZCHK(tm.begin());
        hipLaunchKernelGGL(HIP_KERNEL_NAME(bz_rle<1>), dim3(nb), dim3(64), 0, st, h->recs.p, h->blk_slot.p,
                           h->slots.p, h->sizes.p, h->off.p, h->out.p, h->crcs.p);
        BZCHK(hipGetLastError());
        BZCHK(tm.end(4));
        BZCHK(hipMemcpyAsync(crcs.data(), h->crcs.p, nb * 4, hipMemcpyDeviceToHost, st));
        BZCHK(hipStreamSynchronize(st));
    }
    if (upk::bz_check_crcs(chain, cands, recs, crcs.data(), *info) != UP_BZ_OK) return UP_E_ARG;
    const uint64_t total = off[nb];
    BZCHK(h->h_out.ensure(total + 16));
    if (total) {
        BZCHK(hipMemcpyAsync(h->h_out.p, h->out.p, total, hipMemcpyDeviceToHost, st));
        BZCHK(hipStreamSynchronize(st));
    }
    h->bytes_in += n;
    h->bytes_out += total;
    h->calls++;
    *out = h->h_out.p;
    *n_out = total;
    return UP_OK;
}

int up_bz_timings(up_bz *h, double *v, int n) {
    if (!h || !v || n < 0) return UP_E_ARG;
    for (int k = 0; k < n && k < 5; ++k) v[k] = h->ms[k];
    if (n > 5) v[5] = (double)h->bytes_in;
    if (n > 6) v[6] = (double)h->bytes_out;
    if (n > 7) v[7] = (double)h->calls;
    return UP_OK;
}

int up_bz_decode_host(const void *src, uint64_t n, void *dst, uint64_t cap, uint64_t *n_out, up_bz_info_t *info) {
    return upk::bz_decode_host_capi(src, n, dst, cap, n_out, info);
}

const char *up_bz_reason(int reason) { return upk::bz_reason_text(reason); }

}  // extern "C"
