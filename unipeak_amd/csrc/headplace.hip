// unipeak_amd/csrc/headplace.hip -- quirk-Q1 head units finished on the
// device, inside the pass (up_set_head_place).  #included by api.hip.
//
// A pass with head units (pooled tags at positions <= bw, emulate.hip) has two
// record lists: K3's, one record per region of the parallel scan in K2's
// order (unit-major, left-ascending), and K0's, the exact replay of every
// head chain up to its resync position.  The reference's list is, per unit,
// K0's records in emission order and then K3's records that start at or after
// the unit's resync position (resync 0: the unit was not replayed, all of
// them; 0xFFFFFFFF: replayed to its end, none).  With the mode on K3 writes to
// a device stage of the pass slot, K0 runs on the pass's stream into areas of
// the slot, and two kernels build the merged list where the pass delivers:
//
//   head_table_kernel    one block: per unit its range of staged records
//                        (binary search of K2's unit column), the kept suffix
//                        (lower bound of the resync position over the staged
//                        records' left ends), its K0 record count and its
//                        output offset (block scans with a carry over chunks
//                        of units); the total goes to the status words and to
//                        a record target's header, the resync positions to
//                        pinned host memory (up_unit_replay_profile)
//   head_scatter_kernel  eight threads per record (seven 8-byte words and
//                        the exptSums): stage / K0 area -> destination, plus
//                        per final record what
//                        up_shift_scan needs (stored start, end, unit and the
//                        offset of a replayed record's scores in the slot's
//                        score slab, kHeadNoScores for a K1-K3 record)
//
// A K0 capacity error (EmuParams::err bits 1, 2, 8: an open region longer
// than reg_cap, more than out_cap records, a full score slab) or a contract
// violation (4) makes both kernels pass the staged records through unchanged;
// the host then finishes that pass as it does with the mode off.

namespace upk {

constexpr uint64_t kHeadNoScores = ~0ull;  // HeadLists::soff of a K1-K3 record
constexpr uint32_t kHeadK0Bad = 1u | 2u | 4u | 8u;
constexpr uint32_t kHeadRecWords = sizeof(up_region) / 8;  // 7
static_assert(sizeof(up_region) == 56, "head_scatter_kernel copies seven words per record");

// status words of a placed pass (hp_status[slot]; [0..2] are K2b's, [3] q11place's)
constexpr int kHeadStTotal = 4;  // merged record count + 1
constexpr int kHeadStErr = 5;    // K0's error word
constexpr int kHeadStK0 = 6;     // K0's record count (may exceed its capacity)

// per unit, where its records go
struct HeadPlace {
    uint64_t first;  // the unit's first staged record
    uint64_t keep;   // its first kept staged record
    uint64_t base;   // destination of its first record
    uint32_t k0n;    // K0 records placed first
    uint32_t pad;
};

// K0's outputs of one pass slot
struct HeadK0 {
    const up_region *out;
    const uint32_t *counts;     // [out_cap][S]
    const uint32_t *rank;       // [out_cap]: emission index within the record's unit
    const uint64_t *score_off;  // [out_cap]
    const uint32_t *ctr;        // [0] records emitted, [1] the error word
    const uint32_t *resync;     // [nu]
    const uint32_t *unit_n;     // [nu]: records emitted per unit
    uint32_t out_cap;
};

// per final record (up_shift_scan / up_shift_best)
struct HeadLists {
    uint32_t *start, *end, *unit;
    uint64_t *soff;
};

// layout-time head flags (the pass's own d_head is K2a's): quirk Q1 per unit
template <int POOL>
__global__ void __launch_bounds__(256) head_flags_kernel(const UnitDesc *units, int S, int nnc, const int32_t *nc,
                                                         const double *coef, int bw, uint32_t *head) {
    head_detect_unit<POOL>(units, blockIdx.x, S, nnc, nc, coef, bw, head, nullptr);
}

// first staged record of [lo, hi) whose left end is >= v
__device__ __forceinline__ uint64_t head_lb_left(const up_region *stage, uint64_t lo, uint64_t hi, uint32_t v) {
    while (lo < hi) {
        const uint64_t m = (lo + hi) >> 1;
        if (stage[m].left < v) lo = m + 1;
        else hi = m;
    }
    return lo;
}

__global__ void __launch_bounds__(1024) head_table_kernel(uint32_t nu, const uint32_t *__restrict__ runit,
                                                          const up_region *__restrict__ stage,
                                                          const uint64_t *__restrict__ nreg_p, HeadK0 K,
                                                          HeadPlace *tab, uint32_t *resync_host,
                                                          unsigned long long *status,
                                                          unsigned long long *target_hdr, uint64_t dest_cap) {
    __shared__ uint64_t sh64[16];
    __shared__ uint64_t chunk_tot;
    const uint64_t nreg = *nreg_p;
    const uint32_t t = threadIdx.x;
    const uint32_t err = K.ctr[1];
    const bool bad = (err & kHeadK0Bad) != 0u || K.ctr[0] > K.out_cap;
    const uint32_t nchunks = (nu + 1023) / 1024;
    uint64_t base = 0;
    for (uint32_t ch = 0; ch < nchunks; ++ch) {
        const uint32_t u = ch * 1024 + t;
        uint64_t cnt = 0;
        HeadPlace T{};
        if (u < nu) {
            const uint64_t f = lb_u32(runit, 0, nreg, u);
            const uint64_t e = lb_u32(runit, f, nreg, u + 1);
            const uint32_t x = bad ? 0u : K.resync[u];
            T.first = f;
            T.keep = x == 0u ? f : x == 0xFFFFFFFFu ? e : head_lb_left(stage, f, e, x);
            T.k0n = bad ? 0u : K.unit_n[u];
            cnt = (uint64_t)T.k0n + (e - T.keep);
            resync_host[u] = K.resync[u];
        }
        const uint64_t inc = block_incl_sum(cnt, sh64);
        if (u < nu) {
            T.base = base + inc - cnt;
            tab[u] = T;
        }
        if (t == 1023) chunk_tot = inc;
        __syncthreads();
        base += chunk_tot;
        __syncthreads();
    }
    if (t == 0) {
        status[kHeadStTotal] = base + 1;
        status[kHeadStErr] = err | (K.ctr[0] > K.out_cap ? 2u : 0u);
        status[kHeadStK0] = K.ctr[0];
        if (target_hdr) *target_hdr = base <= dest_cap ? base : 0;
    }
}

// work item = (record, lane of eight): records [0, nreg) are the staged ones,
// [nreg, nreg + K0's count) the replayed ones.  A up_region is 56 bytes, 8-byte
// aligned (seven words, as K3 writes it), so it moves as seven 8-byte words on
// consecutive lanes; 16-byte vectors would straddle records.
__global__ void __launch_bounds__(256) head_scatter_kernel(const up_region *__restrict__ stage,
                                                           const uint32_t *__restrict__ stage_counts,
                                                           const uint64_t *__restrict__ nreg_p, int S, HeadK0 K,
                                                           const HeadPlace *__restrict__ tab, uint32_t nu,
                                                           up_region *out, uint32_t *out_counts,
                                                           uint64_t dest_cap, HeadLists Lst) {
    const uint64_t nreg = *nreg_p;
    const bool bad = (K.ctr[1] & kHeadK0Bad) != 0u || K.ctr[0] > K.out_cap;
    const uint64_t nk0 = bad ? 0u : K.ctr[0];
    const uint64_t items = (nreg + nk0) * 8;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < items;
         w += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = w >> 3;
        const uint32_t q = (uint32_t)(w & 7u);
        const bool rep = i >= nreg;
        const uint64_t k = rep ? i - nreg : i;
        const up_region *src = rep ? K.out + k : stage + k;
        const uint32_t u = src->unit;
        if (u >= nu) continue;  // (cannot happen: both lists name units of this context)
        const HeadPlace T = tab[u];
        uint64_t d;
        if (rep) {
            const uint32_t r = K.rank[k];
            if (r >= T.k0n) continue;
            d = T.base + r;
        } else {
            if (k < T.keep) continue;  // K0's records cover it
            d = T.base + T.k0n + (k - T.keep);
        }
        if (d >= dest_cap) continue;  // the host grows the area and reruns
        if (q < kHeadRecWords) {
            ((uint64_t *)(out + d))[q] = ((const uint64_t *)src)[q];
        } else {  // the eighth lane: exptSums and the up_shift_scan columns
            const uint32_t *srcc = rep ? K.counts + k * (uint64_t)S : stage_counts + k * (uint64_t)S;
            for (int s = 0; s < S; ++s) out_counts[d * (uint64_t)S + s] = srcc[s];
            Lst.unit[d] = u;
            Lst.start[d] = src->left;
            Lst.end[d] = src->right;
            Lst.soff[d] = rep ? K.score_off[k] : kHeadNoScores;
        }
    }
}

}  // namespace upk
