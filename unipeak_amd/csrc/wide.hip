// unipeak_amd/csrc/wide.hip -- K1w: the scan for kernels wider than K1's
// register-resident halo (bw > kMaxBw = 511, up to kMaxWideBw = 32,767: a
// window of at most 65,535 cells -- beyond it the reference's UShort
// retirement count wraps, misc/peakcall.cpp:172-177, and the whole-buffer
// replay runs instead; the reference's -b itself is a UShort,
// misc/kernel.hpp:16).  #included by api.hip.
//
// One wave per strip (16,384 positions), units with a threshold > 0, as K1
// (screen + exact) in one kernel:
//  * screen: the strip's window of chunk sums of its screen plane (the one
//    pooled track's plane, or the unit's weighted pooled plane -- always the
//    pooled plane for a nondirectional unit: it sums both strands; a saturated
//    255 counts as unbounded) as prefix sums in LDS; a 64-position word can
//    hold a flag only if the weighted tag sum over the union of its
//    positions' windows, [x0 - bw, x0 + 63 + bw], exceeds the budget wskip
//    (the same bound K1a uses; it bounds forwardScore + reverseScore as well);
//  * exact: for each such word every lane sums its position's score over the
//    adds of that window in ascending position -- the order the reference's
//    deque cell receives them (peakcall.cpp:186-209) -- as kern[x - a + bw] *
//    countSum in FP64 (the pooled count words come from load_words, so
//    pooled samples, coefficients and the pooled count track behave as in
//    K1b); a nondirectional unit (NONDIR) keeps one such sum per strand and
//    flags forwardScore + reverseScore (peakcall.cpp:57, 207-209);
//  * runs, peaks (first maximum) and the strip's record list and edge flags
//    exactly as K1b writes them, so K2 and K3 (known peaks) follow unchanged.
// The tracks of every unit are padded past len + 2bw (unit_stride), so the
// window loads of positions up to len + bw stay in bounds.
//
// wide_stretch_scores (below): the dense FP64 scores of one strand over a
// stretch of 64 words, the same ascending sums; its users are
//  * wide_profile_kernel: the dense profile of a unit, one strand or both
//    (up_unit_profile*, -w);
//  * wide_corr_kernel: strandCorr(0) of every region of a nondirectional
//    pass, between K2 and K3 (K3's own KDE spans NH <= 8 window words);
//  * wide_fill_kernel: the (f, r) slabs of requested regions for K4
//    (up_shift_scan, up_shift_best);
//  * wide_peak_kernel: the peaks of wide K1q's regions -- a threshold <= 0,
//    whose runs wide_runs_kernel finds; on nondirectional units
//    (up_set_wide_q11_nd) the peaks of forwardScore + reverseScore;
//  * wide_corr_stage_kernel: both strands' scores of the long regions of such
//    a nondirectional pass, which wide_corr_chain_kernel sums in position
//    order (end of this file).

namespace upk {

constexpr uint32_t kWideSat = 1u << 18;  // a saturated chunk in the prefix sums
constexpr int kWideChunks = (kStrip + 2 * kMaxWideBw + 64) / 16 + 4;  // 5,127: the widest strip window

// the score of position x0 + lane on one strand: the adds of [x0 - bw,
// x0 + 63 + bw] in ascending position, the window reloaded word by word
// (K1w's exact walk and the dense scores' fallback)
template <int POOL>
__device__ __forceinline__ double wide_word_score(const ScanParams &P, const UnitDesc &U, int S, int strand, int bw,
                                                  int64_t x0, int lane) {
    const int64_t x = x0 + lane;
    double f = 0.0;
    const int64_t wb0 = ((x0 - bw - 1) >> 6) * 64 + 1;  // 64-aligned word start (position)
    for (int64_t wb = wb0; wb <= x0 + 63 + bw; wb += 64) {
        if (wb + 63 < 1 || wb > (int64_t)U.len) continue;  // no adds outside 1 .. len
        WinT<POOL> cs[1];
        load_words<1, POOL>(cs, U, S, strand, wb, lane, P.nnc, P.nc, P.coef);
        uint64_t m = __ballot(nz(cs[0]) && wb + lane >= 1 && wb + lane <= (int64_t)U.len);
        while (m) {
            const int k = __builtin_ctzll(m);
            m &= m - 1;
            const int64_t a = wb + k;
            const double cnt = rl_cs(cs[0], k);
            const int64_t d = x - a;
            if (d >= -bw && d <= bw) f = f + P.kern[d + bw] * cnt;
        }
    }
    return f;
}

// prefix sums of the chunk sums c0 .. c0 + nch - 1 of plane pl (chunks outside
// the track count 0, a saturated one kWideSat) into pre[0 .. nch]; the block
// is one wave
__device__ __forceinline__ void wide_prefix(gu8 *pl, int64_t nchunk_track, int64_t c0, int nch, uint32_t *pre,
                                            int lane) {
    __syncthreads();  // the previous window's readers are done
    if (lane == 0) pre[0] = 0u;
    uint32_t carry = 0;
    for (int base = 0; base < nch; base += 64) {
        const int i = base + lane;
        const int64_t c = c0 + i;
        uint32_t v = 0;
        if (i < nch && c >= 0 && c < nchunk_track) {
            v = pl[c];
            v = v == 255u ? kWideSat : v;
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)v, o);
            if (lane >= o) v += y;
        }
        if (i < nch) pre[i + 1] = carry + v;
        carry += (uint32_t)__shfl((int)v, 63);
    }
    __syncthreads();
}

template <int POOL, bool NONDIR>
__global__ void __launch_bounds__(64) wide_kernel(ScanParams P) {
    __shared__ uint32_t pre[kWideChunks + 1];
    const int lane = threadIdx.x;
    const int bw = P.bw;
    const int S = P.S;
    for (uint32_t strip = blockIdx.x; strip < P.nstrips; strip += gridDim.x) {
        const uint32_t u = find_unit(P.units, P.nunits, strip);
        const UnitDesc U = P.units[u];
        const uint32_t local = strip - U.strip0;
        const int64_t p0 = 1 + (int64_t)local * kStrip, pend = p0 + kStrip - 1;
        const int64_t dom_end = (int64_t)U.len + bw;  // the last position a flush retires
        // ---- screen: prefix sums of the window's chunk sums ----
        gu8 *pl = (POOL == 0 && !NONDIR) ? plane_u8(U, S, 0, P.nc[0]) : pooled_u8(U, S);
        const int64_t nchunk_track = (int64_t)(U.stride / 4);
        const int64_t c0 = (kPadPos + (p0 - bw) - 1) >> 4;  // (arithmetic shift: floor)
        const int64_t c1 = (kPadPos + (pend + bw) - 1) >> 4;
        const int nch = (int)(c1 - c0 + 1);
        wide_prefix(pl, nchunk_track, c0, nch, pre, lane);
        // candidate words: lane l decides words l, l + 64, l + 128, l + 192
        uint64_t cand[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t x0 = p0 + 64 * (64 * q + lane);
            const int64_t lo = ((kPadPos + x0 - bw - 1) >> 4) - c0, hi = ((kPadPos + x0 + 63 + bw - 1) >> 4) - c0;
            const uint32_t sum = pre[hi + 1] - pre[lo];
            cand[q] = __ballot(x0 <= dom_end && (sum > P.wskip || sum >= kWideSat));
        }
        // ---- exact scores, runs and records (K1b's record protocol) ----
        RecList R_{0, 0, kInline};
        uint64_t F0 = 0;
        bool open = false, pk_ok = false;
        double best = -__builtin_inf();
        uint32_t bpos = 0;
        auto close_run = [&](uint32_t end_pos) {
            rec_end(R_, end_pos, pk_ok ? bpos : 0u, best, P, strip, lane);
            if (!pk_ok && lane == 0) {  // the run open at p0: its part in this strip
                P.spk[4ull * strip] = (uint64_t)__double_as_longlong(best);
                P.spk[4ull * strip + 1] = bpos;
            }
            open = false;
        };
        for (int g = 0; g < kStripWords; ++g) {
            const int64_t x0 = p0 + 64 * g;
            const bool cw = (cand[g >> 6] >> (g & 63)) & 1;
            if (!cw) {
                if (open) close_run((uint32_t)(x0 - 1));
                continue;
            }
            const int64_t x = x0 + lane;
            double f = wide_word_score<POOL>(P, U, S, 0, bw, x0, lane);
            if constexpr (NONDIR) {  // forwardScore + reverseScore, each its own ascending sum
                const double r = wide_word_score<POOL>(P, U, S, 1, bw, x0, lane);
                f = f + r;
            }
            const bool flag = x <= dom_end && f >= P.thr;
            const uint64_t F = __ballot(flag);
            if (g == 0) F0 = F;
            if (open && !(F & 1ull)) close_run((uint32_t)(x0 - 1));
            // no interior start at p0 (K2 joins it to the previous strip's run)
            uint64_t st = F & ~((F << 1) | ((open || g == 0) ? 1ull : 0ull));
            while (st) {
                const int b = __builtin_ctzll(st);
                st &= st - 1;
                rec_start(R_, (uint32_t)(x0 + b), P, strip, lane);
            }
            // each maximal segment of F: its largest score and the first
            // position holding it (Region::addPos keeps the first maximum)
            uint64_t rem = F;
            while (rem) {
                const int a = __builtin_ctzll(rem);
                const uint64_t t = rem >> a;
                const int len = ~t == 0ull ? 64 - a : __builtin_ctzll(~t);
                const uint64_t seg = (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << a;
                rem &= ~seg;
                const bool in = (seg >> lane) & 1ull;
                const double m = wave_max_d(in ? f : -__builtin_inf());
                const uint64_t at = __ballot(in && f == m);
                const uint32_t pp = (uint32_t)(x0 + __builtin_ctzll(at));
                if (!(a == 0 && open)) {  // a new run
                    best = m;
                    bpos = pp;
                    pk_ok = g != 0 || a != 0;  // one at p0 may continue the previous strip
                } else if (m > best) {
                    best = m;
                    bpos = pp;
                }
                open = true;
                if (a + len < 64) close_run((uint32_t)(x0 + a + len - 1));
            }
        }
        if (open && lane == 0) {  // the run open at the strip's last position: its part here
            P.spk[4ull * strip + 2] = (uint64_t)__double_as_longlong(best);
            P.spk[4ull * strip + 3] = bpos;
        }
        const uint64_t info = (uint64_t)R_.ns | ((uint64_t)R_.ne << 16) | ((F0 & 1ull) << 32) |
                              ((uint64_t)open << 33) | ((uint64_t)(local == 0) << 34) |
                              ((uint64_t)(local + 1 == U.nstrips) << 35) | ((uint64_t)(R_.slot != kInline) << 36);
        if (lane == 0) P.strip_info[strip] = info;
    }
}

// ---- dense scores of a wide kernel: one strand over a stretch of words ----
// A stretch is up to kProfWords words of 64 positions from x_lo (64-aligned
// + 1), owned by one wave (the block):
//  * screen (wide_stretch_screen): K1w's prefix sums of the stretch window's
//    chunk sums; a word whose union window holds no tag at all (a saturated
//    chunk counts as tags) scores 0.0 -- "no tags", not wskip: the dense
//    scores need every nonzero one.  The pooled plane of a nondirectional
//    unit holds both strands' tags, so one screen serves both strands;
//  * gather: nearly every word is live, so the window is not reloaded per
//    word -- the strand's hits (position, pooled count as FP64) of the live
//    words' windows are listed once, ascending, in LDS (load words whose
//    four chunks are empty are not loaded at all);
//  * walk: every live word adds the list's sub-range [x0 - bw, x0 + 63 + bw]
//    (two cursors that only move forward), one multiply and one add per hit
//    and lane, in list order = ascending position;
//  * a stretch whose windows hold more than `cap` (<= kProfHits) hits of the
//    strand walks every live word with wide_word_score instead (cap 0:
//    always) -- the same adds in the same order, so the same bits.
constexpr int kProfWords = 64;  // one ballot of live words per stretch
constexpr int kProfHits = 512;  // list entries per wave and strand (12 bytes each)
__host__ __device__ constexpr int prof_chunks(int bw) { return (kProfWords * 64 + 2 * bw) / 16 + 3; }
__host__ __device__ constexpr size_t prof_lds_bytes(int bw) {
    return (size_t)kProfHits * 12 + (((size_t)prof_chunks(bw) + 1) * 4 + 15) / 16 * 16;
}

__device__ __forceinline__ int64_t i64min(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t i64max(int64_t a, int64_t b) { return a > b ? a : b; }

// chunks [a, b] (relative to the window's first chunk, clipped to it) hold a tag
__device__ __forceinline__ bool wide_tags(const uint32_t *pre, int nch, int64_t a, int64_t b) {
    a = a < 0 ? 0 : a;
    b = b > nch - 1 ? nch - 1 : b;
    return a <= b && pre[b + 1] != pre[a];
}

struct WideScreen {
    int64_t c0;     // the window's first chunk
    int nch;        // its chunks (pre[0 .. nch])
    uint64_t cand;  // the stretch's live words
};

__device__ __forceinline__ WideScreen wide_stretch_screen(gu8 *pl, int64_t nchunk_track, int bw, int64_t x_lo,
                                                          int nw, uint32_t *pre, int lane) {
    WideScreen W;
    const int64_t x_hi = x_lo + 64 * nw - 1;
    W.c0 = (kPadPos + (x_lo - bw) - 1) >> 4;  // (arithmetic shift: floor)
    const int64_t c1 = (kPadPos + (x_hi + bw) - 1) >> 4;
    W.nch = (int)i64min(c1 - W.c0 + 1, prof_chunks(bw));  // (c1 - c0 + 1 never exceeds it)
    wide_prefix(pl, nchunk_track, W.c0, W.nch, pre, lane);
    bool live = false;  // lane l decides word l
    if (lane < nw) {
        const int64_t x0 = x_lo + 64 * lane;
        live = wide_tags(pre, W.nch, ((kPadPos + x0 - bw - 1) >> 4) - W.c0, ((kPadPos + x0 + 63 + bw - 1) >> 4) - W.c0);
    }
    W.cand = __ballot(live);
    return W;
}

// store(x, f) for position x = x0 + lane of every live word of the stretch
// (ALL: of its other words too, with 0.0); hcnt / hpos: this strand's list
template <int POOL, bool ALL, class Store>
__device__ __forceinline__ void wide_stretch_scores(const ScanParams &P, const UnitDesc &U, int S, int strand, int bw,
                                                    int64_t x_lo, int nw, const WideScreen &W, const uint32_t *pre,
                                                    uint32_t cap, double *hcnt, uint32_t *hpos, int lane,
                                                    Store store) {
    const uint64_t cand = W.cand;
    const uint64_t below = lane == 0 ? 0ull : ~0ull >> (64 - lane);  // the lanes before this one
    // ---- gather: the hits of the live words' windows, ascending ----
    uint32_t nh = 0;
    bool listed = cap != 0 && cand != 0;
    if (cand) {
        const int64_t glo = i64max(1, x_lo + 64 * (int64_t)__builtin_ctzll(cand) - bw);
        const int64_t ghi = i64min((int64_t)U.len, x_lo + 64 * (int64_t)(63 - __builtin_clzll(cand)) + 63 + bw);
        for (int64_t wb = ((glo - 1) >> 6) * 64 + 1; listed && wb <= ghi; wb += 64 * 64) {
            const int64_t wl = wb + 64 * lane;  // lane l decides load word l of this batch
            const int64_t ci = ((kPadPos + wl - 1) >> 4) - W.c0;
            uint64_t mw = __ballot(wl <= ghi && wide_tags(pre, W.nch, ci, ci + 3));
            while (mw) {
                const int k = __builtin_ctzll(mw);
                mw &= mw - 1;
                const int64_t wk = wb + 64 * k;
                WinT<POOL> cs[1];
                load_words<1, POOL>(cs, U, S, strand, wk, lane, P.nnc, P.nc, P.coef);
                const bool hit = nz(cs[0]) && wk + lane >= glo && wk + lane <= ghi;
                const uint64_t hm = __ballot(hit);
                const uint32_t n = (uint32_t)__builtin_popcountll(hm);
                if (nh + n > cap) {
                    listed = false;
                    break;
                }
                if (hit) {
                    const uint32_t i = nh + (uint32_t)__builtin_popcountll(hm & below);
                    hpos[i] = (uint32_t)(wk + lane);
                    hcnt[i] = (double)cs[0];
                }
                nh += n;
            }
        }
    }
    __syncthreads();
    // ---- walk ----
    uint32_t li = 0, ui = 0;  // the list's sub-range of the current word: [li, ui)
    for (int g = 0; g < nw; ++g) {
        const int64_t x0 = x_lo + 64 * g, x = x0 + lane;
        if (!((cand >> g) & 1ull)) {
            if constexpr (ALL) store(x, 0.0);
            continue;
        }
        double f;
        if (listed) {
            const int64_t a_lo = x0 - bw, a_hi = x0 + 63 + bw;
            for (;;) {  // (ascending list: the lanes that hold an earlier hit form a prefix)
                const uint32_t i = li + lane;
                const int n = __builtin_popcountll(__ballot(i < nh && (int64_t)hpos[i < nh ? i : 0] < a_lo));
                li += n;
                if (n < 64) break;
            }
            ui = ui < li ? li : ui;
            for (;;) {
                const uint32_t i = ui + lane;
                const int n = __builtin_popcountll(__ballot(i < nh && (int64_t)hpos[i < nh ? i : 0] <= a_hi));
                ui += n;
                if (n < 64) break;
            }
            f = 0.0;
#pragma unroll 4
            for (uint32_t i = li; i < ui; ++i) {
                const int64_t j = x - (int64_t)hpos[i] + bw;  // index of kern[x - a + bw]
                const bool in = j >= 0 && j <= 2 * (int64_t)bw;
                const double t = f + P.kern[in ? j : 0] * hcnt[i];
                f = in ? t : f;
            }
        } else {
            f = wide_word_score<POOL>(P, U, S, strand, bw, x0, lane);
        }
        store(x, f);
    }
}

// ---- the dense profile of a wide kernel (up_unit_profile*, bin/regions -w) ----
// FP64 scores of positions [prof_first, prof_first + prof_len) of unit
// prof_unit into the pre-zeroed prof_f (a directional unit: prof_r stays
// zero), each the ascending sum K1w forms.  One wave owns a stretch of
// kProfWords words.  Positions above len + bw are never written.
// NONDIR: forwardScore into prof_f and reverseScore into prof_r, separate
// ascending sums (the host adds them).  The screen is the unit's pooled plane,
// which holds both strands' tags -- a word is live if either strand has a tag
// in its union window -- and each strand takes its own gather and walk, one
// after the other through the same hit list (the LDS stays the directional
// kernel's), so one strand of a stretch may overflow the list and fall back to
// wide_word_score while the other does not; a live word without a hit on a
// strand stores the +0.0 its sum starts from.
template <int POOL, bool NONDIR>
__global__ void __launch_bounds__(64) wide_profile_kernel(ScanParams P, uint32_t cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char prof_lds[];
    double *hcnt = (double *)prof_lds;
    uint32_t *hpos = (uint32_t *)(prof_lds + (size_t)kProfHits * 8);
    uint32_t *pre = hpos + kProfHits;
    const int lane = threadIdx.x;
    const int bw = P.bw;
    const int S = P.S;
    const UnitDesc U = P.units[P.prof_unit];
    const int64_t dom_end = (int64_t)U.len + bw;  // the last position a flush retires
    const int64_t last = i64min(P.prof_first + (int64_t)P.prof_len - 1, dom_end);
    if (last < P.prof_first) return;
    const int64_t w_first = (P.prof_first - 1) >> 6, w_last = (last - 1) >> 6;  // words of 64 positions
    const int64_t nstretch = (w_last - w_first) / kProfWords + 1;
    gu8 *pl = (POOL == 0 && !NONDIR) ? plane_u8(U, S, 0, P.nc[0]) : pooled_u8(U, S);
    const int64_t nchunk_track = (int64_t)(U.stride / 4);
    for (int64_t s = blockIdx.x; s < nstretch; s += gridDim.x) {
        const int64_t w0 = w_first + s * kProfWords;
        const int nw = (int)i64min(kProfWords, w_last - w0 + 1);
        const int64_t x_lo = 1 + 64 * w0;
        const WideScreen W = wide_stretch_screen(pl, nchunk_track, bw, x_lo, nw, pre, lane);
        if (!W.cand) continue;
        wide_stretch_scores<POOL, false>(P, U, S, 0, bw, x_lo, nw, W, pre, cap, hcnt, hpos, lane,
                                         [&](int64_t x, double f) {
                                             const int64_t q = x - P.prof_first;
                                             if (q >= 0 && q < (int64_t)P.prof_len && x <= dom_end) P.prof_f[q] = f;
                                         });
        if constexpr (NONDIR) {
            __syncthreads();  // the forward walk has read the list the reverse gather refills
            wide_stretch_scores<POOL, false>(P, U, S, 1, bw, x_lo, nw, W, pre, cap, hcnt, hpos, lane,
                                             [&](int64_t x, double r) {
                                                 const int64_t q = x - P.prof_first;
                                                 if (q >= 0 && q < (int64_t)P.prof_len && x <= dom_end)
                                                     P.prof_r[q] = r;
                                             });
        }
    }
}

// ---- both strands' dense scores of a position range (nondirectional) ----
// LDS of wide_corr_kernel / wide_fill_kernel: a hit list per strand, the
// 64 x 3 products of the correlation's sequential sums, the prefix sums
constexpr int kCorrSlab = kProfWords * 64;  // positions of one wave's global (f, r) slab: a stretch
__host__ __device__ constexpr size_t corr_lds_bytes(int bw) {
    return 2 * (size_t)kProfHits * 12 + 64 * 3 * 8 + (((size_t)prof_chunks(bw) + 1) * 4 + 15) / 16 * 16;
}
struct WideLds {
    double *hcnt[2];
    double *prod;
    uint32_t *hpos[2];
    uint32_t *pre;
};
__device__ __forceinline__ WideLds wide_lds(unsigned char *lds) {
    WideLds L;
    L.hcnt[0] = (double *)lds;
    L.hcnt[1] = L.hcnt[0] + kProfHits;
    L.prod = L.hcnt[1] + kProfHits;
    L.hpos[0] = (uint32_t *)(L.prod + 64 * 3);
    L.hpos[1] = L.hpos[0] + kProfHits;
    L.pre = L.hpos[1] + kProfHits;
    return L;
}

// forwardScore and reverseScore of positions a .. b (1 <= a <= b) of unit U ->
// of[x - a], orr[x - a]: every position is written, each score the ascending
// sum the reference's Region::scores holds; block-wide visible on return
template <int POOL>
__device__ __forceinline__ void wide_range_scores(const ScanParams &P, const UnitDesc &U, int S, int bw, int64_t a,
                                                  int64_t b, double *of, double *orr, const WideLds &L, uint32_t cap,
                                                  int lane) {
    gu8 *pl = pooled_u8(U, S);
    const int64_t nchunk_track = (int64_t)(U.stride / 4);
    const int64_t w_first = (a - 1) >> 6, w_last = (b - 1) >> 6;
    for (int64_t w0 = w_first; w0 <= w_last; w0 += kProfWords) {
        const int nw = (int)i64min(kProfWords, w_last - w0 + 1);
        const int64_t x_lo = 1 + 64 * w0;
        const WideScreen W = wide_stretch_screen(pl, nchunk_track, bw, x_lo, nw, L.pre, lane);
        wide_stretch_scores<POOL, true>(P, U, S, 0, bw, x_lo, nw, W, L.pre, cap, L.hcnt[0], L.hpos[0], lane,
                                        [&](int64_t x, double f) {
                                            if (x >= a && x <= b) of[x - a] = f;
                                        });
        wide_stretch_scores<POOL, true>(P, U, S, 1, bw, x_lo, nw, W, L.pre, cap, L.hcnt[1], L.hpos[1], lane,
                                        [&](int64_t x, double r) {
                                            if (x >= a && x <= b) orr[x - a] = r;
                                        });
    }
    __syncthreads();  // (global slab writes: visible to the wave's other lanes)
}

// ---- strandCorr(0) of every region of a wide nondirectional pass ----
// Between K2 and K3, one wave per region [left, right] of starts / ends:
// Region::strandCorr(0) (misc/data.cpp:38-58, 184-193) over the dense f and r
// with exactly the arithmetic of K3's pass 3 -- sequential sums for the two
// means, then sequential sums of d1*d1, d2*d2 and d1*d2, sqrt(ss / (n - 1)),
// NaN for n <= 3 -- one double per region into `out`; K3 then takes it
// (StatParams::corr_in) instead of running its own KDE.
// Memory: one slab of kCorrSlab (f, r) positions per wave, whatever the
// regions hold; a region that fits keeps its scores for the second pass, a
// longer one forms them again slab by slab (the same sums, so the same bits).
// Regions of more than long_n stored positions are left out (behind wide K1q
// the stage and chain kernels at the end of this file take them; K1w passes
// ~0: every region).
template <int POOL>
__global__ void __launch_bounds__(64) wide_corr_kernel(ScanParams P, const uint32_t *starts, const uint32_t *ends,
                                                       const uint32_t *reg_unit, const uint64_t *nreg_p,
                                                       uint64_t reg_cap, double *slabs, uint32_t cap, double *out,
                                                       uint64_t long_n) {
    extern __shared__ __attribute__((aligned(16))) unsigned char corr_lds[];
    const WideLds L = wide_lds(corr_lds);
    const int lane = threadIdx.x;
    const int bw = P.bw;
    const int S = P.S;
    const uint64_t nreg = *nreg_p < reg_cap ? *nreg_p : reg_cap;
    double *sf_ = slabs + (uint64_t)blockIdx.x * 2 * kCorrSlab, *sr_ = sf_ + kCorrSlab;
    for (uint64_t ri = blockIdx.x; ri < nreg; ri += gridDim.x) {
        const uint32_t left = starts[ri], right = ends[ri];
        const UnitDesc U = P.units[reg_unit[ri]];
        const uint32_t n = right - left + 1;
        if (n > long_n) continue;  // (wave-uniform) the stage and chain kernels' region
        double corr = __builtin_nan("");
        if (n > 3) {
            const bool one = n <= (uint32_t)kCorrSlab;  // the slab keeps the whole region
            double sf = 0.0, sr = 0.0;  // sequential sums of f and r (the means)
            for (int64_t a = left; a <= (int64_t)right; a += kCorrSlab) {
                const int64_t b = i64min(right, a + kCorrSlab - 1);
                wide_range_scores<POOL>(P, U, S, bw, a, b, sf_, sr_, L, cap, lane);
                for (int64_t x0 = a; x0 <= b; x0 += 64) {
                    const int nvalid = (int)i64min(64, b - x0 + 1);
                    if (lane < nvalid) {
                        L.prod[2 * lane] = sf_[x0 - a + lane];
                        L.prod[2 * lane + 1] = sr_[x0 - a + lane];
                    }
                    __syncthreads();
                    for (int l = 0; l < nvalid; ++l) {  // (wave-uniform LDS broadcasts)
                        sf = sf + L.prod[2 * l];
                        sr = sr + L.prod[2 * l + 1];
                    }
                    __syncthreads();  // prod reused by the next word
                }
            }
            const double m1 = sf / (double)n, m2 = sr / (double)n;
            double ss1 = 0.0, ss2 = 0.0, ssr = 0.0;
            for (int64_t a = left; a <= (int64_t)right; a += kCorrSlab) {
                const int64_t b = i64min(right, a + kCorrSlab - 1);
                if (!one) wide_range_scores<POOL>(P, U, S, bw, a, b, sf_, sr_, L, cap, lane);
                for (int64_t x0 = a; x0 <= b; x0 += 64) {
                    const int nvalid = (int)i64min(64, b - x0 + 1);
                    if (lane < nvalid) {
                        const double d1 = sf_[x0 - a + lane] - m1, d2 = sr_[x0 - a + lane] - m2;
                        L.prod[3 * lane] = d1 * d1;
                        L.prod[3 * lane + 1] = d2 * d2;
                        L.prod[3 * lane + 2] = d1 * d2;
                    }
                    __syncthreads();
                    for (int l = 0; l < nvalid; ++l) {
                        ss1 = ss1 + L.prod[3 * l];
                        ss2 = ss2 + L.prod[3 * l + 1];
                        ssr = ssr + L.prod[3 * l + 2];
                    }
                    __syncthreads();
                }
            }
            const double sd1 = sqrt(ss1 / ((double)n - 1));
            const double sd2 = sqrt(ss2 / ((double)n - 1));
            corr = ssr / (((double)n - 1) * sd1 * sd2);
            __syncthreads();  // the slab's readers are done before the next region fills it
        }
        if (lane == 0) out[ri] = corr;
    }
}

// ---- K4's slabs of wide regions (up_shift_scan, up_shift_best) ----
// Requested region j (idx[j]) with fill[j] == 2: its dense f and r into
// slab + slab_off[j] as [f[0 .. len) | r[0 .. len)], which shift_kernel then
// reads as a prefilled region.  One wave per region, grid-stride.
template <int POOL>
__global__ void __launch_bounds__(64) wide_fill_kernel(ScanParams P, const uint32_t *starts, const uint32_t *ends,
                                                       const uint32_t *reg_unit, const uint64_t *idx, uint32_t n,
                                                       const uint64_t *slab_off, const uint8_t *fill, double *slab,
                                                       uint32_t cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char corr_lds[];
    const WideLds L = wide_lds(corr_lds);
    const int lane = threadIdx.x;
    for (uint32_t j = blockIdx.x; j < n; j += gridDim.x) {
        if (fill[j] != 2) continue;
        const uint64_t ri = idx[j];
        const uint32_t left = starts[ri], right = ends[ri];
        const UnitDesc U = P.units[reg_unit[ri]];
        const uint32_t len = right - left + 1;
        double *fs = slab + slab_off[j];
        wide_range_scores<POOL>(P, U, P.S, P.bw, left, right, fs, fs + len, L, cap, lane);
    }
}

// ------------------------------------------------------------------------
// wide K1q: the region scan of a threshold <= 0 (quirk Q11 live) for kernels
// wider than K1q's register halo (kMaxBw < bw <= kMaxWideBw, directional
// units, non-negative scores).  The rule is proc_runs_kernel's (kernels.hip):
// every maximal run of processed positions -- the positions within bw of an
// add, a tag of any sample, controls included -- is one region.  A run starts
// at a - bw for an add a with no add in [a - 2bw - 1, a - 1] and ends at
// a + bw for an add with none in [a + 1, a + 2bw + 1].
//   wide_runs_kernel        one wave per strip: the strip's run boundaries in
//                           K1b's record format with peaks unknown
//   wide_peak_prefix_kernel per region its stretches of kProfWords words ->
//                           the exclusive prefix the next two kernels index
//   wide_peak_kernel        one wave per (region, stretch): the stretch's
//                           largest score and the lowest position holding it
//   wide_peak_merge_kernel  one wave per region: its stretches' partials ->
//                           peak_pos / peak_val, which K3 then takes as known
//                           peaks (no KDE of its own, as behind K1w)

constexpr int64_t kWqNone = -((int64_t)1 << 40);  // no add (kWqNone before, -kWqNone after)

// presence bits of the 64-position word j (positions 64 j + 1 .. 64 j + 64) of
// unit U over every track; a word outside [1, len] holds no add and is not
// loaded (the tracks' padding covers the last word's fields past len)
__device__ __forceinline__ uint64_t wq_word(const UnitDesc &U, int S, int64_t j) {
    if (j < 0 || 64 * j + 1 > (int64_t)U.len) return 0;
    uint64_t m = 0;
    for (int st = 0; st < U.nstrands; ++st)
        for (int k = 0; k < S; ++k)
            m |= nz_bits64((u32x4)((gu32x4 *)(track_u8(U, S, st, k) + fbyte(kPadPos)))[j]);
    return m & range_bits(64 * j + 1, 1, (int64_t)U.len);
}

__device__ __forceinline__ int64_t wq_wave_max(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = i64max(v, (int64_t)__shfl_xor((long long)v, o));
    return v;
}
__device__ __forceinline__ int64_t wq_wave_min(int64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = i64min(v, (int64_t)__shfl_xor((long long)v, o));
    return v;
}

// the first and the last add of [lo, hi] (-kWqNone / kWqNone: none), the wave
// together: lane l takes the words l, l + 64, ... of the range.  At most
// 2bw + 1 positions: 1,025 words, 17 per lane at bw 32,767.
__device__ __forceinline__ void wq_span(const UnitDesc &U, int S, int64_t lo, int64_t hi, int lane, int64_t &first,
                                        int64_t &last) {
    lo = i64max(lo, 1);
    hi = i64min(hi, (int64_t)U.len);
    int64_t f = -kWqNone, l = kWqNone;
    if (lo <= hi) {
        const int64_t jh = (hi - 1) >> 6;
        for (int64_t j = ((lo - 1) >> 6) + lane; j <= jh; j += 64) {
            const int64_t base = 64 * j + 1;
            const uint64_t m = wq_word(U, S, j) & range_bits(base, lo, hi);
            if (m) {
                f = i64min(f, base + __builtin_ctzll(m));
                l = i64max(l, base + 63 - __builtin_clzll(m));
            }
        }
    }
    first = wq_wave_min(f);
    last = wq_wave_max(l);
}

// The add that owns a boundary of strip k sits bw away from it, up to two
// strips from k, so the strip does not widen a halo around itself: it takes
// the exact presence words of the two strip-sized add windows -- the adds of
// (p0 + bw, pend + bw] can start a run in (p0, pend], those of [p0 - bw,
// pend - bw) can end one in [p0, pend) -- five words per lane each, and the
// previous add before the start window / the next add after the end window
// from one span query over the 2bw + 1 positions beside it (only the
// window's first / last add can depend on it).  The 2-bit fields answer the
// queries, so a pass needs no index for this kernel; F0 / FL (the strip's
// first / last position is processed) are two more span queries.
constexpr int kWqRounds = (kStrip / 64 + 1 + kWave - 1) / kWave;  // 257 words of a window: 5 per lane

__global__ void __launch_bounds__(64) wide_runs_kernel(ScanParams P) {
    const int lane = threadIdx.x;
    const int64_t bw = P.bw, gap = 2 * bw + 1;
    const int S = P.S;
    for (uint32_t strip = blockIdx.x; strip < P.nstrips; strip += gridDim.x) {
        const uint32_t u = find_unit(P.units, P.nunits, strip);
        const UnitDesc U = P.units[u];
        const uint32_t local = strip - U.strip0;
        const int64_t p0 = 1 + (int64_t)local * kStrip, pend = p0 + kStrip - 1;
        RecList R_{0, 0, kInline};
        int64_t none_lo, none_hi;  // (the unused end of a span query)
        // ---- starts in (p0, pend]: the adds of [ws, we] ----
        {
            const int64_t ws = p0 + bw + 1, we = pend + bw;
            const int64_t j0 = (ws - 1) >> 6;
            int64_t carry;  // the last add before the words seen so far
            wq_span(U, S, ws - gap, ws - 1, lane, none_lo, carry);
#pragma unroll
            for (int r = 0; r < kWqRounds; ++r) {
                const int64_t j = j0 + 64 * r + lane, base = 64 * j + 1;
                const uint64_t m = base <= we ? wq_word(U, S, j) & range_bits(base, ws, we) : 0ull;
                int64_t v = m ? base + 63 - __builtin_clzll(m) : kWqNone;
                for (int d = 1; d < 64; d <<= 1) {  // inclusive prefix maximum of the words' last adds
                    const int64_t o = __shfl_up((long long)v, d);
                    if (lane >= d && o > v) v = o;
                }
                const int64_t ex = __shfl_up((long long)v, 1);
                int64_t prev = lane == 0 ? carry : i64max(ex, carry);
                carry = i64max(carry, (int64_t)__shfl((long long)v, 63));
                uint64_t sa = 0, mm = m;  // the word's adds that start a run
                while (mm) {
                    const int b = __builtin_ctzll(mm);
                    mm &= mm - 1;
                    const int64_t a = base + b;
                    if (prev == kWqNone || a - prev > gap) sa |= 1ull << b;
                    prev = a;
                }
                uint64_t live = __ballot(sa != 0);
                while (live) {
                    const int l = __builtin_ctzll(live);
                    live &= live - 1;
                    uint64_t bits = rl_u64(sa, l);
                    const int64_t lbase = 64 * (j0 + 64 * r + l) + 1;
                    while (bits) {
                        const int b = __builtin_ctzll(bits);
                        bits &= bits - 1;
                        rec_start(R_, (uint32_t)(lbase + b - bw), P, strip, lane);
                    }
                }
            }
        }
        // ---- ends in [p0, pend): the adds of [es, ee] ----
        {
            const int64_t es = p0 - bw, ee = pend - bw - 1;
            const int64_t j0 = (es - 1) >> 6;  // (arithmetic shift: floor; words before position 1 hold no add)
            int64_t carry;  // the first add after the words seen so far
            wq_span(U, S, ee + 1, ee + gap, lane, carry, none_hi);
            uint64_t m[kWqRounds];
            int64_t nxt[kWqRounds];
#pragma unroll
            for (int r = kWqRounds - 1; r >= 0; --r) {
                const int64_t j = j0 + 64 * r + lane, base = 64 * j + 1;
                m[r] = base <= ee ? wq_word(U, S, j) & range_bits(base, es, ee) : 0ull;
                int64_t v = m[r] ? base + __builtin_ctzll(m[r]) : -kWqNone;
                for (int d = 1; d < 64; d <<= 1) {  // inclusive suffix minimum of the words' first adds
                    const int64_t o = __shfl_down((long long)v, d);
                    if (lane + d < 64 && o < v) v = o;
                }
                const int64_t ex = __shfl_down((long long)v, 1);
                nxt[r] = lane == 63 ? carry : i64min(ex, carry);
                carry = i64min(carry, (int64_t)__shfl((long long)v, 0));
            }
#pragma unroll
            for (int r = 0; r < kWqRounds; ++r) {
                const int64_t base = 64 * (j0 + 64 * r + lane) + 1;
                uint64_t ea = 0, mm = m[r];  // the word's adds that end a run
                while (mm) {
                    const int b = __builtin_ctzll(mm);
                    mm &= mm - 1;
                    const int64_t nx = mm ? base + __builtin_ctzll(mm) : nxt[r];
                    if (nx == -kWqNone || nx - (base + b) > gap) ea |= 1ull << b;
                }
                uint64_t live = __ballot(ea != 0);
                while (live) {
                    const int l = __builtin_ctzll(live);
                    live &= live - 1;
                    uint64_t bits = rl_u64(ea, l);
                    const int64_t lbase = 64 * (j0 + 64 * r + l) + 1;
                    while (bits) {
                        const int b = __builtin_ctzll(bits);
                        bits &= bits - 1;
                        rec_end(R_, (uint32_t)(lbase + b + bw), 0u, -__builtin_inf(), P, strip, lane);
                    }
                }
            }
        }
        // ---- the strip's first / last position is processed ----
        int64_t a0, a1;
        wq_span(U, S, p0 - bw, p0 + bw, lane, a0, none_hi);
        wq_span(U, S, pend - bw, pend + bw, lane, a1, none_hi);
        const bool F0 = a0 != -kWqNone, FL = a1 != -kWqNone;
        const uint64_t info = (uint64_t)R_.ns | ((uint64_t)R_.ne << 16) | ((uint64_t)F0 << 32) |
                              ((uint64_t)FL << 33) | ((uint64_t)(local == 0) << 34) |
                              ((uint64_t)(local + 1 == U.nstrips) << 35) | ((uint64_t)(R_.slot != kInline) << 36);
        if (lane == 0) P.strip_info[strip] = info;
    }
}

// the positions a region [s, e] of starts / ends scores for its peak: s + 1 ..
// e -- the run's first position joined by a leap with peakPos 0, so
// Region::addPos re-seeds the peak at the next one (peakcall.cpp:76-78,
// data.cpp:98-101; K3's StatParams::q11 states the same rule for its KDE) --
// and the stretches of kProfWords words that cover them
__device__ __forceinline__ int64_t wq_peak_first(uint32_t s, uint32_t e) { return e > s ? (int64_t)s + 1 : (int64_t)s; }
__device__ __forceinline__ uint64_t wq_stretches(uint32_t s, uint32_t e) {
    const int64_t w_first = (wq_peak_first(s, e) - 1) >> 6, w_last = ((int64_t)e - 1) >> 6;
    return (uint64_t)((w_last - w_first) / kProfWords + 1);
}

// off[i] = the stretches of the regions before region i, off[n] = all of
// them (n = the pass's regions, at most reg_cap).  One block of 1,024.
__global__ void __launch_bounds__(1024) wide_peak_prefix_kernel(const uint32_t *__restrict__ starts,
                                                                const uint32_t *__restrict__ ends,
                                                                const uint64_t *__restrict__ nreg_p,
                                                                uint64_t reg_cap, uint64_t *off) {
    __shared__ uint64_t sh[16];
    __shared__ uint64_t chunk_tot;
    const uint64_t n = *nreg_p < reg_cap ? *nreg_p : reg_cap;
    uint64_t base = 0;
    for (uint64_t c0 = 0; c0 < n; c0 += 1024) {
        const uint64_t i = c0 + threadIdx.x;
        const uint64_t cnt = i < n ? wq_stretches(starts[i], ends[i]) : 0;
        const uint64_t inc = block_incl_sum(cnt, sh);
        if (i < n) off[i] = base + inc - cnt;
        if (threadIdx.x == 1023) chunk_tot = inc;
        __syncthreads();
        base += chunk_tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[n] = base;
}

// Regions here are few and can be millions of positions long, so the work
// items are (region, stretch) pairs: item `it` belongs to the last region r
// with off[r] <= it (a cursor that only moves forward through the prefix).
// Every score is the wide_stretch_scores ascending sum; the wave reduces its
// stretch to (largest score, lowest position holding it) -> part_val /
// part_pos[it].  No floating-point atomics.
// NONDIR: the score of a position is forwardScore + reverseScore, each its own
// ascending sum and one FP64 add as in Region::addPos: the forward walk parks
// the stretch's scores in the workgroup's slab of fstash (kCorrSlab doubles per
// workgroup; every lane reads back only what it wrote), the reverse walk adds
// and reduces.  The screen is the pooled plane, which holds both strands' tags.
template <int POOL, bool NONDIR>
__global__ void __launch_bounds__(64) wide_peak_kernel(ScanParams P, const uint32_t *__restrict__ starts,
                                                       const uint32_t *__restrict__ ends,
                                                       const uint32_t *__restrict__ reg_unit,
                                                       const uint64_t *__restrict__ nreg_p, uint64_t reg_cap,
                                                       const uint64_t *__restrict__ off, uint32_t cap,
                                                       double *part_val, uint32_t *part_pos, uint64_t part_cap,
                                                       double *fstash) {
    extern __shared__ __attribute__((aligned(16))) unsigned char prof_lds[];
    double *hcnt = (double *)prof_lds;
    uint32_t *hpos = (uint32_t *)(prof_lds + (size_t)kProfHits * 8);
    uint32_t *pre = hpos + kProfHits;
    const int lane = threadIdx.x;
    const int bw = P.bw;
    const int S = P.S;
    const uint64_t n = *nreg_p < reg_cap ? *nreg_p : reg_cap;
    const uint64_t total = off[n] < part_cap ? off[n] : part_cap;
    uint64_t cur = 0;
    for (uint64_t it = blockIdx.x; it < total; it += gridDim.x) {
        uint64_t hi = n;  // off[cur] <= it < off[hi]
        while (hi - cur > 1) {
            const uint64_t mid = (cur + hi) >> 1;
            if (off[mid] <= it) cur = mid;
            else hi = mid;
        }
        const uint32_t s = starts[cur], e = ends[cur];
        const UnitDesc U = P.units[reg_unit[cur]];
        const int64_t first = wq_peak_first(s, e);
        const int64_t w_first = (first - 1) >> 6, w_last = ((int64_t)e - 1) >> 6;
        const int64_t w0 = w_first + (int64_t)(it - off[cur]) * kProfWords;
        const int nw = (int)i64min(kProfWords, w_last - w0 + 1);
        const int64_t x_lo = 1 + 64 * w0;
        gu8 *pl = (POOL == 0 && !NONDIR) ? plane_u8(U, S, 0, P.nc[0]) : pooled_u8(U, S);
        const WideScreen W = wide_stretch_screen(pl, (int64_t)(U.stride / 4), bw, x_lo, nw, pre, lane);
        // (ALL: a word without a pooled tag in reach -- beside a control-only
        // add -- is still a processed position, with the score 0.0)
        double best = -__builtin_inf();
        int64_t bx = -kWqNone;
        auto take = [&](int64_t x, double f) {  // (ascending x per lane: the first maximum)
            if (x >= first && x <= (int64_t)e && f > best) {
                best = f;
                bx = x;
            }
        };
        if constexpr (!NONDIR) {
            wide_stretch_scores<POOL, true>(P, U, S, 0, bw, x_lo, nw, W, pre, cap, hcnt, hpos, lane, take);
        } else {
            double *fs = fstash + (uint64_t)blockIdx.x * kCorrSlab;
            wide_stretch_scores<POOL, true>(P, U, S, 0, bw, x_lo, nw, W, pre, cap, hcnt, hpos, lane,
                                            [&](int64_t x, double f) { fs[x - x_lo] = f; });
            __syncthreads();  // the forward walk has read the list the reverse gather refills
            wide_stretch_scores<POOL, true>(P, U, S, 1, bw, x_lo, nw, W, pre, cap, hcnt, hpos, lane,
                                            [&](int64_t x, double r) { take(x, fs[x - x_lo] + r); });
        }
        const double m = wave_max_d(best);
        const int64_t at = wq_wave_min(best == m ? bx : -kWqNone);
        if (lane == 0) {
            part_val[it] = m;
            part_pos[it] = at == -kWqNone ? 0u : (uint32_t)at;
        }
    }
}

// each region's partials in stretch order -> its peak: the largest score, on
// equal scores the lower position (positions ascend with the stretches, so
// this is the first maximum whatever order the lanes meet them in).  One wave
// per region.
__global__ void __launch_bounds__(256) wide_peak_merge_kernel(const uint64_t *__restrict__ nreg_p, uint64_t reg_cap,
                                                              const uint64_t *__restrict__ off,
                                                              const double *__restrict__ part_val,
                                                              const uint32_t *__restrict__ part_pos,
                                                              uint64_t part_cap, uint32_t *peak_pos,
                                                              double *peak_val) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t n = *nreg_p < reg_cap ? *nreg_p : reg_cap;
    for (uint64_t r = wave; r < n; r += nwaves) {
        const uint64_t a = off[r], b = off[r + 1] < part_cap ? off[r + 1] : part_cap;
        double best = -__builtin_inf();
        uint32_t bx = 0xFFFFFFFFu;
        for (uint64_t i = a + lane; i < b; i += 64) {
            const double v = part_val[i];
            const uint32_t p = part_pos[i];
            if (v > best || (v == best && p < bx)) {
                best = v;
                bx = p;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double ov = __shfl_xor(best, o);
            const uint32_t op = (uint32_t)__shfl_xor((int)bx, o);
            if (ov > best || (ov == best && op < bx)) {
                best = ov;
                bx = op;
            }
        }
        if (lane == 0) {
            peak_pos[r] = bx;
            peak_val[r] = best;
        }
    }
}

// ------------------------------------------------------------------------
// strandCorr(0) of the long regions of a nondirectional wide K1q pass.  A run
// of processed positions can span a contig, and wide_corr_kernel would hand
// all of it to one wave: both the dense scores (the expensive part) and the
// five sequential FP64 sums (which cannot be split and stay bit-exact).  So a
// region of more than kCorrLong stored positions s .. e (the reported left and
// right are one higher; the peak range is s + 1 .. e) splits the two:
//   wide_corr_prefix_kernel  per region its stretches and its stored positions
//                            if it is long, else 0 -> two exclusive prefixes:
//                            the items of the stage kernel and one cumulative
//                            position axis that lays the long regions end to end
//   wide_corr_stage_kernel   one wave per (long region, stretch): f and r of
//                            the stretch's stored positions -- the
//                            wide_stretch_scores sums wide_range_scores forms,
//                            so the same bits -- into the staging area, 16 bytes
//                            per position, at the position's place on the axis
//   wide_corr_chain_kernel   one wave per long region: the staged scores in
//                            position order with exactly wide_corr_kernel's
//                            arithmetic -- sweep 1 carries the sums of f and r,
//                            sweep 2 those of d1*d1, d2*d2 and d1*d2 -- then
//                            sqrt(ss / (n - 1)) and the correlation into out[ri]
// The staging area holds `tile` positions (kCorrTile).  Round k of a sweep
// covers [k * tile, (k + 1) * tile) of the axis; a region cut by a round
// boundary keeps its five sums in carry[5 ri ..] between rounds.  The host
// enqueues a fixed number of rounds from the context's positions (which bound
// the axis); a round past the axis' end exits at once, and when the whole
// axis fits one round, sweep 2 finds sweep 1's scores still staged and the
// stage kernel of sweep 2 exits at once as well.  The kernels are ordered by
// the pass stream alone: no wave waits for another.
constexpr uint64_t kCorrLong = 16ull * kCorrSlab;  // stored positions wide_corr_kernel still takes: 65,536
constexpr uint64_t kCorrTile = 64ull << 20;        // positions of the staging area: 1 GiB

__device__ __forceinline__ uint64_t wc_stretches(uint32_t s, uint32_t e) {
    return (uint64_t)(((((int64_t)e - 1) >> 6) - (((int64_t)s - 1) >> 6)) / kProfWords + 1);
}

// the last i in [0, n) with off[i] <= v (off ascending, off[0] = 0 <= v < off[n]):
// a region without items / positions shares its offset with the next one, so
// this is the region that owns item / axis position v
__device__ __forceinline__ uint64_t wc_owner(const uint64_t *__restrict__ off, uint64_t n, uint64_t v, uint64_t lo) {
    uint64_t hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// One block of 1,024 (wide_peak_prefix_kernel's scheme, two sums at once).
__global__ void __launch_bounds__(1024) wide_corr_prefix_kernel(const uint32_t *__restrict__ starts,
                                                                const uint32_t *__restrict__ ends,
                                                                const uint64_t *__restrict__ nreg_p,
                                                                uint64_t reg_cap, uint64_t long_n, uint64_t *ioff,
                                                                uint64_t *aoff) {
    __shared__ uint64_t sh[16];
    __shared__ uint64_t tot[2];
    const uint64_t n = *nreg_p < reg_cap ? *nreg_p : reg_cap;
    uint64_t ibase = 0, abase = 0;
    for (uint64_t c0 = 0; c0 < n; c0 += 1024) {
        const uint64_t i = c0 + threadIdx.x;
        uint64_t items = 0, len = 0;
        if (i < n) {
            const uint32_t s = starts[i], e = ends[i];
            const uint64_t m = (uint64_t)e - s + 1;
            if (m > long_n) {
                items = wc_stretches(s, e);
                len = m;
            }
        }
        const uint64_t iinc = block_incl_sum(items, sh);
        const uint64_t ainc = block_incl_sum(len, sh);
        if (i < n) {
            ioff[i] = ibase + iinc - items;
            aoff[i] = abase + ainc - len;
        }
        if (threadIdx.x == 1023) {
            tot[0] = iinc;
            tot[1] = ainc;
        }
        __syncthreads();
        ibase += tot[0];
        abase += tot[1];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ioff[n] = ibase;
        aoff[n] = abase;
    }
}

// stage: [f, r] of axis position A at stage[2 (A - round * tile)], A inside the
// round and the area (stage_cap positions)
template <int POOL>
__global__ void __launch_bounds__(64) wide_corr_stage_kernel(ScanParams P, const uint32_t *__restrict__ starts,
                                                             const uint32_t *__restrict__ ends,
                                                             const uint32_t *__restrict__ reg_unit,
                                                             const uint64_t *__restrict__ nreg_p, uint64_t reg_cap,
                                                             const uint64_t *__restrict__ ioff,
                                                             const uint64_t *__restrict__ aoff, uint64_t tile,
                                                             uint64_t stage_cap, uint64_t round, int sweep,
                                                             uint32_t cap, double *stage) {
    extern __shared__ __attribute__((aligned(16))) unsigned char prof_lds[];
    double *hcnt = (double *)prof_lds;
    uint32_t *hpos = (uint32_t *)(prof_lds + (size_t)kProfHits * 8);
    uint32_t *pre = hpos + kProfHits;
    const int lane = threadIdx.x;
    const int bw = P.bw;
    const int S = P.S;
    const uint64_t n = *nreg_p < reg_cap ? *nreg_p : reg_cap;
    const uint64_t total = aoff[n];
    const uint64_t A0 = round * tile;
    if (A0 >= total) return;                   // a round past the axis' end
    if (sweep == 2 && total <= tile) return;   // one round holds everything: sweep 1's scores are still staged
    const uint64_t A1 = A0 + tile < total ? A0 + tile : total;
    // the items that hold the round's first and last position
    uint64_t it_lo, it_hi;
    {
        const uint64_t r0 = wc_owner(aoff, n, A0, 0), r1 = wc_owner(aoff, n, A1 - 1, r0);
        const int64_t x0 = (int64_t)starts[r0] + (int64_t)(A0 - aoff[r0]);
        const int64_t x1 = (int64_t)starts[r1] + (int64_t)(A1 - 1 - aoff[r1]);
        it_lo = ioff[r0] + (uint64_t)((((x0 - 1) >> 6) - (((int64_t)starts[r0] - 1) >> 6)) / kProfWords);
        it_hi = ioff[r1] + (uint64_t)((((x1 - 1) >> 6) - (((int64_t)starts[r1] - 1) >> 6)) / kProfWords);
    }
    uint64_t cur = 0;
    for (uint64_t it = it_lo + blockIdx.x; it <= it_hi; it += gridDim.x) {
        cur = wc_owner(ioff, n, it, cur);
        const uint32_t s = starts[cur], e = ends[cur];
        const UnitDesc U = P.units[reg_unit[cur]];
        const uint64_t a0 = aoff[cur];
        const int64_t w_first = ((int64_t)s - 1) >> 6, w_last = ((int64_t)e - 1) >> 6;
        const int64_t w0 = w_first + (int64_t)(it - ioff[cur]) * kProfWords;
        const int nw = (int)i64min(kProfWords, w_last - w0 + 1);
        const int64_t x_lo = 1 + 64 * w0;
        const WideScreen W = wide_stretch_screen(pooled_u8(U, S), (int64_t)(U.stride / 4), bw, x_lo, nw, pre, lane);
        auto put = [&](int64_t x, double v, int strand) {
            if (x < (int64_t)s || x > (int64_t)e) return;
            const uint64_t A = a0 + (uint64_t)(x - (int64_t)s);
            if (A >= A0 && A < A1 && A - A0 < stage_cap) stage[2 * (A - A0) + strand] = v;
        };
        wide_stretch_scores<POOL, true>(P, U, S, 0, bw, x_lo, nw, W, pre, cap, hcnt, hpos, lane,
                                        [&](int64_t x, double f) { put(x, f, 0); });
        __syncthreads();  // the forward walk has read the list the reverse gather refills
        wide_stretch_scores<POOL, true>(P, U, S, 1, bw, x_lo, nw, W, pre, cap, hcnt, hpos, lane,
                                        [&](int64_t x, double r) { put(x, r, 1); });
        __syncthreads();
    }
}

// chain: the piece of every long region inside the round, one wave per region;
// carry[5 ri + 0 .. 4] = sf, sr, ss1, ss2, ssr of region ri so far.
// The wave takes kChainBlk words of 64 staged positions at a time, lane l the
// l-th position of each word (one 16-byte load per word, the next block's
// issued before this block's sums), forms its position's terms and hands them
// round lane by lane through v_readlane: every lane then adds them in
// position order, so each sum is the one sequential chain -- no LDS round
// trip between two dependent adds (a first version read the terms back from
// LDS one position at a time and spent ~50 ns per position waiting for it).
constexpr int kChainBlk = 4;

struct WcPair {
    double f, r;
};

// the staged pairs of positions j0 + 64 c + lane (c < kChainBlk) below hi
__device__ __forceinline__ void wc_load(WcPair (&v)[kChainBlk], const double *__restrict__ stage, uint64_t j0,
                                        uint64_t hi, uint64_t A0, uint64_t stage_cap, int lane) {
#pragma unroll
    for (int c = 0; c < kChainBlk; ++c) {
        const uint64_t j = j0 + 64 * (uint64_t)c + lane, q = j - A0;
        v[c].f = 0.0;
        v[c].r = 0.0;
        if (j < hi && q < stage_cap) {
            const double2 t = ((const double2 *)stage)[q];
            v[c].f = t.x;
            v[c].r = t.y;
        }
    }
}

__global__ void __launch_bounds__(64) wide_corr_chain_kernel(const uint32_t *__restrict__ starts,
                                                             const uint32_t *__restrict__ ends,
                                                             const uint64_t *__restrict__ nreg_p, uint64_t reg_cap,
                                                             const uint64_t *__restrict__ aoff, uint64_t long_n,
                                                             uint64_t tile, uint64_t stage_cap, uint64_t round,
                                                             int sweep, const double *__restrict__ stage,
                                                             double *carry, double *out) {
    const int lane = threadIdx.x;
    const uint64_t nreg = *nreg_p < reg_cap ? *nreg_p : reg_cap;
    const uint64_t total = aoff[nreg];
    const uint64_t A0 = round * tile;
    if (A0 >= total) return;
    const uint64_t A1 = A0 + tile < total ? A0 + tile : total;
    constexpr uint64_t kBlk = 64ull * kChainBlk;
    for (uint64_t ri = blockIdx.x; ri < nreg; ri += gridDim.x) {
        const uint32_t left = starts[ri], right = ends[ri];
        const uint64_t n = (uint64_t)right - left + 1;
        const uint64_t a0 = aoff[ri], a1 = a0 + n;
        if (n <= long_n || a0 >= A1 || a1 <= A0) continue;  // (wave-uniform)
        const uint64_t lo = a0 > A0 ? a0 : A0, hi = a1 < A1 ? a1 : A1;
        const bool fresh = a0 >= A0;  // the region begins in this round
        double *cr = carry + 5 * ri;
        WcPair cur[kChainBlk], nxt[kChainBlk];
        wc_load(cur, stage, lo, hi, A0, stage_cap, lane);
        if (sweep == 1) {
            double sf = fresh ? 0.0 : cr[0], sr = fresh ? 0.0 : cr[1];
            for (uint64_t j0 = lo; j0 < hi; j0 += kBlk) {
                wc_load(nxt, stage, j0 + kBlk, hi, A0, stage_cap, lane);
#pragma unroll
                for (int c = 0; c < kChainBlk; ++c) {
                    const uint64_t base = j0 + 64 * (uint64_t)c;
                    if (base + 64 <= hi) {
#pragma unroll
                        for (int l = 0; l < 64; ++l) {
                            sf = sf + rl_d(cur[c].f, l);
                            sr = sr + rl_d(cur[c].r, l);
                        }
                    } else if (base < hi) {
                        const int nvalid = (int)(hi - base);
                        for (int l = 0; l < nvalid; ++l) {
                            sf = sf + rl_d(cur[c].f, l);
                            sr = sr + rl_d(cur[c].r, l);
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < kChainBlk; ++c) cur[c] = nxt[c];
            }
            if (lane == 0) {
                cr[0] = sf;
                cr[1] = sr;
            }
        } else {
            const double m1 = cr[0] / (double)n, m2 = cr[1] / (double)n;
            double ss1 = fresh ? 0.0 : cr[2], ss2 = fresh ? 0.0 : cr[3], ssr = fresh ? 0.0 : cr[4];
            for (uint64_t j0 = lo; j0 < hi; j0 += kBlk) {
                wc_load(nxt, stage, j0 + kBlk, hi, A0, stage_cap, lane);
#pragma unroll
                for (int c = 0; c < kChainBlk; ++c) {
                    const uint64_t base = j0 + 64 * (uint64_t)c;
                    const double d1 = cur[c].f - m1, d2 = cur[c].r - m2;
                    const double p1 = d1 * d1, p2 = d2 * d2, p3 = d1 * d2;
                    if (base + 64 <= hi) {
#pragma unroll
                        for (int l = 0; l < 64; ++l) {
                            ss1 = ss1 + rl_d(p1, l);
                            ss2 = ss2 + rl_d(p2, l);
                            ssr = ssr + rl_d(p3, l);
                        }
                    } else if (base < hi) {
                        const int nvalid = (int)(hi - base);
                        for (int l = 0; l < nvalid; ++l) {
                            ss1 = ss1 + rl_d(p1, l);
                            ss2 = ss2 + rl_d(p2, l);
                            ssr = ssr + rl_d(p3, l);
                        }
                    }
                }
#pragma unroll
                for (int c = 0; c < kChainBlk; ++c) cur[c] = nxt[c];
            }
            if (lane == 0) {
                cr[2] = ss1;
                cr[3] = ss2;
                cr[4] = ssr;
            }
            if (a1 <= A1) {  // the region ends in this round
                double corr = __builtin_nan("");
                if (n > 3) {
                    const double sd1 = sqrt(ss1 / ((double)n - 1));
                    const double sd2 = sqrt(ss2 / ((double)n - 1));
                    corr = ssr / (((double)n - 1) * sd1 * sd2);
                }
                if (lane == 0) out[ri] = corr;
            }
        }
    }
}

}  // namespace upk
