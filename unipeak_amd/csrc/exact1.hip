// unipeak_amd/csrc/exact1.hip -- K1b for one pooled directional sample with
// the Q keys on (pool mode 0, one strand per unit, 2-bit tracks, no profile:
// BASELINE configs[1]).  Included by nh_tu.hip and api.hip after kernels.hip.
//
// Same outputs, bit for bit, as scan_kernel<NH, 0, false, false, kModeExact>
// with ScanParams::qmode set (strip summaries, inline and overflow run
// records with their peaks, spk, ovf_count), from the same work list (xref,
// xlist, xcount).  That kernel is latency-bound beside K1a: every work item
// starts with four dependent round trips (xref word, entry, unit descriptor,
// window bytes) and every further exact block with one more, one wave per
// SIMD and nothing in flight meanwhile.  Here a wave's share of the list is
// one stream of (item, exact block) pairs behind a lookahead cursor:
//  * the 16-byte lane load of the next block's window -- the next exact block
//    of this item, or the first one of the wave's next item -- is issued
//    before the current block is computed;
//  * the next item's header is carried while the current one runs: its strip,
//    block mask, chunk masks (one VGPR) and, of its unit, the track address of
//    the strip and the strip's place in the unit; the entry of the item after
//    it and the xref word one item further are loaded at the same point, so
//    the three loads of an item step are independent of one another;
//  * the whole unit descriptor is read only where a window holds an escape.
// The lookahead issues only loads the generic kernel issues later -- nothing
// past xcount[0] + xcount[1], no address that kernel would not touch.
//
// LDS: the weight table is sized for the pass's bw, and the block's keys are
// uint32 (a flagged position's Q >= 1, 0 otherwise; the FP64 scores of the
// undecided words stay in registers): 21.4 KB per workgroup at bw 50 where
// scan_kernel takes 44 KB.
#pragma once

namespace upk {

__host__ __device__ constexpr int exact1_wave_words(int nh) { return kStepWords * kWave + 4 * (kStepWords + 2 * nh); }
// dynamic LDS of a 4-wave workgroup: the padded weight table, then per wave
// the keys of a block's 16 words and the window's bytes
inline size_t exact1_lds(int bw, int nh) {
    return (size_t)(2 * kKPad + 2 * bw + 2) * sizeof(double) + 4 * (size_t)exact1_wave_words(nh) * sizeof(uint32_t);
}

template <int NH>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(UPK_K1B_WPE))) exact1_kernel(ScanParams P) {
    extern __shared__ double lds_[];
    constexpr int SW = kStepWords;
    constexpr int NWIN = SW + 2 * NH;
    static_assert(kTB == 2 && NWIN <= 64, "2-bit tracks, one wave load per window");
    const int bw = P.bw;
    const int ktab_n = 2 * kKPad + 2 * bw + 2;  // doubles (even: the areas behind stay 16-byte aligned)
    for (int i = threadIdx.x; i < ktab_n; i += blockDim.x) {
        const int j = i - kKPad;
        lds_[i] = (j >= 0 && j <= 2 * bw) ? P.kern[j] : 0.0;
    }
    __syncthreads();
    const double *ktab = lds_ + kKPad;
    uint32_t *keys = (uint32_t *)(lds_ + ktab_n) + (threadIdx.x >> 6) * exact1_wave_words(NH);
    uint8_t *stage = (uint8_t *)(keys + SW * kWave);

    const auto *units = cptr(P.units);
    const int lane = threadIdx.x & 63;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    // (readfirstlane: the grid stride otherwise counts as divergent, and with
    // it the item loop, the headers and the strip's run state -- vector
    // registers and vector loads of the unit table in the item step)
    const uint32_t nwaves = __builtin_amdgcn_readfirstlane(gridDim.x * (blockDim.x >> 6));
    const int nc0 = cptr(P.nc)[0];
    const uint32_t bw2 = (uint32_t)(bw * bw);
    // (the Q window sums' lane rotations: see scan_kernel)
    const int hadr = 4 * ((lane + bw) & 63), ladr = 4 * ((lane - bw - 1) & 63);
    const bool hsel = ((((lane - bw) & 63) + bw - 64 * (NH - 1)) >> 6) != 0;
    const bool lsel = ((((lane + bw + 1) & 63) - bw - 1 + 64 * NH) >> 6) != 0;
    const uint32_t sh = fshift(lane);
    const int wl = lane < NWIN ? lane : NWIN - 1;  // (lanes past the window repeat its last piece)

    // the work list: front (multi-block) items first, this wave's every nwaves-th
    const uint32_t n = __builtin_amdgcn_readfirstlane(P.xcount[0] + P.xcount[1]);
    const auto *xref = cptr(P.xref);
    uint32_t it = wave;
    if (it >= n) return;

    struct Hdr {  // of the work-list entry
        uint32_t strip, eb, cur;
    };
    struct Loc {  // of the entry's unit
        gu8 *tb;  // the track's byte of the strip's first position
        uint32_t local, unstrips;
    };
    auto load_hdr = [&](uint32_t ei, Hdr &h, uint32_t &mch) {
        const uint32_t *e = P.xlist + (uint64_t)ei * kXEntry;
        const auto *es = cptr(e);  // the uniform words through scalar loads
        h.strip = es[0];
        const uint32_t e1 = es[1];
        h.eb = e1 & 0xFFFFu;
        mch = (e[2 + (lane >> 1)] >> (16 * (lane & 1))) & 0xFFFFu;
        h.cur = e1 >> 16;  // K1a stored the unit with the entry
        if (h.cur == 0xFFFFu) h.cur = find_unit(units, P.nunits, h.strip);
    };
    auto load_loc = [&](const Hdr &h, Loc &l) {
        const uint64_t base = units[h.cur].base, stride = units[h.cur].stride;
        const uint32_t s0 = units[h.cur].strip0;
        l.local = h.strip - s0;
        l.unstrips = units[h.cur].nstrips;
        l.tb = (gu8 *)base + (uint64_t)nc0 * stride + fbyte(kPadPos) + (uint64_t)l.local * kStripBytes;
    };
    // window of exact block j: words 16j - NH .. 16j + 15 + NH of the strip
    auto win_load = [&](const Loc &l, int j) -> u32x4 {
        return *((gu32x4 *)(l.tb + (int64_t)kWordBytes * (j * SW - NH)) + wl);
    };
    // Invariant the stream depends on: every listed entry holds an exact block
    // (both K1a writers stash an entry only when exact_blocks != 0: scan_kernel's
    // and k1a_fields_kernel's `if (exact_blocks == 0) ... else` stash).  An
    // entry without one would skip the block loop and leave its prefetched
    // window to the next item.  The guard only keeps ctz(0) out of an address.
    auto first_block = [](uint32_t eb) { return eb ? __builtin_ctz(eb) : 0; };

    Hdr h0{}, h1{}, h2{};
    Loc l0{}, l1{};
    uint32_t m0 = 0, m1 = 0, m2 = 0, xr2 = 0;
    load_hdr(xref[it], h0, m0);
    load_loc(h0, l0);
    if (it + nwaves < n) load_hdr(xref[it + nwaves], h1, m1);
    if (it + 2 * nwaves < n) xr2 = xref[it + 2 * nwaves];
    u32x4 wv = win_load(l0, first_block(h0.eb));  // the stream's next window

    for (;;) {
        // the item step's loads, independent of one another: the next item's
        // unit, the entry after it, the xref word one further
        const bool v1 = it + nwaves < n, v2 = it + 2 * nwaves < n;
        if (v1) load_loc(h1, l1);
        if (v2) load_hdr(xr2, h2, m2);
        uint32_t xr3 = 0;
        if (it + 3 * nwaves < n) xr3 = xref[it + 3 * nwaves];

        const uint32_t strip = h0.strip;
        const int64_t p0 = 1 + (int64_t)l0.local * kStrip;  // first position of the strip
        // run state of the strip (scan_kernel's, the keys as integers)
        RecList R_{0, 0, kInline};
        uint64_t F0 = 0;
        bool open = false;
        int last = -2;
        bool pk_ok = false;
        uint32_t best = 0, bpos = 0;
        bool btie = false;
        auto run_key = [&]() { return btie ? (double)best + 0.5 : (double)best; };
        auto close_run = [&](uint32_t end_pos) {
            const double m = run_key();
            rec_end(R_, end_pos, pk_ok ? bpos : 0u, m, P, strip, lane);
            if (!pk_ok && lane == 0) {
                P.spk[4ull * strip] = (uint64_t)__double_as_longlong(m);
                P.spk[4ull * strip + 1] = bpos;
            }
            open = false;
        };

        for (uint32_t eb = h0.eb; eb;) {
            const int j = __builtin_ctz(eb);
            eb &= eb - 1u;
            uint32_t lw = 0;  // words of this block that can hold a flag
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint64_t bq = __ballot(((m0 >> (4 * q)) & 0xFu) != 0u) >> (4 * j);
#pragma unroll
                for (int i = 0; i < 4; ++i) lw |= (uint32_t)((bq >> i) & 1ull) << (4 * i + q);
            }
            const int64_t x0 = p0 + 64 * (j * SW - NH);  // position of window word 0, lane 0

            // ---- this block's window (in flight since the block before), then
            // the next one's load
            const u32x4 v = wv;
            __builtin_amdgcn_wave_barrier();  // earlier readers of the stage are done
            uint32_t ebits = 0;  // escaped fields in this lane's 16 bytes
            if (lane < NWIN) {
                *(u32x4 *)(stage + 16 * lane) = v;
                ebits = fbig32(v.x) | fbig32(v.y) | fbig32(v.z) | fbig32(v.w);
            }
            if (eb) wv = win_load(l0, __builtin_ctz(eb));
            else if (v1) wv = win_load(l1, first_block(h1.eb));
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            uint32_t wf[NWIN];
#pragma unroll
            for (int w = 0; w < NWIN; ++w) wf[w] = ((uint32_t)stage[kWordBytes * w + fbyte(lane)] >> sh) & kTMask;
            if (__ballot(ebits != 0u)) {
                const UnitDesc U = units[h0.cur];
                resolve_escapes<NWIN>(wf, U, (uint32_t)nc0, x0, lane);
            }

            // ---- keys: exact integer Q of every live word (scan_kernel), and
            // for a word with an undecided lane its FP64 scores at once
            // (kde_word's ascending walk over the hits of window words k .. k +
            // 2NH: the same multiply-add sequence per position as scan_kernel's
            // scatter -- pairs out of reach add +0 from the padded table in
            // both -- with one accumulator live instead of 16).  key = Q of a
            // flagged position (proven by Q, or by the FP64 score of an
            // undecided lane), 0 otherwise; the keys go straight to LDS
            uint32_t anykey = 0;
            // (an opaque copy of the lane index per block: the per-word index
            // terms below are otherwise hoisted out of the item loop, some 80
            // loop-invariant VGPRs that the allocator then spills)
            uint32_t ln = (uint32_t)lane;
            asm volatile("" : "+v"(ln));
            // (the weight reads through a volatile view, as in scatter_hits: a
            // batch's kHB reads stay ahead of its first add, one LDS latency
            // per batch.  It is not a register matter -- tools/resources.py
            // gives the same row without it, 89 VGPRs and no scratch at NH 1
            // (ROCm 7.2) -- and its effect on the time was not measured here)
            typedef const volatile __attribute__((address_space(3))) double lds_vd;
            lds_vd *vk = (lds_vd *)ktab;
            {
                uint32_t P0[NWIN], P1[NWIN], P2[NWIN];
                uint32_t c0 = 0, c1 = 0, c2 = 0;
                uint32_t nd = lw;
#pragma unroll
                for (int d = 1; d <= 2 * NH; ++d) nd |= lw << d;
                WordLoop<0, NWIN>::run([&](auto wc) {
                    constexpr int w = decltype(wc)::value;
                    uint64_t any = 0;
                    if ((nd >> w) & 1u) {
                        any = __ballot(nz(wf[w]));
                    } else {
                        c0 = c1 = c2 = 0u;
                    }
                    if (any == 0) {
                        P0[w] = c0;
                        P1[w] = c1;
                        P2[w] = c2;
                    } else {
                        const uint32_t c = wf[w];
                        const uint32_t jj = 64u * w + ln;
                        const uint32_t s0 = wave_scan_u32(c), s1 = wave_scan_u32(c * jj),
                                       s2 = wave_scan_u32(c * (jj * jj));
                        P0[w] = s0 + c0;
                        P1[w] = s1 + c1;
                        P2[w] = s2 + c2;
                        c0 += rl_u(s0, 63);
                        c1 += rl_u(s1, 63);
                        c2 += rl_u(s2, 63);
                    }
                    constexpr int k = w - 2 * NH;  // output word whose window ends with word w
                    if constexpr (k >= 0) {
                        if ((lw >> k) & 1u) {
                            auto win = [&](const uint32_t (&Pa)[NWIN]) {
                                const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(
                                    hadr, (int)(hsel ? Pa[k + 2 * NH] : Pa[k + 2 * NH - 1]));
                                const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(
                                    ladr, (int)(lsel ? Pa[k + 1] : Pa[k]));
                                return hi - lo;
                            };
                            const uint32_t W0 = win(P0), W1 = win(P1), W2 = win(P2);
                            const uint32_t i = 64u * (k + NH) + ln;
                            const uint32_t q = bw2 * W0 - (i * i) * W0 + 2u * i * W1 - W2;
                            double f = 0.0;
                            if (__ballot(q > P.qno && q < P.qyes)) {
                                WordLoop<0, 2 * NH + 1>::run([&](auto dc) {
                                    constexpr int d = decltype(dc)::value - NH;
                                    uint64_t m = __ballot(nz(wf[k + NH + d])) & win_mask(d, bw);
                                    while (m) {  // batches of kHB hits: weight reads first, adds in order
                                        int hb[kHB];
                                        double hc[kHB], kv[kHB];
                                        next_hits(m, wf[k + NH + d], hb, hc);
#pragma unroll
                                        for (int h = 0; h < kHB; ++h)
                                            kv[h] = vk[lane + (bw - 64 * d - hb[h])];  // 0 outside
#pragma unroll
                                        for (int h = 0; h < kHB; ++h) f = f + kv[h] * hc[h];
                                    }
                                });
                            }
                            const bool fl = q >= P.qyes || (q > P.qno && f >= P.thr);
                            const uint32_t key = fl ? q : 0u;
                            keys[64 * k + lane] = key;
                            anykey |= key;
                        }
                    }
                });
            }
            // ---- flags and run boundaries (only blocks touching a run) ----
            if (__ballot(anykey != 0u) || open) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll 1
                for (uint32_t lm = lw; lm; lm &= lm - 1u) {
                    const int k = __builtin_ctz(lm);
                    const int g = j * SW + k;  // word of the strip
                    const int64_t wpos = p0 + 64 * g;
                    if (open && g != last + 1) close_run((uint32_t)(p0 + 64 * (last + 1) - 1));
                    last = g;
                    const uint32_t sck = keys[64 * k + lane];
                    const uint64_t F = __ballot(sck != 0u);
                    if (g == 0) F0 = F;
                    if (open && !(F & 1ull)) close_run((uint32_t)(wpos - 1));
                    uint64_t st = F & ~((F << 1) | ((open || g == 0) ? 1ull : 0ull));
                    while (st) {
                        const int b = __builtin_ctzll(st);
                        st &= st - 1;
                        rec_start(R_, (uint32_t)(wpos + b), P, strip, lane);
                    }
                    uint64_t rem = F;
                    while (rem) {
                        const int a = __builtin_ctzll(rem);
                        const uint64_t up = ~(rem >> a);
                        const int len = up ? __builtin_ctzll(up) : 64 - a;
                        rem = len + a >= 64 ? 0ull : rem & (~0ull << (a + len));
                        const bool in = lane >= a && lane < a + len;
                        const uint32_t kq = in ? sck : 0u;
                        const uint32_t mq = wave_max_u32(kq);
                        const uint64_t at = __ballot(kq == mq);
                        if (!(a == 0 && open)) {  // a new run
                            best = mq;
                            bpos = (uint32_t)(wpos + __builtin_ctzll(at));
                            btie = (at & (at - 1)) != 0;
                            pk_ok = g != 0 || a != 0;
                        } else if (mq > best) {
                            best = mq;
                            bpos = (uint32_t)(wpos + __builtin_ctzll(at));
                            btie = (at & (at - 1)) != 0;
                        } else if (mq == best) {
                            btie = true;
                        }
                        open = true;
                        if (a + len < 64) close_run((uint32_t)(wpos + a + len - 1));
                    }
                }
                __builtin_amdgcn_wave_barrier();  // keys reused by the next block
            }
        }
        if (open && last != kStripWords - 1) close_run((uint32_t)(p0 + 64 * (last + 1) - 1));
        if (open) {  // the run open at the strip's last position: its part here
            if (lane == 0) {
                P.spk[4ull * strip + 2] = (uint64_t)__double_as_longlong(run_key());
                P.spk[4ull * strip + 3] = bpos;
            }
        }
        const uint64_t info = (uint64_t)R_.ns | ((uint64_t)R_.ne << 16) | ((F0 & 1ull) << 32) |
                              ((uint64_t)open << 33) | ((uint64_t)(l0.local == 0) << 34) |
                              ((uint64_t)(l0.local + 1 == l0.unstrips) << 35) |
                              ((uint64_t)(R_.slot != kInline) << 36);
        if (lane == 0) P.strip_info[strip] = info;

        if (!v1) break;
        it += nwaves;
        h0 = h1;
        l0 = l1;
        m0 = m1;
        h1 = h2;
        m1 = m2;
        xr2 = xr3;
    }
}

}  // namespace upk
