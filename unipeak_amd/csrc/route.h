// unipeak_amd/csrc/route.h -- which scan a pass takes and what a context of
// that route may ask for: the one statement of the policy (DESIGN.md §1
// "Routes"); api.hip reads route_for's result.  Plain C++, no HIP
// (tests/route_table.cpp enumerates it on the CPU).
#pragma once

namespace upk {

enum class Scan {
    K1,       // the narrow parallel scan (K1a / K1x / K1b)
    K1w,      // the wide parallel scan (wide.hip)
    K1q,      // runs of processed positions, threshold <= 0 (proc_runs_kernel)
    K1qWide,  // the same above the narrow halo (wide_runs_kernel, wide_peak_kernel)
    Replay,   // every unit through K0, the exact state machine (emulate.hip)
};

// the integers up_last_scan_kind documents (include/unipeak_hip.h)
constexpr int scan_kind(Scan s) { return s == Scan::K1 ? 0 : s == Scan::K1w ? 1 : s == Scan::Replay ? 3 : 2; }
// the dense scores are wide.hip's and the index planes are always wanted
constexpr bool is_wide(Scan s) { return s == Scan::K1w || s == Scan::K1qWide; }
constexpr bool is_q11(Scan s) { return s == Scan::K1q || s == Scan::K1qWide; }

// Environment switches, read once at up_open (A/B and tests): each takes a context off a parallel scan
struct Switches {
    bool wide = true;         // UNIPEAK_WIDE=0: the replay above the narrow halo
    bool wide_nd = true;      // UNIPEAK_WIDE_ND=0: ... for nondirectional units only
    bool wide_q11 = true;     // UNIPEAK_WIDE_Q11=0: the replay instead of wide K1q
    bool wide_q11_nd = true;  // UNIPEAK_WIDE_Q11_ND=0: ... for nondirectional units, whatever up_set_wide_q11_nd says
    bool q11_replay = false;  // UNIPEAK_Q11_REPLAY=1: the replay for every threshold <= 0
    bool q11_heads_replay = false;  // UNIPEAK_Q11_HEADS=replay: no part of the route (run_q11's fallback for head units)
};

struct RouteIn {
    int bw;
    bool thr_pos;       // region threshold > 0
    bool coef_nonneg;   // every -z coefficient >= 0 (none given: true; a NaN: false)
    bool nondir;
    bool capture;       // the -w capture (up_set_profile_capture)
    bool wide_nd_full;  // up_set_wide_nd_full
    bool wide_q11_nd;   // up_set_wide_q11_nd
    int track_bits;     // 2 or 4 (UPK_TRACK_BITS)
    Switches sw;
};

struct Route {
    Scan scan;
    bool async_ok;    // a caller may enqueue the pass (up_run_async)
    bool profile_ok;  // the dense profile (up_unit_profile*) is available
};

// max_bw, max_wide_bw: the widest kernels of the narrow and of the wide scans (kernels.h kMaxBw, kMaxWideBw)
constexpr Route route_for(const RouteIn &in, int max_bw, int max_wide_bw) {
    const bool narrow = in.bw <= max_bw;
    // The wide scans assume a window of at most 65,535 cells: the reference
    // counts the cells add() retires in a UShort (misc/peakcall.cpp:172-177),
    // so from bw 32,768 on a gap of 2bw + 1 or more retires (gap mod 65,536)
    // cells, the rest of the window stays misaligned and a flush leaks into
    // the buffer's next unit -- only the whole-buffer replay models that.
    // They screen on the index planes, which 2-bit tracks have.
    const bool wide_ok = in.sw.wide && in.track_bits == 2 && in.bw <= max_wide_bw;
    Scan s = Scan::Replay;
    if (in.thr_pos) {
        // Directional K1w keeps the -w capture (head units hand their
        // retirements over from the K0 head replay, wide_profile_kernel gives
        // the dense rest); two strands only with up_set_wide_nd_full.
        if (narrow) s = Scan::K1;
        else if (wide_ok && (!in.nondir || (in.sw.wide_nd && (!in.capture || in.wide_nd_full)))) s = Scan::K1w;
    } else if (in.track_bits == 2 && in.coef_nonneg && !in.sw.q11_replay) {
        // A threshold <= 0 makes the leap branch of processPosition live
        // (quirk Q11: the leap position joins a region without setting its
        // left end).  With no negative coefficient no score is negative, every
        // processed position qualifies and the regions are the runs of
        // processed positions; otherwise only the state machine knows.
        // Narrow K1q takes its peaks from K3's KDE, whose window spans NH <= 8
        // words; wider, wide_peak_kernel finds them, with the -w capture off
        // (nothing hands a K1q pass's retirements over).  On two strands the
        // peaks are those of forwardScore + reverseScore and one region can
        // span a contig (launch_wide_corr_long): opt-in.
        if (narrow) s = Scan::K1q;
        else if (wide_ok && in.sw.wide_q11 && !in.capture && (!in.nondir || (in.wide_q11_nd && in.sw.wide_q11_nd)))
            s = Scan::K1qWide;
    }
    // The replay keeps no pass in flight and scores only what it retires.
    // K1w over two strands: its pass state is per slot (d_wcorr, d_wslab, the
    // correlation kernel on the pass stream, no captured graph), so nothing
    // needs the pass to block -- but two tests pin the refusals from when
    // these units replayed, so lifting them is opt-in (up_set_wide_nd_full).
    const bool ok = s != Scan::Replay && !(s == Scan::K1w && in.nondir && !in.wide_nd_full);
    // K1q passes run one at a time inside the blocking up_run: their records
    // are finished on the host (q11_finish) and K3's stage is the context's,
    // not the slot's (pipelined they measured slower).
    return Route{s, ok && !is_q11(s), ok};
}

}  // namespace upk
