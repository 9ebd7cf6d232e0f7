// tests/route_table.cpp -- csrc/route.h against the predicates it replaced
// (tests/test_route.py builds and runs this; plain C++, no HIP).
//
//   route_table                 every combination of the inputs: exit status 0
//                               if route_for agrees with the reference below
//                               row by row, else the first mismatching row
//   route_table ROW [ROW ...]   one line "scan async profile" per row; a row is
//                               a comma-separated list of key=value over the
//                               defaults (bw=1,thr=1, everything else as a
//                               fresh library context with no variable set)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../unipeak_amd/csrc/route.h"

using namespace upk;

// the bounds the enumeration straddles (kernels.h kMaxBw, kMaxWideBw)
constexpr int kMaxBw = 511, kMaxWideBw = 32767;

// ---- the reference: the seven predicates of api.hip before route.h, over
// the same inputs, with both "blocking pass in progress" flags clear
static bool q11_scores_ok(const RouteIn &c) {
    if (c.thr_pos || c.track_bits != 2) return false;
    if (!c.coef_nonneg) return false;
    return !c.sw.q11_replay;
}
static bool wide_mode(const RouteIn &c) {
    return c.sw.wide && c.bw > kMaxBw && c.bw <= kMaxWideBw && c.track_bits == 2 && c.thr_pos &&
           (!c.nondir || (c.sw.wide_nd && (!c.capture || c.wide_nd_full)));
}
static bool wide_nd_mode(const RouteIn &c) { return c.nondir && wide_mode(c); }
static bool wide_q11_mode(const RouteIn &c) {
    return c.sw.wide_q11 && c.sw.wide && q11_scores_ok(c) && c.bw > kMaxBw && c.bw <= kMaxWideBw &&
           (!c.nondir || (c.wide_q11_nd && c.sw.wide_q11_nd)) && !c.capture;
}
static bool q11_mode(const RouteIn &c) { return q11_scores_ok(c) && (c.bw <= kMaxBw || wide_q11_mode(c)); }
static bool replay_mode(const RouteIn &c) {
    return (c.bw > kMaxBw && !wide_mode(c) && !wide_q11_mode(c)) || (!c.thr_pos && !q11_mode(c));
}
static bool check_runnable(const RouteIn &c, bool profile) {
    if (replay_mode(c)) return false;
    if (profile && c.bw > kMaxBw && !wide_mode(c) && !wide_q11_mode(c)) return false;
    if (wide_nd_mode(c) && !c.wide_nd_full) return false;
    return !(q11_mode(c) && !profile);
}
// up_run's order: the replay, then K1q, then the bandwidth
static Route reference(const RouteIn &c) {
    const Scan s = replay_mode(c) ? Scan::Replay
                   : q11_mode(c)  ? (c.bw <= kMaxBw ? Scan::K1q : Scan::K1qWide)
                   : c.bw > kMaxBw ? Scan::K1w
                                   : Scan::K1;
    return Route{s, check_runnable(c, false), check_runnable(c, true)};
}
// ----

static const char *name(Scan s) {
    switch (s) {
    case Scan::K1: return "K1";
    case Scan::K1w: return "K1w";
    case Scan::K1q: return "K1q";
    case Scan::K1qWide: return "K1qWide";
    default: return "Replay";
    }
}

static void print_row(FILE *f, const RouteIn &c) {
    fprintf(f, "bw=%d,thr=%d,neg=%d,nondir=%d,capture=%d,wide_nd_full=%d,wide_q11_nd=%d,bits=%d,WIDE=%d,WIDE_ND=%d,"
               "WIDE_Q11=%d,WIDE_Q11_ND=%d,Q11_REPLAY=%d,Q11_HEADS=%d",
            c.bw, c.thr_pos, !c.coef_nonneg, c.nondir, c.capture, c.wide_nd_full, c.wide_q11_nd, c.track_bits,
            c.sw.wide, c.sw.wide_nd, c.sw.wide_q11, c.sw.wide_q11_nd, c.sw.q11_replay, c.sw.q11_heads_replay);
}

static int enumerate() {
    const int bws[] = {1, 511, 512, 32767, 32768, 65535};
    long rows = 0;
    for (int bw : bws)
        for (int bits = 2; bits <= 4; bits += 2)
            for (unsigned m = 0; m < (1u << 12); ++m) {
                auto bit = [&](int i) { return ((m >> i) & 1u) != 0; };
                RouteIn c{};
                c.bw = bw;
                c.track_bits = bits;
                c.thr_pos = bit(0);
                c.coef_nonneg = bit(1);
                c.nondir = bit(2);
                c.capture = bit(3);
                c.wide_nd_full = bit(4);
                c.wide_q11_nd = bit(5);
                c.sw.wide = bit(6);
                c.sw.wide_nd = bit(7);
                c.sw.wide_q11 = bit(8);
                c.sw.wide_q11_nd = bit(9);
                c.sw.q11_replay = bit(10);
                c.sw.q11_heads_replay = bit(11);
                const Route got = route_for(c, kMaxBw, kMaxWideBw), want = reference(c);
                ++rows;
                if (got.scan != want.scan || got.async_ok != want.async_ok || got.profile_ok != want.profile_ok) {
                    print_row(stdout, c);
                    printf(": route_for %s %d %d, the reference %s %d %d\n", name(got.scan), got.async_ok,
                           got.profile_ok, name(want.scan), want.async_ok, want.profile_ok);
                    return 1;
                }
            }
    printf("%ld rows agree\n", rows);
    return 0;
}

static bool parse_row(const char *arg, RouteIn &c) {
    c = RouteIn{};
    c.bw = 1;
    c.thr_pos = true;
    c.coef_nonneg = true;
    c.track_bits = 2;
    std::string s(arg);
    size_t at = 0;
    while (at < s.size()) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        const std::string kv = s.substr(at, end - at);
        at = end + 1;
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) return false;
        const std::string k = kv.substr(0, eq);
        const int v = atoi(kv.c_str() + eq + 1);
        if (k == "bw") c.bw = v;
        else if (k == "thr") c.thr_pos = v != 0;
        else if (k == "neg") c.coef_nonneg = v == 0;
        else if (k == "nondir") c.nondir = v != 0;
        else if (k == "capture") c.capture = v != 0;
        else if (k == "wide_nd_full") c.wide_nd_full = v != 0;
        else if (k == "wide_q11_nd") c.wide_q11_nd = v != 0;
        else if (k == "bits") c.track_bits = v;
        else if (k == "WIDE") c.sw.wide = v != 0;
        else if (k == "WIDE_ND") c.sw.wide_nd = v != 0;
        else if (k == "WIDE_Q11") c.sw.wide_q11 = v != 0;
        else if (k == "WIDE_Q11_ND") c.sw.wide_q11_nd = v != 0;
        else if (k == "Q11_REPLAY") c.sw.q11_replay = v != 0;
        else if (k == "Q11_HEADS") c.sw.q11_heads_replay = v != 0;
        else return false;
    }
    return true;
}

int main(int argc, char **argv) {
    static_assert(scan_kind(Scan::K1) == 0 && scan_kind(Scan::K1w) == 1 && scan_kind(Scan::K1q) == 2 &&
                      scan_kind(Scan::K1qWide) == 2 && scan_kind(Scan::Replay) == 3,
                  "the integers of up_last_scan_kind");
    if (argc == 1) return enumerate();
    for (int i = 1; i < argc; ++i) {
        RouteIn c;
        if (!parse_row(argv[i], c)) {
            fprintf(stderr, "route_table: bad row '%s'\n", argv[i]);
            return 2;
        }
        const Route r = route_for(c, kMaxBw, kMaxWideBw);
        printf("%s %d %d\n", name(r.scan), r.async_ok, r.profile_ok);
    }
    return 0;
}
