// tools/g6_sweep.cpp -- stand-alone host sweep of csrc/fmt_g6.h against
// snprintf("%g"): the carries and ties, powers of ten and two with their
// neighbours, every tie (n + 0.5) * 10^j of six-digit n for j = -3 .. 6, and N
// seeded log-uniform values over 1e-20 .. 1e18; and of g6_to_float against
// (float)strtod of that text on the same values (answered exactly for texts
// D * 10^k with |k| <= 22).  Exit status 1 on a difference.
//
//   g++ -O2 -std=c++17 -fsanitize=address,undefined -I unipeak_amd/csrc \
//       -o build/g6_sweep tools/g6_sweep.cpp && build/g6_sweep [N]
#include "fmt_g6.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

static long bad = 0, refused = 0, unanswered = 0;

static void chk(double v) {
    uint64_t b;
    memcpy(&b, &v, 8);
    char o[32];
    const int n = upk::g6_format(b, o);
    if (!n) {
        const double a = std::fabs(v);
        if (a >= 1e-20 && a < 1e18 && bad++ < 20) printf("refused inside the range: %a\n", v);
        ++refused;
        return;
    }
    o[n] = 0;
    char r[64];
    snprintf(r, sizeof r, "%g", v);
    uint32_t D;
    int X;
    bool neg;
    upk::g6_digits(b, &D, &X, &neg);
    if ((strcmp(o, r) || upk::g6_len(D, X, neg) != n || n > upk::kG6Max) && bad++ < 20)
        printf("%.17g: %s, snprintf %s\n", v, o, r);
    // the float a reader of the text gets
    uint32_t fb = 0, want;
    const bool ok = upk::g6_to_float(b, &fb);
    const float f = (float)strtod(r, nullptr);
    memcpy(&want, &f, 4);
    const bool inside = X - 5 >= -upk::kG6FloatMaxK && X - 5 <= upk::kG6FloatMaxK;
    if ((ok != inside || (ok && fb != want)) && bad++ < 20)
        printf("%.17g: float bits %08x (ok %d), strtod %08x\n", v, fb, (int)ok, want);
    if (!ok) ++unanswered;
}

int main(int argc, char **argv) {
    const long N = argc > 1 ? atol(argv[1]) : 30000000;
    const double sp[] = {999999.5, 0.00009999995, 9.999995, 123456.5, 123457.5, 1234565.0, 1e-4, 1e-5,
                         1e5, 1e6, 0.5, 1, 100000, 999999, 1e17, 1e-20, 1.5, 0.1, 0.2, 0.3};
    for (double v : sp) {
        chk(v);
        chk(-v);
    }
    for (int j = -20; j <= 17; ++j) {
        char s[16];
        snprintf(s, sizeof s, "1e%d", j);
        const double v = strtod(s, nullptr);
        chk(v);
        chk(std::nextafter(v, 0));
        chk(std::nextafter(v, 1e300));
    }
    for (int j = -3; j <= 6; ++j)
        for (long n = 100000; n <= 999999; ++n) chk((n + 0.5) * std::pow(10, j));  // (ties where exact)
    for (int x = -68; x <= 60; ++x) {
        chk(std::ldexp(1.0, x));
        chk(std::nextafter(std::ldexp(1.0, x), 0));
    }
    std::mt19937_64 g(1);
    std::uniform_real_distribution<double> u(std::log(1e-20), std::log(1e18));
    for (long i = 0; i < N; ++i) chk(std::exp(u(g)));
    printf("differences %ld, refused %ld (outside the range), no float for %ld (text below 1e-17)\n", bad, refused,
           unanswered);
    return bad != 0;
}
