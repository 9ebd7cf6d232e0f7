// unipeak_amd/csrc/fmt_g6.h -- printf("%g", v) for doubles, the same routine on
// the host (up_format_g6) and on the device (proftext.hip): six significant
// digits correctly rounded from the exact binary value, ties to even, in
// integer arithmetic only -- no libm, no printf, no floating-point operation
// on the value at all.
//
// Range.  g6_digits() formats every finite v with 2^-67 <= |v| < 2^60 (that
// contains 1e-20 <= |v| < 1e18) and reports "not formatted" for everything
// else: zero, subnormals, smaller and larger magnitudes, NaN, infinities.
//
// Exactness.  v = m * 2^e with m a 53-bit integer.  x = e + 52 is floor(log2
// v), so E0 = floor(x * log10 2) satisfies 10^E0 <= 2^x <= v < 2^(x+1) <
// 10^(E0+2): the decimal exponent E is E0 or E0 + 1.
//  * E0 <= 5: k = 5 - E0 is in [0, 26].  P = m * 5^k < 2^53 * 2^61 is exact in
//    128 bits and v * 10^k = P / 2^s with s = -(e + k) in [29, 97], a value in
//    [1e5, 1e7).  I = P >> s is its integer part and the s bits shifted out
//    are its fraction, compared against 2^(s-1) exactly.  When I >= 1e6 the
//    exponent is E0 + 1 and the six digits are I / 10: the dropped digit and
//    "fraction != 0" decide the rounding.
//  * E0 >= 6: v < 2^60 has the integer part N = m * 2^e (a shift) in 64 bits
//    and, for e < 0, a fraction that only matters as "!= 0".  With j = E - 5
//    (E = E0 + 1 exactly when N >= 10^(E0+1)), the digits are N / 10^j and the
//    remainder N % 10^j is compared against 10^j / 2, an integer.
// Both ways a round-up to 1,000,000 becomes 100000 with the exponent one
// higher, which is how 999999.5 prints as 1e+06 and 9.999995 as 10.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UPK_HD __host__ __device__
#else
#define UPK_HD
#endif

namespace upk {

constexpr int kG6Max = 12;  // longest output: "-1.23456e-05", "-0.000123456"

UPK_HD inline uint64_t g6_pow5(int k) {  // 5^k, k = 0..27
    constexpr uint64_t t[28] = {1ull,
                                5ull,
                                25ull,
                                125ull,
                                625ull,
                                3125ull,
                                15625ull,
                                78125ull,
                                390625ull,
                                1953125ull,
                                9765625ull,
                                48828125ull,
                                244140625ull,
                                1220703125ull,
                                6103515625ull,
                                30517578125ull,
                                152587890625ull,
                                762939453125ull,
                                3814697265625ull,
                                19073486328125ull,
                                95367431640625ull,
                                476837158203125ull,
                                2384185791015625ull,
                                11920928955078125ull,
                                59604644775390625ull,
                                298023223876953125ull,
                                1490116119384765625ull,
                                7450580596923828125ull};
    return t[k];
}

UPK_HD inline uint64_t g6_pow10(int k) {  // 10^k, k = 0..19
    constexpr uint64_t t[20] = {1ull,
                                10ull,
                                100ull,
                                1000ull,
                                10000ull,
                                100000ull,
                                1000000ull,
                                10000000ull,
                                100000000ull,
                                1000000000ull,
                                10000000000ull,
                                100000000000ull,
                                1000000000000ull,
                                10000000000000ull,
                                100000000000000ull,
                                1000000000000000ull,
                                10000000000000000ull,
                                100000000000000000ull,
                                1000000000000000000ull,
                                10000000000000000000ull};
    return t[k];
}

// The six digits D (100000..999999), the decimal exponent X of the first one
// and the sign of v, given as its IEEE-754 bits.  false: not formatted here.
UPK_HD inline bool g6_digits(uint64_t bits, uint32_t *D, int *X, bool *neg) {
    *neg = (bits >> 63) != 0;
    const int be = (int)((bits >> 52) & 0x7ff);
    const int x = be - 1023;  // floor(log2 |v|) of a normal number
    if (x < -67 || x > 59) return false;  // (zero, subnormals, NaN and infinities: be = 0 / 2047)
    const uint64_t m = (bits & 0xfffffffffffffull) | (1ull << 52);
    const int e = x - 52;
    int E = (x * 78913) >> 18;  // floor(x * log10 2), |x| <= 67 (arithmetic shift)
    uint32_t d;
    int up;  // the dropped part against one half: -1 below, 0 a tie, 1 above
    if (E <= 5) {
        const int k = 5 - E;
        const unsigned __int128 P = (unsigned __int128)m * g6_pow5(k);
        const int s = -(e + k);
        const uint32_t I = (uint32_t)(uint64_t)(P >> s);  // < 1e7
        const unsigned __int128 frac = P & ((((unsigned __int128)1) << s) - 1);
        const unsigned __int128 half = ((unsigned __int128)1) << (s - 1);
        if (I >= 1000000u) {
            ++E;
            d = I / 10u;
            const uint32_t last = I - d * 10u;
            up = last > 5u ? 1 : last < 5u ? -1 : frac != 0 ? 1 : 0;
        } else {
            d = I;
            up = frac > half ? 1 : frac < half ? -1 : 0;
        }
    } else {
        uint64_t N;
        bool sticky = false;
        if (e >= 0) {
            N = m << e;
        } else {
            N = m >> -e;
            sticky = (m & ((1ull << -e) - 1)) != 0;
        }
        if (N >= g6_pow10(E + 1)) ++E;
        const uint64_t p = g6_pow10(E - 5);
        const uint64_t q = N / p, rem = N - q * p, half = p >> 1;
        d = (uint32_t)q;
        up = rem > half ? 1 : rem < half ? -1 : sticky ? 1 : 0;
    }
    if (up > 0 || (up == 0 && (d & 1u))) ++d;
    if (d == 1000000u) {
        d = 100000u;
        ++E;
    }
    *D = d;
    *X = E;
    return true;
}

// significant digits of D that %g keeps (trailing zeros dropped), 1..6
UPK_HD inline int g6_ndig(uint32_t D) {
    int n = 6;
    while (n > 1 && D % 10u == 0) {
        D /= 10u;
        --n;
    }
    return n;
}

// bytes of the %g text of (D, X, neg)
UPK_HD inline int g6_len(uint32_t D, int X, bool neg) {
    const int n = g6_ndig(D);
    int len = neg ? 1 : 0;
    if (X >= -4 && X < 6) {
        if (X >= 0) len += (X + 1) + (n > X + 1 ? 1 + n - (X + 1) : 0);
        else len += 2 + (-X - 1) + n;
    } else {
        const int ax = X < 0 ? -X : X;
        len += 1 + (n > 1 ? n : 0) + 2 + (ax >= 100 ? 3 : 2);
    }
    return len;
}

// the %g text of (D, X, neg) into out (no terminator); returns its length
template <typename Ptr>
UPK_HD inline int g6_put(Ptr out, uint32_t D, int X, bool neg) {
    uint64_t packed = 0;  // digit i in byte i: no indexed array, so nothing lives in scratch
    {
        uint32_t t = D;
        for (int i = 5; i >= 0; --i) {
            packed |= (uint64_t)('0' + t % 10u) << (8 * i);
            t /= 10u;
        }
    }
#define UPK_G6_DIG(i) ((char)((packed >> (8 * (i))) & 0xff))
    const int n = g6_ndig(D);
    int o = 0;
    if (neg) out[o++] = '-';
    if (X >= -4 && X < 6) {
        if (X >= 0) {
            for (int i = 0; i <= X; ++i) out[o++] = UPK_G6_DIG(i);
            if (n > X + 1) {
                out[o++] = '.';
                for (int i = X + 1; i < n; ++i) out[o++] = UPK_G6_DIG(i);
            }
        } else {
            out[o++] = '0';
            out[o++] = '.';
            for (int i = 0; i < -X - 1; ++i) out[o++] = '0';
            for (int i = 0; i < n; ++i) out[o++] = UPK_G6_DIG(i);
        }
    } else {
        out[o++] = UPK_G6_DIG(0);
        if (n > 1) {
            out[o++] = '.';
            for (int i = 1; i < n; ++i) out[o++] = UPK_G6_DIG(i);
        }
        out[o++] = 'e';
        int ax = X;
        if (X < 0) {
            out[o++] = '-';
            ax = -X;
        } else {
            out[o++] = '+';
        }
        if (ax >= 100) out[o++] = (char)('0' + ax / 100);
        out[o++] = (char)('0' + (ax / 10) % 10);
        out[o++] = (char)('0' + ax % 10);
    }
#undef UPK_G6_DIG
    return o;
}

// printf("%g", v) of the double with these bits into out (at most kG6Max
// bytes, no terminator); 0: outside the range g6_digits formats
UPK_HD inline int g6_format(uint64_t bits, char *out) {
    uint32_t D;
    int X;
    bool neg;
    if (!g6_digits(bits, &D, &X, &neg)) return 0;
    return g6_put(out, D, X, neg);
}

// ---- the float a reader of the %g text gets: (float)strtod("<%g of v>")
//
// The text's value is D * 10^k with k = X - 5.  For |k| <= 22 both D (< 2^20)
// and 10^|k| (5^22 < 2^52) are exact doubles, so one IEEE multiply (k >= 0) or
// one IEEE divide (k < 0) returns the double nearest to D * 10^k -- what a
// correctly rounding strtod returns for that text -- and the conversion to
// float rounds that double to nearest even, as the reader's cast does (its
// double rounding is part of the result).  No text is made.  The digit
// routine's range gives k in [-26, 13]; k < -22 (|v| below about 1e-17) is
// refused.  Needs a real FP64 multiply / divide: no fast-math, no contraction.

UPK_HD inline double g6_pow10d(int k) {  // 10^k, k = 0..22, each exact
    constexpr double t[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                              1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    return t[k];
}

constexpr int kG6FloatMaxK = 22;

// the float (as bits) of the text of (D, X, neg); false: |X - 5| > 22
UPK_HD inline bool g6_digits_to_float(uint32_t D, int X, bool neg, uint32_t *fbits) {
    const int k = X - 5;
    if (k < -kG6FloatMaxK || k > kG6FloatMaxK) return false;
    const double d = k >= 0 ? (double)D * g6_pow10d(k) : (double)D / g6_pow10d(-k);
    const float f = (float)d;
    union {
        float f;
        uint32_t u;
    } c;
    c.f = neg ? -f : f;
    *fbits = c.u;
    return true;
}

// (float)strtod(printf("%g", v)) of the double with these bits, as the float's
// bits; false: outside g6_digits' range, or its text is below 1e-17
UPK_HD inline bool g6_to_float(uint64_t bits, uint32_t *fbits) {
    uint32_t D;
    int X;
    bool neg;
    if (!g6_digits(bits, &D, &X, &neg)) return false;
    return g6_digits_to_float(D, X, neg, fbits);
}

}  // namespace upk
