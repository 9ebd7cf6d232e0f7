"""up_format_g6 (csrc/fmt_g6.h), the digit routine the device's -w formatter
runs, against libc's snprintf("%g") -- and Python's '%g' against libc too,
since the GPU tests build their reference text with it.

The routine states its range as 2^-67 <= |v| < 2^60 (it contains 1e-20 <=
|v| < 1e18): inside it every value must come back formatted and equal to
libc's bytes, outside it the answer is None."""
import ctypes
import ctypes.util
import math
from fractions import Fraction

import numpy as np
import pytest

from unipeak_amd import capi

LO, HI = 2.0 ** -67, 2.0 ** 60  # the range fmt_g6.h states


@pytest.fixture(scope="module")
def libc():
    c = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    c.snprintf.restype = ctypes.c_int
    c.snprintf.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_double]
    buf = ctypes.create_string_buffer(64)

    def g(v):
        n = c.snprintf(buf, 64, b"%g", float(v))
        return buf.raw[:n]
    return g


@pytest.fixture(scope="module")
def fmt():
    """format_g6 without the per-call wrapper cost: (v) -> bytes or None"""
    L = capi.load_library()
    buf = ctypes.create_string_buffer(16)
    n = ctypes.c_int(0)
    ref = ctypes.byref(n)
    f = L.up_format_g6

    def g(v):
        assert f(v, buf, ref) == 0
        return buf.raw[:n.value] if n.value else None
    return g


def check(fmt, libc, v):
    """inside the stated range: libc's bytes, never None; outside: None"""
    got = fmt(v)
    want = libc(v)
    assert want == ("%g" % v).encode(), v  # the GPU tests' yardstick is libc's
    a = abs(v)
    if LO <= a < HI:  # (NaN compares false)
        assert got == want, (v, float(v).hex(), got, want)
        assert len(got) <= 12
    else:
        assert got is None, (v, got)


def test_wrapper_and_symbol():
    assert capi.format_g6(1.5) == b"1.5"
    assert capi.format_g6(-0.25) == b"-0.25"
    assert capi.format_g6(0.0) is None
    assert capi.format_g6(float("nan")) is None


CARRIES = {999999.5: b"1e+06", 0.00009999995: b"0.0001", 9.999995: b"10",
           123456.5: b"123456", 123457.5: b"123458", 1234565.0: b"1.23456e+06"}


def test_carries_and_ties(fmt, libc):
    for v, s in CARRIES.items():
        assert fmt(v) == s, v
        assert fmt(-v) == b"-" + s, v
        check(fmt, libc, v)
        check(fmt, libc, -v)


def test_powers_of_ten_and_neighbours(fmt, libc):
    for j in range(-20, 18):
        v = float("1e%d" % j)
        for x in (v, math.nextafter(v, 0.0), math.nextafter(v, math.inf)):
            check(fmt, libc, x)
            check(fmt, libc, -x)
            if x >= 1e-20:  # the least the routine has to format itself
                assert fmt(x) is not None
    for v in (1e-4, 1e-5, 1e5, 1e6):  # notation boundaries
        for x in (v, math.nextafter(v, 0.0), math.nextafter(v, math.inf)):
            check(fmt, libc, x)
    assert fmt(1e-4) == b"0.0001" and fmt(1e-5) == b"1e-05"
    assert fmt(1e5) == b"100000" and fmt(1e6) == b"1e+06"
    assert fmt(math.nextafter(1e-4, 0.0)) == b"0.0001"  # rounds back up into fixed notation
    assert fmt(999999.4) == b"999999"


def test_powers_of_two(fmt, libc):
    for x in range(-70, 63):
        v = math.ldexp(1.0, x)
        for y in (v, math.nextafter(v, 0.0), math.nextafter(v, math.inf)):
            check(fmt, libc, y)


def test_exact_ties(fmt, libc):
    """(n + 0.5) * 10^j, j = -3 .. 6, for six-digit n wherever that value is a
    double: always for j >= 0 (an integer or half-integer below 2^53), for j < 0
    when 5^-j divides 2n + 1.  A sample of n plus both ends of the decade."""
    rng = np.random.default_rng(66)
    ns = np.unique(np.concatenate([rng.integers(100000, 1000000, 20000),
                                   np.arange(100000, 100200), np.arange(999800, 1000000)])).tolist()
    seen = {j: 0 for j in range(-3, 7)}
    for j in range(-3, 7):
        for n in ns:
            num = 2 * n + 1  # the tie is num * 10^j / 2
            if j >= 0:
                v = float(num * 10 ** j) / 2.0
            else:
                if num % 5 ** -j:
                    continue
                v = float(num // 5 ** -j) / 2.0 ** (1 - j)
            assert Fraction(v) == Fraction(num) * Fraction(10) ** j / 2
            seen[j] += 1
            check(fmt, libc, v)
            check(fmt, libc, -v)
    assert all(k > 100 for k in seen.values()), seen
    # ties to even, spelled out
    assert fmt(100000.5) == b"100000" and fmt(100001.5) == b"100002"
    assert fmt(0.5 * 1.0) == b"0.5" and fmt(2500000.0 + 0.0) == b"2.5e+06"
    assert fmt(1000005.0) == b"1e+06" and fmt(1000015.0) == b"1.00002e+06"
    assert fmt(100.0005) == libc(100.0005)


def test_outside_the_range(fmt, libc):
    for v in (2.2250738585072014e-308, 5e-324, 1e300, float("inf"), float("-inf"), 0.0, -0.0,
              1e-21, 2e18, math.nextafter(LO, 0.0), HI):
        assert fmt(v) is None, v
    assert fmt(float("nan")) is None
    assert fmt(LO) is not None and fmt(math.nextafter(HI, 0.0)) is not None
    check(fmt, libc, LO)
    check(fmt, libc, math.nextafter(HI, 0.0))


def test_random_sweep(fmt, libc):
    """2 million seeded doubles, log-uniform over the stated range, both signs;
    libc's own formatting is vectorised through Python's '%g' being pinned to it
    above, so the sweep compares with '%g' and spot-checks libc"""
    rng = np.random.default_rng(20260)
    n = 2_000_000
    v = np.exp(rng.uniform(math.log(LO), math.log(HI), n))
    v = np.clip(v, LO, math.nextafter(HI, 0.0))
    v[::2] = -v[::2]
    L = capi.load_library()
    f = L.up_format_g6
    buf = ctypes.create_string_buffer(16)
    k = ctypes.c_int(0)
    ref = ctypes.byref(k)
    bad = []
    for x in v.tolist():
        f(x, buf, ref)
        if buf.raw[:k.value] != b"%g" % x:
            bad.append(x)
    assert not bad, [(x, fmt(x), "%g" % x) for x in bad[:10]]
    for x in v[:20000].tolist():
        assert libc(x) == b"%g" % x
