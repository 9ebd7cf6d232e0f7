"""up_g6_to_float (csrc/fmt_g6.h): the float a reader of a -w line gets,
(float)strtod(snprintf("%g", v)), made from the six digits without any text --
the value rule of regions -W and the device's bigWig kernels.  Compared bit for
bit with libc: snprintf, strtod, and the cast to float (numpy.float32 of the
double, round to nearest even).  Runs on the CPU, no device.

The routine answers for 2^-67 <= |v| < 2^60 whose text D * 10^k has |k| <= 22
(k = the first digit's decimal exponent - 5); the digit routine's range gives
k in [-26, 13], so the refusals inside that range are exactly k < -22."""
import ctypes
import ctypes.util
import math

import numpy as np
import pytest

from unipeak_amd import capi
from tests.test_format_g6 import CARRIES

LO, HI = 2.0 ** -67, 2.0 ** 60  # the digit routine's range


@pytest.fixture(scope="module")
def libc_float():
    """(v) -> bits of (float)strtod(snprintf("%g", v)) by libc"""
    c = ctypes.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    c.snprintf.restype = ctypes.c_int
    c.snprintf.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_double]
    c.strtod.restype = ctypes.c_double
    c.strtod.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    buf = ctypes.create_string_buffer(64)

    def g(v):
        c.snprintf(buf, 64, b"%g", float(v))
        d = c.strtod(buf, None)
        assert d == float(b"%g" % v)  # Python's '%g' and float() are pinned to libc's here
        return int(np.float32(d).view(np.uint32))
    return g


@pytest.fixture(scope="module")
def conv():
    """(v) -> the float's bits, or None when refused"""
    L = capi.load_library()
    out, ok = ctypes.c_float(0), ctypes.c_int(0)
    po, pk = ctypes.byref(out), ctypes.byref(ok)
    view = ctypes.cast(ctypes.pointer(out), ctypes.POINTER(ctypes.c_uint32))

    def g(v):
        assert L.up_g6_to_float(v, po, pk) == 0
        if not ok.value:
            assert view[0] == 0
            return None
        return int(view[0])
    return g


def text_k(v):
    """k of the %g text D * 10^k of v"""
    return int(("%.5e" % abs(v)).split("e")[1]) - 5


def answered(v):
    a = abs(v)
    return LO <= a < HI and abs(text_k(v)) <= 22  # (NaN compares false)


def check(conv, libc_float, v):
    got = conv(v)
    if answered(v):
        want = libc_float(v)
        assert got == want, (v, float(v).hex(), got and hex(got), hex(want))
    else:
        assert got is None, (v, got)


def test_wrapper():
    assert capi.g6_to_float(1.5) == np.float32(1.5)
    assert capi.g6_to_float(-0.1234567) == np.float32(-0.123457)
    assert capi.g6_to_float(0.1234567) != np.float32(0.1234567)  # the text's value, not the score's
    assert capi.g6_to_float(0.0) is None and capi.g6_to_float(float("nan")) is None
    bits, ok = capi.g6_to_float_bits([2.5, 1e-30, -3.0])
    assert ok.tolist() == [True, False, True]
    assert bits.tolist() == [0x40200000, 0, 0xC0400000]


def test_carries_and_ties(conv, libc_float):
    for v in CARRIES:
        check(conv, libc_float, v)
        check(conv, libc_float, -v)
    assert conv(999999.5) == int(np.float32(1e6).view(np.uint32))
    assert conv(123457.5) == int(np.float32(123458.0).view(np.uint32))
    assert conv(100000.5) == int(np.float32(100000.0).view(np.uint32))
    # the ties of test_format_g6.py's (n + 0.5) * 10^j, a sample
    rng = np.random.default_rng(67)
    for n in rng.integers(100000, 1000000, 3000).tolist():
        for j in range(0, 7):
            v = float((2 * n + 1) * 10 ** j) / 2.0
            check(conv, libc_float, v)
            check(conv, libc_float, -v)
        if (2 * n + 1) % 5 == 0:
            check(conv, libc_float, float((2 * n + 1) // 5) / 4.0)  # j = -1


def test_powers_of_ten_and_two(conv, libc_float):
    for j in range(-24, 19):
        v = float("1e%d" % j)
        for x in (v, math.nextafter(v, 0.0), math.nextafter(v, math.inf)):
            check(conv, libc_float, x)
            check(conv, libc_float, -x)
    for x in range(-70, 63):
        v = math.ldexp(1.0, x)
        for y in (v, math.nextafter(v, 0.0), math.nextafter(v, math.inf)):
            check(conv, libc_float, y)


def test_texts_next_to_a_float_rounding_boundary(conv, libc_float):
    """texts D * 10^k whose double lies on, or within 2^10 double ulps of, the
    midpoint of two neighbouring floats: where the rounding to double and then to
    float (ties to even) decides the last bit"""
    D = np.arange(100000, 1000000, dtype=np.float64)
    picked = []
    for k in range(-22, 14):
        d = D * 10.0 ** k if k >= 0 else D / 10.0 ** -k  # one correctly rounded operation: the text's double
        low = d.view(np.uint64) & np.uint64((1 << 29) - 1)
        near = np.abs(low.astype(np.int64) - (1 << 28)) <= (1 << 10)
        picked += d[near].tolist()
    exact = [v for v in picked if (np.float64(v).view(np.uint64) & np.uint64((1 << 29) - 1)) == (1 << 28)]
    assert len(picked) > 100 and len(exact) > 20, (len(picked), len(exact))
    for v in picked:
        assert float("%g" % v) == v  # the double prints as its six digits
        for x in (v, math.nextafter(v, 0.0), math.nextafter(v, math.inf), -v):
            check(conv, libc_float, x)
    # the doubles around the midpoints of neighbouring floats themselves
    rng = np.random.default_rng(68)
    f = np.exp(rng.uniform(math.log(1e-17), math.log(1e17), 5000)).astype(np.float32)
    for a in f.tolist():
        m = (a + float(np.nextafter(np.float32(a), np.float32(np.inf)))) / 2.0  # exact in double
        for x in (m, math.nextafter(m, 0.0), math.nextafter(m, math.inf)):
            check(conv, libc_float, x)


def test_range_ends_and_refusals(conv, libc_float):
    # k = -22 is answered, k = -23 refused, on both sides of the step
    lo22 = 9.999995e-18  # prints as 1e-17: D = 100000, X = -17, k = -22
    assert text_k(lo22) == -22 and text_k(math.nextafter(lo22, 0.0)) == -23
    assert conv(lo22) == libc_float(lo22) and conv(-lo22) == libc_float(-lo22)
    assert conv(math.nextafter(lo22, 0.0)) is None
    for v in (1.00000e-17, 1.23456e-17, 9.99999e-17, 3e-17):
        assert text_k(v) == -22
        check(conv, libc_float, v)
        assert conv(v) is not None
    for v in (9.99999e-18, 5e-18, 1.5e-19, 1e-20, LO):
        assert text_k(v) <= -23 and conv(v) is None and conv(-v) is None
    # k = 13 at the top of the digit routine's range
    top = math.nextafter(HI, 0.0)
    assert text_k(top) == 13 and text_k(1e18) == 13
    for v in (1e18, 1.15292e18, top, -top):
        check(conv, libc_float, v)
        assert conv(v) is not None
    for v in (HI, 2e18, math.nextafter(LO, 0.0), 0.0, -0.0, 5e-324, 1e300, float("inf"), float("-inf")):
        assert conv(v) is None, v
    assert conv(float("nan")) is None


def test_random_sweep(libc_float):
    """1 million seeded doubles, log-uniform over the digit routine's range, both
    signs; the reference is vectorised through Python's '%g' and float(), which
    the fixture pins to libc's snprintf and strtod on a sample"""
    rng = np.random.default_rng(20261)
    n = 1_000_000
    v = np.exp(rng.uniform(math.log(LO), math.log(HI), n))
    v = np.clip(v, LO, math.nextafter(HI, 0.0))
    v[::2] = -v[::2]
    bits, ok = capi.g6_to_float_bits(v)
    vl = v.tolist()
    txt = [b"%g" % x for x in vl]
    want = np.array([float(t) for t in txt], np.float64).astype(np.float32).view(np.uint32)
    k = np.array([int(("%.5e" % abs(x)).split("e")[1]) - 5 for x in vl])
    inside = np.abs(k) <= 22
    assert inside.sum() > 0.8 * n and (~inside).sum() > 10_000
    assert np.array_equal(ok, inside)
    bad = np.flatnonzero(inside & (bits != want))
    assert bad.size == 0, [(vl[i], hex(bits[i]), hex(want[i])) for i in bad[:10]]
    assert not bits[~inside].any()
    for x in vl[:20000]:
        if answered(x):
            libc_float(x)  # (asserts libc's strtod == float() of the text)
