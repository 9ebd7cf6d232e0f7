"""The dense profile, the -w capture and pipelined passes of nondirectional
units at bandwidths 512..32767 (a threshold > 0), opted into per context with
up_set_wide_nd_full: wide_profile_kernel<POOL, true> (csrc/wide.hip) behind
up_unit_profile / up_unit_profile_range, K1w with the capture on (head units
hand over the K0 head replay's retirements), up_run_async admitted.  With the
switch off everything stays as tests/test_gpu_replay.py and
tests/test_gpu_wide_nondir.py pin it.

Every score bit for bit (tobytes): f against the oracle's profile of the
forward counts alone, r against that of the reverse counts alone, f + r
(numpy FP64) against the oracle's nondirectional profile; past len against
the ascending sum of tests/test_gpu_wide_profile.py; bin/regions -w byte for
byte against the oracle CLI.  A strip is 16,384 positions, a stretch of the
profile kernel 4,096; contigs of 60,000 positions except at bw 32,767.
tests/test_wide_nd_profile_oracle.py shows on the CPU that the inputs hold
what the cases rely on."""
import os

import numpy as np
import pytest

from tests import wide_nd_inputs as W
from tests import wide_nd_profile_inputs as I
from tests.test_cli import BIN, make_inputs, run
from tests.test_gpu_replay import compare
from tests.test_gpu_wide_profile import ascending_sum

pytestmark = pytest.mark.gpu

K1W = 1  # up_last_scan_kind
_refs = {}


def refs(oracle, key, bw, bg, unit, **kw):
    """strand_refs of a unit, computed once per key and shared (read-only)"""
    if key not in _refs:
        _refs[key] = I.strand_refs(oracle, bw, bg, *unit, **kw)
    return _refs[key]


def load(g, unit):
    length, pos, cf, cr = unit
    u = g.add_unit(length)
    for st, c in enumerate((cf, cr)):
        for s in range(c.shape[1]):
            m = c[:, s] != 0
            if m.any():
                g.scatter(u, st, s, pos[m], c[m, s])
    return u


def setup(g, bw, bg, unit, full=True, capture=False, **kw):
    g.set_params(bw, unit[2].shape[1], bg, nondir=True, **kw)
    if full:
        g.set_wide_nd_full(True)
    if capture:
        g.set_profile_capture(True)
    return load(g, unit)


def whole_profile(capi, bw, bg, unit, **kw):
    with capi.Lib(0) as g:
        u = setup(g, bw, bg, unit, **kw)
        return g.profile(u, unit[0])


def check(f, r, ref):
    rf, rr, both = ref
    assert f.tobytes() == rf.tobytes()
    assert r.tobytes() == rr.tobytes()
    assert (f + r).tobytes() == both.tobytes()


# ---- 1. parity ------------------------------------------------------------------

@pytest.mark.parametrize("bw", sorted(I.PARITY_SEEDS))
def test_parity(gpu_lib, oracle, bw):
    unit = I.parity_unit(bw)
    f, r = whole_profile(gpu_lib, bw, W.BG, unit)
    assert r.any()
    check(f, r, refs(oracle, ("parity", bw), bw, W.BG, unit))


# ---- 2. refusals keep their shape -------------------------------------------------

def test_refusals(gpu_lib):
    capi = gpu_lib
    unit = I.parity_unit(700)
    with capi.Lib(0) as g:  # the switch off: as before
        u = setup(g, 700, W.BG, unit, full=False)
        assert g.run() >= 0 and g.last_scan_kind() == K1W
        with pytest.raises(capi.UpError):
            g.profile(u, unit[0])
        with pytest.raises(capi.UpError):
            g.run_async()
    with capi.Lib(0) as g:  # the switch on: bw 32,768 and a threshold of 0 stay outside
        u = setup(g, 700, W.BG, unit)
        g.profile(u, unit[0])
        g.set_params(32768, 1, W.BG, nondir=True)
        with pytest.raises(capi.UpError):
            g.profile(u, unit[0])
        g.set_params(700, 1, W.BG, nondir=True, region_thr=0.0)
        with pytest.raises(capi.UpError):
            g.profile(u, unit[0])


# ---- 3. ranges ---------------------------------------------------------------------

def test_ranges(gpu_lib, oracle):
    bw = I.RANGE_BW
    unit = I.tail_unit()
    length, pos, cf, cr = unit
    rf, rr, _ = refs(oracle, "tail", bw, W.BG, unit)
    kern = oracle.kernel(bw, 1.0 / W.BG)
    tails = []
    for c in (cf, cr):
        m = c[:, 0] != 0
        tails.append(ascending_sum(kern, bw, length, pos[m], c[m, 0], range(length + 1, length + bw + 1)))
        assert np.count_nonzero(tails[-1]) > 0
    dom = -(-(length + bw) // W.STRIP) * W.STRIP  # whole strips covering [1, len + bw]
    with gpu_lib.Lib(0) as g:
        u = setup(g, bw, W.BG, unit)
        # mid-word, across a strip edge, a single position (in the scores and at position 1)
        for first, count in ((4_100, 64), (16_380, 100), (33_000, 1), (1, 1)):
            f, r = g.profile_range(u, first, count)
            assert f.tobytes() == rf[first - 1:first - 1 + count].tobytes(), (first, count)
            assert r.tobytes() == rr[first - 1:first - 1 + count].tobytes(), (first, count)
        # ... ending at len + bw: the contig's tail, then the flush's positions
        first = length - 300
        f, r = g.profile_range(u, first, length + bw - first + 1)
        for got, ref, tail in ((f, rf, tails[0]), (r, rr, tails[1])):
            assert got[:301].tobytes() == ref[first - 1:].tobytes()
            assert got[301:].tobytes() == tail.tobytes()
        # ... and to the end of the scan domain: exactly 0.0 above len + bw
        first = length + bw - 50
        f, r = g.profile_range(u, first, dom - first + 1)
        for got, tail in ((f, tails[0]), (r, tails[1])):
            assert got[:51].tobytes() == tail[-51:].tobytes()
            assert got.size > 51 and got[51:].tobytes() == bytes(8 * (got.size - 51))


# ---- 4. one-strand windows ------------------------------------------------------------

def test_one_strand_windows(gpu_lib, oracle):
    """a screen on strand 0's plane alone would leave the reverse-only
    windows at 0.0"""
    bw = W.ONE_STRAND_BW
    unit = W.one_strand_unit()
    f, r = whole_profile(gpu_lib, bw, W.BG, unit)
    a, b = slice(15_000 - 300, 15_000 + 300), slice(40_000 - 300, 40_000 + 300)
    assert f[a].all() and r[a].tobytes() == bytes(8 * 600)
    assert r[b].all() and f[b].tobytes() == bytes(8 * 600)
    check(f, r, refs(oracle, "one_strand", bw, W.BG, unit))


# ---- 5. branches ------------------------------------------------------------------------

def test_branches(gpu_lib, oracle):
    """one stretch whose forward windows overflow the hit list (the fallback
    walk) while its reverse windows use it; escaped counts; a saturated
    reverse chunk (hit counts: tests/test_wide_nd_profile_oracle.py)"""
    bw = W.STRESS_BW
    unit = W.stress_unit()
    f, r = whole_profile(gpu_lib, bw, W.BG, unit)
    check(f, r, refs(oracle, "stress", bw, W.BG, unit))


# ---- 6. pooling ---------------------------------------------------------------------------

@pytest.mark.parametrize("coeffs", I.POOL_COEFFS)
def test_pooled(gpu_lib, oracle, coeffs):
    unit = I.pooled_unit()
    kw = dict(control=I.POOL_CONTROL, coeffs=coeffs)
    f, r = whole_profile(gpu_lib, 700, W.BG, unit, **kw)
    assert r.any()
    check(f, r, refs(oracle, ("pooled", str(coeffs)), 700, W.BG, unit, **kw))


# ---- 7. the widest kernel --------------------------------------------------------------------

def test_widest_kernel(gpu_lib, oracle):
    capi = gpu_lib
    bw = W.LIMIT_BW
    unit = W.limit_unit()
    with capi.Lib(0) as g:
        u = setup(g, bw, W.LIMIT_BG, unit)
        f, r = g.profile(u, unit[0])
        check(f, r, refs(oracle, "limit", bw, W.LIMIT_BG, unit))
        g.set_params(bw + 1, 1, W.LIMIT_BG, nondir=True)
        with pytest.raises(capi.UpError):
            g.profile(u, unit[0])


# ---- 8. capture without heads ------------------------------------------------------------------

def test_capture_without_heads(gpu_lib, oracle):
    """K1w's records with the capture on (not the whole-buffer replay's), no
    unit replayed, the dense profile, two pipelined passes"""
    bw = 700
    unit = I.parity_unit(bw)
    length, pos, cf, cr = unit
    ref, ref_sums = oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    assert len(ref) > 0
    with gpu_lib.Lib(0) as g:
        u = setup(g, bw, W.BG, unit, capture=True, corr_thr=0.3, want_corr=True)
        n = g.run()
        assert g.last_scan_kind() == K1W
        regs, k = g.regions(n)
        regs, k = regs.copy(), k.copy()
        compare(ref, ref_sums, regs, k, corr=True)
        resync, ev, p, sc = g.replay_profile(u)
        assert resync == 0 and ev.size == 0 and p.size == 0 and sc.size == 0
        f, r = g.profile(u, length)
        check(f, r, refs(oracle, ("parity", bw), bw, W.BG, unit))
        g.run_async()
        g.run_async()
        for _ in range(2):
            n = g.run_wait()
            assert g.last_scan_kind() == K1W
            regs2, k2 = g.regions(n)
            assert regs2.tobytes() == regs.tobytes() and k2.tobytes() == k.tobytes()


# ---- 9. capture with a head unit ----------------------------------------------------------------

def test_capture_with_a_head_unit(gpu_lib, oracle):
    """tags at positions <= bw on the reverse strand (quirk Q1): the K0 head
    replay hands over its retirements (f + r) up to its resync point, the
    dense profile serves the rest"""
    bw = I.HEAD_BW
    unit = I.head_gap_unit()
    length, pos, cf, cr = unit
    ref, ref_sums = oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    prof = oracle.profile(bw, W.BG, length, pos, cf, cr, nondir=True)
    with gpu_lib.Lib(0) as g:
        u = setup(g, bw, W.BG, unit, capture=True, corr_thr=0.3, want_corr=True)
        n = g.run()
        assert g.last_scan_kind() == K1W
        regs, k = g.regions(n)
        compare(ref, ref_sums, regs, k, corr=True)
        resync, ev, p, sc = g.replay_profile(u)
        assert bw < resync <= length  # (not UP_FLUSH_EVENT: the head replay resynced)
        nzp = np.flatnonzero(prof[:resync - 1])
        assert nzp.size > 0
        assert np.array_equal(p, nzp + 1)
        assert sc.tobytes() == prof[nzp].tobytes()
        f, r = g.profile_range(u, resync, length - resync + 1)
        assert r.any()
        assert (f + r).tobytes() == prof[resync - 1:].tobytes()


# ---- 10. pipelined passes alone --------------------------------------------------------------------

def test_pipelined_passes(gpu_lib, oracle):
    """MAX_IN_FLIGHT passes in flight over two units, the correlation wanted:
    every pass delivers the blocking pass's records"""
    capi = gpu_lib
    bw = 700
    units = [I.parity_unit(bw), I.tail_unit()]
    with capi.Lib(0) as g:
        setup(g, bw, W.BG, units[0], corr_thr=0.3, want_corr=True)
        load(g, units[1])
        n = g.run()
        assert g.last_scan_kind() == K1W
        regs, k = g.regions(n)
        regs, k = regs.copy(), k.copy()
        for u, (length, pos, cf, cr) in enumerate(units):
            ref, ref_sums = oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
            m = regs["unit"] == u
            assert len(ref) > 0
            compare(ref, ref_sums, regs[m], k[m], corr=True)
        for _ in range(capi.MAX_IN_FLIGHT):
            g.run_async()
        for _ in range(capi.MAX_IN_FLIGHT):
            n = g.run_wait()
            assert g.last_scan_kind() == K1W
            regs2, k2 = g.regions(n)
            assert regs2.tobytes() == regs.tobytes() and k2.tobytes() == k.tobytes()


# ---- 11. CLI -----------------------------------------------------------------------------------------

CONTIGS = [("chrA", 200_000), ("chrB", 90_000), ("chrC", 40_000)]


@pytest.mark.parametrize("lo", [2100, 300], ids=["no_heads", "heads"])
@pytest.mark.parametrize("bw", ["700", "2000"])
def test_regions_cli_profile(orc_bin, gpu_lib, tmp_path, bw, lo):
    """bin/regions -D -w at a wide -b: region table and profile byte-identical
    to the oracle CLI's, without (first tags above bw) and with head units
    (-m: the background that lets these inputs reach the default -r 25)"""
    ct, files = make_inputs(tmp_path, 170 + int(bw) + lo, CONTIGS, 1, lo=lo, shift_rev=100, n_cl=12, sd=200)
    common = ["-q", "-c", ct, "-D", "-y", "-f", "-k", "0", "-b", bw, "-m", "20000000"]
    (tmp_path / "ref").mkdir()
    (tmp_path / "got").mkdir()
    run([orc_bin, "regions"] + common + ["-w", "ref/p.wig", "-o", "ref/r.txt"] + files, tmp_path)
    run([os.path.join(BIN, "regions")] + common + ["-w", "got/p.wig", "-o", "got/r.txt"] + files, tmp_path)
    assert (tmp_path / "ref/r.txt").read_bytes() == (tmp_path / "got/r.txt").read_bytes()
    a, b = (tmp_path / "ref/p.wig").read_bytes(), (tmp_path / "got/p.wig").read_bytes()
    assert a.count(b"\n") > 1000
    assert a == b, "profile differs at byte %d" % next(
        (i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
