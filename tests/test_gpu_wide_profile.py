"""The dense score profile of kernels wider than K1's halo (511 < bw <=
32,767, directional units, a threshold > 0): wide_profile_kernel
(csrc/wide.hip) behind up_unit_profile / up_unit_profile_range, and the -w
capture on K1w passes (up_set_profile_capture no longer sends them to the
whole-buffer replay).

Every score bit for bit: against the oracle's profile on 1 .. len, against
the ascending sum restated below past len (positions up to len + bw are
retired by the flush; above it nothing is scored), and bin/regions -w byte
for byte against the oracle CLI.  A strip is 16,384 positions, a stretch of
the profile kernel 4,096; the lengths span 4 - 13 strips."""
import os

import numpy as np
import pytest

from tests.gen import random_unit
from tests.test_cli import BIN, make_inputs, run
from tests.test_gpu_replay import compare

pytestmark = pytest.mark.gpu

BG = 0.003
LENGTHS = {512: 60_000, 700: 60_000, 2000: 70_000, 6000: 80_000}
_cases = {}


def case(oracle, bw):
    """(length, pos, cnt, oracle profile) of the single-sample unit of `bw`:
    no head hits (first tag above bw), tags up to the contig end; computed
    once and shared"""
    if bw not in _cases:
        rng = np.random.default_rng(9000 + bw)
        length = LENGTHS[bw]
        pos, cnt = random_unit(rng, length, bw, lo=bw + 1, hi=length)
        ref = oracle.profile(bw, BG, length, pos, cnt)
        ref.setflags(write=False)
        _cases[bw] = (length, pos, cnt, ref)
    return _cases[bw]


def ascending_sum(kern, bw, length, pos, cs, xs):
    """score of every x in xs: the pooled count times kern[x - a + bw] over the
    adds a in [x - bw, x + bw] and [1, len], ascending, one multiply and one
    add each, from +0.0"""
    out = np.zeros(len(xs), np.float64)
    for i, x in enumerate(xs):
        f = 0.0
        lo, hi = np.searchsorted(pos, max(1, x - bw)), np.searchsorted(pos, min(length, x + bw), "right")
        for a, c in zip(pos[lo:hi].tolist(), cs[lo:hi].tolist()):
            f = f + float(kern[x - a + bw]) * float(c)
        out[i] = f
    return out


def load(g, length, pos, cnt, buffer_id=0):
    u = g.add_unit(length, buffer_id)
    for s in range(cnt.shape[1]):
        m = cnt[:, s] != 0
        if m.any():
            g.scatter(u, 0, s, pos[m], cnt[m, s])
    return u


def gpu_profile(capi, bw, length, pos, cnt, **kw):
    with capi.Lib(0) as g:
        g.set_params(bw, cnt.shape[1], BG, **kw)
        u = load(g, length, pos, cnt)
        return g.profile(u, length)


@pytest.mark.parametrize("bw", [512, 700, 2000, 6000])
def test_profile_matches_oracle(gpu_lib, oracle, bw):
    length, pos, cnt, ref = case(oracle, bw)
    assert pos[0] > bw and pos[-1] > length - bw
    f, r = gpu_profile(gpu_lib, bw, length, pos, cnt)
    assert f.tobytes() == ref.tobytes()
    assert np.count_nonzero(ref) > length // 2
    assert not r.any()


def test_profile_bw_32767_and_refusal_above(gpu_lib, oracle):
    """the widest K1w window (65,535 cells); from bw 32,768 on (the UShort
    wrap: the whole-buffer replay) the dense profile stays refused"""
    capi = gpu_lib
    rng = np.random.default_rng(32767)
    length, bw = 120_000, 32767
    pos = np.unique(rng.integers(bw + 1, length + 1, 200)).astype(np.uint32)
    cnt = rng.integers(1, 4, (pos.size, 1)).astype(np.uint32)
    ref = oracle.profile(bw, BG, length, pos, cnt)
    with capi.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, pos, cnt)
        f, r = g.profile(u, length)
        assert f.tobytes() == ref.tobytes()
        assert not r.any()
        g.set_params(32768, 1, BG)
        with pytest.raises(capi.UpError):
            g.profile(u, length)


def test_profile_ranges(gpu_lib, oracle):
    """ranges starting in mid-word and crossing a strip edge, ending at
    len + bw, and reaching past it to the end of the scan domain"""
    bw = 700
    length, pos, cnt, ref = case(oracle, bw)
    kern = oracle.kernel(bw, 1.0 / BG)
    dom = -(-(length + bw) // 16384) * 16384  # whole strips covering [1, len + bw]
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, pos, cnt)
        for first, count in ((16_380, 100), (1, 1), (4_097, 64), (33_000, 5_000)):
            f, r = g.profile_range(u, first, count)
            assert f.tobytes() == ref[first - 1:first - 1 + count].tobytes(), (first, count)
            assert not r.any()
        # ... ending at len + bw: the contig's tail, then the flush's positions
        first = length - 300
        f, _ = g.profile_range(u, first, length + bw - first + 1)
        assert f[:301].tobytes() == ref[first - 1:].tobytes()
        tail = ascending_sum(kern, bw, length, pos, cnt[:, 0], range(length + 1, length + bw + 1))
        assert np.count_nonzero(tail) > 0
        assert f[301:].tobytes() == tail.tobytes()
        # ... and past it to the end of the scan domain: exactly 0.0 above len + bw
        first = length + bw - 50
        f, _ = g.profile_range(u, first, dom - first + 1)
        assert f[:51].tobytes() == tail[-51:].tobytes()
        assert f.size > 51 and not f[51:].any()


def test_restated_sum_is_the_oracle_profile(oracle):
    """the restatement used past len, checked where the oracle reaches"""
    bw = 700
    length, pos, cnt, ref = case(oracle, bw)
    kern = oracle.kernel(bw, 1.0 / BG)
    xs = list(range(length - 900, length + 1)) + list(range(20_000, 20_200))
    got = ascending_sum(kern, bw, length, pos, cnt[:, 0], xs)
    assert got.tobytes() == ref[np.array(xs) - 1].tobytes()


def test_screen_and_edges(gpu_lib, oracle):
    """lone tags on both sides of a strip edge (16,384 | 16,385; 65,536 |
    65,537) and at the contig end, counts through the escape tile (3, 254)
    and the overflow search (255, 300, 70,000), empty stretches longer than
    2 bw + 16,384 between them: whole stretches the screen leaves at 0.0"""
    length, bw = 200_000, 700
    pos = np.array([16_384, 16_385, 65_536, 65_537, length], np.uint32)
    cnt = np.array([[3], [254], [255], [300], [70_000]], np.uint32)
    ref = oracle.profile(bw, BG, length, pos, cnt)
    f, r = gpu_profile(gpu_lib, bw, length, pos, cnt)
    assert f.tobytes() == ref.tobytes()
    assert not r.any()
    assert 65_536 - 16_385 - 2 * bw > 2 * bw + 16_384
    assert not f[16_385 + bw:65_536 - bw - 1].any()  # positions 16,385 + bw + 1 .. 65,536 - bw - 1
    assert f[16_385 + bw - 2] != 0.0 and f[65_536 - bw] != 0.0 and f[length - 1] != 0.0


@pytest.mark.parametrize("coeffs", [None, [0.6, 1.7]])
def test_pooled_control_and_coefficients(gpu_lib, oracle, coeffs):
    rng = np.random.default_rng(71)
    length, bw, S = 60_000, 700, 3
    pos, cnt = random_unit(rng, length, bw, S=S, lo=bw + 1, hi=length)
    control = [0, 1, 0]
    ref = oracle.profile(bw, BG, length, pos, cnt, control=control, coeffs=coeffs)
    f, r = gpu_profile(gpu_lib, bw, length, pos, cnt, control=control, coeffs=coeffs)
    assert f.tobytes() == ref.tobytes()
    assert not r.any()


def test_reverse_buffer_unit(gpu_lib, oracle):
    rng = np.random.default_rng(72)
    length, bw = 60_000, 700
    pos, cnt = random_unit(rng, length, bw, lo=bw + 1, hi=length)
    ref = oracle.profile(bw, BG, length, pos, None, cnt, buffer_forward=False)
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, pos, cnt, buffer_id=1)
        f, r = g.profile(u, length)
    assert f.tobytes() == ref.tobytes()
    assert not r.any()


def test_dense_background(gpu_lib, oracle):
    """One tag position in about nine: the hit list of a stretch (kProfHits =
    512 entries per 64-word stretch, csrc/wide.hip) is sized for sparse
    tracks; here every window of a whole stretch (4,096 + 2 x 2,000
    positions) holds more than 700 hits, so those stretches overflow the list
    and take the direct per-word window walk.  Parity only."""
    rng = np.random.default_rng(73)
    length, bw = 60_000, 2000
    pos, cnt = random_unit(rng, length, bw, n_bg=length // 8, lo=bw + 1, hi=length)
    assert pos.size > length // 10
    ref = oracle.profile(bw, BG, length, pos, cnt)
    f, r = gpu_profile(gpu_lib, bw, length, pos, cnt)
    assert f.tobytes() == ref.tobytes()
    assert not r.any()


def test_capture_without_heads(gpu_lib, oracle):
    """the -w capture on a K1w pass: K1w's records (not the whole-buffer
    replay's), no unit replayed, the dense profile, pipelined passes"""
    capi = gpu_lib
    bw = 700
    length, pos, cnt, prof = case(oracle, bw)
    ref, ref_sums = oracle.run_unit(bw, BG, pos, cnt, cap=1 << 20)
    assert len(ref) > 0
    with capi.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, pos, cnt)
        g.set_profile_capture(True)
        n = g.run()
        regs, k = g.regions(n)
        compare(ref, ref_sums, regs, k)
        resync, ev, p, sc = g.replay_profile(u)
        assert resync == 0 and ev.size == 0 and p.size == 0 and sc.size == 0
        f, r = g.profile(u, length)
        assert f.tobytes() == prof.tobytes()
        assert not r.any()
        g.run_async()
        g.run_async()
        for _ in range(2):
            n = g.run_wait()
            regs, k = g.regions(n)
            compare(ref, ref_sums, regs.copy(), k.copy())


def test_capture_with_a_head_unit(gpu_lib, oracle):
    """tags at positions <= bw (quirk Q1): the K0 head replay hands over its
    retirements up to its resync point, the dense profile serves the rest"""
    capi = gpu_lib
    rng = np.random.default_rng(62)
    length, bw = 60_000, 1200
    pos, cnt = random_unit(rng, length, bw, lo=1, hi=length)
    d = {int(p): int(c) for p, c in zip(pos, cnt[:, 0])}
    for p, c in {3: 5, 40: 9, 700: 30}.items():
        d[p] = d.get(p, 0) + c
    pos = np.array(sorted(d), np.uint32)
    cnt = np.array([[d[int(p)]] for p in pos], np.uint32)
    ref, ref_sums = oracle.run_unit(bw, BG, pos, cnt, cap=1 << 20)
    prof = oracle.profile(bw, BG, length, pos, cnt)
    with capi.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, pos, cnt)
        g.set_profile_capture(True)
        n = g.run()
        regs, k = g.regions(n)
        compare(ref, ref_sums, regs, k)
        resync, ev, p, sc = g.replay_profile(u)
        assert bw < resync <= length  # (not UP_FLUSH_EVENT: the head replay resynced)
        nzp = np.flatnonzero(prof[:resync - 1])
        assert nzp.size > bw
        assert np.array_equal(p, nzp + 1)
        assert sc.tobytes() == prof[nzp].tobytes()
        assert np.all(ev < pos.size)
        f, r = g.profile_range(u, resync, length - resync + 1)
        assert f.tobytes() == prof[resync - 1:].tobytes()
        assert not r.any()


@pytest.mark.parametrize("lo", [2100, 300], ids=["no_heads", "heads"])
@pytest.mark.parametrize("bw", ["700", "2000"])
def test_regions_cli_profile(orc_bin, gpu_lib, tmp_path, bw, lo):
    """bin/regions -w at a wide -b: region table and profile byte-identical
    to the oracle CLI's, without (first tags above bw) and with head units"""
    contigs = [("chrA", 200_000), ("chrB", 90_000), ("chrC", 40_000)]
    ct, files = make_inputs(tmp_path, 170 + int(bw) + lo, contigs, 2, lo=lo, n_cl=12, sd=200)
    common = ["-q", "-f", "-c", ct, "-b", bw, "-k", "0"]
    (tmp_path / "ref").mkdir()
    (tmp_path / "got").mkdir()
    run([orc_bin, "regions"] + common + ["-w", "ref/p.wig", "-o", "ref/r.txt"] + files, tmp_path)
    run([os.path.join(BIN, "regions")] + common + ["-w", "got/p.wig", "-o", "got/r.txt"] + files, tmp_path)
    assert (tmp_path / "ref/r.txt").read_bytes() == (tmp_path / "got/r.txt").read_bytes()
    a, b = (tmp_path / "ref/p.wig").read_bytes(), (tmp_path / "got/p.wig").read_bytes()
    assert a.count(b"\n") > 1000
    assert a == b, "profile differs at byte %d" % next(
        (i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
