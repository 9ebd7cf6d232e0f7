"""CPU check of the inputs of tests/test_gpu_wide_nd_profile.py: the oracle
alone must yield what the GPU cases rely on -- f + r of the two one-strand
profiles is the nondirectional profile bit for bit, both strands score, the
one-strand windows are one-strand, the stress stretch overflows the hit list
on one strand only, the head input resyncs -- so a bad seed shows up without
a GPU."""
import numpy as np
import pytest

from tests import wide_nd_inputs as W
from tests import wide_nd_profile_inputs as I
from tests.test_gpu_wide_profile import ascending_sum


def check_sum(f, r, both):
    assert (f + r).tobytes() == both.tobytes()


@pytest.mark.parametrize("bw", sorted(I.PARITY_SEEDS))
def test_parity_inputs(oracle, bw):
    length, pos, cf, cr = I.parity_unit(bw)
    assert length == I.LENGTH and pos.min() > bw  # no head unit
    f, r, both = I.strand_refs(oracle, bw, W.BG, length, pos, cf, cr)
    check_sum(f, r, both)
    assert f.any() and r.any()
    assert np.any((f != 0) & (r == 0)) and np.any((r != 0) & (f == 0))
    ref, _ = oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    assert len(ref) >= 2


def test_tail_inputs(oracle):
    """the range case: both strands score past the contig end, and the
    restated ascending sum is the oracle's profile where the oracle reaches"""
    bw = I.RANGE_BW
    length, pos, cf, cr = I.tail_unit()
    assert pos.min() > bw and pos.max() == length
    f, r, both = I.strand_refs(oracle, bw, W.BG, length, pos, cf, cr)
    check_sum(f, r, both)
    kern = oracle.kernel(bw, 1.0 / W.BG)
    xs = list(range(length - 400, length + 1)) + [16_380, 16_384, 16_385]
    for c, ref in ((cf, f), (cr, r)):
        m = c[:, 0] != 0
        assert ascending_sum(kern, bw, length, pos[m], c[m, 0], xs).tobytes() == ref[np.array(xs) - 1].tobytes()
        tail = ascending_sum(kern, bw, length, pos[m], c[m, 0], [length + 1, length + bw])
        assert tail[0] != 0.0
    # a range starting mid-word and one across a strip edge see scores on both strands
    for first, count in ((4_100, 64), (16_380, 100)):
        assert f[first - 1:first - 1 + count].any() and r[first - 1:first - 1 + count].any()


def test_one_strand_inputs(oracle):
    bw = W.ONE_STRAND_BW
    length, pos, cf, cr = W.one_strand_unit()
    f, r, both = I.strand_refs(oracle, bw, W.BG, length, pos, cf, cr)
    check_sum(f, r, both)
    a, b = slice(15_000 - 300, 15_000 + 300), slice(40_000 - 300, 40_000 + 300)
    assert np.all(f[a] != 0) and not r[a].any()
    assert np.all(r[b] != 0) and not f[b].any()


def test_stress_inputs(oracle):
    """the stretch of position 20,000: the forward strand's windows hold more
    hits than the LDS list (the fallback walk), the reverse strand's fewer
    (the listed walk) -- in one stretch"""
    bw = W.STRESS_BW
    length, pos, cf, cr = W.stress_unit()
    fpos, rpos = pos[cf[:, 0] != 0], pos[cr[:, 0] != 0]
    nf, nr = I.stretch_hits(fpos, bw, 20_000), I.stretch_hits(rpos, bw, 20_000)
    assert nf > W.LIST and 0 < nr <= W.LIST
    assert nf >= 1_000 and 50 <= nr <= 70
    assert np.any(cf[:, 0] >= 3)  # escaped counts
    chunk = (rpos.astype(np.int64) - 1) // 16
    assert np.bincount(chunk, weights=cr[cr[:, 0] != 0, 0]).max() >= 255  # a saturated plane entry
    f, r, both = I.strand_refs(oracle, bw, W.BG, length, pos, cf, cr)
    check_sum(f, r, both)
    assert f[19_999:20_999].all() and r[20_299:20_699].all()


@pytest.mark.parametrize("coeffs", I.POOL_COEFFS)
def test_pooled_inputs(oracle, coeffs):
    length, pos, cf, cr = I.pooled_unit()
    assert cf.shape[1] == 3 and pos.min() > 700
    f, r, both = I.strand_refs(oracle, 700, W.BG, length, pos, cf, cr, control=I.POOL_CONTROL, coeffs=coeffs)
    check_sum(f, r, both)
    assert f.any() and r.any()
    assert cf[:, 1].any() and cr[:, 1].any()  # the control holds tags: its adds retire positions


def test_limit_inputs(oracle):
    bw = W.LIMIT_BW
    length, pos, cf, cr = W.limit_unit()
    assert pos.min() > bw
    f, r, both = I.strand_refs(oracle, bw, W.LIMIT_BG, length, pos, cf, cr)
    check_sum(f, r, both)
    assert np.count_nonzero(f) > length // 2 and np.count_nonzero(r) > length // 2


def test_head_gap_inputs(oracle):
    """head tags on the reverse strand only, then a gap in which the window
    drains; behind the gap the nondirectional profile is the plain sum again"""
    bw = I.HEAD_BW
    length, pos, cf, cr = I.head_gap_unit()
    fpos, rpos = pos[cf[:, 0] != 0], pos[cr[:, 0] != 0]
    assert list(rpos[:3]) == [3, 40, 650] and fpos.min() > I.HEAD_GAP[1] and rpos[3] > I.HEAD_GAP[1]
    assert I.HEAD_GAP[1] - I.HEAD_GAP[0] + 1 > 2 * bw + 1
    both = oracle.profile(bw, W.BG, length, pos, cf, cr, nondir=True)
    assert both[:I.HEAD_GAP[0] + bw].any()  # the head's own scores
    # (quirk Q1 misaligns the head's window: its scores are not the plain sum)
    mf, mr = cf[:, 0] != 0, cr[:, 0] != 0
    f = oracle.profile(bw, W.BG, length, pos[mf], cf[mf])
    body = cr.copy()
    body[:3] = 0  # the reverse strand without its head tags: no Q1
    mb = body[:, 0] != 0
    r = oracle.profile(bw, W.BG, length, pos[mb], body[mb])
    # up to the first aligned add + bw the window may carry misaligned density
    # (the head replay's horizon); behind it the plain sums hold
    lo = int(min(fpos.min(), rpos[3])) + bw
    assert lo < 2 * I.HEAD_GAP[1]
    assert (f + r)[lo:].tobytes() == both[lo:].tobytes()
    assert (f + r)[:lo].tobytes() != both[:lo].tobytes()
    ref, _ = oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    assert len(ref) >= 2 and np.sum(ref["left"] > I.HEAD_GAP[1]) >= 2
