"""CPU check of the inputs of tests/test_gpu_wide_nondir.py: the oracle alone
must yield what the GPU cases rely on (region counts, one region accepted and
one rejected by the correlation filter, a run crossing a strip edge, the hit
density of the stress unit), so a bad seed shows up without a GPU."""
import numpy as np
import pytest

from tests import wide_nd_inputs as W


@pytest.mark.parametrize("bw", sorted(W.PARITY_SEEDS))
def test_parity_inputs(oracle, bw):
    length, pos, cf, cr = W.parity_unit(bw)
    assert pos.min() > bw  # no head unit
    with_corr, _ = oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    no_corr, _ = oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=-1.0)
    assert len(with_corr) == len(no_corr) >= 10
    assert np.any(with_corr["accepted"] == 1)
    assert np.any((no_corr["accepted"] == 1) & (with_corr["accepted"] == 0))  # rejected by the correlation
    assert np.any(W.crosses_strip(with_corr))
    if bw == 700:  # the K4 case: a region shorter than 2 * 600 + 3 and a longer one
        n = with_corr["right"] - with_corr["left"] + 1
        assert np.any(n <= 1203) and np.any(n > 1203)


def test_one_strand_inputs(oracle):
    length, pos, cf, cr = W.one_strand_unit()
    f, r = pos[cf[:, 0] != 0], pos[cr[:, 0] != 0]
    assert r.min() - f.max() > 2 * W.ONE_STRAND_BW
    ref, _ = oracle.run_unit(W.ONE_STRAND_BW, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    assert len(ref) == 2
    assert np.all(np.isnan(ref["corr"])) and not ref["accepted"].any()
    ref, _ = oracle.run_unit(W.ONE_STRAND_BW, W.BG, pos, cf, cr, nondir=True, corr_thr=-1.0)
    assert ref["accepted"].all()  # the correlation filter alone rejects them


def test_stress_inputs(oracle):
    bw = W.STRESS_BW
    length, pos, cf, cr = W.stress_unit()
    ref, _ = oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    assert len(ref) == 3
    n = ref["right"] - ref["left"] + 1
    assert n.max() > 2 * W.SLAB  # formed again slab by slab, more than once
    # the first region's first stretch (4,096 positions from the 64-position
    # word that holds `left`: wide_range_scores) sees more forward hits in its
    # windows than one LDS list holds, and fewer reverse ones
    fpos, rpos = pos[cf[:, 0] != 0], pos[cr[:, 0] != 0]
    x_lo = 1 + (int(ref["left"][0]) - 1) // 64 * 64
    win = lambda p: int(np.sum((p >= x_lo - bw) & (p <= x_lo + 4095 + bw)))
    assert win(fpos) > W.LIST and 0 < win(rpos) <= W.LIST
    assert np.any(cf[:, 0] >= 3)  # escaped counts
    # a reverse chunk (16 positions from 1 + 16 k) of >= 255 tags: a saturated plane entry
    chunk = (pos[cr[:, 0] != 0].astype(np.int64) - 1) // 16
    sums = np.bincount(chunk, weights=cr[cr[:, 0] != 0, 0])
    assert sums.max() >= 255


def test_head_inputs(oracle):
    bw = W.HEAD_BW
    length, pos, cf, cr = W.head_unit()
    f, r = pos[cf[:, 0] != 0], pos[cr[:, 0] != 0]
    assert f.min() > bw and r.min() <= bw  # head tags on the reverse strand only
    assert f.max() == length
    ref, _ = oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    assert ref["left"][0] <= bw < ref["right"][0]  # a region that starts inside the head
    assert np.sum(ref["left"] > 4 * bw) >= 5       # and regions far behind it
    assert ref["right"][-1] > length               # the right end past the contig end


def test_limit_inputs(oracle):
    bw = W.LIMIT_BW
    length, pos, cf, cr = W.limit_unit()
    assert pos.min() > bw  # no head unit
    assert 200 < np.sum(cf[:, 0] != 0) + np.sum(cr[:, 0] != 0) < 2 * W.LIST
    assert max(np.sum(cf[:, 0] != 0), np.sum(cr[:, 0] != 0)) <= W.LIST  # the listed walk
    ref, _ = oracle.run_unit(bw, W.LIMIT_BG, pos, cf, cr, nondir=True, cap=1 << 20, **W.LIMIT_KW)
    assert len(ref) >= 1
    assert np.any(ref["right"] - ref["left"] + 1 > 4 * W.SLAB)  # many slabs of the correlation
