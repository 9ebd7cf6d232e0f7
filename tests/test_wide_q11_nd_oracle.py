"""The inputs of tests/test_gpu_wide_q11_nd.py, checked on the CPU against the
oracle alone: each one has the property its GPU case relies on (region counts,
stored lengths on both sides of the long-region limit and of the tile
boundaries, both outcomes of the correlation filter, a one-strand region whose
correlation is NaN, peaks of f + r where neither strand has its own)."""
import os

import numpy as np
import pytest

from tests import wide_q11_nd_inputs as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(oracle, bw, unit, **kw):
    return oracle.run_unit(bw, N.BG, unit[1], unit[2], unit[3], nondir=True, **kw)[0]


def test_the_switch_is_declared():
    from unipeak_amd import capi
    assert hasattr(capi.Lib, "set_wide_q11_nd") and hasattr(capi.load_library(), "up_set_wide_q11_nd")
    header = open(os.path.join(ROOT, "include", "unipeak_hip.h")).read()
    assert "int up_set_wide_q11_nd(up_ctx *ctx, int on);" in header
    assert "UNIPEAK_WIDE_Q11_ND=0" in header and "UNIPEAK_WIDE_CORR_TILE" in header


@pytest.mark.parametrize("bw", N.WIDTHS)
def test_clustered_units(oracle, bw):
    unit = N.clustered_unit(bw)
    assert int(unit[1].min()) > bw + 1  # no head
    refs = [run(oracle, bw, unit, region_thr=t) for t in N.THRESHOLDS]
    assert len(refs[0]) >= 3
    assert unit[2].any() and unit[3].any() and not np.isnan(refs[0]["corr"]).any()  # both strands in every run
    for r in refs[1:]:
        assert r.tobytes() == refs[0].tobytes()


def test_corr_unit_has_both_outcomes_and_a_nan(oracle):
    ref = run(oracle, N.CORR_BW, N.corr_unit(), region_thr=0.0, corr_thr=N.CORR_THR)
    free = run(oracle, N.CORR_BW, N.corr_unit(), region_thr=0.0, corr_thr=-1.0)
    assert len(ref) == 3 and list(ref["accepted"]) == [1, 0, 0]
    assert list(free["accepted"]) == [1, 1, 1]  # the correlation alone rejects B and C
    assert ref["corr"][0] > N.CORR_THR > ref["corr"][1] and np.isnan(ref["corr"][2])


@pytest.mark.parametrize("coeffs", N.RULE_COEFFS)
def test_rule_unit(oracle, coeffs):
    bw, gap = N.RULE_BW, 2 * N.RULE_BW + 1
    unit = N.rule_unit()
    ref = run(oracle, bw, unit, region_thr=0.0, kurt_thr=0.0, control=N.RULE_CONTROL, coeffs=coeffs)
    b = [(int(l), int(r)) for l, r in zip(ref["left"], ref["right"])]
    assert len(b) == 5
    assert b[0] == (9_950 - bw + 1, 12_350 + bw + 1)  # bridged by the reverse-only add at 11,150
    assert 21_201 - 20_000 == gap and 22_403 - 21_201 == gap + 1
    assert b[1] == (20_000 - bw + 1, 21_201 + bw + 1) and b[2] == (22_403 - bw + 1, 22_403 + bw + 1)
    assert b[3][1] == 32_200 + bw + 1  # extended by the control-only adds
    assert b[4] == (40_000 - bw + 1, 40_900 + bw + 1)
    # the control-only run: every score 0.0, and the peak is not the run's first stored position
    # (left is the first stored position + 1, and so is a peak there: the peak is the second one)
    assert ref["peak_score"][4] == 0.0 and int(ref["peak"][4]) == b[4][0] + 1
    # without the reverse strand the first region splits
    fwd = oracle.run_unit(bw, N.BG, unit[1], unit[2], np.zeros_like(unit[3]), nondir=True, region_thr=0.0,
                          kurt_thr=0.0, control=N.RULE_CONTROL, coeffs=coeffs)[0]
    assert int(fwd["right"][0]) < 12_000


def test_peak_unit(oracle):
    bw = N.PEAK_BW
    ref = run(oracle, bw, N.peak_unit(), region_thr=0.0)
    assert len(ref) == 2
    # (peaks are reported one higher than the stored position)
    assert N.BETWEEN_F + 1 < int(ref["peak"][0]) < N.BETWEEN_R + 1
    assert int(ref["peak"][1]) == N.TIE_A + 1
    first = (int(ref["left"][1]) - 1) // 64
    assert ((N.TIE_B - 1) // 64 - first) // (N.STRETCH // 64) > ((N.TIE_A - 1) // 64 - first) // (N.STRETCH // 64)
    # the tie is one bit for bit: f at the forward pair == r at the reverse pair
    length, pos, cf, cr = N.peak_unit()
    f = oracle.profile(bw, N.BG, length, pos[cf[:, 0] != 0], cf[cf[:, 0] != 0])
    r = oracle.profile(bw, N.BG, length, pos[cr[:, 0] != 0], cr[cr[:, 0] != 0])
    s = f + r
    assert s[N.TIE_A - 1] == s[N.TIE_A] == s[N.TIE_B - 1] == s[N.TIE_B]
    lo, hi = int(ref["left"][1]) - 1, int(ref["right"][1]) - 1
    assert s[lo:hi].max() == s[N.TIE_A - 1]


@pytest.mark.parametrize("limit,bw", [(N.TEST_LONG, 600), (N.CORR_LONG, 2000)])
def test_long_unit_lengths(oracle, limit, bw):
    unit, lens = N.long_unit(limit, bw)
    ref = run(oracle, bw, unit, region_thr=0.0)
    assert tuple(N.stored(ref)) == lens == (limit - 1, limit, limit + 1, 2 * limit - 100)
    assert not np.isnan(ref["corr"]).any()
    s = ref["left"].astype(np.int64) - 1  # stored starts
    e = ref["right"].astype(np.int64) - 1
    assert (s[0] - 1) % 64 != 0 and (s[2] - 1) % 64 != 0 and (s[3] - 1) % 64 != 0  # mid-word
    if limit == N.TEST_LONG:
        assert unit[0] < 50_000
        strip = lambda x: (x - 1) // N.STRIP
        assert strip(s[1]) != strip(e[1]) and strip(s[3]) != strip(e[3])
        # the axis of the long regions: [0, limit + 1) and [limit + 1, 3 limit - 99)
        a = [0, limit + 1, 3 * limit - 99]
        big, small = N.TEST_TILES
        cuts = lambda t, lo, hi: len([k for k in range(t, hi, t) if lo < k < hi])
        assert a[1] < big and cuts(big, a[1], a[2]) == 1          # two regions in round 0, the second cut once
        assert cuts(small, a[0], a[1]) == 2 and cuts(small, a[1], a[2]) >= 3


def test_k4_units_have_a_head(oracle):
    u0, u1 = N.k4_units()
    assert int(u0[1].min()) <= N.K4_BW and int(u1[1].min()) > N.K4_BW + 1
    assert len(run(oracle, N.K4_BW, u0, region_thr=0.0)) >= 2 and len(run(oracle, N.K4_BW, u1, region_thr=0.0)) >= 2


def test_switch_unit(oracle):
    unit, ep, ec = N.switch_unit()
    bw = N.SWITCH_BW
    assert int(unit[1].min()) > bw + 1
    assert len(run(oracle, bw, unit, region_thr=25.0, corr_thr=0.3)) >= 2
    a = run(oracle, bw, unit, region_thr=0.0, corr_thr=0.3)
    b = run(oracle, bw, N.with_extra(unit, ep, ec), region_thr=0.0, corr_thr=0.3)
    assert len(b) == len(a) + 1  # the scatter closes what was the last run
