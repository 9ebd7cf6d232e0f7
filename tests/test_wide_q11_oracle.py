"""The inputs of tests/test_gpu_wide_q11.py, checked on the CPU against the
oracle alone: each one has the property its GPU case relies on (region counts
and bounds, ties that are ties bit for bit, head units that are heads)."""
import numpy as np
import pytest

from tests import wide_q11_inputs as Q


def bounds(ref):
    return [(int(l), int(r)) for l, r in zip(ref["left"], ref["right"])]


@pytest.mark.parametrize("bw", Q.WIDTHS)
def test_clustered_units_have_a_region_per_cluster(oracle, bw):
    length, pos, cnt = Q.clustered_unit(bw)
    assert int(pos.min()) > bw + 1  # no head
    refs = [oracle.run_unit(bw, Q.BG, pos, cnt, region_thr=t)[0] for t in Q.THRESHOLDS]
    assert len(refs[0]) >= 3 and bounds(refs[0]) == Q.expected_bounds(pos, bw)
    for r in refs[1:]:
        assert r.tobytes() == refs[0].tobytes()
    if bw == 32_767:
        assert 290_000 <= length <= 310_000
        assert int(np.sum(np.diff(pos.astype(np.int64)) > 65_535)) >= 2


@pytest.mark.parametrize("bw", Q.EDGE_WIDTHS)
def test_gap_edges(oracle, bw):
    gap = 2 * bw + 1
    (l0, p0, c0), (l1, p1, c1) = Q.edge_units(bw)
    a = [int(x) for x in p0]
    b = [int(x) for x in p1]
    assert max(l0, l1) <= 400_000 and a[0] > bw + 1 and b[0] > bw + 1
    # adds 2bw + 1 apart share a run, adds 2bw + 2 apart do not
    assert a[1] - a[0] == gap and a[2] - a[1] == gap + 1
    r0 = bounds(oracle.run_unit(bw, Q.BG, p0, c0, region_thr=0.0)[0])
    assert r0 == Q.expected_bounds(p0, bw) == [(a[0] - bw + 1, a[1] + bw + 1), (a[2] - bw + 1, a[2] + bw + 1),
                                                (a[3] - bw + 1, a[3] + bw + 1)]
    r1 = bounds(oracle.run_unit(bw, Q.BG, p1, c1, region_thr=0.0)[0])
    assert r1 == Q.expected_bounds(p1, bw) == [(b[0] - bw + 1, b[0] + bw + 1), (b[1] - bw + 1, b[1] + bw + 1)]
    # the raw run boundaries against the strips
    assert (a[0] - bw - 1) % Q.STRIP == 0 and (b[0] - bw - 1) % Q.STRIP == 1
    assert (a[3] + bw) % Q.STRIP == 0 and (b[1] + bw) % Q.STRIP == Q.STRIP - 1
    strip = lambda x: (x - 1) // Q.STRIP
    if bw == 32_767:  # the owning add one strip (unit 0) and two strips (unit 1) from its boundary
        assert strip(a[0]) - strip(a[0] - bw) == 1 and strip(a[3] + bw) - strip(a[3]) == 1
        assert strip(b[0]) - strip(b[0] - bw) == 2 and strip(b[1] + bw) - strip(b[1]) == 2


@pytest.mark.parametrize("coeffs", Q.POOL_COEFFS)
def test_pooled_unit_controls_shape_the_runs(oracle, coeffs):
    bw = Q.POOL_BW
    length, pos, cnt = Q.pooled_unit()
    ref, sums = oracle.run_unit(bw, Q.BG, pos, cnt, control=Q.POOL_CONTROL, coeffs=coeffs, region_thr=0.0,
                                kurt_thr=0.0)
    assert bounds(ref) == Q.expected_bounds(pos, bw) and len(ref) == 6
    # without the control-only adds: A and B apart, C's run shorter
    keep = ~np.isin(pos, (11_000, 21_000))
    assert int((~keep).sum()) == 2 and not cnt[~keep][:, (0, 2)].any() and cnt[~keep][:, 1].all()
    bare, _ = oracle.run_unit(bw, Q.BG, pos[keep], cnt[keep], control=Q.POOL_CONTROL, coeffs=coeffs,
                              region_thr=0.0, kurt_thr=0.0)
    assert len(bare) == 7
    assert bare["right"][0] < bare["left"][1] and ref["left"][0] == bare["left"][0]
    assert ref["right"][0] == bare["right"][1]
    assert ref["right"][1] == 21_000 + bw + 1 > bare["right"][2]
    # the heavy centres sit at their regions' peaks (Region::peak = position + 1 here)
    for k, c in enumerate(Q.POOL_PEAKS):
        centre = 30_000 + 3_000 * k
        assert int(cnt[np.searchsorted(pos, centre), 0]) == c
        assert ref["left"][2 + k] < centre < ref["right"][2 + k]
        assert abs(int(ref["peak"][2 + k]) - 1 - centre) <= (2 if c >= 254 else 60)


@pytest.mark.parametrize("where", ["last", "first"])
def test_long_region_peak_in_an_outer_stretch(oracle, where):
    bw = Q.LONG_BW
    length, pos, cnt = Q.long_unit(where)
    assert int(np.diff(pos.astype(np.int64))[:-1].max()) <= 4_000
    ref, _ = oracle.run_unit(bw, Q.BG, pos, cnt, region_thr=0.0)
    assert len(ref) == 1
    left, right, peak = int(ref["left"][0]), int(ref["right"][0]), int(ref["peak"][0])
    assert right - left + 1 >= 150_000
    assert (right - 1) // Q.STRIP - (left - 1) // Q.STRIP > 9
    nstretch = Q.stretch_of(left, right) + 1
    assert nstretch > 36
    # (the record's coordinates are the raw run's + 1, as is its peak: the same stretch arithmetic holds)
    assert Q.stretch_of(left, peak) == (nstretch - 1 if where == "last" else 0)
    prof = oracle.profile(bw, Q.BG, length, pos, cnt)
    assert int(np.sum(prof == prof.max())) == 1  # unique


def test_tie_is_a_tie_bit_for_bit(oracle):
    bw = Q.TIE_BW
    length, pos, cnt = Q.tie_unit()
    prof = oracle.profile(bw, Q.BG, length, pos, cnt)
    four = [prof[p - 1] for p in (Q.TIE_A, Q.TIE_A + 1, Q.TIE_B, Q.TIE_B + 1)]
    assert len({np.float64(v).tobytes() for v in four}) == 1
    assert four[0] == prof.max() and int(np.sum(prof == prof.max())) == 4
    assert (Q.TIE_A - 1) // Q.STRIP != (Q.TIE_B - 1) // Q.STRIP
    ref, _ = oracle.run_unit(bw, Q.BG, pos, cnt, region_thr=0.0)
    assert len(ref) == 1 and bounds(ref) == Q.expected_bounds(pos, bw)
    # (the run was reached by a leap: Region::peak = position + 1)
    assert int(ref["peak"][0]) == Q.TIE_A + 1 and ref["peak_score"][0] == four[0]


@pytest.mark.parametrize("bw", Q.CLI_WIDTHS)
@pytest.mark.parametrize("layout", Q.CLI_LAYOUTS)
def test_cli_layouts_hold_heads_gaps_and_leaks(layout, bw):
    contigs = Q.cli_contigs(layout, bw)
    assert len(contigs) in (3, 4)
    for tracks in Q.cli_tracks(layout, bw):
        for name, L, kind in contigs:
            p = [x for x, _ in tracks.get(name, [])]
            if kind == "empty":
                assert not p
            elif kind == "tiny":
                assert p and max(p) <= bw
            elif kind == "head":
                assert min(p) <= bw + 1 and max(p) > 4 * bw
            else:
                assert min(p) > bw + 1 and len(Q.runs_of(p, bw)) == 3


def test_profile_and_switch_units(oracle):
    length, pos, cnt = Q.profile_unit()
    assert int(pos.min()) > Q.PROFILE_BW + 1
    assert np.count_nonzero(oracle.profile(Q.PROFILE_BW, Q.BG, length, pos, cnt)) > length // 2
    length, pos, cnt, ep, ec = Q.switch_unit()
    bw = Q.SWITCH_BW
    assert int(pos.min()) > bw + 1 and int(ep.max()) <= length
    p2, c2 = Q.with_extra(pos, cnt, ep, ec)
    n = {}
    for key, (p, c) in (("before", (pos, cnt)), ("after", (p2, c2))):
        for thr in (25.0, 0.0):
            n[key, thr] = len(oracle.run_unit(bw, Q.BG, p, c, region_thr=thr)[0])
    assert n["before", 25.0] >= 1 and n["before", 0.0] >= 3
    assert n["after", 25.0] == n["before", 25.0] + 1 and n["after", 0.0] == n["before", 0.0] + 1


def test_first_replayed_unit(oracle):
    length, pos, cnt = Q.first_replayed_unit()
    assert len(oracle.run_unit(32_768, Q.BG, pos, cnt, region_thr=0.0)[0]) >= 1
