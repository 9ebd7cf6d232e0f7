"""The reference behind tests/test_gpu_shift_table.py, on the CPU: the oracle's
table of Region::strandCorr(0 .. max_shift) per candidate region
(orc_run_unit_shifts; misc/data.cpp:22-58, 184-193, src/strand_shift.cpp:
205-217) against two restatements it shares no code with --

* column 0 against the correlation orc_run_unit reports for the same region;
* the whole table against numpy's sequential sums over the oracle's dense
  profile of each strand alone (tests/shift_ref.py).

All three add in the reference's index order without contraction, so the
comparison is of bit patterns.  Then every input of the GPU cases is shown to
hold the shape it was built for, with every region's best shift clear of near
ties (shift_table_inputs.MARGIN)."""
import numpy as np
import pytest

from tests import shift_table_inputs as T
from tests.shift_ref import host_shift_table


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(both_nan | (a.view(np.uint64) == b.view(np.uint64))))


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("bw", [1, 50, 511])
def test_table_against_run_unit_and_numpy(oracle, bw, S):
    """units without head hits, threshold > 0"""
    rng = np.random.default_rng(9000 + 10 * bw + S)
    length, pos, cf, cr = T._blocks_unit(rng, bw, S=S, n=3)
    assert pos.min() > bw
    kw = dict(control=[0, 1, 0], coeffs=[0.6, 1.7]) if S == 3 else {}
    # (a hit threshold that rejects the short region alone: rejected candidates have table rows too)
    pooled = [0, 2] if S == 3 else [0]
    kw["hit_thr"] = float(np.sort(oracle.run_unit(bw, T.BG, pos, cf, cr, nondir=True)[1][:, pooled].sum(axis=1))[0] + 1)
    plain, plain_sums = oracle.run_unit(bw, T.BG, pos, cf, cr, nondir=True, **kw)
    max_shift = int(plain["npos"].min()) // 2 + 2  # (the shortest region runs out of shifts)
    regs, sums, tab = oracle.run_unit_shifts(bw, T.BG, pos, cf, cr, nondir=True, max_shift=max_shift, **kw)
    # orc_run_unit is unchanged by the table: the same records either way
    assert plain.tobytes() == regs.tobytes() and np.array_equal(plain_sums, sums)
    assert len(regs) >= 4 and (regs["accepted"] == 0).any() and (regs["accepted"] == 1).any()
    assert tab.shape == (len(regs), max_shift + 1)
    assert same_bits(tab[:, 0], regs["corr"])
    assert T.nan_cells_follow_length(regs, tab)
    assert np.isnan(tab).any() and not np.isnan(tab).all()
    want = host_shift_table(oracle, bw, T.BG, pos, cf, cr, regs, max_shift, control=kw.get("control"),
                            coeffs=kw.get("coeffs"))
    assert same_bits(want, tab)


@pytest.mark.parametrize("with_heads", [False, True], ids=["plain", "heads"])
def test_threshold_zero_regions_store_left_minus_one(oracle, with_heads):
    """region threshold 0 (quirk Q11): a region is reached by a leap, which
    stores the leap position without setting the left end (misc/peakcall.cpp:
    76-78), so the stored scores are those of left - 1 .. right - 1 of the
    reported record: the table equals numpy's over the dense profile at those
    positions, and differs from it over left .. right"""
    case = T.q11(with_heads)
    u = case["units"][0]
    (regs, _, tab), = T.oracle_tables(oracle, case)
    T.holds_q11((regs, None, tab))
    assert np.array_equal(regs["npos"], regs["right"] - regs["left"] + 1)
    if with_heads:
        return  # (the window of a head unit is misaligned, quirk Q1: no dense profile to compare with)
    stored = np.zeros(len(regs), [("left", "<u4"), ("right", "<u4")])
    stored["left"], stored["right"] = regs["left"] - 1, regs["right"] - 1
    over = lambda q: host_shift_table(oracle, case["bw"], T.BG, u["pos"], u["cf"], u["cr"], q, case["max_shift"])
    assert same_bits(over(stored), tab)
    assert not same_bits(over(regs), tab)


def test_missing_symbol_names_the_rebuild(oracle):
    """a library built before orc_run_unit_shifts existed fails with the
    command that rebuilds it, and still serves run_unit"""
    class Stale:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            if name == "orc_run_unit_shifts":
                raise AttributeError(name)
            return getattr(self._lib, name)

    from tests.oracle_binding import Oracle
    old = Oracle.__new__(Oracle)
    old.L = Stale(oracle.L)
    u = T.shortest()["units"][0]
    assert len(old.run_unit(1, T.BG, u["pos"], u["cf"], u["cr"], nondir=True)[0]) == 4
    with pytest.raises(RuntimeError, match="make -C oracle"):
        old.run_unit_shifts(1, T.BG, u["pos"], u["cf"], u["cr"], nondir=True, max_shift=2)


# ---- the GPU cases' inputs ---------------------------------------------------------

def all_cases(oracle):
    return ([T.widths(bw) for bw in T.WIDTHS] + [T.pooling(bw, m) for bw in (50, 300) for m in T.POOLING] +
            [T.lds(oracle), T.shortest(), T.degenerate(), T.contig_end(), T.several_units()] +
            [T.heads(bw) for bw in (50, 150)] + [T.q11(False), T.q11(True)])


def test_every_case_is_small_and_clear_of_ties(oracle):
    for case in all_cases(oracle):
        for u, (regs, sums, tab) in zip(case["units"], T.oracle_tables(oracle, case)):
            assert u["length"] <= 60_000 and u["pos"].max() <= u["length"], case["name"]
            assert len(regs) > 0 and tab.shape == (len(regs), case["max_shift"] + 1), case["name"]
            assert T.clear_of_ties(tab), case["name"]
            assert same_bits(tab[:, 0], regs["corr"]), case["name"]


@pytest.mark.parametrize("bw", T.WIDTHS)
def test_widths_inputs(oracle, bw):
    T.holds_widths(T.oracle_tables(oracle, T.widths(bw))[0])


@pytest.mark.parametrize("mode", T.POOLING)
@pytest.mark.parametrize("bw", [50, 300])
def test_pooling_inputs(oracle, bw, mode):
    case = T.pooling(bw, mode)
    T.holds_pooling(case, T.oracle_tables(oracle, case)[0])


def test_other_inputs(oracle):
    T.holds_lds(T.oracle_tables(oracle, T.lds(oracle))[0])
    T.holds_shortest(T.oracle_tables(oracle, T.shortest())[0])
    T.holds_degenerate(T.oracle_tables(oracle, T.degenerate())[0])
    T.holds_contig_end(T.contig_end(), T.oracle_tables(oracle, T.contig_end())[0])
    refs = T.oracle_tables(oracle, T.several_units())
    assert len(refs) == 3 and all(len(r[0]) >= 2 for r in refs)
    for bw in (50, 150):
        regs, _, tab = T.oracle_tables(oracle, T.heads(bw))[0]
        assert regs["left"][0] <= bw and len(regs) >= 3 and not np.isnan(tab).all()


def test_reference_best_rule():
    """shifts ascending, `>` from -1, NaN never wins, the first of equal maxima"""
    nan = np.nan
    tab = np.array([[nan, nan, nan], [0.5, 0.7, 0.7], [-1.0, nan, -1.0], [nan, -0.5, nan], [0.2, nan, 0.1]])
    best, corr = T.reference_best(tab)
    assert best.tolist() == [0, 1, 0, 1, 0] and corr.tolist() == [-1.0, 0.7, -1.0, -0.5, 0.2]
    assert not T.clear_of_ties(tab) and T.clear_of_ties(tab[[0, 2, 3, 4]])
