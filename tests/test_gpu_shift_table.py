"""K4 at bandwidths up to 511 (shift_kernel<NH, POOL>, kernels.hip): the table
of up_shift_scan and the choice of up_shift_best against the reference's
Region::strandCorr(shift) (misc/data.cpp:22-58, 184-193) and its rule for the
best shift (src/strand_shift.cpp:209-217), both from the oracle
(orc_run_unit_shifts), never from another GPU path.

Every case: the record list equals the oracle's in order; the table has NaN
in the oracle's cells and the oracle's bits everywhere else (shift_kernel adds
in the reference's index order, the library is built without contraction, and
add, multiply, divide and sqrt are correctly rounded on the device); the best
shift is the reference's rule applied to the ORACLE's table, whose rows are
asserted clear of near ties (shift_table_inputs.MARGIN), and the best
correlation has that cell's bits.  What a case was built to reach -- region
lengths around kShiftLds, NaN cells, replayed records, a pooling mode -- is
asserted from the oracle's output (shift_table_inputs.holds_*), and
tests/test_oracle_shift.py shows the same on the CPU."""
import numpy as np
import pytest

from tests import shift_table_inputs as T

pytestmark = pytest.mark.gpu

UP_CLOSE_RULE = 0xFFFFFFFF
K1, K1Q = 0, 2           # up_last_scan_kind
HOST, PLACED = 0, 1      # up_last_head_kind
UP_E_ARG, UP_E_STATE, UP_E_UNSUPPORTED = -1, -4, -5


def ulp_distance(a, b):
    """largest distance in units of the last place between two arrays of finite doubles of equal sign"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.size == 0:
        return 0
    return int(np.abs(a.view(np.int64) - b.view(np.int64)).max())


def load(g, case):
    g.set_params(case["bw"], case["S"], case["bg"], region_thr=case["thr"], kurt_thr=case["kurt_thr"],
                 hit_thr=case["hit_thr"], nondir=True, control=case["control"], coeffs=case["coeffs"])
    for u in case["units"]:
        uid = g.add_unit(u["length"], u["buffer"])
        for st, c in enumerate((u["cf"], u["cr"])):
            for s in range(case["S"]):
                m = c[:, s] != 0
                if m.any():
                    g.scatter(uid, st, s, u["pos"][m], c[m, s])


def reference(oracle, case):
    """the oracle's records (unit, left, right, sum), exptSums and table, unit-major"""
    refs = T.oracle_tables(oracle, case)
    unit = np.concatenate([np.full(len(r[0]), i) for i, r in enumerate(refs)])
    regs = np.concatenate([r[0] for r in refs])
    sums = np.concatenate([r[1] for r in refs])
    tab = np.concatenate([r[2] for r in refs])
    assert T.clear_of_ties(tab), "an input with a near tie for the best shift"
    return unit, regs, sums, tab


def check(g, oracle, case, idx=None, kind=K1):
    """run the loaded context, compare the records, then up_shift_scan and
    up_shift_best of the regions `idx` (default: all, descending) with the
    oracle's rows -> the records"""
    unit, ref, ref_sums, ref_tab = reference(oracle, case)
    n = g.run()
    regs, cnt = g.regions(n)
    assert g.last_scan_kind() == kind
    assert n == len(ref), (n, len(ref))
    for k, want in (("unit", unit), ("left", ref["left"]), ("right", ref["right"]), ("sum", ref["sum"])):
        assert np.array_equal(regs[k], want), k
    assert np.array_equal(cnt, ref_sums)
    if idx is None:
        idx = np.arange(n, dtype=np.uint64)[::-1].copy()
    max_shift = case["max_shift"]
    tab = g.shift_scan(idx, max_shift)
    best, best_corr = g.shift_best(idx, max_shift)
    want = ref_tab[idx.astype(np.int64)]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(tab), nan), "NaN in other cells than the reference's"
    print(case["name"], "regions", n, "cells", want.size, "NaN", int(nan.sum()), "largest ulp distance",
          ulp_distance(tab[~nan], want[~nan]))
    assert tab[~nan].tobytes() == want[~nan].tobytes()
    want_best, want_corr = T.reference_best(want)
    assert np.array_equal(best, want_best)
    assert best_corr.tobytes() == want_corr.tobytes()
    return regs


def run_case(gpu_lib, oracle, case, **kw):
    with gpu_lib.Lib(0) as g:
        load(g, case)
        return check(g, oracle, case, **kw)


# ---- window widths: both sides of every NH = bw / 64 + 1 step ----------------------

@pytest.mark.parametrize("bw", T.WIDTHS)
def test_widths(gpu_lib, oracle, bw):
    case = T.widths(bw)
    T.holds_widths(T.oracle_tables(oracle, case)[0])
    run_case(gpu_lib, oracle, case)


# ---- pooling modes (the context has no query for it: shift_table_inputs.pooling argues
# each case's mode from its inputs against api.hip pool_mode(), holds_pooling evaluates it) --

@pytest.mark.parametrize("mode", T.POOLING)
@pytest.mark.parametrize("bw", [50, 300])
def test_pooling_modes(gpu_lib, oracle, bw, mode):
    case = T.pooling(bw, mode)
    T.holds_pooling(case, T.oracle_tables(oracle, case)[0])
    run_case(gpu_lib, oracle, case)


# ---- LDS / slab boundary and the loops' tails ---------------------------------------

def test_lds_slab_boundary(gpu_lib, oracle):
    """regions of 2,047, 2,048, 2,049 and 4,200 positions requested in mixed
    order in one call, each several times (shift_table_inputs.LDS_IDX): slab
    offsets for a mixture of LDS and slab regions; max_shift 1,100"""
    case = T.lds(oracle)
    T.holds_lds(T.oracle_tables(oracle, case)[0])
    run_case(gpu_lib, oracle, case, idx=T.LDS_IDX)


# ---- shortest regions ------------------------------------------------------------------

def test_shortest_regions(gpu_lib, oracle):
    """1, 3, 4 and 5 positions at max_shift 2: NaN for len <= 3, shift 0 alone for 4 and 5"""
    case = T.shortest()
    T.holds_shortest(T.oracle_tables(oracle, case)[0])
    run_case(gpu_lib, oracle, case)


# ---- degenerate strands -------------------------------------------------------------------

def test_degenerate_strands(gpu_lib, oracle):
    """a region without reverse tags: every cell 0 / 0, best (0, -1.0); one whose
    reverse scores are constant from some shift on"""
    case = T.degenerate()
    T.holds_degenerate(T.oracle_tables(oracle, case)[0])
    with gpu_lib.Lib(0) as g:
        load(g, case)
        check(g, oracle, case)
        best, corr = g.shift_best(np.array([0], np.uint64), case["max_shift"])
    assert best[0] == 0 and corr[0] == -1.0


# ---- contig end -----------------------------------------------------------------------------

def test_region_past_the_contig_end(gpu_lib, oracle):
    case = T.contig_end()
    T.holds_contig_end(case, T.oracle_tables(oracle, case)[0])
    run_case(gpu_lib, oracle, case)


# ---- several units ----------------------------------------------------------------------------

def test_three_units_two_buffers(gpu_lib, oracle):
    """idx descending across the units (the reg_unit lookup)"""
    case = T.several_units()
    assert [u["buffer"] for u in case["units"]] == [0, 1, 1]
    regs = run_case(gpu_lib, oracle, case)
    assert set(regs["unit"]) == {0, 1, 2}


# ---- replayed regions (quirk Q1) ------------------------------------------------------------------

@pytest.mark.parametrize("placed", [False, True], ids=["host_merge", "placed"])
@pytest.mark.parametrize("bw", [50, 150])
def test_replayed_regions(gpu_lib, oracle, bw, placed):
    """a head unit: the replay's records bring the scores the state machine
    stored (h_score_off with the host merge, d_hp_soff when placed inside the
    pass), the others are formed by K4's own KDE; all against the oracle"""
    case = T.heads(bw)
    with gpu_lib.Lib(0) as g:
        load(g, case)
        g.set_head_place(placed)
        regs = check(g, oracle, case)
        assert g.last_head_kind() == (PLACED if placed else HOST)
    replayed = regs["close_pos"] != UP_CLOSE_RULE
    assert replayed.any() and not replayed.all()


# ---- threshold <= 0 on narrow nondirectional units (K1q, placed by q11place.hip) --------------------

@pytest.mark.parametrize("with_heads", [False, True], ids=["plain", "heads"])
def test_threshold_zero(gpu_lib, oracle, with_heads):
    """K1q records are reached by a leap: the region stores the positions
    left - 1 .. right - 1 of its record -- as many as right - left + 1, one
    position to the left (tests/test_oracle_shift.py holds the oracle's rows
    against numpy's over exactly those positions of the dense profile)"""
    case = T.q11(with_heads)
    regs, _, tab = T.oracle_tables(oracle, case)[0]
    T.holds_q11((regs, None, tab))
    assert np.array_equal(regs["npos"], regs["right"] - regs["left"] + 1)
    assert (regs["left"][0] == 1) == with_heads  # the head unit processes position 1
    run_case(gpu_lib, oracle, case, kind=K1Q)


# ---- refusals ------------------------------------------------------------------------------------------

def test_refusals(gpu_lib, oracle):
    case = T.shortest()
    idx = np.zeros(1, np.uint64)
    with gpu_lib.Lib(0) as g:
        load(g, case)
        for call in (g.shift_scan, g.shift_best):  # before any run
            with pytest.raises(gpu_lib.UpError) as e:
                call(idx, 2)
            assert e.value.code == UP_E_STATE
        n = g.run()
        for call in (g.shift_scan, g.shift_best):  # an index past the record list
            with pytest.raises(gpu_lib.UpError) as e:
                call(np.array([0, n], np.uint64), 2)
            assert e.value.code == UP_E_ARG
        assert g.shift_scan(np.array([n - 1], np.uint64), 2).shape == (1, 3)
    u = case["units"][0]
    with gpu_lib.Lib(0) as g:  # a directional context
        g.set_params(1, 1, T.BG, kurt_thr=0.0, hit_thr=0.0)
        uid = g.add_unit(u["length"])
        m = u["cf"][:, 0] != 0
        g.scatter(uid, 0, 0, u["pos"][m], u["cf"][m, 0])
        assert g.run() > 0
        for call in (g.shift_scan, g.shift_best):
            with pytest.raises(gpu_lib.UpError) as e:
                call(idx, 2)
            assert e.value.code == UP_E_UNSUPPORTED
