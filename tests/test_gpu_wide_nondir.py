"""K1w on nondirectional units (csrc/wide.hip, NONDIR): bandwidths 512..32767
with both strands in one buffer and a threshold > 0, through the blocking
up_run -- the screen on the unit's pooled plane, one ascending FP64 sum per
strand and forwardScore + reverseScore for the flags and the peak
(misc/peakcall.cpp:57, 207-209); strandCorr(0) of every region from
wide_corr_kernel between K2 and K3 (misc/data.cpp:38-58, 184-193), and the
dense (f, r) of requested regions for K4 from wide_fill_kernel.

The checker is the oracle (tests/oracle_binding.py), never the replay: every
candidate region (accepted and rejected), peak, counts and FP64 peak score
bit-exact, kurtosis and correlation within 1e-12; CLI outputs byte-identical
to the oracle CLI (the CLI cases add -m to their command lines: MAPPABLE
below).  up_last_scan_kind tells which path found the regions, so
a change of the dispatch cannot turn these into tests of the replay.
tests/test_wide_nd_oracle.py shows on the CPU that the inputs hold what the
cases rely on."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import wide_nd_inputs as W
from tests.shift_ref import host_shift_table
from tests.test_cli import compare_tool, make_inputs, run
from tests.test_gpu_replay import close, compare
from tests.wig import write_contigs, write_wig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP_CLOSE_RULE = 0xFFFFFFFF
K1W, REPLAY = 1, 3  # up_last_scan_kind


def run_kind(capi, bw, bg, units, policy=None, passes=1, capture=False, **kw):
    """tests.test_gpu_replay.run_units for nondirectional units, with the scan kind of the pass
    -> (records, counts, kind) of the last of `passes` runs, every run's
    records asserted identical"""
    S = units[0][2].shape[1]
    with capi.Lib(0) as g:
        g.set_params(bw, S, bg, nondir=True, **kw)
        if policy is not None:
            g.set_index_policy(policy)
        if capture:
            g.set_profile_capture(True)
        for length, pos, cf, cr in units:
            u = g.add_unit(length)
            for st, c in enumerate((cf, cr)):
                for s in range(S):
                    m = c[:, s] != 0
                    if m.any():
                        g.scatter(u, st, s, pos[m], c[m, s])
        first = None
        for _ in range(passes):
            n = g.run()
            regs, cnt = g.regions(n)
            if first is None:
                first = (regs.tobytes(), cnt.tobytes())
            assert (regs.tobytes(), cnt.tobytes()) == first
        return regs, cnt, g.last_scan_kind()


# ---- 1. parity, one sample ----------------------------------------------------

@pytest.fixture(scope="module")
def parity_ref(oracle):
    """oracle records of the parity inputs, with and without the correlation filter"""
    out = {}
    for bw in W.PARITY_SEEDS:
        length, pos, cf, cr = W.parity_unit(bw)
        out[bw] = (length, pos, cf, cr,
                   oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3),
                   oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=-1.0))
    return out


@pytest.mark.parametrize("want_corr", [True, False])
@pytest.mark.parametrize("bw", sorted(W.PARITY_SEEDS))
def test_parity_one_sample(gpu_lib, parity_ref, bw, want_corr):
    length, pos, cf, cr, with_corr, no_corr = parity_ref[bw]
    ref, ref_sums = with_corr if want_corr else no_corr
    # what the seed was chosen for, from the oracle alone
    assert np.any(with_corr[0]["accepted"] == 1)
    assert np.any((no_corr[0]["accepted"] == 1) & (with_corr[0]["accepted"] == 0))
    assert np.any(W.crosses_strip(ref))
    regs, cnt, kind = run_kind(gpu_lib, bw, W.BG, [(length, pos, cf, cr)],
                               corr_thr=0.3 if want_corr else -1.0, want_corr=want_corr)
    assert kind == K1W
    assert np.all(regs["close_pos"] == UP_CLOSE_RULE)
    compare(ref, ref_sums, regs, cnt, corr=want_corr)
    if not want_corr:  # (the oracle always evaluates it; the library only when asked to)
        assert np.all(np.isnan(regs["corr"]))


# ---- 2. pooling ---------------------------------------------------------------

@pytest.mark.parametrize("coeffs", [None, [0.6, 1.7]])
def test_pooled_control(gpu_lib, oracle, coeffs):
    bw, S, control = 700, 3, [0, 1, 0]
    length, pos, cf, cr = W.parity_unit(bw, S=S, length=150_000, seed=702)
    ref, ref_sums = oracle.run_unit(bw, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3, control=control,
                                    coeffs=coeffs)
    regs, cnt, kind = run_kind(gpu_lib, bw, W.BG, [(length, pos, cf, cr)], corr_thr=0.3, want_corr=True,
                               control=control, coeffs=coeffs)
    assert kind == K1W and len(ref) > 3
    compare(ref, ref_sums, regs, cnt, corr=True)


# ---- 3. one-strand regions ------------------------------------------------------

def test_one_strand_regions(gpu_lib, oracle):
    """one strand's scores all zero: the reference's 0/0 correlation (NaN) and
    what its filter makes of it"""
    length, pos, cf, cr = W.one_strand_unit()
    ref, ref_sums = oracle.run_unit(W.ONE_STRAND_BW, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    assert len(ref) == 2 and np.all(np.isnan(ref["corr"])) and not ref["accepted"].any()
    regs, cnt, kind = run_kind(gpu_lib, W.ONE_STRAND_BW, W.BG, [(length, pos, cf, cr)], corr_thr=0.3,
                               want_corr=True)
    assert kind == K1W
    compare(ref, ref_sums, regs, cnt, corr=True)


# ---- 4. heads and ends ----------------------------------------------------------

def test_head_unit_and_contig_end(gpu_lib, oracle):
    """two units of one buffer; the first has tags at positions <= bw on the
    reverse strand only (quirk Q1: the K0 replay of its start, which emits the
    region that starts there), a tag at len and a region whose right end lies
    past the contig end.  Then K4 over all of them: replayed regions (their
    stored scores) beside K1w regions (wide_fill_kernel) in one up_shift_scan"""
    bw = W.HEAD_BW
    u0 = W.head_unit()
    length = u0[0]
    u1 = W.parity_unit(bw, length=50_000, seed=412)
    refs = [oracle.run_unit(bw, W.BG, u[1], u[2], u[3], nondir=True, corr_thr=0.3) for u in (u0, u1)]
    assert np.any(refs[0][0]["right"] > length) and refs[0][0]["left"][0] <= bw
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, W.BG, nondir=True, corr_thr=0.3, want_corr=True)
        for L, pos, cf, cr in (u0, u1):
            u = g.add_unit(L)
            for st, c in enumerate((cf, cr)):
                m = c[:, 0] != 0
                g.scatter(u, st, 0, pos[m], c[m, 0])
        n = g.run()
        regs, cnt = g.regions(n)
        assert g.last_scan_kind() == K1W  # (the head unit's K0 chain does not change it)
        tab = g.shift_scan(np.arange(n, dtype=np.uint64), 150)
    for u, (ref, ref_sums) in enumerate(refs):
        m = regs["unit"] == u
        compare(ref, ref_sums, regs[m], cnt[m], corr=True)
    replayed = regs["close_pos"] != UP_CLOSE_RULE  # the head chain's records
    assert replayed.any() and not replayed.all() and not replayed[regs["unit"] == 1].any()
    # strandCorr(0) of every region, replayed or not, is the record's own
    # correlation (compared with the oracle above)
    assert close(regs["corr"], tab[:, 0])
    # the K1w regions against the host recomputation over the oracle's dense f and r
    for u, (L, pos, cf, cr) in enumerate((u0, u1)):
        k = np.flatnonzero((regs["unit"] == u) & ~replayed)
        assert close(host_shift_table(oracle, bw, W.BG, pos, cf, cr, regs[k], 150), tab[k])


def test_q1_leak_into_next_unit_cli(orc_bin, gpu_lib, tmp_path):
    """every add of contig c1 sits at a position <= bw, so the buffer's state
    leaks into c2 (quirk Q1): tables byte-identical to the oracle CLI (-m: the
    background that lets these few tags reach the default -r 25, see MAPPABLE)"""
    bw = 700
    rng = np.random.default_rng(42)
    contigs = [("c0", 60_000), ("c1", 30_000), ("c2", 50_000)]
    fwd, rev = {}, {}
    for d, shift in ((fwd, 0), (rev, 100)):
        for name, L in contigs:
            dense = {}
            if name != "c1":
                for c in rng.integers(3 * bw, L - 3 * bw, 4):
                    for o in np.rint(rng.normal(0, 150, 120)).astype(int):
                        p = int(c) + shift + int(o)
                        dense[p] = dense.get(p, 0) + 1
            if name != "c0":  # head tags
                for p in rng.integers(1, bw + 1, 6):
                    dense[int(p)] = dense.get(int(p), 0) + int(rng.integers(3, 9))
            d[name] = sorted(dense.items())
    write_contigs(tmp_path / "contigs.txt", contigs)
    write_wig(tmp_path / "s0.wig", "s0", fwd, rev)
    out = compare_tool(orc_bin, tmp_path, "regions",
                       ["-q", "-c", "contigs.txt", "-D", "-y", "-f", "-k", "0", "-b", str(bw), "-m", "5000000",
                        "s0.wig"])
    assert sum(1 for l in out.splitlines() if l.startswith("c2:")) >= 1  # a region of the unit leaked into


# ---- 5. stress of the new kernels' branches -------------------------------------

def test_stress_fallback_escapes_saturation_long_region(gpu_lib, oracle):
    """a stretch whose windows hold more hits than the LDS list (the fallback
    walk), counts >= 3 (escape table), a reverse chunk of >= 255 tags (a
    saturated plane entry) and a region longer than wide_corr_kernel's slab"""
    length, pos, cf, cr = W.stress_unit()
    ref, ref_sums = oracle.run_unit(W.STRESS_BW, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    assert np.any(ref["right"] - ref["left"] + 1 > 2 * W.SLAB)
    regs, cnt, kind = run_kind(gpu_lib, W.STRESS_BW, W.BG, [(length, pos, cf, cr)], corr_thr=0.3, want_corr=True)
    assert kind == K1W
    compare(ref, ref_sums, regs, cnt, corr=True)
    with gpu_lib.Lib(0) as g:  # K4's fill of the same regions (fallback walk, several stretches)
        tab, want = shift_tables(g, oracle, W.STRESS_BW, length, pos, cf, cr, 150)
    assert close(want, tab)


# ---- 6. limits -------------------------------------------------------------------

def wrap_unit(seed, length=480_000):
    """clusters 75,000 - 120,000 apart with nothing between them, on both
    strands (the layout of test_gpu_wide.py::test_ushort_retirement_wrap)"""
    rng = np.random.default_rng(seed)
    df, dr = {}, {}
    for d, shift in ((df, 0), (dr, 200)):
        for c, n in ((20_000, 300), (95_000, 260), (215_000, 400), (290_000, 220), (400_000, 350)):
            for o in np.rint(rng.normal(0, 80, n)).astype(np.int64):
                d[int(c + shift + o)] = d.get(int(c + shift + o), 0) + 1
    return (length,) + W.from_dense(df, dr)


def test_widest_kernel(gpu_lib, oracle):
    """bw 32767 on 120,000 positions with a few hundred tags, none at a
    position <= bw: no head unit, so the records, the correlation and K4's
    scores all come from the wide kernels (31 KB of LDS in wide_corr_kernel,
    a region of 24 slabs)"""
    bw = W.LIMIT_BW
    length, pos, cf, cr = W.limit_unit()
    assert pos.min() > bw
    ref, ref_sums = oracle.run_unit(bw, W.LIMIT_BG, pos, cf, cr, nondir=True, cap=1 << 20, **W.LIMIT_KW)
    assert len(ref) >= 1
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, W.LIMIT_BG, nondir=True, want_corr=True, **W.LIMIT_KW)
        u = g.add_unit(length)
        for st, c in enumerate((cf, cr)):
            m = c[:, 0] != 0
            g.scatter(u, st, 0, pos[m], c[m, 0])
        n = g.run()
        regs, cnt = g.regions(n)
        assert g.last_scan_kind() == K1W
        tab = g.shift_scan(np.arange(n, dtype=np.uint64), 3)
    assert np.all(regs["close_pos"] == UP_CLOSE_RULE)  # no replayed record
    compare(ref, ref_sums, regs, cnt, corr=True)
    assert close(host_shift_table(oracle, bw, W.LIMIT_BG, pos, cf, cr, regs, 3), tab)


def test_first_replayed_kernel(gpu_lib, oracle):
    """bw 32768: the reference's UShort retirement count wraps, the
    whole-buffer replay"""
    bw = 32768
    length, pos, cf, cr = wrap_unit(bw)
    ref, ref_sums = oracle.run_unit(bw, W.LIMIT_BG, pos, cf, cr, nondir=True, cap=1 << 20, **W.LIMIT_KW)
    assert len(ref) > 0
    regs, cnt, kind = run_kind(gpu_lib, bw, W.LIMIT_BG, [(length, pos, cf, cr)], want_corr=True, **W.LIMIT_KW)
    assert kind == REPLAY
    compare(ref, ref_sums, regs, cnt, corr=True)


def test_threshold_zero_and_capture_keep_the_replay(gpu_lib, oracle):
    length, pos, cf, cr = W.one_strand_unit()  # (clusters far apart: a leap closes the first region)
    ref, ref_sums = oracle.run_unit(600, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3, region_thr=0.0)
    regs, cnt, kind = run_kind(gpu_lib, 600, W.BG, [(length, pos, cf, cr)], corr_thr=0.3, want_corr=True,
                               region_thr=0.0)
    assert kind == REPLAY and len(ref) == 1
    compare(ref, ref_sums, regs, cnt, corr=True)
    length, pos, cf, cr = W.parity_unit(700, length=60_000, seed=611)
    ref, ref_sums = oracle.run_unit(600, W.BG, pos, cf, cr, nondir=True, corr_thr=0.3)
    regs, cnt, kind = run_kind(gpu_lib, 600, W.BG, [(length, pos, cf, cr)], corr_thr=0.3, want_corr=True,
                               capture=True)
    assert kind == REPLAY
    compare(ref, ref_sums, regs, cnt, corr=True)


# ---- 7. index states --------------------------------------------------------------

@pytest.mark.parametrize("policy,passes", [("INDEX_AUTO", 2), ("INDEX_NEVER", 1)])
def test_index_states(gpu_lib, parity_ref, policy, passes):
    length, pos, cf, cr, (ref, ref_sums), _ = parity_ref[700]
    regs, cnt, kind = run_kind(gpu_lib, 700, W.BG, [(length, pos, cf, cr)], policy=getattr(gpu_lib, policy),
                               passes=passes, corr_thr=0.3, want_corr=True)
    assert kind == K1W
    compare(ref, ref_sums, regs, cnt, corr=True)


# ---- 8. K4 -------------------------------------------------------------------------

def shift_tables(g, oracle, bw, length, pos, cf, cr, max_shift):
    """(up_shift_scan's table, the host recomputation) of every region of one
    unit without head hits, in reverse index order"""
    g.set_params(bw, 1, W.BG, nondir=True)
    u = g.add_unit(length)
    for st, c in enumerate((cf, cr)):
        m = c[:, 0] != 0
        g.scatter(u, st, 0, pos[m], c[m, 0])
    n = g.run()
    assert g.last_scan_kind() == K1W and n > 0
    regs, _ = g.regions(n)
    idx = np.arange(n, dtype=np.uint64)[::-1].copy()
    tab = g.shift_scan(idx, max_shift)
    return tab, host_shift_table(oracle, bw, W.BG, pos, cf, cr, regs[::-1], max_shift)


@pytest.mark.parametrize("max_shift", [0, 150, 600])
def test_shift_scan_and_best(gpu_lib, oracle, parity_ref, max_shift):
    bw = 700
    length, pos, cf, cr = parity_ref[bw][:4]
    with gpu_lib.Lib(0) as g:
        tab, want = shift_tables(g, oracle, bw, length, pos, cf, cr, max_shift)
        n = tab.shape[0]
        idx = np.arange(n, dtype=np.uint64)[::-1].copy()
        best, bc = g.shift_best(idx, max_shift)
    assert close(want, tab)
    if max_shift == 600:  # a region shorter than 2 * shift + 3
        assert np.isnan(want).any() and not np.isnan(want).all()
    for k in range(n):
        b, c = 0, -1.0
        for s in range(max_shift + 1):
            if tab[k, s] > c:
                b, c = s, tab[k, s]
        assert best[k] == b and bc[k] == c, (k, max_shift)


# ---- 9. CLIs -----------------------------------------------------------------------

CONTIGS = [("chrA", 200_000), ("chrB", 90_000), ("chrC", 40_000)]
# The command lines are the ones the cases name plus -m: the background is
# tags over -m mappable positions, and over the contigs' own 330,000 positions
# no score of these inputs reaches the default -r 25 at these bandwidths -- the
# tables and the strand_shift histogram would be empty.  (The Q1 leak case
# above adds -m 5000000 for the same reason.)
MAPPABLE = ["-m", "20000000"]


@pytest.mark.parametrize("bw", ["700", "2000"])
def test_regions_cli(orc_bin, gpu_lib, tmp_path, bw):
    ct, files = make_inputs(tmp_path, 170 + int(bw), CONTIGS, 1, shift_rev=100, n_cl=12, sd=200)
    out = compare_tool(orc_bin, tmp_path, "regions", ["-q", "-c", ct, "-D", "-y", "-f", "-k", "0", "-b", bw] + MAPPABLE
                       + files)
    assert sum(1 for l in out.splitlines() if l.startswith("chr")) >= 10


def test_strand_shift_cli(orc_bin, gpu_lib, tmp_path):
    ct, files = make_inputs(tmp_path, 171, CONTIGS, 1, shift_rev=100, n_cl=12, sd=200)
    out = compare_tool(orc_bin, tmp_path, "strand_shift", ["-c", ct, "-x", "100", "-b", "700"] + MAPPABLE + files)
    assert "# best_shift=" in out and "# regions_tested=0" not in out


def test_regions_cli_capture_keeps_the_replay(orc_bin, gpu_lib, tmp_path):
    """-w on a nondirectional wide unit: still the replay; table and profile
    byte-identical to the oracle CLI"""
    ct, files = make_inputs(tmp_path, 172, CONTIGS, 1, shift_rev=100, n_cl=12, sd=200)
    common = ["-q", "-c", ct, "-D", "-y", "-f", "-k", "0", "-b", "600"] + MAPPABLE
    (tmp_path / "ref").mkdir()
    (tmp_path / "got").mkdir()
    run([orc_bin, "regions"] + common + ["-w", "ref/p.wig", "-o", "ref/r.txt"] + files, tmp_path)
    run([os.path.join(ROOT, "bin", "regions")] + common + ["-w", "got/p.wig", "-o", "got/r.txt"] + files,
        tmp_path)
    assert (tmp_path / "ref/r.txt").read_bytes() == (tmp_path / "got/r.txt").read_bytes()
    a, b = (tmp_path / "ref/p.wig").read_bytes(), (tmp_path / "got/p.wig").read_bytes()
    assert a.count(b"\n") > 1000 and a == b


# ---- 10. A/B switch ------------------------------------------------------------------

AB_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
if torch.cuda.is_available():
    torch.cuda.init()
from unipeak_amd import capi
from tests import wide_nd_inputs as W
from tests.test_gpu_wide_nondir import run_kind
length, pos, cf, cr = W.parity_unit(700)
regs, cnt, kind = run_kind(capi, 700, W.BG, [(length, pos, cf, cr)], corr_thr=0.3, want_corr=True)
np.savez(sys.argv[2], regs=regs, cnt=cnt, kind=kind)
"""


def test_wide_nd_switch_keeps_the_replay(gpu_lib, parity_ref, tmp_path):
    """UNIPEAK_WIDE_ND=0 (read at up_open): a fresh process takes the replay
    and finds the same records"""
    out = tmp_path / "ab.npz"
    env = dict(os.environ, UNIPEAK_WIDE_ND="0")
    r = subprocess.run([sys.executable, "-c", AB_CHILD, ROOT, str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert int(z["kind"]) == REPLAY
    ref, ref_sums = parity_ref[700][4]
    compare(ref, ref_sums, z["regs"], z["cnt"], corr=True)
