"""Wide K1q (csrc/wide.hip): a threshold <= 0 at bandwidths 512..32767 on
directional units in parallel -- wide_runs_kernel finds the runs of processed
positions, wide_peak_kernel / wide_peak_merge_kernel their first maxima, K2,
K3 (known peaks), the K1q placement and the K0 head chains follow as behind
narrow K1q.

The checker is the oracle (tests/oracle_binding.py), never the replay: every
record's left / right / peak / sum / accepted and per-sample counts equal, the
FP64 peak score byte-equal, kurtosis within 1e-12; CLI tables byte-identical
to the oracle CLI's.  up_last_scan_kind tells which path found the regions (2:
K1q; the parent commit reports 3, the replay, for every parity case here).
tests/test_wide_q11_oracle.py shows on the CPU that the inputs hold what the
cases rely on."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import wide_nd_inputs as W
from tests import wide_q11_inputs as Q
from tests.test_cli import BIN, compare_tool
from tests.test_gpu_replay import compare
from tests.wig import write_contigs, write_wig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K1W, K1Q, REPLAY = 1, 2, 3  # up_last_scan_kind


def load(g, unit, buffer_id=0):
    length, pos, cnt = unit
    u = g.add_unit(length, buffer_id=buffer_id)
    for s in range(cnt.shape[1]):
        m = cnt[:, s] != 0
        if m.any():
            g.scatter(u, 0, s, pos[m], cnt[m, s])
    return u


def run_kind(capi, bw, unit, capture=False, policy=None, **kw):
    """one blocking pass over one directional unit -> (records, counts, scan kind, K1b kind)"""
    with capi.Lib(0) as g:
        g.set_params(bw, unit[2].shape[1], Q.BG, **kw)
        if policy is not None:
            g.set_index_policy(policy)
        if capture:
            g.set_profile_capture(True)
        load(g, unit)
        n = g.run()
        regs, cnt = g.regions(n)
        return regs, cnt, g.last_scan_kind(), g.last_exact_kind()


def check(capi, oracle, bw, unit, kind=K1Q, **kw):
    ref, ref_sums = oracle.run_unit(bw, Q.BG, unit[1], unit[2], **kw)
    regs, cnt, k, k1b = run_kind(capi, bw, unit, **kw)
    assert k == kind
    if kind == K1Q:
        assert k1b == -1
    compare(ref, ref_sums, regs, cnt)
    return ref


# ---- 2. widths and thresholds ---------------------------------------------------------

@pytest.fixture(scope="module")
def clustered():
    return {bw: Q.clustered_unit(bw) for bw in Q.WIDTHS}


@pytest.mark.parametrize("thr", Q.THRESHOLDS)
@pytest.mark.parametrize("bw", Q.WIDTHS)
def test_widths_and_thresholds(gpu_lib, oracle, clustered, bw, thr):
    ref = check(gpu_lib, oracle, bw, clustered[bw], region_thr=thr)
    assert len(ref) >= 3


# ---- 3. gap edges ----------------------------------------------------------------------

@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("bw", Q.EDGE_WIDTHS)
def test_gap_edges(gpu_lib, oracle, bw, which):
    unit = Q.edge_units(bw)[which]
    ref = check(gpu_lib, oracle, bw, unit, region_thr=0.0)
    assert [(int(l), int(r)) for l, r in zip(ref["left"], ref["right"])] == Q.expected_bounds(unit[1], bw)


@pytest.mark.parametrize("bw", Q.EDGE_WIDTHS)
def test_run_to_the_domain_end_and_an_empty_unit_cli(orc_bin, gpu_lib, tmp_path, bw):
    """contig c0 ends with an add at its last position (a run ending at len + bw,
    reported by the buffer's next unit with records), c1 holds no tag, c2 a few"""
    L = 8 * bw
    contigs = [("c0", L), ("c1", 3 * bw), ("c2", L)]
    fwd = {"c0": [(2 * bw, 1), (5 * bw, 2), (L, 3)], "c2": [(2 * bw, 1), (5 * bw, 1)]}
    rev = {"c0": [(3 * bw, 2), (L - 1, 1), (L, 1)], "c2": [(3 * bw, 4), (6 * bw, 1)]}
    write_contigs(tmp_path / "contigs.txt", contigs)
    write_wig(tmp_path / "s0.wig", "s0", fwd, rev)
    out = compare_tool(orc_bin, tmp_path, "regions",
                       ["-q", "-c", "contigs.txt", "-b", str(bw), "-m", "3000", "-f", "-r", "0", "-k", "0", "-t", "0",
                        "s0.wig"])
    # (the moved record: the next unit's name, the previous unit's positions)
    assert f"c2:{L - bw + 1}-{L + bw + 1}\t" in out


# ---- 4. controls and pooling --------------------------------------------------------------

@pytest.mark.parametrize("coeffs", Q.POOL_COEFFS)
def test_controls_and_pooling(gpu_lib, oracle, coeffs):
    ref = check(gpu_lib, oracle, Q.POOL_BW, Q.pooled_unit(), control=Q.POOL_CONTROL, coeffs=coeffs, region_thr=0.0,
                kurt_thr=0.0)
    assert len(ref) == 6


# ---- 5. peak reduction ---------------------------------------------------------------------

@pytest.mark.parametrize("where", ["last", "first"])
def test_long_region_peak(gpu_lib, oracle, where):
    ref = check(gpu_lib, oracle, Q.LONG_BW, Q.long_unit(where), region_thr=0.0)
    assert len(ref) == 1 and ref["right"][0] - ref["left"][0] + 1 >= 150_000


def test_tie_takes_the_first_maximum(gpu_lib, oracle):
    ref = check(gpu_lib, oracle, Q.TIE_BW, Q.tie_unit(), region_thr=0.0)
    assert int(ref["peak"][0]) == Q.TIE_A + 1


# ---- 1. what keeps the replay ------------------------------------------------------------------

def test_negative_coefficient_keeps_the_replay(gpu_lib, oracle):
    check(gpu_lib, oracle, Q.POOL_BW, Q.pooled_unit(), kind=REPLAY, control=Q.POOL_CONTROL, coeffs=[-0.5, 1.5],
          region_thr=0.0, kurt_thr=0.0)


def test_capture_keeps_the_replay(gpu_lib, oracle):
    unit = Q.clustered_unit(600)
    ref, ref_sums = oracle.run_unit(600, Q.BG, unit[1], unit[2], region_thr=0.0)
    regs, cnt, kind, _ = run_kind(gpu_lib, 600, unit, capture=True, region_thr=0.0)
    assert kind == REPLAY
    compare(ref, ref_sums, regs, cnt)


def test_nondirectional_keeps_the_replay(gpu_lib, oracle):
    length, pos, cf, cr = W.one_strand_unit()
    ref, ref_sums = oracle.run_unit(600, W.BG, pos, cf, cr, nondir=True, region_thr=0.0)
    with gpu_lib.Lib(0) as g:
        g.set_params(600, 1, W.BG, nondir=True, region_thr=0.0)
        u = g.add_unit(length)
        for st, c in enumerate((cf, cr)):
            m = c[:, 0] != 0
            g.scatter(u, st, 0, pos[m], c[m, 0])
        regs, cnt = g.regions(g.run())
        assert g.last_scan_kind() == REPLAY
    compare(ref, ref_sums, regs, cnt)


def test_bw_32768_keeps_the_replay(gpu_lib, oracle):
    check(gpu_lib, oracle, 32_768, Q.first_replayed_unit(), kind=REPLAY, region_thr=0.0)


AB_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
if torch.cuda.is_available():
    torch.cuda.init()
from unipeak_amd import capi
from tests import wide_q11_inputs as Q
from tests.test_gpu_wide_q11 import run_kind
regs, cnt, kind, _ = run_kind(capi, 2000, Q.clustered_unit(2000), region_thr=0.0)
np.savez(sys.argv[2], regs=regs, cnt=cnt, kind=kind)
"""


def test_switch_keeps_the_replay(gpu_lib, oracle, clustered, tmp_path):
    """UNIPEAK_WIDE_Q11=0 (read at up_open): a fresh process takes the replay
    and finds the same records"""
    out = tmp_path / "ab.npz"
    env = dict(os.environ, UNIPEAK_WIDE_Q11="0")
    r = subprocess.run([sys.executable, "-c", AB_CHILD, ROOT, str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    assert int(z["kind"]) == REPLAY
    unit = clustered[2000]
    ref, ref_sums = oracle.run_unit(2000, Q.BG, unit[1], unit[2], region_thr=0.0)
    compare(ref, ref_sums, z["regs"], z["cnt"])


# ---- 6. buffers and heads ----------------------------------------------------------------------

@pytest.mark.parametrize("args", [["-f", "-r", "0"], ["-f", "-r", "-2", "-k", "0"]], ids=["r0", "r-2"])
@pytest.mark.parametrize("bw", Q.CLI_WIDTHS)
@pytest.mark.parametrize("layout", Q.CLI_LAYOUTS)
def test_buffers_and_heads_cli(orc_bin, gpu_lib, tmp_path, layout, bw, args):
    """three- and four-unit buffers: the moved last record, a unit without records
    in between, a head unit first / in the middle / last, the Q1 leak chain --
    byte-identical to the oracle CLI and to the replay (UNIPEAK_WIDE_Q11=0)"""
    write_contigs(tmp_path / "contigs.txt", [(n, L) for n, L, _ in Q.cli_contigs(layout, bw)])
    fwd, rev = Q.cli_tracks(layout, bw)
    write_wig(tmp_path / "s0.wig", "s0", fwd, rev)
    full = ["-q", "-c", "contigs.txt", "-b", str(bw), "-m", "3000"] + args + ["s0.wig"]
    out = compare_tool(orc_bin, tmp_path, "regions", full)
    assert out.count("\n") > 6
    replay = tmp_path / "replay.txt"
    r = subprocess.run([os.path.join(BIN, "regions")] + full + ["-o", str(replay)], cwd=tmp_path,
                       capture_output=True, text=True, env=dict(os.environ, UNIPEAK_WIDE_Q11="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert replay.read_bytes() == (tmp_path / "ref_out.txt").read_bytes()


# ---- 7. the dense profile ----------------------------------------------------------------------

def test_profile(gpu_lib, oracle):
    capi = gpu_lib
    bw = Q.PROFILE_BW
    length, pos, cnt = Q.profile_unit()
    ref = oracle.profile(bw, Q.BG, length, pos, cnt)
    with capi.Lib(0) as g:
        g.set_params(bw, 1, Q.BG, region_thr=0.0)
        u = load(g, (length, pos, cnt))
        assert g.run() >= 1 and g.last_scan_kind() == K1Q
        with pytest.raises(capi.UpError):
            g.run_async()  # K1q passes run inside the blocking up_run only
        f, r = g.profile(u, length)
        assert ref.tobytes() == f.tobytes() and not r.any()
        for first, count in ((Q.STRIP - 700, 1_500), (40_001, 333)):  # (the first one crosses a strip edge)
            f, r = g.profile_range(u, first, count)
            assert ref[first - 1:first - 1 + count].tobytes() == f.tobytes() and not r.any()
        g.set_profile_capture(True)  # the context is on the replay now
        with pytest.raises(capi.UpError):
            g.profile(u, length)
        with pytest.raises(capi.UpError):
            g.profile_range(u, 1, 100)


# ---- 8. mode switches in one context ---------------------------------------------------------------

@pytest.mark.parametrize("policy", ["INDEX_NEVER", "INDEX_AUTO"])
def test_mode_switches_in_one_context(gpu_lib, oracle, policy):
    bw = Q.SWITCH_BW
    length, pos, cnt, ep, ec = Q.switch_unit()
    p2, c2 = Q.with_extra(pos, cnt, ep, ec)
    with gpu_lib.Lib(0) as g:
        g.set_index_policy(getattr(gpu_lib, policy))
        g.set_params(bw, 1, Q.BG, region_thr=25.0)
        u = load(g, (length, pos, cnt))

        def one(thr, p, c, kind):
            g.set_params(bw, 1, Q.BG, region_thr=thr)
            regs, gcnt = g.regions(g.run())
            assert g.last_scan_kind() == kind
            compare(*oracle.run_unit(bw, Q.BG, p, c, region_thr=thr), regs, gcnt)

        one(25.0, pos, cnt, K1W)
        one(0.0, pos, cnt, K1Q)
        g.scatter(u, 0, 0, ep, ec)
        one(0.0, p2, c2, K1Q)
        one(25.0, p2, c2, K1W)
