"""Wide K1q on nondirectional units (csrc/wide.hip, up_set_wide_q11_nd): a
threshold <= 0 at bandwidths 512..32767 with both strands in one buffer --
wide_runs_kernel over every strand's tracks, wide_peak_kernel<POOL, true> for
the peaks of forwardScore + reverseScore, wide_corr_kernel for the strand
correlation of regions up to kCorrLong stored positions and
wide_corr_stage_kernel / wide_corr_chain_kernel for longer ones, K2, K3 (known
peaks, correlation handed in), the K1q placement, the K0 head chains, K4's
wide_fill_kernel and wide_profile_kernel<POOL, true>.

The checker is the oracle (tests/oracle_binding.py, orc_bin), never the
replay: every record's left / right / peak / sum / accepted and per-sample
counts equal, the FP64 peak score byte-equal, kurtosis and correlation within
1e-12; CLI tables byte-identical to the oracle CLI's.  up_last_scan_kind tells
which path found the regions (2: K1q).  On the parent commit every case fails
at set_wide_q11_nd: the symbol is missing.  tests/test_wide_q11_nd_oracle.py
shows on the CPU that the inputs hold what the cases rely on."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import wide_q11_nd_inputs as N
from tests.shift_ref import host_shift_table
from tests.test_cli import BIN, compare_tool, make_inputs
from tests.test_gpu_replay import close, compare
from tests.wig import write_contigs, write_wig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K1W, K1Q, REPLAY = 1, 2, 3  # up_last_scan_kind
UP_CLOSE_Q11 = 0xFFFFFFFE


def load(g, unit, buffer_id=0):
    length, pos, cf, cr = unit
    u = g.add_unit(length, buffer_id=buffer_id)
    for st, c in enumerate((cf, cr)):
        for s in range(c.shape[1]):
            m = c[:, s] != 0
            if m.any():
                g.scatter(u, st, s, pos[m], c[m, s])
    return u


def run_kind(capi, bw, units, switch=True, capture=False, **kw):
    """one blocking pass over the nondirectional units of one buffer -> (records, counts, scan kind, K1b kind)"""
    kw.setdefault("want_corr", True)
    with capi.Lib(0) as g:
        g.set_params(bw, units[0][2].shape[1], N.BG, nondir=True, **kw)
        g.set_wide_q11_nd(switch)
        if capture:
            g.set_profile_capture(True)
        for u in units:
            load(g, u)
        regs, cnt = g.regions(g.run())
        return regs, cnt, g.last_scan_kind(), g.last_exact_kind()


def check(capi, oracle, bw, unit, kind=K1Q, switch=True, capture=False, **kw):
    ref, ref_sums = oracle.run_unit(bw, N.BG, unit[1], unit[2], unit[3], nondir=True, **kw)
    regs, cnt, k, k1b = run_kind(capi, bw, [unit], switch=switch, capture=capture, **kw)
    assert k == kind
    if kind == K1Q:
        assert k1b == -1
    compare(ref, ref_sums, regs, cnt, corr=True)
    return ref, regs


# ---- 1. widths and thresholds ---------------------------------------------------------

@pytest.mark.parametrize("thr", N.THRESHOLDS)
@pytest.mark.parametrize("bw", N.WIDTHS)
def test_widths_and_thresholds(gpu_lib, oracle, bw, thr):
    ref, _ = check(gpu_lib, oracle, bw, N.clustered_unit(bw), region_thr=thr)
    assert len(ref) >= 3


# ---- 2. acceptance by the correlation -------------------------------------------------

def test_acceptance_by_correlation(gpu_lib, oracle):
    ref, regs = check(gpu_lib, oracle, N.CORR_BW, N.corr_unit(), region_thr=0.0, corr_thr=N.CORR_THR)
    assert list(regs["accepted"]) == list(ref["accepted"]) == [1, 0, 0]
    assert np.isnan(ref["corr"][2]) and np.isnan(regs["corr"][2])  # tags on one strand only


# ---- 3. the run rule over two strands ----------------------------------------------------

@pytest.mark.parametrize("coeffs", N.RULE_COEFFS)
def test_run_rule_over_two_strands(gpu_lib, oracle, coeffs):
    ref, _ = check(gpu_lib, oracle, N.RULE_BW, N.rule_unit(), region_thr=0.0, kurt_thr=0.0, control=N.RULE_CONTROL,
                   coeffs=coeffs)
    assert len(ref) == 5


# ---- 4. the peak of f + r ---------------------------------------------------------------

def test_peak_of_f_plus_r(gpu_lib, oracle):
    ref, regs = check(gpu_lib, oracle, N.PEAK_BW, N.peak_unit(), region_thr=0.0)
    assert N.BETWEEN_F + 1 < int(regs["peak"][0]) < N.BETWEEN_R + 1
    assert int(regs["peak"][1]) == N.TIE_A + 1


def test_first_position_is_not_the_peak(gpu_lib, oracle):
    """the control-only run of rule_unit: every score 0.0, so the first maximum is the
    run's first stored position -- the peak is the next one"""
    ref, regs = check(gpu_lib, oracle, N.RULE_BW, N.rule_unit(), region_thr=0.0, kurt_thr=0.0,
                      control=N.RULE_CONTROL)
    assert regs["peak_score"][4] == 0.0 and int(regs["peak"][4]) == int(regs["left"][4]) + 1


# ---- 5. the long path and its rounds -----------------------------------------------------

def test_long_regions_default_limit(gpu_lib, oracle):
    """kCorrLong - 1, kCorrLong (wide_corr_kernel), kCorrLong + 1 and 2 kCorrLong - 100
    (stage + chain, one round) stored positions at bw 2,000"""
    unit, lens = N.long_unit(N.CORR_LONG, 2000)
    ref, _ = check(gpu_lib, oracle, 2000, unit, region_thr=0.0)
    assert tuple(N.stored(ref)) == lens


LONG_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
if torch.cuda.is_available():
    torch.cuda.init()
from unipeak_amd import capi
from tests import wide_q11_nd_inputs as N
from tests.test_gpu_wide_q11_nd import run_kind
unit, _ = N.long_unit(N.TEST_LONG, 600)
regs, cnt, kind, _ = run_kind(capi, 600, [unit], switch=sys.argv[3] == "1", region_thr=0.0)
np.savez(sys.argv[2], regs=regs, cnt=cnt, kind=kind)
"""


def child(tmp_path, name, script, env, switch=True):
    out = tmp_path / (name + ".npz")
    r = subprocess.run([sys.executable, "-c", script, ROOT, str(out), "1" if switch else "0"],
                       env=dict(os.environ, **env), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def long_default(gpu_lib, oracle):
    """the long unit at bw 600 with the default settings, where wide_corr_kernel alone
    forms every correlation: (oracle records, oracle counts, this library's records)"""
    unit, lens = N.long_unit(N.TEST_LONG, 600)
    ref, ref_sums = oracle.run_unit(600, N.BG, unit[1], unit[2], unit[3], nondir=True, region_thr=0.0)
    assert tuple(N.stored(ref)) == lens
    regs, cnt, kind, _ = run_kind(gpu_lib, 600, [unit], region_thr=0.0)
    assert kind == K1Q
    compare(ref, ref_sums, regs, cnt, corr=True)
    return ref, ref_sums, regs


@pytest.mark.parametrize("tile", (None,) + N.TEST_TILES)
def test_long_regions_and_rounds(long_default, tmp_path, tile):
    """UNIPEAK_WIDE_CORR_LONG=8192 makes the last two regions long; the default tile
    holds them in one round (sweep 2 reuses the staged scores), a tile of 12,288 holds
    both in round 0 and cuts the second once, a tile of 4,096 cuts them two and four
    times (every round of sweep 2 stages again): the same correlation bits as with the
    default settings"""
    ref, ref_sums, regs = long_default
    env = {"UNIPEAK_WIDE_CORR_LONG": str(N.TEST_LONG)}
    if tile:
        env["UNIPEAK_WIDE_CORR_TILE"] = str(tile)
    z = child(tmp_path, "long", LONG_CHILD, env)
    assert int(z["kind"]) == K1Q
    compare(ref, ref_sums, z["regs"], z["cnt"], corr=True)
    assert z["regs"]["corr"].tobytes() == regs["corr"].tobytes()


# ---- 6. CLIs -------------------------------------------------------------------------

def cli_case(orc_bin, tmp_path, tool, full, min_lines):
    out = compare_tool(orc_bin, tmp_path, tool, full)
    assert out.count("\n") > min_lines
    replay = tmp_path / "replay.txt"
    r = subprocess.run([os.path.join(BIN, tool)] + full + ["-o", str(replay)], cwd=tmp_path, capture_output=True,
                       text=True, env=dict(os.environ, UNIPEAK_WIDE_Q11_ND="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert replay.read_bytes() == (tmp_path / "ref_out.txt").read_bytes()
    return out


@pytest.mark.parametrize("args", [["-r", "0"], ["-r", "-2", "-k", "0"]], ids=["r0", "r-2"])
@pytest.mark.parametrize("bw", N.CLI_WIDTHS)
@pytest.mark.parametrize("layout", N.CLI_LAYOUTS)
def test_buffers_and_heads_cli(orc_bin, gpu_lib, tmp_path, layout, bw, args):
    """bin/regions -D: three- and four-unit buffers, a head unit first / in the middle /
    last, the Q1 leak chain -- byte-identical to the oracle CLI and to the replay
    (UNIPEAK_WIDE_Q11_ND=0)"""
    write_contigs(tmp_path / "contigs.txt", [(n, L) for n, L, _ in N.cli_contigs(layout, bw)])
    fwd, rev = N.cli_tracks(layout, bw)
    write_wig(tmp_path / "s0.wig", "s0", fwd, rev)
    cli_case(orc_bin, tmp_path, "regions",
             ["-q", "-c", "contigs.txt", "-D", "-y", "-f", "-b", str(bw), "-m", "3000"] + args + ["s0.wig"], 3)


def test_shifted_units_are_all_heads_cli(orc_bin, gpu_lib, tmp_path):
    """-s 2000 moves the first tags of every unit with tags to positions <= bw: each is a head unit"""
    write_contigs(tmp_path / "contigs.txt", [(n, L) for n, L, _ in N.cli_contigs("head_middle", 600)])
    fwd, rev = N.cli_tracks("head_middle", 600)
    write_wig(tmp_path / "s0.wig", "s0", fwd, rev)
    cli_case(orc_bin, tmp_path, "regions",
             ["-q", "-c", "contigs.txt", "-D", "-y", "-f", "-b", "600", "-m", "3000", "-r", "0", "-s", "2000",
              "s0.wig"], 2)


def test_strand_shift_cli(orc_bin, gpu_lib, tmp_path):
    ct, files = make_inputs(tmp_path, 173, [("chrA", 90_000), ("chrB", 40_000)], 1, shift_rev=100, n_cl=6, sd=200)
    out = cli_case(orc_bin, tmp_path, "strand_shift", ["-c", ct, "-x", "60", "-r", "0", "-b", "600"] + files, 3)
    assert "# best_shift=" in out


# ---- 7. K4 ------------------------------------------------------------------------------

@pytest.mark.parametrize("max_shift", [0, 40])
def test_shift_scan_and_best(gpu_lib, oracle, max_shift):
    """a head unit (the K0 chain's records keep their stored scores) and a plain unit:
    strandCorr(0) of every record is the record's own correlation; the K1q records that
    did not move against the host recomputation over the oracle's dense f and r"""
    bw = N.K4_BW
    units = N.k4_units()
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, N.BG, nondir=True, region_thr=0.0, want_corr=True)
        g.set_wide_q11_nd(True)
        for u in units:
            load(g, u)
        n = g.run()
        assert g.last_scan_kind() == K1Q and n >= 4
        regs, _ = g.regions(n)
        idx = np.arange(n, dtype=np.uint64)[::-1].copy()
        tab = g.shift_scan(idx, max_shift)[::-1]
        best, bc = g.shift_best(idx, max_shift)
        best, bc = best[::-1], bc[::-1]
    assert close(regs["corr"], tab[:, 0])
    own = regs["close_pos"] == UP_CLOSE_Q11  # found by K1q in their own unit
    replayed = regs["close_pos"] < 0xFFFFFFFD  # (the chain's records name their closing add)
    assert own.any() and replayed.any()
    for u, (L, pos, cf, cr) in enumerate(units):
        k = np.flatnonzero(own & (regs["unit"] == u))
        st = regs[k].copy()
        st["left"] -= 1  # the stored positions
        st["right"] -= 1
        assert close(host_shift_table(oracle, bw, N.BG, pos, cf, cr, st, max_shift), tab[k])
    for k in range(n):
        b, c = 0, -1.0
        for s in range(max_shift + 1):
            if tab[k, s] > c:
                b, c = s, tab[k, s]
        assert best[k] == b and bc[k] == c, (k, max_shift)


# ---- 8. the dense profile -----------------------------------------------------------------

def test_profile(gpu_lib):
    capi = gpu_lib
    bw = N.PROFILE_BW
    unit = N.profile_unit()
    length = unit[0]
    ranges = ((N.STRIP - 700, 1_500), (40_001, 333))
    with capi.Lib(0) as g:  # the reference: the same unit at -r 25 behind up_set_wide_nd_full
        g.set_params(bw, 1, N.BG, nondir=True, region_thr=25.0)
        g.set_wide_nd_full(True)
        u = load(g, unit)
        want = [g.profile(u, length)] + [g.profile_range(u, a, n) for a, n in ranges]
    with capi.Lib(0) as g:
        g.set_params(bw, 1, N.BG, nondir=True, region_thr=0.0, want_corr=True)
        u = load(g, unit)
        with pytest.raises(capi.UpError):  # the switch off: the replay's refusal
            g.profile(u, length)
        g.set_wide_q11_nd(True)
        g.run()  # (background tags everywhere: one run, never closed, no record)
        assert g.last_scan_kind() == K1Q
        got = [g.profile(u, length)] + [g.profile_range(u, a, n) for a, n in ranges]
    for (wf, wr), (gf, gr) in zip(want, got):
        assert wf.any() and wr.any()
        assert wf.tobytes() == gf.tobytes() and wr.tobytes() == gr.tobytes()


# ---- 9. what stays ---------------------------------------------------------------------------

def test_switch_off_keeps_the_replay(gpu_lib, oracle):
    check(gpu_lib, oracle, 600, N.clustered_unit(600), kind=REPLAY, switch=False, region_thr=0.0)


def test_capture_keeps_the_replay(gpu_lib, oracle):
    check(gpu_lib, oracle, 600, N.clustered_unit(600), kind=REPLAY, capture=True, region_thr=0.0)


def test_negative_coefficient_keeps_the_replay(gpu_lib, oracle):
    check(gpu_lib, oracle, N.RULE_BW, N.rule_unit(), kind=REPLAY, region_thr=0.0, kurt_thr=0.0,
          control=N.RULE_CONTROL, coeffs=[-0.5, 1.5])


def test_bw_32768_keeps_the_replay(gpu_lib, oracle):
    check(gpu_lib, oracle, 32_768, N.clustered_unit(32_768), kind=REPLAY, region_thr=0.0)


ENV_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
if torch.cuda.is_available():
    torch.cuda.init()
from unipeak_amd import capi
from tests import wide_q11_nd_inputs as N
from tests.test_gpu_wide_q11_nd import run_kind
regs, cnt, kind, _ = run_kind(capi, 2000, [N.clustered_unit(2000)], region_thr=0.0)
np.savez(sys.argv[2], regs=regs, cnt=cnt, kind=kind)
"""


@pytest.mark.parametrize("var", ["UNIPEAK_WIDE_Q11_ND", "UNIPEAK_WIDE_Q11"])
def test_environment_switches_keep_the_replay(gpu_lib, oracle, tmp_path, var):
    z = child(tmp_path, "env", ENV_CHILD, {var: "0"})
    assert int(z["kind"]) == REPLAY
    unit = N.clustered_unit(2000)
    ref, ref_sums = oracle.run_unit(2000, N.BG, unit[1], unit[2], unit[3], nondir=True, region_thr=0.0)
    compare(ref, ref_sums, z["regs"], z["cnt"], corr=True)


def test_run_async_is_refused(gpu_lib):
    capi = gpu_lib
    with capi.Lib(0) as g:
        g.set_params(600, 1, N.BG, nondir=True, region_thr=0.0, want_corr=True)
        g.set_wide_q11_nd(True)
        load(g, N.clustered_unit(600))
        with pytest.raises(capi.UpError):
            g.run_async()  # K1q passes run inside the blocking up_run only
        assert g.run() >= 3 and g.last_scan_kind() == K1Q


@pytest.mark.parametrize("policy", ["INDEX_NEVER", "INDEX_AUTO"])
def test_mode_switches_in_one_context(gpu_lib, oracle, policy):
    bw = N.SWITCH_BW
    unit, ep, ec = N.switch_unit()
    unit2 = N.with_extra(unit, ep, ec)
    with gpu_lib.Lib(0) as g:
        g.set_index_policy(getattr(gpu_lib, policy))
        g.set_params(bw, 1, N.BG, nondir=True, region_thr=25.0, corr_thr=0.3, want_corr=True)
        g.set_wide_q11_nd(True)
        u = load(g, unit)

        def one(thr, un, kind):
            g.set_params(bw, 1, N.BG, nondir=True, region_thr=thr, corr_thr=0.3, want_corr=True)
            regs, gcnt = g.regions(g.run())
            assert g.last_scan_kind() == kind
            compare(*oracle.run_unit(bw, N.BG, un[1], un[2], un[3], nondir=True, region_thr=thr, corr_thr=0.3),
                    regs, gcnt, corr=True)

        one(25.0, unit, K1W)
        one(0.0, unit, K1Q)
        g.scatter(u, 1, 0, ep, ec)
        one(0.0, unit2, K1Q)
        one(25.0, unit2, K1W)
