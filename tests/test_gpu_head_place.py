"""up_set_head_place: quirk-Q1 head units replayed (K0) and merged with the
parallel scan's records on the device, inside the pass (headplace.hip).

Every parity case runs one context with the mode off (the host merge) and on,
compares both lists and the exptSums with the oracle and with each other --
integers exactly, peak_score / kurtosis / corr between the modes as bit
patterns (NaN as NaN), against the oracle as tests/test_gpu_unit.py does
(peak_score bit-exact, kurtosis and corr within 1e-12 relative) -- and checks
on the off-mode run that the case exercises the merge: a unit with a resync
position, a replayed record in the list, a record of the headless list that
started before the resync position and is gone."""
import numpy as np
import pytest

from tests import head_place_inputs as hp

pytestmark = pytest.mark.gpu

REL = 1e-12
RULE = 0xFFFFFFFF   # UP_CLOSE_RULE: a K1-K3 record (a replayed one names its closing add, or 0)
ALL = 0xFFFFFFFF    # resync: replayed to the unit's end
HOST, PLACED, NONE = 0, 1, -1
K1W = 1
REC = 56            # sizeof(up_region)
FLOATS = ("peak_score", "kurtosis", "corr")
INTS = ("unit", "left", "right", "peak", "sum", "nonctl_sum", "accepted", "close_pos")


def close(a, b, rel=REL):
    a, b = np.asarray(a, float), np.asarray(b, float)
    both_nan = np.isnan(a) & np.isnan(b)
    ok = both_nan | (a == b) | (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)))
    return bool(np.all(ok))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    both_nan = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and bool(np.all(both_nan | (a.view(np.uint64) == b.view(np.uint64))))


def load(g, case, *, capture=False):
    g.set_params(case["bw"], case["S"], case["bg"], region_thr=case["thr"], kurt_thr=case["kurt_thr"],
                 corr_thr=case["corr_thr"], hit_thr=case["hit_thr"], nondir=case["nondir"],
                 control=case["control"], coeffs=case["coeffs"], want_corr=case["want_corr"])
    if case["nondir"] and case["bw"] > 511:
        g.set_wide_nd_full(True)
    g.set_profile_capture(capture)
    for u in case["units"]:
        uid = g.add_unit(u["length"], u["buffer"])
        for st, c in enumerate([u["cf"]] if not case["nondir"] else [u["cf"], u["cr"]]):
            for s in range(case["S"]):
                m = c[:, s] != 0
                g.scatter(uid, st, s, u["pos"][m], c[m, s])


def run_mode(g, case, on):
    g.set_head_place(on)
    n = g.run()
    regs, cnt = g.regions(n)
    resync = [g.unit_resync(u) for u in range(len(case["units"]))]
    return regs, cnt, g.last_head_kind(), resync


def same_lists(a, ca, b, cb):
    assert len(a) == len(b), (len(a), len(b))
    for k in INTS:
        assert np.array_equal(a[k], b[k]), k
    for k in FLOATS:
        assert same_bits(a[k], b[k]), k
    assert np.array_equal(ca, cb)


def matches_oracle(case, ref, ref_sums, regs, cnt):
    assert len(ref) == len(regs), (len(ref), len(regs))
    for k in ("unit", "left", "right", "peak", "sum", "accepted"):
        assert np.array_equal(ref[k], regs[k]), k
    assert np.array_equal(ref_sums, cnt)
    assert ref["peak_score"].tobytes() == regs["peak_score"].tobytes()
    assert close(ref["kurtosis"], regs["kurtosis"])
    if case["want_corr"]:
        assert close(ref["corr"], regs["corr"])


def exercises_merge(oracle, case, regs, resync, dropped=True):
    assert any(x != 0 for x in resync), resync
    assert (regs["close_pos"] != RULE).any(), "no replayed record in the list"
    if not dropped:
        return
    bare, _ = hp.oracle_list(oracle, hp.headless(case))
    have = set(hp.keys(regs))
    gone = [k for k, r in zip(hp.keys(bare), bare)
            if resync[int(r["unit"])] != 0 and int(r["left"]) < resync[int(r["unit"])] and k not in have]
    assert gone, "no record that starts before a resync position was dropped"


def parity(gpu_lib, oracle, case, *, scan_kind=None):
    ref, ref_sums = hp.oracle_list(oracle, case)
    with gpu_lib.Lib(0) as g:
        load(g, case)
        off, off_cnt, off_kind, off_resync = run_mode(g, case, False)
        off, off_cnt = off.copy(), off_cnt.copy()
        if scan_kind is not None:
            assert g.last_scan_kind() == scan_kind
        on, on_cnt, on_kind, on_resync = run_mode(g, case, True)
        if scan_kind is not None:
            assert g.last_scan_kind() == scan_kind
    print(case["name"], "records", len(ref), "off", len(off), "on", len(on), "kinds", off_kind, on_kind,
          "resync", off_resync, on_resync)
    assert off_kind == HOST and on_kind == PLACED
    matches_oracle(case, ref, ref_sums, off, off_cnt)
    matches_oracle(case, ref, ref_sums, on, on_cnt)
    same_lists(off, off_cnt, on, on_cnt)
    assert off_resync == on_resync
    exercises_merge(oracle, case, off, off_resync)


@pytest.mark.parametrize("bw,seed", hp.DIRECTIONAL)
def test_directional(gpu_lib, oracle, bw, seed):
    parity(gpu_lib, oracle, hp.directional(bw, seed))


def test_nondirectional_with_corr(gpu_lib, oracle):
    parity(gpu_lib, oracle, hp.nondirectional())


def test_two_buffers_seven_units(gpu_lib, oracle):
    case = hp.chains()
    parity(gpu_lib, oracle, case)
    ref, _ = hp.oracle_list(oracle, case)
    assert {int(u) for u in ref["unit"]} >= {0, 1, 3, 5, 6}  # unit-major over both buffers


def test_three_samples_control_coefficients(gpu_lib, oracle):
    parity(gpu_lib, oracle, hp.three_samples())


@pytest.mark.parametrize("nondir", [False, True], ids=["dir", "nondir"])
def test_wide(gpu_lib, oracle, nondir):
    parity(gpu_lib, oracle, hp.wide(nondir), scan_kind=K1W)


def _target_list(t, cap, S):
    """(records, exptSums) of a record target [n][cap x up_region][cap x S x uint32]"""
    from unipeak_amd.capi import REGION_DTYPE
    raw = t.cpu().numpy()
    n = int(raw[:8].view(np.uint64)[0])
    assert n <= cap
    regs = raw[8:8 + n * REC].view(REGION_DTYPE).copy()
    cnt = raw[8 + cap * REC:8 + cap * REC + n * S * 4].view(np.uint32).reshape(n, S).copy()
    return regs, cnt


@pytest.mark.parametrize("delivery", ["host", "device"])
def test_pipelined(gpu_lib, delivery):
    """UP_MAX_IN_FLIGHT placed passes in flight, each equal to the blocking
    off-mode list; then the threshold changes (5 -> 25) and a second batch"""
    import torch
    case = hp.chains()
    S, depth, cap = case["S"], gpu_lib.MAX_IN_FLIGHT, 4096
    with gpu_lib.Lib(0) as g:
        load(g, case)
        targets = [torch.zeros(8 + cap * (REC + 4 * S), dtype=torch.uint8, device="cuda") for _ in range(depth)]
        torch.cuda.synchronize()
        for thr in (5.0, 25.0):
            g.set_record_target(0, 0)
            g.set_params(case["bw"], S, case["bg"], region_thr=thr, kurt_thr=case["kurt_thr"],
                         hit_thr=case["hit_thr"])
            g.set_head_place(False)
            n = g.run()
            want, want_cnt = (a.copy() for a in g.regions(n))
            assert g.last_head_kind() == HOST and n > 0 and (want["close_pos"] != RULE).any()
            g.set_head_place(True)
            for i in range(depth):
                if delivery == "device":
                    g.set_record_target(targets[i].data_ptr(), cap)
                g.run_async()
            for i in range(depth):
                n = g.run_wait()
                assert g.last_head_kind() == PLACED
                if delivery == "device":
                    regs, cnt = _target_list(targets[i], cap, S)
                else:
                    regs, cnt = (a.copy() for a in g.regions_view())
                assert n == len(want)
                same_lists(want, want_cnt, regs, cnt)


def test_captured_graphs(gpu_lib, monkeypatch):
    """launches on the caller's thread replay the pass's K1x..K3 and the
    placement as a cached graph: the first pass captures it, the next replay it"""
    monkeypatch.setenv("UNIPEAK_LAUNCHER", "0")
    case = hp.directional(50, 1)
    with gpu_lib.Lib(0) as g:
        load(g, case)
        g.set_timing(0)
        g.set_head_place(False)
        n = g.run()
        want, want_cnt = (a.copy() for a in g.regions(n))
        g.set_head_place(True)
        for _ in range(3):
            n = g.run()
            assert g.last_head_kind() == PLACED
            regs, cnt = g.regions(n)
            same_lists(want, want_cnt, regs, cnt)


def test_capacity_fallback(gpu_lib, oracle):
    """an open region longer than the in-pass capacity: that pass is finished
    by the host path (kind 0) with the right records, the capacities grow, and
    the next pass places its records itself"""
    case = hp.long_region()
    ref, ref_sums = hp.oracle_list(oracle, case)
    with gpu_lib.Lib(0) as g:
        load(g, case)
        first, first_cnt, kind1, resync = run_mode(g, case, True)
        first, first_cnt = first.copy(), first_cnt.copy()
        second, second_cnt, kind2, _ = run_mode(g, case, True)
    print("long region: records", len(ref), "kinds", kind1, kind2, "resync", resync)
    assert kind1 == HOST
    matches_oracle(case, ref, ref_sums, first, first_cnt)
    assert kind2 == PLACED
    matches_oracle(case, ref, ref_sums, second, second_cnt)
    same_lists(first, first_cnt, second, second_cnt)
    exercises_merge(oracle, case, first, resync, dropped=False)


def test_small_device_target(gpu_lib, oracle):
    import torch
    case = hp.directional(50, 1)
    ref, ref_sums = hp.oracle_list(oracle, case)
    S, cap = case["S"], len(ref) - 1
    assert cap >= 1
    with gpu_lib.Lib(0) as g:
        load(g, case)
        g.set_head_place(True)
        small = torch.zeros(8 + cap * (REC + 4 * S), dtype=torch.uint8, device="cuda")
        big = torch.zeros(8 + 4096 * (REC + 4 * S), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        g.set_record_target(small.data_ptr(), cap)
        g.run_async()
        with pytest.raises(gpu_lib.UpError) as e:
            g.run_wait()
        assert e.value.code == gpu_lib.UP_E_NOMEM
        g.set_record_target(big.data_ptr(), 4096)
        n = g.run()
        assert g.last_head_kind() == PLACED and n == len(ref)
        regs, cnt = _target_list(big, 4096, S)
    matches_oracle(case, ref, ref_sums, regs, cnt)


@pytest.mark.parametrize("wide", [False, True], ids=["bw50", "bw600"])
def test_shift_scan_and_best(gpu_lib, wide):
    """up_shift_scan / up_shift_best over every region longer than
    2 max_shift + 3: the same bits from the host-merged and the placed list"""
    case = hp.wide(True) if wide else hp.nondirectional()
    max_shift = 40
    out = []
    with gpu_lib.Lib(0) as g:
        load(g, case)
        for on in (False, True):
            regs, _, kind, _ = run_mode(g, case, on)
            assert kind == (PLACED if on else HOST)
            length = regs["right"].astype(np.int64) - regs["left"] + 1
            idx = np.flatnonzero(length > 2 * max_shift + 3).astype(np.uint64)
            assert (regs["close_pos"][idx.astype(np.int64)] != RULE).any(), "no replayed region requested"
            tab = g.shift_scan(idx, max_shift)
            best, corr = g.shift_best(idx, max_shift)
            out.append((idx, tab, best, corr))
    (i0, t0, b0, c0), (i1, t1, b1, c1) = out
    assert np.array_equal(i0, i1) and i0.size > 0
    assert same_bits(t0, t1) and np.array_equal(b0, b1) and same_bits(c0, c1)


def test_profile_capture_keeps_the_host_path(gpu_lib):
    case = hp.directional(50, 1)
    got = []
    with gpu_lib.Lib(0) as g:
        load(g, case, capture=True)
        for on in (False, True):
            g.set_head_place(on)
            n = g.run()
            regs, cnt = (a.copy() for a in g.regions(n))
            got.append((regs, cnt, g.last_head_kind(), g.replay_profile(0)))
    (r0, c0, k0, p0), (r1, c1, k1, p1) = got
    assert k0 == HOST and k1 == HOST
    same_lists(r0, c0, r1, c1)
    assert p0[0] == p1[0] != 0 and p0[1].size > 0
    for a, b in zip(p0[1:], p1[1:]):
        assert a.tobytes() == b.tobytes()


def test_pass_without_head_units(gpu_lib):
    case = hp.no_heads()
    got = []
    with gpu_lib.Lib(0) as g:
        load(g, case)
        for on in (False, True):
            regs, cnt, kind, resync = run_mode(g, case, on)
            got.append((regs.copy(), cnt.copy()))
            assert kind == NONE and resync == [0]
    assert len(got[0][0]) > 0
    same_lists(*got[0], *got[1])


def test_set_head_place_in_flight(gpu_lib):
    case = hp.directional(13, 0)
    with gpu_lib.Lib(0) as g:
        load(g, case)
        g.run_async()
        with pytest.raises(gpu_lib.UpError) as e:
            g.set_head_place(True)
        assert e.value.code == gpu_lib.UP_E_STATE
        g.run_wait()
        g.set_head_place(True)
        g.run()
        assert g.last_head_kind() == PLACED
