"""K3 with one lane per region (stats1L_kernel, "K3L", csrc/stats1.hip:360-905).

dispatch_stats (csrc/api.hip) picks K3L only for a pass whose predecessor in
the same context produced >= 16,384 regions, so a test that opens a context
and runs it once gets the wave-per-region stats1_kernel.  Here K3L runs
 * forced, in child processes (tests/k3l_worker.py): UNIPEAK_K3_LANE=2, the
   same with UNIPEAK_K3L_HEAVY=8 and with UNIPEAK_K3L_W2=0 (the three are
   read once per process), and UNIPEAK_K3_LANE=0 for the wave kernel's answer;
 * for real, in-process: a context of 17,000 regions whose second pass takes it.
Every case is compared with the oracle (integers equal, peak_score byte-equal,
kurtosis equal as bits or NaN in both: test_gpu_k3.py's rule), bit for bit
with the wave kernel (the LANE=0 child) and with the general K3
(UNIPEAK_K3_ONE=0, in-process), and asserts the kernel that ran
(up_last_stats_kind): without that, a change of the dispatch rule would turn
these back into tests of the wave kernel.

Cases (one directional sample, background 0.003) and the branch each aims at:
 stage    dense blocks (every position hit, counts 1-2) whose regions span
          470..530 positions from first-field offsets 0, 1, 8, 15: regions of
          nd == 32 dwords (staged in the lane's row) and nd == 33 (chunked),
          stats1.hip:483-485.  Regions of 1, 2, 3 positions and of exactly 16
          on a dword boundary: the first/last-dword masks with
          (f1 & 15) == 15 (:449-450, :467-468); a single position's kurtosis
          is NaN (sum2 == 0, :784).
 long     blocks of 600, 1,100, 2,100 positions, 70 % of them hit (more than
          512 hits: the wave's path at the default threshold, :629, :732-783);
          one of 3,300 with escaped counts in its
          third and fourth overflow block, past ti0/ti1 (the ovf_lookup
          fallback, :582-584, :602-603); one of 70,000 hit positions (the
          uint16 offset walk :618-623, nh = ~0, the heavy path reading 64
          dwords at a time from HBM, :750); a block that ends at the contig's
          last position (Q16).
 esc      counts 3, 4, 254, 255, 256 at positions 1024k - 1 .. 1024k + 2 (the
          overflow-block edge lies between 1024k and 1024k + 1) inside staged
          regions that straddle the edge (:580-583, tile byte 255 -> :602);
          a staged and a chunked region with more than 64 escaped fields
          (kK3LEsc full, :605, :648, :694) and counts >= 255 among the first
          64 (cached as the sentinel 255, looked up again); a second unit
          with no overflow table (has_ovf false, :532-538) in the same pass.
          Q keys are on at every bandwidth (K3L's own window sum, :789-837),
          so it also runs at bw 120.
 escbig   the same plus 65,535 and 2^24: the keys are off
          (bw^2 (2bw + 1) max >= 2^32), K1b's FP64 peak stands (:787-789).
 ties     test_batched_k3_tied_keys' input (tied keys inside a strip and at
          2 * 16,384 - 1) and runs across strip edges whose parts hold equal
          largest keys (fv == fk, :433-435, then the wave's KDE, :842-876), a
          larger one in the later part (:430-432) and in the earlier part.
 rem<N>   N = 1, 63, 64, 65, 127, 128, 129, 257 single-cluster regions: the
          waves' and blocks' remainders (kK3LThreads = 128); lanes past the end
          shadow the wave's first region (:415) and must not write (:884, :900).
 thr      stage's unit with kurt_thr / hit_thr at the oracle's medians: both
          values of `accepted` (:879-890).
 keysoff  esc's first unit with one count of 2^30: q_mode off at every bw.
UNIPEAK_K3L_HEAVY=8 reruns stage/long/esc/escbig: every staged region above 8
hits takes the wave's sums from the lane's row (hst, :745-750), unreachable
at the default threshold.  UNIPEAK_K3L_W2=0 reruns them with the per-dword
second walk (terms, :637-663) instead of hits4 (:668-713).

Checked once against mutated builds of stats1L_kernel: without the
`c == 255u` re-lookup (:602) esc, escbig and keysoff fail; with the wave's
path starting at cb = hj0 + 64 (:748) long, esc, escbig, keysoff and
stage under UNIPEAK_K3L_HEAVY=8 fail.  Dropping `(f1 & 15) != 15` in stage
(:468) changes nothing as compiled today -- the mask is built as
(4 << 2 * (f1 & 15)) - 1, which wraps to all ones at field 15 -- but with
the shift count taken modulo 32, as a 32-bit shift instruction would,
stage, thr, long, esc and the 17,000-region passes fail.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = 0.003
K_PAD_POS = 1024   # kernels.h kPadPos
K_STRIP = 16_384   # kernels.h kStrip
LANE_MIN = 16_384  # api.hip kK3LaneMin
KNOBS = ("UNIPEAK_K3_LANE", "UNIPEAK_K3L_HEAVY", "UNIPEAK_K3L_W2")
CHILDREN = {  # name: (knobs, which cases)
    "lane": ({"UNIPEAK_K3_LANE": "2"}, "all"),
    "heavy8": ({"UNIPEAK_K3_LANE": "2", "UNIPEAK_K3L_HEAVY": "8"}, "c123"),
    "w2off": ({"UNIPEAK_K3_LANE": "2", "UNIPEAK_K3L_W2": "0"}, "c123"),
    "wave": ({"UNIPEAK_K3_LANE": "0"}, "all"),
}
REM_COUNTS = (1, 63, 64, 65, 127, 128, 129, 257)
STAGE_SPANS = (470, 481, 496, 497, 511, 512, 513, 528, 530)
STAGE_OFFSETS = (0, 1, 8, 15)

CASES_123 = [f"{k}_bw{bw}" for k in ("stage", "long", "esc", "escbig") for bw in (20, 50)] + ["esc_bw120"]
CASES = (CASES_123 + [f"ties_bw{bw}" for bw in (20, 50, 120)] +
         [f"rem{n}_bw{bw}" for n in REM_COUNTS for bw in (20, 50)] +
         [f"{k}_bw{bw}" for k in ("thr", "keysoff") for bw in (20, 50)])

FIELDS = ("unit", "left", "right", "peak", "sum", "nonctl_sum", "accepted", "close_pos")


# ---------------------------------------------------------------- generators
def _unit(d, length):
    pos = np.array(sorted(d), np.uint32)
    assert pos[0] > 512 and pos[-1] <= length  # (no unit takes the K0 head replay, quirk Q1)
    return length, pos, np.array([[d[int(p)]] for p in pos], np.uint32)


def _block(d, rng, a, n, density=1.0, hi=2):
    """positions a .. a + n - 1, the two ends always hit, counts 1..hi"""
    for p in range(a, a + n):
        if density >= 1.0 or p in (a, a + n - 1) or rng.random() < density:
            d[p] = int(rng.integers(1, hi + 1))


THR = 25.0  # region_thr of every case


def _reach(kern, bw):
    """how far the run of a block whose outer 128 positions hold 2 tags each
    extends beyond its ends (positions whose score reaches THR)"""
    m = 0
    while 2.0 * kern[bw + m + 1:].sum() >= THR:
        m += 1
    return m


# tags ((offset, count), ...) from a position p whose scores reach THR at
# exactly n positions from p + lead on, none of them within 1e-9 of THR (found
# by search over the kernel weights; test_generators_meet_their_conditions
# holds them to it): TINY[bw][n] = (tags, lead).  bw 20's two positions hold
# no tag at all (count 0, x_bar 0 / 0)
TINY = {
    20: {1: (((0, 2),), 0), 2: (((0, 1), (3, 1), (28, 1), (31, 1)), 15),
         3: (((0, 1), (22, 1), (26, 1)), 15), 16: (((0, 2), (17, 1)), -2)},
    50: {1: (((0, 5),), 0), 2: (((0, 1), (5, 4), (63, 2)), 20),
         3: (((0, 4), (24, 1), (66, 3)), 27), 16: (((0, 2), (15, 3), (62, 1), (72, 2)), 24)},
}


def stage_unit(bw, kern):
    rng = np.random.default_rng(4101)
    d = {}
    m = _reach(kern, bw)
    a = 2048
    for span in STAGE_SPANS:
        for off in STAGE_OFFSETS:
            left = (a + 15) // 16 * 16 + off + 1  # (left - 1) % 16 == off: the region's first field
            n = span - 2 * m
            _block(d, rng, left + m, n)
            for p in list(range(left + m, left + m + 128)) + list(range(left + m + n - 128, left + m + n)):
                d[p] = 2
            a = left + span + 700
    # regions of 1, 2, 3 and 16 positions, first field `off`
    for n, offs in ((1, (0, 1, 8, 15)), (2, (0, 14, 15)), (3, (0, 13, 15)), (16, (0, 5))):
        tags, lead = TINY[bw][n]
        for off in offs:
            left = (a + 15) // 16 * 16 + 128 + off + 1
            for o, c in tags:
                d[left - lead + o] = c
            a = left + 700
    return _unit(d, a + 2_000)


def long_unit():
    rng = np.random.default_rng(4102)
    d = {}
    _block(d, rng, 5_000, 600, 0.7, 4)
    _block(d, rng, 8_000, 1_100, 0.7, 4)
    # 3,300 positions from overflow block 10: escapes in blocks 12 and 13
    _block(d, rng, 10_740, 3_300, 0.7, 2)
    for k, p in enumerate((12 * 1024 + 1, 12 * 1024 + 2, 12 * 1024 + 700, 13 * 1024, 13 * 1024 + 1, 13 * 1024 + 17,
                           13 * 1024 + 300, 13 * 1024 + 301)):
        d[p] = (3, 7, 254, 255, 256, 300, 4, 1_000)[k]
    _block(d, rng, 16_000, 2_100, 0.7, 4)  # (across the strip edge at 16,384)
    _block(d, rng, 20_000, 70_000)  # every position hit: offsets wrap at 65,536
    for k, p in enumerate((20_000, 20_001, 21_023, 21_024, 50_000, 85_535, 85_536, 85_537, 89_999)):
        d[p] = (3, 300, 255, 5, 254, 4, 256, 3, 9)[k]
    length = 95_000
    _block(d, rng, length - 300, 301, 0.8, 4)  # tags up to len
    return _unit(d, length)


def esc_units(big=False, keysoff=False):
    rng = np.random.default_rng(4103)
    vals = [3, 4, 254, 255, 256] + ([65_535, 1 << 24] if big else [])
    d = {}
    for i in range(2 * len(vals)):
        e = 1024 * (3 + 2 * i)  # the overflow blocks' edge lies between e and e + 1
        _block(d, rng, e - 40, 81)
        for t in range(4):
            d[e - 1 + t] = vals[(i + t) % len(vals)]
    a = 1024 * (3 + 4 * len(vals)) + 500
    # staged, 100 escaped fields: 255 and 256 among the first 64 and after them
    for k in range(100):
        d[a + k] = {10: 255, 20: 256, 70: 255, 90: 256}.get(k, 3 + k % 7)
    a += 2_000
    # chunked (700 positions), ~350 escaped fields
    _block(d, rng, a, 700, 1.0, 4)
    d[a + 5], d[a + 40], d[a + 600] = 255, 300 if not big else 70_000, 256
    if keysoff:
        d[a + 300] = 1 << 30
    u0 = _unit(d, a + 3_000)
    d = {}
    for k in range(6):
        _block(d, rng, 2_000 + 2_500 * k, 90 + 130 * k, 0.8)
    return [u0, _unit(d, 20_000)]


def ties_unit():
    d = {}
    # test_batched_k3_tied_keys: equal counts at c and c + 1 with symmetric flanks
    for c in (10_000, 20_000, 30_000, 2 * K_STRIP - 1):
        for o, n in ((0, 10), (1, 10), (-30, 3), (31, 3)):
            d[c + o] = d.get(c + o, 0) + n
    # runs across a strip edge (between e and e + 1): mirror images hold equal
    # largest keys; a heavier later part; a heavier earlier part
    for e, lo, hi in ((3 * K_STRIP, 10, 10), (K_STRIP, 10, 12), (4 * K_STRIP, 12, 10)):
        d[e - 5], d[e + 1 + 5] = lo, hi
        d[e - 35], d[e + 1 + 35] = 3, 3
    return _unit(d, 80_000)


def rem_unit(n):
    d = {}
    for i in range(n):
        c = 1_000 + 512 * i
        for o, k in ((-2, 2), (-1, 2), (0, 12 + i % 5), (1, 2), (2, 1 + i % 2)):
            d[c + o] = k
    return _unit(d, 1_000 + 512 * n + 1_000)


def switch_units():
    """17,000 tight clusters (12-39 tags, N(0, 4) offsets, pitch 128) in three
    units, and the same with every 17th cluster cleared (16,000 left)
    -> (units, cleared units, per unit the positions to clear)"""
    rng = np.random.default_rng(4108)
    units, cleared, zeros = [], [], []
    for ncl in (6_000, 5_000, 6_000):
        ntag = rng.integers(12, 40, ncl)
        which = np.repeat(np.arange(ncl), ntag)
        p = 1_024 + 128 * which + np.clip(np.rint(rng.normal(0, 4, which.size)), -40, 40).astype(np.int64)
        pos, cnt = np.unique(p, return_counts=True)
        length = 1_024 + 128 * ncl + 1_024
        gone = ((pos - 1_024 + 64) // 128) % 17 == 3
        units.append((length, pos.astype(np.uint32), cnt.astype(np.uint32)[:, None]))
        cleared.append((length, pos[~gone].astype(np.uint32), cnt[~gone].astype(np.uint32)[:, None]))
        zeros.append(pos[gone].astype(np.uint32))
    return units, cleared, zeros


def build_case(name, oracle):
    """-> dict(bw, units [(length, pos, cnt[n, 1])], kurt_thr, hit_thr); `oracle`
    for the kernel weights (stage, thr) and thr's medians"""
    kind, bw = name.rsplit("_bw", 1)
    case = dict(bw=int(bw), kurt_thr=50.0, hit_thr=10.0)
    if kind in ("stage", "thr"):
        case["units"] = [stage_unit(case["bw"], oracle.kernel(case["bw"], 1.0 / BG))]
        if kind == "thr":
            _, pos, cnt = case["units"][0]
            ref, _ = oracle.run_unit(case["bw"], BG, pos, cnt)
            case["kurt_thr"] = float(np.nanmedian(ref["kurtosis"]))
            case["hit_thr"] = float(np.median(ref["sum"]))
    elif kind == "long":
        case["units"] = [long_unit()]
    elif kind in ("esc", "escbig"):
        case["units"] = esc_units(big=kind == "escbig")
    elif kind == "keysoff":
        case["units"] = esc_units(keysoff=True)[:1]
    elif kind == "ties":
        case["units"] = [ties_unit()]
    elif kind.startswith("rem"):
        case["units"] = [rem_unit(int(kind[3:]))]
    else:
        raise KeyError(name)
    return case


def run_case(capi, case):
    """one context, one pass -> (records, counts, K3 kind)"""
    with capi.Lib(0) as g:
        g.set_params(case["bw"], 1, BG, region_thr=THR, kurt_thr=case["kurt_thr"], corr_thr=-1.0,
                     hit_thr=case["hit_thr"])
        for length, pos, cnt in case["units"]:
            g.scatter(g.add_unit(length), 0, 0, pos, cnt[:, 0])
        regs, cnt = g.regions(g.run())
        return regs, cnt, g.last_k3_kind()


def case_names(which):
    return {"all": CASES, "c123": CASES_123}[which]


# ---------------------------------------------------------------- comparisons
_refs = {}


def ref_of(oracle, name):
    """the oracle's (records, counts) per unit of a case, computed once"""
    if name not in _refs:
        c = build_case(name, oracle)
        _refs[name] = [oracle.run_unit(c["bw"], BG, pos, cnt, kurt_thr=c["kurt_thr"], hit_thr=c["hit_thr"],
                                       cap=1 << 20 if len(pos) > 60_000 else 1 << 16)
                       for _, pos, cnt in c["units"]]
        for r, s in _refs[name]:
            r.flags.writeable = s.flags.writeable = False
    return _refs[name]


def same_as_oracle(refs, regs, cnt):
    assert np.all(np.diff(regs["unit"].astype(np.int64)) >= 0)
    assert len(regs) == sum(len(r) for r, _ in refs), (len(regs), [len(r) for r, _ in refs])
    for u, (ref, ref_sums) in enumerate(refs):
        m = regs["unit"] == u
        g = regs[m]
        assert len(g) == len(ref), (u, len(g), len(ref))
        for k in ("left", "right", "peak", "sum", "accepted"):
            assert np.array_equal(ref[k], g[k]), (u, k, np.flatnonzero(ref[k] != g[k])[:8])
        assert np.array_equal(ref_sums, cnt[m]), u
        assert ref["peak_score"].tobytes() == g["peak_score"].tobytes(), \
            (u, np.flatnonzero(ref["peak_score"] != g["peak_score"])[:8])
        a, b = ref["kurtosis"], g["kurtosis"]
        ok = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        assert np.all(ok), (u, np.flatnonzero(~ok)[:8], a[~ok][:4], b[~ok][:4])


def same_bits(a, b):  # (test_gpu_k3.same_bits)
    assert len(a) == len(b)
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), k
    for k in ("peak_score", "kurtosis", "corr"):
        assert a[k].tobytes() == b[k].tobytes(), k


def dwords(ref):
    """dwords a region's fields span (stats1.hip:445-446, :483)"""
    n0 = K_PAD_POS + ref["left"].astype(np.int64) - 1
    n1 = K_PAD_POS + ref["right"].astype(np.int64) - 1
    return (n1 >> 4) - (n0 >> 4) + 1


# ---------------------------------------------------------------- the children
@pytest.fixture(scope="module")
def children(gpu_lib, oracle, tmp_path_factory):
    """{child: {case: (records, counts, kind)}}: one fresh process per knob
    setting (the knobs are read once per process)"""
    out = {}
    for child, (knobs, which) in CHILDREN.items():
        d = tmp_path_factory.mktemp("k3l_" + child)
        env = {k: v for k, v in os.environ.items() if k not in KNOBS + ("UNIPEAK_K3_ONE", "UNIPEAK_K3L_CUT")}
        env.update(knobs)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "k3l_worker.py"), str(d), which],
                           env=env, cwd=ROOT, timeout=240, capture_output=True, text=True)
        if p.returncode != 0:  # (nothing further is started)
            pytest.fail(f"k3l_worker {child} ended with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        z = np.load(os.path.join(d, "cases.npz"))
        out[child] = {n: (z[n + "__regs"], z[n + "__cnt"], int(z[n + "__kind"])) for n in case_names(which)}
    return out


def run_general(capi, case):
    old = os.environ.get("UNIPEAK_K3_ONE")
    os.environ["UNIPEAK_K3_ONE"] = "0"  # (read per context)
    try:
        return run_case(capi, case)
    finally:
        if old is None:
            del os.environ["UNIPEAK_K3_ONE"]
        else:
            os.environ["UNIPEAK_K3_ONE"] = old


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_lane_k3_matches_oracle_wave_and_general_k3(gpu_lib, oracle, children, name):
    regs, cnt, kind = children["lane"][name]
    assert kind == 2
    same_as_oracle(ref_of(oracle, name), regs, cnt)
    wregs, wcnt, wkind = children["wave"][name]
    assert wkind == 1
    same_bits(regs, wregs)
    assert np.array_equal(cnt, wcnt)
    gregs, gcnt, gkind = run_general(gpu_lib, build_case(name, oracle))
    assert gkind == 0
    same_bits(regs, gregs)
    assert np.array_equal(cnt, gcnt)


@pytest.mark.gpu
@pytest.mark.parametrize("child", ["heavy8", "w2off"])
@pytest.mark.parametrize("name", CASES_123)
def test_lane_k3_forced_paths(oracle, children, child, name):
    """the wave's sums from the lane's staged row (UNIPEAK_K3L_HEAVY=8) and
    the per-dword second walk (UNIPEAK_K3L_W2=0): the default's bits"""
    regs, cnt, kind = children[child][name]
    assert kind == 2
    same_as_oracle(ref_of(oracle, name), regs, cnt)
    dregs, dcnt, _ = children["lane"][name]
    same_bits(regs, dregs)
    assert np.array_equal(cnt, dcnt)


# ---------------------------------------------------------------- the real switch
_switch = {}


def switch_refs(oracle):
    if not _switch:
        units, cleared, zeros = switch_units()
        _switch.update(units=units, cleared=cleared, zeros=zeros,
                       full=[oracle.run_unit(20, BG, p, c) for _, p, c in units],
                       less=[oracle.run_unit(20, BG, p, c) for _, p, c in cleared])
    return _switch


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["blocking", "pipelined", "index_never", "index_always"])
def test_lane_k3_takes_over_after_a_large_pass(gpu_lib, oracle, mode):
    """no knob: the pass after one of >= 16,384 regions runs K3L, the pass after
    one of fewer the wave kernel again (the estimate is the last completed
    pass's count when the pass is enqueued); every pass gives the oracle's
    records for the counts it read"""
    s = switch_refs(oracle)
    n_full, n_less = (sum(len(r) for r, _ in s[k]) for k in ("full", "less"))
    assert n_full >= LANE_MIN > n_less >= 1024
    with gpu_lib.Lib(0) as g:
        if mode.startswith("index"):
            g.set_index_policy(gpu_lib.INDEX_NEVER if mode == "index_never" else gpu_lib.INDEX_ALWAYS)
        g.set_params(20, 1, BG, region_thr=THR, kurt_thr=50.0, corr_thr=-1.0, hit_thr=10.0)
        for length, pos, cnt in s["units"]:
            g.scatter(g.add_unit(length), 0, 0, pos, cnt[:, 0])

        def done(ref, kind):
            regs, cnt = g.regions(g.run_wait() if mode == "pipelined" else g.run())
            assert g.last_k3_kind() == kind
            same_as_oracle(s[ref], regs, cnt)

        def clear():
            for u, z in enumerate(s["zeros"]):
                g.scatter(u, 0, 0, z, np.zeros(z.size, np.uint32))

        if mode != "pipelined":
            done("full", 1)
            done("full", 2)
            clear()
            done("less", 2)  # (the estimate is the pass before's)
            done("less", 1)
        else:  # two deep: a pass's estimate is the count of the pass two before it
            g.run_async()
            g.run_async()
            done("full", 1)
            g.run_async()
            done("full", 1)
            g.run_async()
            done("full", 2)
            done("full", 2)
            clear()
            g.run_async()
            g.run_async()
            done("less", 2)
            g.run_async()
            done("less", 2)
            g.run_async()
            done("less", 1)
            done("less", 1)


# ---------------------------------------------------------------- the generators, without a GPU
def test_generators_meet_their_conditions(oracle):
    """what the cases above rely on, asserted on the oracle's answer"""
    for bw in (20, 50):
        (ref, _), = ref_of(oracle, f"stage_bw{bw}")
        nd = dwords(ref)
        assert {32, 33} <= set(nd.tolist())
        span = ref["right"].astype(np.int64) - ref["left"] + 1
        for n in STAGE_SPANS:  # each at every first-field offset
            assert {int(x) for x in (ref["left"][span == n] - 1) % 16} == set(STAGE_OFFSETS), n
        for n in (1, 2, 3):  # (of them one whose last field is a dword's last: offset 15, 14, 13)
            assert ((ref["right"][span == n] - 1) % 16 == 15).any(), n
        assert ((span == 16) & ((ref["left"] - 1) % 16 == 0)).any()
        assert np.isnan(ref["kurtosis"][span == 1]).all()
        (ref, _), = ref_of(oracle, f"thr_bw{bw}")
        assert set(ref["accepted"].tolist()) == {0, 1}
        (ref, _), = ref_of(oracle, f"long_bw{bw}")
        span = ref["right"].astype(np.int64) - ref["left"] + 1
        for n in (600, 1_100, 2_100, 3_300, 70_000):  # (the blocks, plus the scores' reach)
            assert ((span >= n) & (span < n + 100)).sum() == 1, (n, span)
        assert ref["right"].max() >= 95_000
        for n in REM_COUNTS:
            (ref, _), = ref_of(oracle, f"rem{n}_bw{bw}")
            assert len(ref) == n
    for name in ("esc_bw20", "esc_bw50", "esc_bw120"):
        (ref, _), (ref1, _) = ref_of(oracle, name)
        _, pos, cnt = build_case(name, oracle)["units"][0]
        esc = pos[cnt[:, 0] >= 3]
        nesc = np.array([np.count_nonzero((esc >= a) & (esc <= b)) for a, b in zip(ref["left"], ref["right"])])
        assert (nesc[dwords(ref) <= 32] > 64).any() and (nesc[dwords(ref) > 32] > 64).any()
        assert len(ref1) >= 6
    s = switch_refs(oracle)
    assert [len(r) for r, _ in s["full"]] == [6_000, 5_000, 6_000]
    assert sum(len(r) for r, _ in s["less"]) == 16_000
