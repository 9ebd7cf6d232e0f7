"""K3L (stats1L_kernel, csrc/stats1.hip) after it was cut to fit beside three
K1a waves per SIMD: the places where the narrower kernel can go wrong.

What changed in the kernel and the case that aims at it:
 * the lane's row is staged in batches of 16 dwords (kK3LBatch), and a batch
   no lane of the wave needs is skipped -- `edges`: regions of exactly 16,
   17, 32 and 33 track dwords (the batch edge; 32 / 33 is the staged /
   chunked edge), each once from field 0 and once starting in field 15 of a
   dword and ending in field 0 of one; `only16`: the same 15- and 16-dword
   regions alone, so every wave skips the second batch;
 * dword indices are 32-bit and relative to the unit's track, the masks of
   the first and last dword come from (left - 1) & 15 and (right - 1) & 15
   -- the same cases;
 * a lane keeps of its unit the track pointer, the escape tiles' pointer and
   two tile indices, and reads the descriptor again on the rare paths --
   `twounits`: one wave whose 64 regions lie in two units (40 + 30 regions,
   both with overflow tables of different sizes); `escends`: regions with
   more than 64 escaped fields, an escaped field in their first and in their
   last dword, and counts of 255 and 256 among them (the tile byte 255 sends
   the lane to the whole descriptor); `ties2`: test_gpu_k3_lane's tied keys
   and runs across strip edges in a SECOND unit (strip0 != 0: the
   `kpos == 0` merge reads strip0 from the descriptor, then the wave's KDE);
 * the workgroup's shape (UPK_K3L_THREADS: 128 or 256) -- `rem<N>`: 127,
   128, 129, 255, 256, 257 single-cluster regions, the workgroup edges of
   either shape; lanes past the end shadow the wave's first region and must
   not write.
Every case runs in two fresh child processes (the knobs are read once per
process): UNIPEAK_K3_LANE=2, the lane kernel whatever the region count, and
UNIPEAK_K3_LANE=0, the wave-per-region kernel.  The lane kernel's records and
counts are compared with the oracle (test_gpu_k3_lane.same_as_oracle:
integers equal, peak_score byte-equal, kurtosis equal as bits or NaN in both)
and bit for bit, every field, with the wave kernel's.
test_fit_generators_meet_their_conditions holds the generators to the
properties above on the oracle's answer, without a GPU.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import test_gpu_k3_lane as base  # noqa: E402  (generators, comparisons)

BG, THR = base.BG, base.THR
REM_COUNTS = (127, 128, 129, 255, 256, 257)
# (dwords, first field, last field) -> span in positions
EDGE_SHAPES = tuple((nd, f0, f1, 16 * (nd - 1) - f0 + f1 + 1)
                    for nd in (16, 17, 32, 33) for f0, f1 in ((0, 15), (0, 0), (15, 0), (15, 15)))
ONLY16_SHAPES = tuple(s for s in EDGE_SHAPES if s[0] == 16) + ((15, 0, 15, 240), (15, 15, 0, 210))
ESC_LENGTHS = tuple(range(100, 116))

CASES = ([f"{k}_bw{bw}" for k in ("edges", "only16", "twounits", "escends", "ties2") for bw in (20, 50)] +
         [f"rem{n}_bw50" for n in REM_COUNTS])
CHILDREN = {"lane": {"UNIPEAK_K3_LANE": "2"}, "wave": {"UNIPEAK_K3_LANE": "0"}}


# ---------------------------------------------------------------- generators
def shaped_unit(shapes, bw, kern):
    """dense blocks (every position hit, the outer 128 positions 2 tags each)
    whose runs span exactly `span` positions from first field f0"""
    rng = np.random.default_rng(5201)
    d = {}
    m = base._reach(kern, bw)
    a = 2048
    for _, f0, _, span in shapes:
        left = (a + 15) // 16 * 16 + f0 + 1  # (left - 1) % 16 == f0
        n = span - 2 * m
        assert n >= 2 * bw + 2, (span, m)  # (an edge's score sees the 2-tag positions only)
        base._block(d, rng, left + m, n)
        for p in list(range(left + m, left + m + min(128, n))) + list(range(left + m + n - min(128, n), left + m + n)):
            d[p] = 2
        a = left + span + 700
    return base._unit(d, a + 2_000)


def escends_unit():
    """blocks of 100..115 positions, every one an escaped count (3..9, and
    255 / 256 among the first 64 and after them), with a single tag of 3 (an
    escape too) 24 positions before and after each block.  At bw 20 a lone
    tag of 3 carries the run 11 positions beyond itself and the block keeps
    the score up from there on, so the run starts 11 positions before the
    leading tag -- in field 0 or 3 of a dword, the tag in the same dword --
    and ends 11 after the trailing one, in a field that the sixteen lengths
    move through all sixteen values"""
    d = {}
    a = 4096
    for n in ESC_LENGTHS:
        for f0 in (0, 3):
            e = a + f0 + 1 + 11  # the run's first position: a + f0 + 1
            s = e + 24
            d[e] = d[s + n - 1 + 24] = 3
            for k in range(n):
                d[s + k] = {10: 255, 20: 256, 70: 255, 90: 256}.get(k, 3 + k % 7)
            a += 1024
    return base._unit(d, a + 2_000)


def build_case(name, oracle):
    kind, bw = name.rsplit("_bw", 1)
    case = dict(bw=int(bw), kurt_thr=50.0, hit_thr=10.0)
    if kind in ("edges", "only16"):
        kern = oracle.kernel(case["bw"], 1.0 / BG)
        case["units"] = [shaped_unit(EDGE_SHAPES if kind == "edges" else ONLY16_SHAPES, case["bw"], kern)]
    elif kind == "twounits":
        case["units"] = [base.rem_unit(40), base.rem_unit(30)]
    elif kind == "escends":
        case["units"] = [escends_unit()]
    elif kind == "ties2":
        case["units"] = [base.rem_unit(5), base.ties_unit()]
    elif kind.startswith("rem"):
        case["units"] = [base.rem_unit(int(kind[3:]))]
    else:
        raise KeyError(name)
    return case


_refs = {}


def ref_of(oracle, name):
    """the oracle's (records, counts) per unit of a case, computed once"""
    if name not in _refs:
        c = build_case(name, oracle)
        _refs[name] = [oracle.run_unit(c["bw"], BG, pos, cnt, kurt_thr=c["kurt_thr"], hit_thr=c["hit_thr"])
                       for _, pos, cnt in c["units"]]
        for r, s in _refs[name]:
            r.flags.writeable = s.flags.writeable = False
    return _refs[name]


# ---------------------------------------------------------------- the children
def _worker(argv):
    """python tests/test_gpu_k3_lane_fit.py OUTDIR: every case through capi.Lib
    -> OUTDIR/cases.npz (records, counts, K3 kind)"""
    from tests.oracle_binding import Oracle
    from unipeak_amd import capi

    capi.load_library()
    if capi.device_count() < 1:
        raise SystemExit("k3l fit worker: no HIP device visible")
    oracle = Oracle()
    out = {}
    for n in CASES:
        regs, cnt, kind = base.run_case(capi, build_case(n, oracle))
        out[n + "__regs"], out[n + "__cnt"], out[n + "__kind"] = regs, cnt, np.int32(kind)
    np.savez(os.path.join(argv[0], "cases.npz"), **out)
    print(f"k3l fit worker: {len(CASES)} cases")


@pytest.fixture(scope="module")
def children(gpu_lib, tmp_path_factory):
    """{child: {case: (records, counts, kind)}}: one fresh process per knob setting"""
    out = {}
    for child, knobs in CHILDREN.items():
        d = tmp_path_factory.mktemp("k3lfit_" + child)
        env = {k: v for k, v in os.environ.items()
               if k not in base.KNOBS + ("UNIPEAK_K3_ONE", "UNIPEAK_K3L_CUT")}
        env.update(knobs)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), str(d)], env=env, cwd=ROOT, timeout=240,
                           capture_output=True, text=True)
        if p.returncode != 0:  # (nothing further is started)
            pytest.fail(f"k3l fit worker {child} ended with {p.returncode}:\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
        z = np.load(os.path.join(d, "cases.npz"))
        out[child] = {n: (z[n + "__regs"], z[n + "__cnt"], int(z[n + "__kind"])) for n in CASES}
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_fitted_lane_k3_matches_oracle_and_wave_k3(oracle, children, name):
    regs, cnt, kind = children["lane"][name]
    assert kind == 2
    base.same_as_oracle(ref_of(oracle, name), regs, cnt)
    wregs, wcnt, wkind = children["wave"][name]
    assert wkind == 1
    base.same_bits(regs, wregs)
    assert np.array_equal(cnt, wcnt)


# ---------------------------------------------------------------- the generators, without a GPU
def _fields(ref):
    return (ref["left"].astype(np.int64) - 1) % 16, (ref["right"].astype(np.int64) - 1) % 16


def test_fit_generators_meet_their_conditions(oracle):
    for bw in (20, 50):
        for kind, shapes in (("edges", EDGE_SHAPES), ("only16", ONLY16_SHAPES)):
            (ref, _), = ref_of(oracle, f"{kind}_bw{bw}")
            assert len(ref) == len(shapes) < 64  # one wave
            nd = base.dwords(ref)
            f0, f1 = _fields(ref)
            got = sorted(zip(nd.tolist(), f0.tolist(), f1.tolist()))
            assert got == sorted((n, a, b) for n, a, b, _ in shapes), (kind, bw, got)
        (ref, _), = ref_of(oracle, f"only16_bw{bw}")
        assert base.dwords(ref).max() == 16  # no lane needs the second batch
        (ref, _), = ref_of(oracle, f"edges_bw{bw}")
        nd = base.dwords(ref)
        f0, f1 = _fields(ref)
        for n in (16, 17, 32, 33):  # each from field 15 to field 0
            assert ((nd == n) & (f0 == 15) & (f1 == 0)).any(), n
        # one wave, two units
        (r0, _), (r1, _) = ref_of(oracle, f"twounits_bw{bw}")
        assert len(r0) == 40 and len(r1) == 30
        # escapes: more than 64 in a lane, in the first and in the last dword
        (ref, _), = ref_of(oracle, f"escends_bw{bw}")
        _, pos, cnt = build_case(f"escends_bw{bw}", oracle)["units"][0]
        assert (cnt[:, 0] >= 3).all()
        assert len(ref) == 2 * len(ESC_LENGTHS)
        assert (base.dwords(ref) <= 32).all()
        first = last = both = False
        for a, b in zip(ref["left"].astype(np.int64), ref["right"].astype(np.int64)):
            inside = pos[(pos >= a) & (pos <= b)].astype(np.int64)
            assert inside.size > 64
            fd = ((inside - 1) >> 4 == (a - 1) >> 4).any()
            ld = ((inside - 1) >> 4 == (b - 1) >> 4).any()
            first, last, both = first or fd, last or ld, both or (fd and ld)
        if bw == 20:  # (bw 50's runs reach further than a dword beyond the blocks)
            assert first and last and both
        # the tied keys across strip edges sit in the second unit
        (r0, _), (r1, _) = ref_of(oracle, f"ties2_bw{bw}")
        assert len(r0) == 5
        crossing = (r1["left"].astype(np.int64) - 1) // base.K_STRIP != (r1["right"].astype(np.int64) - 1) // base.K_STRIP
        assert crossing.sum() >= 3
    for n in REM_COUNTS:
        (ref, _), = ref_of(oracle, f"rem{n}_bw50")
        assert len(ref) == n


if __name__ == "__main__":
    _worker(sys.argv[1:])
