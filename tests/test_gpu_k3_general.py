"""Branch-by-branch parity of the general K3 (stats_kernel<NH, POOL, NONDIR>,
csrc/kernels.hip) with the oracle, through the C-ABI.

The inputs are those of tests/k3_general_inputs.py; tests/test_k3_general_oracle.py
shows on the CPU that each reaches the branch it is named after.  Every case
runs without the index (K3 reads the tracks' dwords) and with it (plane bytes
and the pooled count track), and every record must equal the oracle's:
positions, sums, per-sample counts and the accept bit exactly, peak score,
kurtosis and strand correlation bit for bit (NaN matching NaN) -- K3 performs
the reference's operations in the reference's order, so no
tolerance applies."""
import os

import numpy as np
import pytest

from tests import k3_general_inputs as K

pytestmark = pytest.mark.gpu

POLICIES = ["never", "always"]


def policy_of(capi, name):
    return {"never": capi.INDEX_NEVER, "always": capi.INDEX_ALWAYS}[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def hexd(v):
    return f"{float(v)!r} (0x{np.float64(v).view(np.uint64):016x})"


def strict(ref, ref_sums, regs, cnt, what="", corr=True):
    """every record equal; FP64 fields bit for bit (corr false: the pass did
    not ask for the strand correlation, which the oracle always works out --
    the records then carry NaN)"""
    assert len(ref) == len(regs), (what, len(ref), len(regs))
    span = ref["right"].astype(np.int64) - ref["left"] + 1
    for k in ("left", "right", "peak", "sum", "accepted"):
        bad = np.flatnonzero(ref[k] != regs[k])
        assert bad.size == 0, (f"{what}: {k} of region {bad[0]} ({ref['left'][bad[0]]}-{ref['right'][bad[0]]}, "
                               f"{span[bad[0]]} positions): oracle {ref[k][bad[0]]}, GPU {regs[k][bad[0]]}; "
                               f"{bad.size} regions differ")
    bad = np.flatnonzero((ref_sums != cnt).any(axis=1))
    assert bad.size == 0, (f"{what}: exptSums of region {bad[0]} ({span[bad[0]]} positions): oracle "
                           f"{ref_sums[bad[0]][:8]}, GPU {cnt[bad[0]][:8]}; {bad.size} regions differ")
    if not corr:
        assert np.isnan(regs["corr"]).all(), f"{what}: a correlation nobody asked for"
    for k in ("peak_score", "kurtosis", "corr") if corr else ("peak_score", "kurtosis"):
        bad = np.flatnonzero(~same_bits(ref[k], regs[k]))
        assert bad.size == 0, (f"{what}: {k} of region {bad[0]} ({ref['left'][bad[0]]}-{ref['right'][bad[0]]}, "
                               f"{span[bad[0]]} positions): oracle {hexd(ref[k][bad[0]])}, GPU "
                               f"{hexd(regs[k][bad[0]])}; {bad.size} regions differ")
    return len(regs)


def open_case(capi, c, policy, **over):
    g = capi.Lib(0)
    try:
        g.set_index_policy(policy_of(capi, policy))
        p = dict(region_thr=c["thr"], kurt_thr=c["kurt_thr"], corr_thr=c["corr_thr"], hit_thr=c["hit_thr"],
                 nondir=c["nondir"], control=c["control"], coeffs=c["coeffs"], want_corr=c["want_corr"])
        p.update(over)
        g.set_params(c["bw"], c["S"], c["bg"], **p)
        u = g.add_unit(c["length"])
        for st, cc in enumerate((c["cf"], c["cr"])):
            if cc is None:
                continue
            for s in range(c["S"]):
                m = cc[:, s] != 0
                if m.any():
                    g.scatter(u, st, s, c["pos"][m], cc[m, s])
    except BaseException:
        g.close()
        raise
    return g


def gpu_pass(g, policy):
    regs, cnt = g.regions(g.run())
    assert g.last_k3_kind() == 0, "not the general K3"
    assert g.last_scan_kind() == 0, "not K1's regions"
    assert g.index_state()[0] == (policy == "always")
    return regs, cnt


def run_case(capi, oracle, c, policy, **over):
    """one pass of the case's unit against the oracle -> (oracle's regions and sums, GPU's)"""
    ref, ref_sums = K.oracle_run(oracle, c, **{("region_thr" if k == "thr" else k): v for k, v in over.items()})
    g = open_case(capi, c, policy, **over)
    try:
        regs, cnt = gpu_pass(g, policy)
    finally:
        g.close()
    assert len(ref) > 0
    strict(ref, ref_sums, regs, cnt, f"{c['name']} [{policy}]", corr=c["want_corr"] or not c["nondir"])
    return ref, ref_sums, regs, cnt


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("kurt_thr", [50.0, 0.0])
@pytest.mark.parametrize("config", ["pool1", "coeffs", "nondir2", "s40"])
def test_length_ladder(gpu_lib, oracle, config, kurt_thr, policy):
    """A: regions of 1 .. 5, 64, 65, 1,023, 1,024, 1,025 and 4,500 positions: the
    LDS cache of pass-1 totals (1,024 positions) and pass 2's recount past it,
    in the staged, the coefficient, the both-strand and the range-sum path"""
    ref, *_ = run_case(gpu_lib, oracle, K.ladder(config), policy, kurt_thr=kurt_thr)
    assert len(ref) == 11


@pytest.mark.parametrize("policy", POLICIES)
def test_length_ladder_one_sample(gpu_lib, oracle, policy):
    """the ladder with one directional sample through the general kernel
    (UNIPEAK_K3_ONE=0), 2,056 regions in one pass of a new context (1,024
    waves): every run has a unique largest key, so its peak is known and, up
    to 1,024 positions, it takes the cached count path; within one wave a run
    of 1,024 positions (count bytes fetched one region ahead) is followed by
    one of 1,025 (refused), and the other way round"""
    c = K.ladder_one()
    old = os.environ.get("UNIPEAK_K3_ONE")
    os.environ["UNIPEAK_K3_ONE"] = "0"
    try:
        ref, _, regs, _ = run_case(gpu_lib, oracle, c, policy)
    finally:
        if old is None:
            del os.environ["UNIPEAK_K3_ONE"]
        else:
            os.environ["UNIPEAK_K3_ONE"] = old
    assert len(ref) == c["expect"]["n_regions"]
    # (the peaks the oracle found are those of the unique keys, test_ladder_one)
    assert np.array_equal(regs["peak"], ref["peak"])


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("which", list(K.B_COEFFS))
def test_cancelled_hits(gpu_lib, oracle, which, policy):
    """B: coefficients (-1.0, 0.5): a position holding sample 0 alone pools to
    0 and stores no hit vector, in pass 1 and in pass 2's recount past 1,024
    positions; the same unit with positive coefficients"""
    ref, ref_sums, regs, cnt = run_case(gpu_lib, oracle, K.cancelled(which), policy)
    assert np.array_equal(cnt[:, 0], ref_sums[:, 0]), (
        f"exptSums of sample 0: GPU {cnt[:, 0]}, oracle {ref_sums[:, 0]} -- a position whose pooled count "
        "cancels to 0 stores no hit vector (peakcall.cpp:186-219), so its tags are not counted")


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("config", list(K.C_CONFIGS))
def test_staged_boundary(gpu_lib, oracle, config, policy):
    """C: 32 (strand, sample) tracks take the staged fetch, 33 and 34 the
    per-sample path; escapes up to 2^24; left ends on and beside a 16-byte
    boundary of the tracks"""
    run_case(gpu_lib, oracle, K.staged(config), policy)


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("config", list(K.D_CONFIGS))
def test_range_sums(gpu_lib, oracle, config, policy):
    """D: exptSums as range sums over the tracks: every residue of both ends
    mod 16, one chunk, saturated chunks, escapes and foreign tags in the end
    chunks, control tags where nothing is pooled"""
    run_case(gpu_lib, oracle, K.range_sums(config), policy)


@pytest.mark.parametrize("policy", POLICIES)
def test_corr_slab_lengths(gpu_lib, oracle, policy):
    """E: strandCorr read back from the wave's slab (<= 961 positions) and
    recomputed (>= 962); NaN below four positions and on one strand"""
    ref, *_ = run_case(gpu_lib, oracle, K.slab_lengths(), policy)
    assert np.isnan(ref["corr"]).sum() == 2


@pytest.mark.parametrize("policy", POLICIES)
def test_corr_slab_reuse(gpu_lib, oracle, policy):
    """E: 2,200 regions over the first pass's 1,024 waves: a wave's slab holds
    a long region's scores, then a short one's, and the other way round; the
    second pass runs a grid sized by the first's region count"""
    c = K.slab_reuse()
    ref, ref_sums = K.oracle_run(oracle, c)
    g = open_case(gpu_lib, c, policy)
    try:
        for k in range(2):
            regs, cnt = gpu_pass(g, policy)
            strict(ref, ref_sums, regs, cnt, f"{c['name']} [{policy}] pass {k}")
    finally:
        g.close()
    assert len(ref) > 2_100


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("bw,mode", K.F_CASES)
def test_halo_classes(gpu_lib, oracle, bw, mode, policy):
    """F: K3's own KDE at both sides of every window-word count NH = bw / 64 + 1"""
    ref, *_ = run_case(gpu_lib, oracle, K.halo(bw, mode), policy)
    assert len(ref) == 5


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("config", list(K.G_CONFIGS))
def test_strip_crossing_peaks(gpu_lib, oracle, config, policy):
    """G: the peak of a run over strip edges, merged from the strips' parts;
    of two bit-equal maxima in two strips the first"""
    c = K.strips(config)
    _, _, regs, _ = run_case(gpu_lib, oracle, c, policy)
    i = np.flatnonzero(regs["left"] == c["expect"]["regions"]["twin"][0])[0]
    assert regs["peak"][i] == c["expect"]["twin"][0]


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("config", list(K.H_CONFIGS))
def test_position_index_wraps(gpu_lib, oracle, config, policy):
    """H: a region of 70,000 positions: the UShort position index and the
    uint32 position sum wrap; kurt_thr 50 decides on the wrapped value"""
    ref, *_ = run_case(gpu_lib, oracle, K.wraps(config), policy)
    assert (ref["right"] - ref["left"] + 1 > 65_536).all()


@pytest.mark.parametrize("policy", POLICIES)
def test_count_sums_wrap(gpu_lib, oracle, policy):
    """H: 2 x 3,000,000,000 tags of one sample in a region: exptSums, sum and
    the non-control sum compared with hit_thr wrap at 2^32"""
    ref, ref_sums, *_ = run_case(gpu_lib, oracle, K.huge_counts(), policy)
    assert len(ref) == 2 and not ref["accepted"].any() and 2**32 - 2 * K.HUGE < 0 < ref_sums[:, 0].max() < 2 * K.HUGE


@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("config", list(K.I_CONFIGS))
def test_many_samples(gpu_lib, oracle, config, policy):
    """I: more than 256 samples: exptSums in the wave's LDS row, with pass 2's
    recount and the range sums adding into that row"""
    run_case(gpu_lib, oracle, K.many(config), policy)
