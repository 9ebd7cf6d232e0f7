"""K1's screens and K1b's keys on regions that sit on their bounds, through the
C-ABI, against the oracle.

Every screen in front of the exact kernels exists to skip work, and K1b takes
every word the screen left out as holding no flag: a screen that skips one
chunk too many loses a region, or one end of one, and nothing crashes.  The
populations of tests/screen_margin_inputs.py put a region exactly on each
bound -- one tag over the budget wskip, an FP32 bound 1.0001 times fthr, a
cluster at the last chunk and at the last position of the window -- at the
last position before and the first after every edge K1 works in (chunk, word,
plane lane, block, wave load, strip), at position bw + 1 and at the unit's
end, on three units.  tests/test_screen_margin_oracle.py shows on the CPU
that they are marginal.

One context per (configuration, bandwidth); per population the units are
loaded anew and three passes run, at the marginal score's predecessor, at the
score and at its successor (up_set_params between passes; no kurtosis or hit
filter, so every candidate is recorded).  After each pass every unit's records
must equal the oracle's (tests/test_gpu_unit.compare: coordinates, peaks,
counts, filters, the peak score bit for bit); where the dense profile is
served, it must equal the oracle's bit for bit as well.  The expected regions
come from the oracle alone.  Which configuration reaches which screen:
DESIGN.md §4, "Screen-margin tests"."""
import numpy as np
import pytest

from tests import screen_margin_inputs as M
from tests.test_gpu_k1b_one import knobs, same_bits
from tests.test_gpu_unit import compare

pytestmark = pytest.mark.gpu

_REF = {}  # (kind, bw, motif) -> the oracle's answers, shared by the configurations of a kind


def reference(oracle, pop):
    key = (pop["kind"], pop["bw"], pop["name"])
    if key not in _REF:
        s = float(M.marginal_scores(oracle, pop)[0])
        runs = [[M.oracle_run(oracle, pop, u, t) for u in range(3)] for t in M.thresholds(s)]
        _REF[key] = (s, runs)
    return _REF[key]


def load(g, pop):
    g.reset_units()
    for length, pos, cf, cr in pop["units"]:
        u = g.add_unit(length)
        for st, c in enumerate((cf, cr)):
            if c is None:
                continue
            for s in range(pop["S"]):
                m = c[:, s] != 0
                if m.any():
                    g.scatter(u, st, s, pos[m], c[m, s])


def keys_on(pop):
    """q_mode (csrc/api.hip) for one directional sample: the integer Q of the
    fullest possible window stays below 2^32"""
    bw = pop["bw"]
    cmax = max(2, max(int(cf.max()) for _, _, cf, _ in pop["units"]))
    return bw * bw * (2 * bw + 1) * cmax < 4294967295


def run_matrix(capi, oracle, kind, bw, policy, *, profile, checks=lambda g, pop: None):
    """every population of (kind, bw) in one context -> {(motif, pass): (records, counts)}"""
    par = M.KINDS[kind]
    out = {}
    passes = regions = cells = 0
    with capi.Lib(0) as g:
        if policy is not None:
            g.set_index_policy({"never": capi.INDEX_NEVER, "always": capi.INDEX_ALWAYS}[policy])
        common = dict(kurt_thr=0.0, hit_thr=0.0, corr_thr=-1.0, nondir=par["nondir"], control=par["control"],
                      coeffs=par["coeffs"])
        g.set_params(bw, par["S"], M.BG, region_thr=25.0, **common)
        if kind == "wide_nd":
            g.set_wide_nd_full(True)  # (as the CLIs do)
        for pop in M.populations(kind, bw):
            s, runs = reference(oracle, pop)
            load(g, pop)
            for i, thr in enumerate(M.thresholds(s)):
                what = f"{kind} bw {bw} [{policy}] {pop['name']} pass {i} (thr {thr!r})"
                g.set_params(bw, par["S"], M.BG, region_thr=thr, **common)
                regs, cnt = g.regions(g.run())
                assert g.last_scan_kind() == (1 if bw > 511 else 0), what
                if policy is not None:
                    assert g.index_state()[0] == (policy == "always"), what
                checks(g, pop)
                for u in range(3):
                    ref, sums = runs[i][u]
                    m = regs["unit"] == u
                    try:
                        compare(ref, sums, regs[m], cnt[m])
                    except AssertionError as e:
                        lost = sorted(set(zip(ref["left"].tolist(), ref["right"].tolist())) -
                                      set(zip(regs[m]["left"].tolist(), regs[m]["right"].tolist())))
                        raise AssertionError(f"{what}, unit {u}: {e}; oracle regions the GPU lacks: {lost[:6]}; "
                                             f"anchors {[(n, A) for n, uu, A in pop['copies'] if uu == u]}") from e
                    regions += len(ref)
                passes += 1
                out[pop["name"], i] = (regs.copy(), cnt.copy())
            if profile:
                for u, (length, *_rest) in enumerate(pop["units"]):
                    f, r = g.profile(u, length)
                    want = M.oracle_profile(oracle, pop, u)
                    got = f + r if par["nondir"] else f
                    bad = np.flatnonzero(want.view(np.uint64) != got.view(np.uint64))
                    assert bad.size == 0, (f"{kind} bw {bw} [{policy}] {pop['name']}: dense profile of unit {u} differs at "
                                           f"{bad.size} positions, first {bad[0] + 1}: oracle {want[bad[0]]!r}, GPU "
                                           f"{got[bad[0]]!r}")
                    cells += length
    print(f"screen-margin {kind} bw {bw} [{policy}]: passes {passes} regions {regions} profile cells {cells}")
    return out


@pytest.mark.parametrize("bw", M.BWS["one"])
def test_one_sample_fields(gpu_lib, oracle, bw):
    """A: one directional sample without the index: k1a_fields_kernel -- the
    packed pre-screen (R <= 4, wskip < 31, no escape), the register pre-screen,
    screen_bits; from bw 256 on scan_kernel's screen over the fields.  With the
    pipelined K1b and with the generic one: the same bits"""
    def checks(kind):
        def f(g, pop):
            assert g.last_exact_kind() == kind(pop), (pop["name"], g.last_exact_kind())
            assert g.scan_density() == 256
        return f
    with knobs(UNIPEAK_K1B_ONE=1):
        new = run_matrix(gpu_lib, oracle, "one", bw, "never", profile=True, checks=checks(lambda p: int(keys_on(p))))
    with knobs(UNIPEAK_K1B_ONE=0):
        old = run_matrix(gpu_lib, oracle, "one", bw, "never", profile=False, checks=checks(lambda p: 0))
    assert new.keys() == old.keys()
    for k in new:
        same_bits(new[k][0], old[k][0])
        assert np.array_equal(new[k][1], old[k][1]), k


@pytest.mark.parametrize("bw", M.BWS["one"])
def test_one_sample_index(gpu_lib, oracle, bw):
    """B: the same with the index from the first pass: up to bw 255 K1a streams
    the chunk-sum plane (plane_clean, a saturated byte unbounded from wskip 255
    on), above it the fields"""
    def checks(g, pop):
        assert g.scan_density() == (64 if bw <= 255 else 256)
    run_matrix(gpu_lib, oracle, "one", bw, "always", profile=True, checks=checks)


@pytest.mark.parametrize("policy", ["never", "always"])
@pytest.mark.parametrize("bw", M.BWS["pool"])
def test_pooled_samples(gpu_lib, oracle, bw, policy):
    """C: two pooled samples around a control (POOL 1): scan_kernel's screen over
    the fields with pre_bound, and the pooled plane"""
    run_matrix(gpu_lib, oracle, "pool", bw, policy, profile=False)


@pytest.mark.parametrize("policy", ["never", "always"])
@pytest.mark.parametrize("bw", M.BWS["coef"])
def test_coefficients(gpu_lib, oracle, bw, policy):
    """D: coefficients (0, 5), every tag on the sample of coefficient 5 (POOL 2):
    a tag weighs 6 in the screen; weights swapped, or indexed by sample instead
    of by non-control sample, drop the region"""
    run_matrix(gpu_lib, oracle, "coef", bw, policy, profile=False)


@pytest.mark.parametrize("policy", ["never", "always"])
@pytest.mark.parametrize("bw", M.BWS["nondir"])
def test_nondirectional(gpu_lib, oracle, bw, policy):
    """E: one nondirectional sample, the tags split over the strands: the screen
    sums both strands, the score is f + r"""
    run_matrix(gpu_lib, oracle, "nondir", bw, policy, profile=True)


@pytest.mark.parametrize("kind", ["wide", "wide_nd"])
@pytest.mark.parametrize("bw", M.BWS["wide"])
def test_wide(gpu_lib, oracle, bw, kind):
    """F: K1w (bw 512, 700, 2000): the prefix-sum screen over each word's union
    window, a cluster in its last chunk; wide_profile_kernel's window"""
    run_matrix(gpu_lib, oracle, kind, bw, None, profile=True)
