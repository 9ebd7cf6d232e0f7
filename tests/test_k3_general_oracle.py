"""The inputs of tests/k3_general_inputs.py hold the shapes they were built for
(CPU only): every region the GPU test compares exists in the oracle's output
with the exact length, residue, hit pattern or bit pattern that makes the
general K3 (stats_kernel, csrc/kernels.hip) take the branch the case is named
after.  Where a plain restatement is cheap the oracle itself is checked:
exptSums and Region::sum from the counts and the stored-hit rule (uint32
arithmetic, so bit equality), the strand correlation from the per-strand
profiles in the reference's operation order (bit equality), the wrapped
kurtosis (different order of the sums: 1e-9 relative, for at most 1e5 terms of
equal sign at 2^-53 each)."""
import math

import numpy as np
import pytest

from tests import k3_general_inputs as K


def lengths(regs):
    return regs["right"].astype(np.int64) - regs["left"] + 1


def find(regs, l, r):
    """index of the region (l, r); it must exist"""
    i = np.flatnonzero((regs["left"] == l) & (regs["right"] == r))
    assert i.size == 1, f"no region {l}-{r}: {list(zip(regs['left'], regs['right']))[:40]}"
    return int(i[0])


def holding(regs, x):
    i = np.flatnonzero((regs["left"] <= x) & (regs["right"] >= x))
    assert i.size == 1, f"position {x} is in no region"
    return int(i[0])


def stored(case):
    """per strand: positions (indices into case['pos']) that store a hit vector,
    i.e. whose countSum is not 0 (peakcall.cpp:186-219), in its operations"""
    out = []
    ctl = case["control"] or [0] * case["S"]
    nc = [s for s in range(case["S"]) if not ctl[s]]
    for c in (case["cf"], case["cr"]):
        if c is None:
            continue
        cs = np.zeros(len(c), np.float64)
        if case["coeffs"] is None:
            for s in nc:
                cs = cs + c[:, s].astype(np.float64)
        else:
            for k, s in enumerate(nc):
                cs = cs + c[:, s].astype(np.float64) * case["coeffs"][k]
            for s in nc:
                cs = cs + c[:, s].astype(np.float64)
        out.append(cs != 0)
    return out


def numpy_sums(case, l, r):
    """(exptSums [S], Region::sum) of positions l .. r: the counts of every
    stored hit vector, in uint32"""
    m = (case["pos"] >= l) & (case["pos"] <= r)
    tot = np.zeros(case["S"], np.uint64)
    for c, h in zip((case["cf"], case["cr"]), stored(case)):
        tot += c[m & h].astype(np.uint64).sum(axis=0)
    return (tot % 2**32).astype(np.uint32), np.uint32(int(tot.sum()) % 2**32)


def hit_positions(case, l, r):
    """positions of l .. r holding a stored hit vector on either strand"""
    h = stored(case)
    any_h = h[0] | h[1] if len(h) == 2 else h[0]
    p = case["pos"][any_h]
    return p[(p >= l) & (p <= r)].astype(np.int64)


def check_sums(case, regs, sums):
    for i in range(len(regs)):
        es, tot = numpy_sums(case, int(regs["left"][i]), int(regs["right"][i]))
        assert np.array_equal(es, sums[i]), (case["name"], i)
        assert tot == regs["sum"][i], (case["name"], i)


def test_kernel_restated(oracle):
    for bw, bg in ((5, 0.01), (50, 0.004), (63, 0.2 / 63), (511, 0.2 / 511)):
        assert K.kernel(bw, bg).tobytes() == oracle.kernel(bw, 1.0 / bg).tobytes()


# ---- A ---------------------------------------------------------------------------

@pytest.mark.parametrize("config", list(K.A_CONFIGS))
def test_ladder(oracle, config):
    c = K.ladder(config)
    e = c["expect"]
    regs, sums = K.oracle_run(oracle, c)
    check_sums(c, regs, sums)
    strands = 2 if c["nondir"] else 1
    assert c["S"] * strands == {"pool1": 3, "coeffs": 3, "nondir2": 4, "s40": 40}[config]
    # the threshold is the lone count's own score, bit for bit
    prof = K.oracle_profile(oracle, c)
    assert prof[e["short"][1] - 1] == c["thr"]
    assert len(regs) == 11
    regs0, _ = K.oracle_run(oracle, c, kurt_thr=0.0)
    for n, x in e["short"].items():
        i = holding(regs, x)
        assert lengths(regs)[i] == n and regs["left"][i] == x - (n - 1) // 2
        if n == 1:  # kurtosis 0 / 0; the n > 1 rule rejects it unless the filter is off
            assert math.isnan(regs["kurtosis"][i])
            assert regs["accepted"][i] == 0 and regs0["accepted"][i] == 1
    for n, (l, r) in e["runs"].items():
        assert r - l + 1 == n
        find(regs, l, r)
    assert set(e["runs"]) == {64, 65, 1_023, 1_024, 1_025, 4_500}
    # the long region: blocks of 64 positions from its left end with 0, 1, 63
    # and 64 hit positions, inside the cached 1,024 positions and past them
    l, r = e["long"]
    hp = hit_positions(c, l, r)
    per_block = np.bincount((hp - l) // 64, minlength=(r - l) // 64 + 1)
    assert {0, 1, 63, 64} <= set(per_block[:K.CACHE // 64].tolist())
    assert {0, 1, 63, 64} <= set(per_block[K.CACHE // 64:-1].tolist())
    if c["control"]:  # control tags at positions that store nothing, past the cache
        tagged = c["pos"][(c["cf"] != 0).any(axis=1)].astype(np.int64)
        alone = np.setdiff1d(tagged[(tagged >= l + K.CACHE) & (tagged <= r)], hp)
        assert alone.size >= 10


def test_ladder_one(oracle):
    c = K.ladder_one()
    e = c["expect"]
    assert c["S"] == 1 and not c["nondir"] and c["length"] <= 200_000
    regs, sums = K.oracle_run(oracle, c)
    assert len(regs) == e["n_regions"] == 2 * K.ONE_WAVES + len(K.ONE_B)
    n = lengths(regs)
    # the runs, at the indices that put them behind each other in one wave
    assert sorted(e["runs"]) == [K.ONE_WAVES + k for k in range(8)] + [2 * K.ONE_WAVES + k for k in range(8)]
    for i, (l, r) in e["runs"].items():
        assert find(regs, l, r) == i
        assert n[i] == (K.ONE_A[i - K.ONE_WAVES] if i < 2 * K.ONE_WAVES else K.ONE_B[i - 2 * K.ONE_WAVES])
    narrow = np.setdiff1d(np.arange(len(regs)), list(e["runs"]))
    assert set(n[narrow].tolist()) == {1, 2, 3, 4, 5} and set(n[:K.ONE_WAVES].tolist()) == {1, 2, 3, 4, 5}
    check_sums(c, regs[K.ONE_WAVES - 4:K.ONE_WAVES + 12], sums[K.ONE_WAVES - 4:K.ONE_WAVES + 12])
    check_sums(c, regs[-12:], sums[-12:])
    # K1b's key Q(p) = sum of count x (bw^2 - d^2): its largest value is at one
    # position of every run (the key is not marked as tied: the peak is known),
    # and that position is the oracle's peak
    bw = c["bw"]
    dense = np.zeros(c["length"] + 2 * bw + 2, np.int64)
    dense[c["pos"]] = c["cf"][:, 0]
    d = np.arange(-bw, bw + 1)
    q = np.convolve(dense, bw * bw - d * d)[bw:bw + dense.size]
    for i, (l, r) in e["runs"].items():
        top = np.flatnonzero(q[l:r + 1] == q[l:r + 1].max())
        assert top.size == 1 and l + top[0] == regs["peak"][i], (i, top)
    assert int(q.max()) * 4 < 2**32  # the keys fit 32 bits with room: Q keys stay on
    # of the narrow ones, one tag keeps the key, two equal neighbours tie
    for i in narrow[:10]:
        l, r = int(regs["left"][i]), int(regs["right"][i])
        assert ((q[l:r + 1] == q[l:r + 1].max()).sum() == 1) == bool(n[i] % 2)
    # wave k of 1,024 takes regions k, k + 1,024, k + 2,048: the count bytes of
    # a region of at most 16 words are fetched while the wave's previous region
    # is worked on; a longer one is refused
    fits = (regs["right"] - regs["left"]) // 64 + 1 <= K.CACHE // 64
    pairs = {(int(n[i]), int(n[i + K.ONE_WAVES])) for i in range(K.ONE_WAVES, K.ONE_WAVES + 8)}
    assert {(1_024, 1_025), (1_025, 1_024), (1_023, K.A_LONG), (K.A_LONG, 1_023), (64, 65), (65, 64)} <= pairs
    a, b = fits[K.ONE_WAVES:K.ONE_WAVES + 8], fits[2 * K.ONE_WAVES:2 * K.ONE_WAVES + 8]
    assert (a & ~b).sum() >= 3 and (~a & b).sum() >= 3 and (a & b).sum() >= 2
    assert fits[:K.ONE_WAVES].all()
    # the threshold is a lone count's own score
    prof = K.oracle_profile(oracle, c)
    i = int(narrow[n[narrow] == 1][0])
    assert prof[regs["left"][i] - 1] == c["thr"] and math.isnan(regs["kurtosis"][i])
    # the long ones keep the emptied blocks on both sides of the cached positions
    for i in (K.ONE_WAVES + 3, 2 * K.ONE_WAVES + 2):
        l, r = e["runs"][i]
        per_block = np.bincount((hit_positions(c, l, r) - l) // 64, minlength=(r - l) // 64 + 1)
        assert {0, 1, 63, 64} <= set(per_block[:K.CACHE // 64].tolist())
        assert {0, 1, 63, 64} <= set(per_block[K.CACHE // 64:-1].tolist())


# ---- B ---------------------------------------------------------------------------

def test_cancelled(oracle):
    neg, posi = K.cancelled("negative"), K.cancelled("positive")
    assert np.array_equal(neg["pos"], posi["pos"]) and np.array_equal(neg["cf"], posi["cf"])
    first, last = neg["expect"]["block"]
    for c in (neg, posi):
        regs, sums = K.oracle_run(oracle, c)
        check_sums(c, regs, sums)
        assert len(regs) == 1 and regs["left"][0] <= first and regs["right"][0] >= last
        assert lengths(regs)[0] > K.CACHE
        l, r = int(regs["left"][0]), int(regs["right"][0])
        m = (c["pos"] >= l) & (c["pos"] <= r)
        track = int(c["cf"][m, 0].sum())  # what a range sum over sample 0's track gives
        alone = m & (c["cf"][:, 0] != 0) & (c["cf"][:, 1] == 0)
        assert alone.sum() > 500 and (c["pos"][alone] > l + K.CACHE).sum() > 100
        if c is neg:
            # sample 0 alone pools to -c + c = 0: no hit vector, not counted
            assert sums[0, 0] == 7 == len(c["expect"]["both"]) and track > 800
            assert (c["expect"]["both"] > l + K.CACHE).any()
        else:
            assert sums[0, 0] == track


# ---- C ---------------------------------------------------------------------------

@pytest.mark.parametrize("config", list(K.C_CONFIGS))
def test_staged(oracle, config):
    c = K.staged(config)
    regs, sums = K.oracle_run(oracle, c)
    check_sums(c, regs, sums)
    assert c["S"] * (2 if c["nondir"] else 1) == {"s32": 32, "s33": 33, "s16nd": 32, "s17nd": 34}[config]
    assert sum(c["control"]) == 1
    assert len(regs) == 4
    for l, r in c["expect"]["regions"]:
        find(regs, l, r)
    assert sorted(int(l) % 64 for l in regs["left"]) == sorted(K.C_LEFT_MOD)
    assert 0 in [(int(l) - 1) % 64 for l in regs["left"]]  # a 16-byte piece of the track starts here
    # escapes on stored positions of every region, each class of size
    h = stored(c)
    for i in range(4):
        m = (c["pos"] >= regs["left"][i]) & (c["pos"] <= regs["right"][i])
        big = np.concatenate([x[m & hh].ravel() for x, hh in zip((c["cf"], c["cr"]), h)])
        assert ((big >= 3) & (big < 255)).any() and (big == 255).any() and (big > 255).any()
        assert (big == 1 << 24).sum() == ((2 if c["nondir"] else 1) if i == 0 else 0)


# ---- D ---------------------------------------------------------------------------

@pytest.mark.parametrize("config", list(K.D_CONFIGS))
def test_range_sums(oracle, config):
    c = K.range_sums(config)
    e = c["expect"]
    regs, sums = K.oracle_run(oracle, c)
    check_sums(c, regs, sums)
    assert c["S"] * (2 if c["nondir"] else 1) == 40 and c["coeffs"] is None
    assert len(regs) == 34
    for l, r in e["cores"] + [e["sat"]]:
        find(regs, l, r)
    left, right = regs["left"].astype(np.int64), regs["right"].astype(np.int64)
    assert set((left - 1) % 16) == set(range(16)) == set((right - 1) % 16)
    i = holding(regs, e["lone"])
    assert lengths(regs)[i] == 11 and (left[i] - 1) // 16 == (right[i] - 1) // 16
    # saturated chunks strictly inside a region
    i = find(regs, *e["sat"])
    for (x0, s), tags in ((e["c255"], 255), (e["c320"], 320)):
        assert (x0 - 1) % 16 == 0 and (left[i] - 1) // 16 < (x0 - 1) // 16 < (right[i] - 1) // 16
        m = (c["pos"] >= x0) & (c["pos"] < x0 + 16)
        assert int(c["cf"][m, s].sum()) == tags
    # tags of pooled samples just outside both ends in the ends' own chunks,
    # escapes inside both partial end chunks, control tags where nothing is pooled
    ctl = np.array(c["control"], bool)
    out_l = out_r = esc_l = esc_r = alone = 0
    dense = {int(p): k for k, p in enumerate(c["pos"])}

    def pooled_at(x):
        k = dense.get(x)
        return 0 if k is None else int(c["cf"][k, ~ctl].sum()) + (int(c["cr"][k, ~ctl].sum()) if c["nondir"] else 0)

    def escapes(lo, hi):
        n = 0
        for x in range(lo, hi + 1):
            k = dense.get(x)
            if k is not None:
                n += int((c["cf"][k, ~ctl] >= 3).sum()) + (int((c["cr"][k, ~ctl] >= 3).sum()) if c["nondir"] else 0)
        return n

    for l, r in e["cores"]:
        if (l - 1) % 16:
            out_l += pooled_at(l - 1) > 0
            esc_l += escapes(l, ((l - 1) // 16) * 16 + 16) > 0
        if (r - 1) % 16 != 15:
            out_r += pooled_at(r + 1) > 0
            esc_r += escapes(((r - 1) // 16) * 16 + 1, r) > 0
        m = (c["pos"] >= l) & (c["pos"] <= r)
        only = c["cf"][m][:, ctl].any(axis=1) & ~c["cf"][m][:, ~ctl].any(axis=1)
        alone += int(only.sum())
    assert out_l >= 20 and out_r >= 20 and esc_l >= 10 and esc_r >= 10 and alone >= 100


# ---- E ---------------------------------------------------------------------------

def strand_corr(f, r):
    """Region::strandCorr(0), data.cpp:22-58: five sequential passes"""
    n = len(f)
    if n <= 3:
        return math.nan
    s1 = s2 = 0.0
    for a in f:
        s1 += a
    for b in r:
        s2 += b
    m1, m2 = s1 / n, s2 / n
    q1 = q2 = q3 = 0.0
    for a in f:
        q1 += (a - m1) * (a - m1)
    for b in r:
        q2 += (b - m2) * (b - m2)
    sd1, sd2 = math.sqrt(q1 / (n - 1.0)), math.sqrt(q2 / (n - 1.0))
    for a, b in zip(f, r):
        q3 += (a - m1) * (b - m2)
    d = (n - 1.0) * sd1 * sd2
    return q3 / d if d != 0 else (math.nan if q3 == 0 or math.isnan(q3) else math.copysign(math.inf, q3))


def strand_profiles(oracle, c):
    zero = np.zeros_like(c["cf"])
    f = oracle.profile(c["bw"], c["bg"], c["length"], c["pos"], c["cf"], zero, nondir=True,
                       control=c["control"], coeffs=c["coeffs"])
    r = oracle.profile(c["bw"], c["bg"], c["length"], c["pos"], zero, c["cr"], nondir=True,
                       control=c["control"], coeffs=c["coeffs"])
    return f, r


def same_or_nan(a, b):
    return (math.isnan(a) and math.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes()


def test_slab_lengths(oracle):
    c = K.slab_lengths()
    e = c["expect"]
    regs, sums = K.oracle_run(oracle, c)
    check_sums(c, regs, sums)
    assert len(regs) == 8
    f, r = strand_profiles(oracle, c)
    for i in range(len(regs)):
        l, rt = int(regs["left"][i]), int(regs["right"][i])
        assert same_or_nan(strand_corr(f[l - 1:rt].tolist(), r[l - 1:rt].tolist()), regs["corr"][i]), i
    i3, i4 = holding(regs, e["short"][3]), holding(regs, e["short"][4])
    assert lengths(regs)[i3] == 3 and math.isnan(regs["corr"][i3]) and regs["accepted"][i3] == 0
    assert lengths(regs)[i4] == 4 and regs["corr"][i4] < 0.3 and regs["accepted"][i4] == 0  # a number, rejected
    for n in K.E_LENGTHS:
        l, rt = e["runs"][n]
        assert rt - l + 1 == n
        i = find(regs, l, rt)
        assert regs["corr"][i] >= 0.3 and regs["accepted"][i] == 1
    assert K.E_LENGTHS[0] + 63 == K.CORR_CAP and K.E_LENGTHS[1] + 63 == K.CORR_CAP + 1
    i = find(regs, *e["runs"]["fwd"])
    assert math.isnan(regs["corr"][i]) and not r[regs["left"][i] - 1:regs["right"][i]].any()


def test_slab_reuse(oracle):
    c = K.slab_reuse()
    e = c["expect"]
    regs, sums = K.oracle_run(oracle, c)
    assert len(regs) == e["n_regions"] > 2_100
    n = lengths(regs)
    is_long = n + 63 > K.CORR_CAP
    assert np.array_equal(np.flatnonzero(is_long), e["long_at"])
    assert (n > 3).all() and ((n > 64) & ~is_long).sum() >= 30  # every correlation is a number's worth of sums
    a, b = is_long[:-K.E_WAVES], is_long[K.E_WAVES:]
    assert (a & ~b).sum() >= 20 and (~a & b).sum() >= 20
    assert np.isfinite(regs["corr"]).all()
    check_sums(c, regs[:60], sums[:60])


# ---- F ---------------------------------------------------------------------------

@pytest.mark.parametrize("bw,mode", K.F_CASES)
def test_halo(oracle, bw, mode):
    c = K.halo(bw, mode)
    assert c["length"] <= 80_000
    regs, sums = K.oracle_run(oracle, c)
    check_sums(c, regs, sums)
    assert len(regs) == 5
    for x in c["expect"]["runs"]:
        holding(regs, x)
    for k, x in enumerate(c["expect"]["ties"]):
        i = holding(regs, x)
        # K1b's key Q(p) = sum of count * (bw^2 - d^2) over the window: equal at x and x + 1
        cnt = (c["cf"] if k == 0 else c["cr"])[:, 0].astype(np.int64)
        q = [int((cnt * np.maximum(0, bw * bw - (c["pos"].astype(np.int64) - p) ** 2)).sum()) for p in (x, x + 1)]
        assert q[0] == q[1]
        assert regs["peak"][i] in (x, x + 1)


# ---- G ---------------------------------------------------------------------------

@pytest.mark.parametrize("config", list(K.G_CONFIGS))
def test_strips(oracle, config):
    c = K.strips(config)
    e = c["expect"]
    regs, sums = K.oracle_run(oracle, c)
    check_sums(c, regs, sums)
    assert len(regs) == 5
    idx = {name: find(regs, l, r) for name, (l, r) in e["regions"].items()}
    strip = lambda x: (x - 1) // K.STRIP  # noqa: E731
    l, r = e["regions"]["over"]
    assert strip(l) + 1 == strip(r)
    l, r = e["regions"]["first"]
    assert (l - 1) % K.STRIP == 0 and strip(l) == strip(r)
    l, r = e["regions"]["last"]
    assert r % K.STRIP == 0 and strip(l) == strip(r)
    l, r = e["regions"]["three"]
    assert strip(r) - strip(l) == 2
    assert strip(int(regs["peak"][idx["three"]])) == strip(l)  # the first of its three strips holds the peak
    # the twin maxima: the same bits in two strips, nothing larger; the first wins
    x1, x2 = e["twin"]
    l, r = e["regions"]["twin"]
    prof = K.oracle_profile(oracle, c)
    assert strip(x1) + 1 == strip(x2)
    assert prof[x1 - 1:x1].tobytes() == prof[x2 - 1:x2].tobytes()
    assert prof[l - 1:r].max() == prof[x1 - 1] and (prof[l - 1:r] == prof[x1 - 1]).sum() == 2
    assert regs["peak"][idx["twin"]] == x1 and regs["peak_score"][idx["twin"]] == prof[x1 - 1]


# ---- H ---------------------------------------------------------------------------

@pytest.mark.parametrize("config", list(K.H_CONFIGS))
def test_wraps(oracle, config):
    c = K.wraps(config)
    regs, sums = K.oracle_run(oracle, c)
    check_sums(c, regs, sums)
    assert len(regs) == 1 and lengths(regs)[0] > 65_536
    l, r = int(regs["left"][0]), int(regs["right"][0])
    hp = hit_positions(c, l, r)
    pc = np.zeros(r - l + 1, np.uint64)
    h = stored(c)
    for x, hh in zip((c["cf"], c["cr"]), h):
        m = hh & (c["pos"] >= l) & (c["pos"] <= r)
        np.add.at(pc, c["pos"][m].astype(np.int64) - l, x[m].astype(np.uint64).sum(axis=1))
    off = np.arange(r - l + 1, dtype=np.uint64)
    assert np.array_equal(np.flatnonzero(pc) + l, hp)
    # UShort index (data.cpp:137), uint32 sums
    xs = off % np.uint64(65_536)
    s32 = int(((pc * xs) % np.uint64(2**32)).sum() % 2**32)
    cnt = int(pc.sum())
    assert cnt < 2**32 and int((pc * xs).sum()) >= 2**32  # the position sum wraps as well
    w = pc.astype(np.float64)
    d = xs.astype(np.float64) - s32 / float(cnt)
    k_wrap = (cnt - 1.0) * (w * (d * d) ** 2).sum() / ((w * d * d).sum() ** 2)
    assert abs(regs["kurtosis"][0] - k_wrap) <= 1e-9 * abs(k_wrap)
    d = off.astype(np.float64) - float((w * off.astype(np.float64)).sum() / cnt)
    k_true = (cnt - 1.0) * (w * d ** 4).sum() / ((w * d * d).sum() ** 2)
    assert abs(regs["kurtosis"][0] - k_true) > 1e-3 * abs(k_true)


def test_huge_counts(oracle):
    c = K.huge_counts()
    regs, sums = K.oracle_run(oracle, c)
    check_sums(c, regs, sums)
    assert len(regs) == 2
    i = holding(regs, c["expect"]["at"][0])
    assert i == holding(regs, c["expect"]["at"][1])
    m = (c["pos"] >= regs["left"][i]) & (c["pos"] <= regs["right"][i])
    true0 = int(c["cf"][m, 0].astype(np.uint64).sum())
    assert true0 >= 2 * K.HUGE and sums[i, 0] == true0 - 2**32
    nonctl = true0 + int(c["cf"][m, 1].sum())
    # the wrapped sum misses the hit threshold the true one would meet
    assert nonctl >= c["hit_thr"] > nonctl - 2**32 and regs["accepted"][i] == 0
    assert regs["sum"][i] == (nonctl + int(c["cf"][m, 2].sum())) % 2**32


# ---- I ---------------------------------------------------------------------------

@pytest.mark.parametrize("config", list(K.I_CONFIGS))
def test_many(oracle, config):
    c = K.many(config)
    regs, sums = K.oracle_run(oracle, c)
    check_sums(c, regs, sums)
    assert c["S"] > 256 and sum(c["control"]) == 2 and len(regs) == 2
    for n, (l, r) in c["expect"]["runs"].items():
        assert r - l + 1 == n
        i = find(regs, l, r)
        assert (sums[i] != 0).sum() > 256  # more samples counted than the registers hold
        assert sums[i][np.array(c["control"], bool)].all()
    assert set(c["expect"]["runs"]) == {1_025, 3_000}
