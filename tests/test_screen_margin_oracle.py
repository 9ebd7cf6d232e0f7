"""What the screen-margin inputs (tests/screen_margin_inputs.py) rely on, shown
on the CPU with the oracle and a numpy restatement of the screen's parameters
(up_set_params, csrc/api.hip): if an input stops being marginal this fails,
and tests/test_gpu_screen_margin.py does not pass by accident.

Per population (one motif at every anchor):
  * the layout: no tag at a position <= bw, one copy per pair of strips,
    every edge anchor present, one score bit pattern at every anchor;
  * the oracle's regions one ulp below the marginal score, at it and one ulp
    above: a single position 1, 1, 0 regions per copy; the pair [A, A + 1] with
    peak A, then nothing; the far cluster on the right a run from A, A, A + 1;
    on the left a run up to A, A, A - 1;
  * single and pair: the screen's weighted window sum of the anchor's chunk is
    wskip + 1 -- one tag over the budget (wskip = ceil(thr / (kmax (1 + 1e-6)))
    - 1);
  * the far cluster at u = 16 (d - 1) + 1, the anchor on its chunk's edge: the
    FP32 bound of the anchor's chunk exceeds fthr (soundness of fw and fthr: a
    failure here is a bug of the host formula) by a factor below 1.0002 -- (1
    + 1e-4) / (1 - 1e-6) and FP32 rounding -- so the tags d chunks away decide
    whether the chunk is live."""
import numpy as np
import pytest

from tests import screen_margin_inputs as M

CASES = [(kind, bw) for kind in M.KINDS for bw in M.BWS[kind]]


def test_kernel_restated(oracle):
    for bw in (1, 2, 50, 511, 2000):
        assert M.kernel(bw, M.BG).tobytes() == oracle.kernel(bw, 1.0 / M.BG).tobytes()


def test_positions_and_edges():
    """position p: chunk (p - 1) // 16, word // 64, block // 1,024, strip // 16,384 --
    field kPadPos + p - 1 with kPadPos = 1,024 a multiple of all but the strip,
    which K1 counts from position 1 (kernels.h)"""
    for bw in (1, 50, 511, 2000):
        a = {n: A for n, u, A in M.anchors(bw) if u == 0}
        for e in M.EDGE_AT:
            last, first = a[f"before{e}"], a[f"after{e}"]
            assert (last - 1) // e + 1 == (last + 1 - 1) // e  # last and last + 1 on two sides of the edge
            assert (first - 2) // e + 1 == (first - 1) // e
            bigger = [g for g in M.EDGE_AT if g > e]
            if bigger:  # and on no edge of the next granularity
                assert (last - 1) // bigger[0] == last // bigger[0]
                assert (first - 2) // bigger[0] == (first - 1) // bigger[0]
        assert a["head"] == bw + 1 and a["len"] == M.unit_lengths()[0]
    lens = M.unit_lengths()
    assert all(n % M.STRIP for n in lens)  # a partial last strip
    assert sorted((u, n) for n, u, _ in M.anchors(50) if u) == [(1, "head"), (1, "len"), (2, "head"), (2, "len")]


def regions_of(refs, pop, u, A, reach):
    r = refs[u][0]
    return r[(r["right"].astype(np.int64) >= A - reach) & (r["left"].astype(np.int64) <= A + reach)]


@pytest.mark.parametrize("kind,bw", CASES)
def test_populations_are_marginal(oracle, kind, bw):
    pops = M.populations(kind, bw)
    fams = {p["family"] for p in pops}
    assert fams == ({"single"} if bw == 1 else {"single", "pair", "right", "left"})
    k = M.kernel(bw, M.BG)
    kmax = k.max()
    for pop in pops:
        what = f"{kind} bw {bw} {pop['name']}"
        # ---- layout
        names = [n for n, u, _ in pop["copies"] if u == 0]
        for e in M.EDGE_AT:
            assert f"before{e}" in names and f"after{e}" in names, what
        assert {u for _, u, _ in pop["copies"]} == {0, 1, 2}, what
        for u, (length, pos, cf, cr) in enumerate(pop["units"]):
            assert pos.size and pos.min() > bw and pos.max() <= length, what
            As = np.array(sorted(A for _, uu, A in pop["copies"] if uu == u))
            # one copy per pair of strips, and no strip with its halo reaches two copies
            assert np.unique((As - 1) // (2 * M.STRIP)).size == As.size, what
            assert np.all(np.diff(As) > M.STRIP + 4 * bw), what
            # every tag belongs to the copy nearest to it, within the bandwidth
            near = np.abs(pos.astype(np.int64)[:, None] - As[None, :]).min(axis=1)
            assert near.max() < max(bw, 2 * M.CHUNK), what
        # ---- one bit pattern everywhere
        sc = M.marginal_scores(oracle, pop)
        assert np.unique(sc.view(np.uint64)).size == 1, what
        s = float(sc[0])
        lo, at, hi = M.thresholds(s)
        assert lo < at < hi
        # ---- the oracle's regions at the three thresholds
        runs = [[M.oracle_run(oracle, pop, u, t) for u in range(3)] for t in (lo, at, hi)]
        reach = 2 * bw + M.CHUNK
        for aname, u, A in pop["copies"]:
            r = [regions_of(refs, pop, u, A, reach) for refs in runs]
            n = [len(x) for x in r]
            if pop["family"] == "single":
                assert n == [1, 1, 0], (what, aname, n)
                if pop["tags"] != "chunk16":
                    assert (r[1]["left"][0], r[1]["right"][0], r[1]["peak"][0]) == (A, A, A), (what, aname)
                else:
                    first = M.score_positions(pop, u, A)[0]  # inside the chunk it fills
                    assert first <= r[1]["left"][0] <= r[1]["right"][0] < first + M.CHUNK, (what, aname)
            elif pop["family"] == "pair":
                assert n == [1, 1, 0], (what, aname, n)
                assert r[0]["left"][0] <= A and r[0]["right"][0] >= A + 1
                assert (r[1]["left"][0], r[1]["right"][0], r[1]["peak"][0]) == (A, A + 1, A), (what, aname)
            elif pop["family"] == "right":
                assert n == [1, 1, 1], (what, aname, n)
                assert [int(x["left"][0]) for x in r] == [A, A, A + 1], (what, aname)
            else:
                assert n == [1, 1, 1], (what, aname, n)
                assert [int(x["right"][0]) for x in r] == [A, A, A - 1], (what, aname)
        # ---- the screen's parameters at thr = s
        wskip, w, fw, fthr = M.screen_params(pop, at)
        if pop["family"] == "single" and pop["tags"] != "chunk16":
            n = pop["tags"][0][1] * w[-1]  # (coef: the sample of coefficient 5 weighs 6)
            assert wskip == n - 1, what
            if not pop["nondir"]:  # (both strands: the sum of two rounded products)
                assert s == n * kmax, what
        tight = 0
        for u in range(3):
            ch = M.weighted_chunks(pop, u, w)
            for aname, uu, A in pop["copies"]:
                if uu != u:
                    continue
                ws = M.window_sum(ch, A, bw)
                if pop["tags"] == "chunk16":
                    # 256 tags in one chunk, a plane byte saturated at 255: from bw 75 on the
                    # budget is 255 itself (256 - 16 * 344 / bw^2 > 255), the saturation decides
                    assert ws == 256 * w[-1], what
                    assert wskip >= 255 if kind == "coef" else (wskip == 255) == (bw >= 75), (what, wskip)
                elif pop["family"] in ("single", "pair"):
                    assert ws == wskip + 1, (what, aname, ws, wskip)
                else:
                    assert ws > wskip, (what, aname)
                    d = M.tight_distance(pop, aname, A)
                    if bw <= 511:
                        b = M.fine_bound(ch, A, bw, fw)
                        assert b > fthr, (what, aname, float(b), float(fthr))
                        if d is not None:
                            tight += 1
                            assert float(b) / float(fthr) < 1.0002, (what, aname, float(b) / float(fthr))
        if pop["family"] in ("right", "left") and bw <= 511 and (abs(pop["tags"][0][0] or pop["tags"][1][0]) - 1) % M.CHUNK == 0:
            assert tight >= 6, (what, tight)  # the anchors before (after) every edge


def test_limits_bracketed():
    """single: wskip = n - 1 on both sides of the packed pre-screen's `wskip < 31`
    and of the plane's `wskip >= 255`; n >= 3 is an escaped field (the packed
    path off), 1 and 2 are not"""
    assert {30, 31, 254, 255} <= {n - 1 for n in M.SINGLE_N}
    assert {1, 2} <= set(M.SINGLE_N) and min(n for n in M.SINGLE_N if n > 2) >= 3
    six = sorted(6 * n - 1 for n in M.SINGLE_N_COEF)
    assert max(x for x in six if x < 31) == 29 and min(x for x in six if x >= 31) == 35
    assert max(x for x in six if x < 255) == 251 and min(x for x in six if x >= 255) == 257
