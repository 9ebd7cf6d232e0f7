"""Deterministic inputs of the nondirectional wide K1q tests (a threshold <= 0
at bandwidths 512..32767 with both strands in one buffer, up_set_wide_q11_nd
on): shared by tests/test_wide_q11_nd_oracle.py (CPU: the oracle alone shows
that each input has the property it was built for) and
tests/test_gpu_wide_q11_nd.py (GPU: parity with the oracle).

A unit is (length, pos, cf[n, S], cr[n, S]).  With a threshold <= 0 every
maximal run of processed positions -- the positions within bw of an add on
either strand, control samples included -- is one region; its stored positions
are s .. e = a_first - bw .. a_last + bw (e - s + 1 of them: the strand
correlation runs over these), the record reports left = s + 1, right = e + 1,
and the last run of a buffer is never closed, so every unit here ends with a
run of its own that no record reports."""
import numpy as np

from tests import wide_nd_inputs as W
from tests import wide_q11_inputs as Q

STRIP = Q.STRIP
STRETCH = Q.STRETCH
BG = Q.BG
CORR_LONG = 65_536   # kCorrLong: stored positions wide_corr_kernel still takes
TEST_LONG = 8_192    # UNIPEAK_WIDE_CORR_LONG of the child processes
TEST_TILES = (12_288, 4_096)  # UNIPEAK_WIDE_CORR_TILE of the child processes


def dense_unit(length, df, dr, S=1):
    """{pos: count | [counts per sample]} per strand -> a unit"""
    pf, cf = Q.sparse(df, S)
    pr, cr = Q.sparse(dr, S)
    return (length,) + W.merge(pf, cf, pr, cr)


def stored(ref):
    """stored positions of every record (right - left + 1: both ends are one higher)"""
    return ref["right"].astype(np.int64) - ref["left"].astype(np.int64) + 1


# ---- case 1: widths and thresholds ------------------------------------------------
WIDTHS = Q.WIDTHS
THRESHOLDS = Q.THRESHOLDS
REV_SHIFT = 37


def clustered_unit(bw):
    """Q.clustered_unit on the forward strand and the same tags REV_SHIFT downstream
    on the reverse strand: five runs, both strands in each"""
    length, pos, cnt = Q.clustered_unit(bw)
    df = {int(p): int(c) for p, c in zip(pos, cnt[:, 0])}
    dr = {int(p) + REV_SHIFT: int(c) for p, c in zip(pos, cnt[:, 0])}
    return dense_unit(length + REV_SHIFT, df, dr)


# ---- case 2: acceptance by the correlation ------------------------------------------
CORR_BW = 600
CORR_THR = 0.3


def corr_unit():
    """three runs and the closing one at bw 600:
       A around 10,000: the reverse tags are the forward ones 40 downstream (a
         correlation near 1: accepted);
       B around 20,000: a forward cluster and a reverse cluster 1,000 apart (their
         scores rise where the other's fall: rejected);
       C around 30,000: forward tags only (reverseScore 0 everywhere: 0 / 0, NaN)."""
    rng = np.random.default_rng(52)
    df, dr = {}, {}

    def put(d, p, c=1):
        d[int(p)] = d.get(int(p), 0) + c

    for o in np.rint(rng.normal(0, 120, 120)).astype(int):
        put(df, 10_000 + o)
        put(dr, 10_040 + o)
    for o in np.rint(rng.normal(0, 100, 100)).astype(int):
        put(df, 19_500 + o)
    for o in np.rint(rng.normal(0, 100, 100)).astype(int):
        put(dr, 20_500 + o)
    for o in np.rint(rng.normal(0, 120, 120)).astype(int):
        put(df, 30_000 + o)
    put(df, 36_000, 2)
    return dense_unit(36_100, df, dr)


# ---- case 3: the run rule over two strands ------------------------------------------
RULE_BW = 600
RULE_CONTROL = [0, 1, 0]
RULE_COEFFS = (None, [0.6, 1.7], [0.0, 2.0])


def rule_unit():
    """three samples, sample 1 a control, gap = 2bw + 1 = 1,201:
       * forward runs around 10,000 and 12,300 that a reverse-only add at 11,150
         bridges (1,150 from either): one region;
       * 20,000 forward, 21,201 reverse (gap apart: the same run), 22,403 forward
         (gap + 1 apart: a new run);
       * a forward / reverse cluster around 30,000 whose run control-only reverse
         adds at 31,100 and 32,200 extend;
       * a run of control-only adds 40,000 .. 40,900 (every score 0.0: the
         first maximum is the run's first position, which must not be the peak);
       * the closing run."""
    rng = np.random.default_rng(53)
    S = 3
    df, dr = {}, {}

    def put(d, p, s, c=1):
        d.setdefault(int(p), [0] * S)[s] += c

    for c in (10_000, 12_300):
        for o in rng.integers(-50, 51, 20):
            put(df, c + int(o), 0 if o % 2 else 2)
        put(df, c - 50, 0)
        put(df, c + 50, 2)
    put(dr, 11_150, 0)
    put(df, 20_000, 0, 3)
    put(dr, 21_201, 2, 2)
    put(df, 22_403, 0, 4)
    for o in rng.integers(-100, 101, 30):
        put(df, 30_000 + int(o), 0)
        put(dr, 30_060 + int(o), 2)
    put(dr, 31_100, 1, 2)
    put(dr, 32_200, 1, 1)
    for p in range(40_000, 40_901, 300):
        put(dr if (p // 300) % 2 else df, p, 1, 2)
    put(df, 45_000, 0, 2)
    return dense_unit(45_100, df, dr, S)


# ---- case 4: the peak of f + r -----------------------------------------------------------
PEAK_BW = 600
BETWEEN_F, BETWEEN_R = 10_000, 10_800   # the strands' own maxima of the first run
TIE_A, TIE_B = 20_000, 31_000           # the pairs' first positions: strips 1 and 1 / 2


def peak_unit():
    """* run 1: 10 forward tags at 10,000 and 11 reverse tags at 10,800 -- each
         strand's own maximum sits on its add, the maximum of f + r between them;
       * run 2: two adjacent adds of 5 tags at a, a + 1 -- score(a) == score(a + 1) --
         on the forward strand at TIE_A and on the reverse strand at TIE_B, joined
         into one run by single tags 1,100 apart on alternating strands (outside
         each pair's window): f + r ties across stretches, the lower position wins;
       * the closing run."""
    df = {BETWEEN_F: 10, TIE_A: 5, TIE_A + 1: 5}
    dr = {BETWEEN_R: 11, TIE_B: 5, TIE_B + 1: 5}
    for k, p in enumerate(range(TIE_A + 1_100, TIE_B, 1_100)):
        (df if k % 2 else dr)[p] = 1
    df[TIE_B + 4_000] = 1
    return dense_unit(TIE_B + 4_100, df, dr)


# ---- case 5: the long path and its rounds ------------------------------------------------
def long_unit(limit, bw):
    """runs of limit - 1, limit, limit + 1 and 2 * limit - 100 stored positions
    and the closing run, single forward tags at most bw apart from the run's
    first add to its last and reverse tags (1..3 of them) 25 downstream of every
    other one; the first run starts mid-word, and with limit = 8,192 at bw 600
    the second and the fourth run each cross a strip edge.  Only the last two are
    longer than `limit`: on the long path's position axis they lie at
    [0, limit + 1) and [limit + 1, 3 * limit - 99) -- with limit = 8,192 a tile
    of 12,288 holds both in its first round and cuts the second once, a tile of
    4,096 cuts the first twice and the second four times"""
    gap = 2 * bw + 1
    df, dr = {}, {}
    a = bw + 1_000 + 37
    lens = (limit - 1, limit, limit + 1, 2 * limit - 100)
    for n in lens:
        last = a + n - gap  # stored positions a - bw .. last + bw
        p, k = a, 0
        while p < last:
            df[p] = 1 + k % 2
            if k % 2 and p + 25 < last:
                dr[p + 25] = 1 + k % 3
            p += bw - 13 * (k % 5)
            k += 1
        df[last] = 2
        a = last + gap + 500
    df[a] = 1
    return dense_unit(a + 100, df, dr), lens


# ---- case 6: CLIs ---------------------------------------------------------------------
CLI_WIDTHS = Q.CLI_WIDTHS
CLI_LAYOUTS = Q.CLI_LAYOUTS
cli_contigs = Q.cli_contigs
cli_tracks = Q.cli_tracks   # (independent forward and reverse tracks: two strands of one buffer under -D)

# ---- case 7: K4 ---------------------------------------------------------------------------
K4_BW = W.HEAD_BW


def _k4_clusters(rng, centres, df, dr):
    for c in centres:
        for o in np.rint(rng.normal(0, 100, 60)).astype(int):
            df[c + int(o)] = df.get(c + int(o), 0) + 1
        for o in np.rint(rng.normal(0, 100, 60)).astype(int):
            dr[c + 80 + int(o)] = dr.get(c + 80 + int(o), 0) + 1


def k4_units():
    """two units of one buffer, clusters on both strands more than 2bw + 1 apart:
    the first has reverse tags at positions <= bw (a head: the K0 chain's records
    keep their stored scores), the second none"""
    rng = np.random.default_rng(71)
    df, dr = {}, {3: 9, 40: 9, 650: 9}
    _k4_clusters(rng, (4_000, 8_000, 12_000, 16_000), df, dr)
    u0 = dense_unit(18_000, df, dr)
    df, dr = {}, {}
    _k4_clusters(rng, (3_000, 7_000, 11_000, 15_000), df, dr)
    return u0, dense_unit(17_000, df, dr)


# ---- case 8: the dense profile --------------------------------------------------------
PROFILE_BW = 700


def profile_unit():
    return W.parity_unit(PROFILE_BW, length=60_000, seed=611)


# ---- case 9: what stays --------------------------------------------------------------
SWITCH_BW = 700


def switch_unit():
    """a unit with regions at a threshold of 25 and bw 700, and the tags a scatter adds
    between two passes on the reverse strand (a new run past every other)"""
    length, pos, cf, cr = W.parity_unit(SWITCH_BW, length=120_000, seed=902)
    keep = pos < 100_000
    pos, cf, cr = pos[keep], cf[keep], cr[keep]
    free = int(pos.max()) + 2 * SWITCH_BW + 500
    return (length, pos, cf, cr), np.array([free, free + 1, free + 40], np.uint32), np.array([60, 70, 50], np.uint32)


def with_extra(unit, ep, ec):
    length, pos, cf, cr = unit
    df = {int(p): int(c) for p, c in zip(pos, cf[:, 0]) if c}
    dr = {int(p): int(c) for p, c in zip(pos, cr[:, 0]) if c}
    for p, c in zip(ep, ec):
        dr[int(p)] = dr.get(int(p), 0) + int(c)
    return dense_unit(length, df, dr)
