"""Deterministic inputs of the wide K1q tests (threshold <= 0 at bandwidths
512..32767 on directional units): shared by tests/test_wide_q11_oracle.py
(CPU: the oracle alone shows that each input has the property it was built
for) and tests/test_gpu_wide_q11.py (GPU: parity with the oracle).

A unit is (length, pos, cnt[n, S]).  With a threshold <= 0 every maximal run of
processed positions -- the positions within bw of an add -- is one region
[a_first - bw + 1, a_last + bw + 1] (the + 1: the run was reached by a leap),
and the last run of a buffer is never closed, so every unit here ends with a
run of its own that no record reports."""
import numpy as np

from tests.gen import random_unit

STRIP = 16_384     # positions of one strip
STRETCH = 4_096    # positions of one stretch of the peak kernel (64 words)
BG = 0.003


def sparse(dense, S=1):
    """{pos: count | [counts per sample]} -> (pos, cnt[n, S])"""
    pos = np.array(sorted(dense), np.uint32)
    cnt = np.zeros((pos.size, S), np.uint32)
    for i, p in enumerate(pos):
        cnt[i] = dense[int(p)]
    return pos, cnt


def runs_of(pos, bw):
    """the maximal runs of processed positions: [(first add, last add)]"""
    out = []
    for p in (int(x) for x in pos):
        if out and p - out[-1][1] <= 2 * bw + 1:
            out[-1][1] = p
        else:
            out.append([p, p])
    return [tuple(r) for r in out]


def expected_bounds(pos, bw):
    """(left, right) of the records a single-unit buffer reports: every run but the last"""
    return [(a - bw + 1, b + bw + 1) for a, b in runs_of(pos, bw)[:-1]]


# ---- case 2: widths and thresholds ------------------------------------------------
WIDTHS = (512, 600, 2000, 32_767)
THRESHOLDS = (0.0, -1.0, -1e-300)


def clustered_unit(bw, n_clusters=5, tags=40):
    """clusters of single tags, the clusters more than 2bw + 1 apart: one run each"""
    rng = np.random.default_rng(bw)
    sd = 80
    step = 2 * bw + 2 + 12 * sd  # between centres: the clusters' tails never meet
    dense = {}
    first = bw + 2 + 6 * sd
    for k in range(n_clusters):
        c = first + k * step
        for o in np.clip(np.rint(rng.normal(0, sd, tags)), -5 * sd, 5 * sd).astype(int):
            dense[c + int(o)] = dense.get(c + int(o), 0) + 1
    length = first + (n_clusters - 1) * step + 6 * sd + 100
    return (length,) + sparse(dense)


# ---- case 3: gap edges ------------------------------------------------------------
EDGE_WIDTHS = (600, 32_767)


def _next_start(after, gap, bw, off):
    """the smallest add > after + gap whose run start a - bw is `off` past a strip's first position"""
    m = -(-(after + gap + 1 - bw - 1 - off) // STRIP)
    return 1 + m * STRIP + off + bw


def _next_end(after, gap, bw, off):
    """the smallest add > after + gap whose run end a + bw is `off` before a strip's last position"""
    m = -(-(after + gap + 1 + bw + off) // STRIP)
    return m * STRIP - off - bw


def edge_units(bw):
    """two units of single tags:
       0: a1 with a1 - bw on a strip's first position, a1 + (2bw + 1) (the same
          run), then + (2bw + 2) (a new run), an add whose a + bw is a strip's
          last position, and the unit's closing run;
       1: an add with a - bw one past a strip's first position, one with a + bw
          one before a strip's last position, and the closing run.
       At bw 32,767 the adds of unit 0 lie one strip from the boundary they own,
       those of unit 1 two strips."""
    gap = 2 * bw + 1
    a1 = _next_start(bw + 1 - gap, gap, bw, 0)
    adds0 = [a1, a1 + gap, a1 + 2 * gap + 1]
    adds0.append(_next_end(adds0[-1], gap, bw, 0))
    adds0.append(adds0[-1] + gap + 1001)
    b1 = _next_start(bw + 1 - gap, gap, bw, 1)
    adds1 = [b1, _next_end(b1, gap, bw, 1)]
    adds1.append(adds1[-1] + gap + 1001)
    return [(a[-1] + 100,) + sparse({p: 1 for p in a}) for a in (adds0, adds1)]


# ---- case 4: controls and pooling ---------------------------------------------------
POOL_BW = 600
POOL_CONTROL = [0, 1, 0]
POOL_COEFFS = (None, [0.6, 1.7], [0.0, 2.0])
POOL_PEAKS = (3, 254, 255, 320)


def pooled_unit():
    """three samples, sample 1 a control:
       * clusters A (around 10,000) and B (around 12,000) more than 2bw + 1
         apart, bridged by a control-only add at 11,000;
       * cluster C (around 20,000) whose run a control-only add at 21,000 extends;
       * four clusters whose centre holds 3, 254, 255 and 320 tags of sample 0
         (escape table, escape tiles, the saturated chunk sums);
       * the closing run."""
    rng = np.random.default_rng(4)
    S, dense = 3, {}

    def put(p, s, c=1):
        dense.setdefault(int(p), [0] * S)[s] += c

    for c in (10_000, 12_000, 20_000):
        for s in (0, 2):
            for o in rng.integers(-100, 101, 25):
                put(c + int(o), s)
        put(c - 100, 0)
        put(c + 100, 2)
    put(11_000, 1, 2)
    put(21_000, 1, 1)
    for k, peak in enumerate(POOL_PEAKS):
        c = 30_000 + 3_000 * k
        put(c, 0, peak)
        for o in rng.integers(-60, 61, 20):
            put(c + (int(o) or 1), 2 if o % 2 else 0)  # (never on the centre itself)
        put(c + 30, 1, 4)  # a control count beside the peak
    put(45_000, 0, 2)
    return (46_000,) + sparse(dense, S)


# ---- case 5: peak reduction -----------------------------------------------------
LONG_BW = 2000
TIE_BW = 600


def long_unit(where):
    """one run of >= 150,000 positions at bw 2,000 (single tags 3,510 apart), its
    unique maximum (a position of 40 tags) at the run's last add (`last`) or its
    first (`first`); then the closing run"""
    first, step, n = 10_000, 3_510, 46
    dense = {first + step * k: 1 for k in range(n)}
    dense[first + step * (n - 1) if where == "last" else first] = 40
    last = first + step * (n - 1)
    dense[last + 2 * LONG_BW + 3_000] = 2
    return (last + 2 * LONG_BW + 3_100,) + sparse(dense)


def stretch_of(left, x):
    """the peak kernel's stretch of position x in the record with Region::left = left
    (the run [left - 1, ...] scores left .. ; stretches count from the word of `left`)"""
    return ((x - 1) // 64 - (left - 1) // 64) // (STRETCH // 64)


TIE_A, TIE_B = 10_000, 21_000  # the pairs' first positions: strips 0 and 1


def tie_unit():
    """two adjacent adds of 5 tags at a, a + 1 -- score(a) == score(a + 1) -- twice,
    the pairs in different strips and joined into one run by single tags 1,100
    apart (outside each pair's window); then the closing run"""
    dense = {TIE_A: 5, TIE_A + 1: 5, TIE_B: 5, TIE_B + 1: 5}
    for p in range(TIE_A + 1_100, TIE_B, 1_100):
        dense[p] = 1
    dense[TIE_B + 4_000] = 1
    return (TIE_B + 4_100,) + sparse(dense)


# ---- case 6: buffers and heads (bin/regions) ------------------------------------------
CLI_WIDTHS = (600, 2000)
CLI_LAYOUTS = ("head_first", "head_middle", "leak_head_last")


def cli_contigs(layout, bw):
    """[(name, length, kind)]: `plain` clusters past bw + 1, `head` the same plus adds
    at <= bw + 1, `tiny` adds only at <= bw (quirk Q1: the state leaks into the
    next unit), `empty` no tag at all"""
    L = 16 * bw
    return {"head_first": [("h0", L, "head"), ("e", 6 * bw, "empty"), ("b", L, "plain")],
            "head_middle": [("a", L, "plain"), ("e", 6 * bw, "empty"), ("h0", L, "head"), ("b", L, "plain")],
            "leak_head_last": [("a", L, "plain"), ("t", 3 * bw, "tiny"), ("b", L, "plain"),
                               ("h0", L, "head")]}[layout]


def cli_tracks(layout, bw):
    """{contig: [(pos, count)]} for the forward and the reverse strand"""
    rng = np.random.default_rng(bw + 17 * CLI_LAYOUTS.index(layout))
    fwd, rev = {}, {}
    for d in (fwd, rev):
        for name, L, kind in cli_contigs(layout, bw):
            dense = {}
            if kind in ("plain", "head"):
                for c in (4 * bw, 8 * bw, 12 * bw):  # three runs: 4bw apart, clusters within bw / 4
                    for o in rng.integers(-bw // 4, bw // 4 + 1, 30):
                        dense[c + int(o)] = dense.get(c + int(o), 0) + 1
            if kind in ("head", "tiny"):
                for p in {int(x) for x in rng.integers(1, bw + 1, 5)} | ({bw + 1} if kind == "head" else set()):
                    dense[p] = dense.get(p, 0) + int(rng.integers(1, 6))
            if dense:
                d[name] = sorted(dense.items())
    return fwd, rev


# ---- case 7: the dense profile ------------------------------------------------------
PROFILE_BW = 700


def profile_unit():
    rng = np.random.default_rng(7)
    length = 60_000
    pos, cnt = random_unit(rng, length, PROFILE_BW, lo=PROFILE_BW + 2, sd=200)
    return length, pos, cnt


# ---- case 8: mode switches in one context ----------------------------------------------
SWITCH_BW = 700
SWITCH_LEN = 120_000


def switch_unit():
    """clusters that reach a threshold of 25 at bw 700, and the pairs a scatter adds
    between two passes (a new run and a heavier peak)"""
    rng = np.random.default_rng(8)
    pos, cnt = random_unit(rng, SWITCH_LEN, SWITCH_BW, lo=SWITCH_BW + 2, hi=100_000, n_bg=40, n_clusters=8,
                           cluster_tags=(150, 250), sd=150)
    free = int(pos.max()) + 2 * SWITCH_BW + 500  # past every run: a run of its own
    extra_pos = np.array([free, free + 1, free + 40], np.uint32)
    extra_cnt = np.array([60, 70, 50], np.uint32)
    return SWITCH_LEN, pos, cnt, extra_pos, extra_cnt


def with_extra(pos, cnt, extra_pos, extra_cnt):
    d = {int(p): int(c) for p, c in zip(pos, cnt[:, 0])}
    d.update({int(p): int(c) for p, c in zip(extra_pos, extra_cnt)})
    return sparse(d)


# ---- case 1: what keeps the replay ------------------------------------------------------
def first_replayed_unit():
    """bw 32,768: four clusters, the reference's retirement counter wraps"""
    return clustered_unit(32_768, n_clusters=4)
