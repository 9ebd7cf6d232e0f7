"""Inputs of the screen-margin tests: regions that sit on the bounds of K1's
screens (csrc/kernels.hip: K1a's packed and register pre-screens, plane_clean,
screen_bits; csrc/wide.hip: K1w's prefix-sum screen) and of K1b's keys.

A *motif* is a fixed relative layout of tags around an anchor position A, so
its scores have the same bits wherever it is placed.  Four families:

  single  n tags at A (n = 1, 2, 4, 31, 32, 255, 256), thr = n kmax: the
          screen's tag budget wskip is n - 1 and the window holds one tag more;
          and `chunk16`, 256 tags as 16 positions of 16 in A's chunk (a
          saturated plane byte), thr = its largest score
  pair    2 tags at A and 2 at A + 1, thr = score(A) = score(A + 1): the region
          is [A, A + 1], wskip 3 against a window of 4
  right   2 tags at A and 200 at A + u, thr = score(A): the run starts exactly
          at A, one ulp higher at A + 1.  u = 16 (d - 1) + 1 is the smallest
          distance between positions of chunks d apart (d = 1, 2, R - 1, R, R =
          ceil(bw / 16)): where A is its chunk's last position the FP32 bound
          of that chunk is fw[0] 2 + fw[d] 200 = 1.0001 thr, the tags d chunks
          away decide.  u = bw - 1 is the last distance with a weight.
  left    the mirror image: 200 tags at A - u, the run ends exactly at A

A *population* is one motif copied to every anchor of three units: the
last position before and the first after an edge of every granularity K1
works in (chunk 16, word 64, plane lane 256, block 1,024, the fields path's
wave load 4,096, strip 16,384), position bw + 1 (the first that is no head
hit), and the unit's last position, the last two on every unit.  Every copy
has a pair of strips of its own, more than a strip and four bandwidths from
the next, so a strip-level pre-screen sees one copy alone; no tag lies at a
position <= bw, so no unit takes the head replay.

A *kind* says how a motif's tags are spread over strands and samples:

  one       one directional sample
  pool      three samples, the middle one a control holding 1,000 tags at A;
            the tags split over the two pooled samples (POOL 1)
  coef      the same with coefficients (0, 5): every tag on the sample of
            coefficient 5, a tag there weighs 6 (POOL 2, quirk Q5)
  nondir    one sample, the tags split over the two strands
  wide, wide_nd   `one` and `nondir` at bandwidths above 511 (K1w)

tests/test_screen_margin_oracle.py shows on the CPU that every population is
marginal in the way described; tests/test_gpu_screen_margin.py runs them."""
import functools

import numpy as np

from tests.k3_general_inputs import kernel

BG = 0.003
CHUNK, WORD, LANE, BLOCK, LOAD, STRIP = 16, 64, 256, 1024, 4096, 16384
FAR = 200        # tags of the far cluster
CONTROL = 1000   # control tags on the anchor (pool, coef)
K_SCR_HALO = 32  # kScrHalo (kernels.h)
K_BIG = 1 << 22  # kBig

KINDS = {
    "one": dict(S=1, nondir=False, control=None, coeffs=None),
    "pool": dict(S=3, nondir=False, control=[0, 1, 0], coeffs=None),
    "coef": dict(S=3, nondir=False, control=[0, 1, 0], coeffs=[0.0, 5.0]),
    "nondir": dict(S=1, nondir=True, control=None, coeffs=None),
    "wide": dict(S=1, nondir=False, control=None, coeffs=None),
    "wide_nd": dict(S=1, nondir=True, control=None, coeffs=None),
}
BWS = {
    "one": (1, 2, 16, 50, 64, 65, 100, 255, 256, 300, 511),
    "pool": (50, 64, 100, 256, 511),
    "coef": (50, 64, 100, 256, 511),
    "nondir": (50, 100, 256, 511),
    "wide": (512, 700, 2000),
    "wide_nd": (512, 700, 2000),
}
SINGLE_N = (1, 2, 4, 31, 32, 255, 256)
# coefficient 5: a tag weighs 6, so 6 n brackets the same limits (wskip 29 | 35, 251 | 257)
SINGLE_N_COEF = (1, 3, 5, 6, 42, 43)

# where an edge of each granularity lies inside a copy's strip pair: on no edge
# of the next granularity
EDGE_AT = {CHUNK: 7 * BLOCK + 3 * CHUNK, WORD: 5 * BLOCK + 3 * WORD, LANE: 9 * BLOCK + LANE,
           BLOCK: 3 * BLOCK, LOAD: 2 * LOAD, STRIP: STRIP}
for _e, _x in EDGE_AT.items():
    assert _x % _e == 0 and (_e == STRIP or _x % (4 * _e) != 0)


def unit_lengths():
    """three units: 28 strips with a partial last one, then two short ones"""
    return (27 * STRIP + 6000, 2 * STRIP + 3000, 3 * STRIP - 100)


@functools.lru_cache(maxsize=None)
def anchors(bw):
    """[(name, unit, A)]: unit 0 holds every edge; all three position bw + 1
    and their last position"""
    out = [("head", 0, bw + 1)]
    j = 1
    for e, x in EDGE_AT.items():
        for side, name in ((0, "before"), (1, "after")):
            out.append((f"{name}{e}", 0, 2 * STRIP * j + x + side))
            j += 1
    lens = unit_lengths()
    out.append(("len", 0, lens[0]))
    for u in (1, 2):
        out += [("head", u, bw + 1), ("len", u, lens[u])]
    return tuple(out)


def far_distances(bw):
    """u of the far families: 16 (d - 1) + 1 for d in {1, 2, R - 1, R} and bw - 1,
    those with a weight (u < bw); above bw 511 (K1w) 1 and bw - 1"""
    if bw > 511:
        return [1, bw - 1]
    R = -(-bw // CHUNK)
    us = {CHUNK * (d - 1) + 1 for d in (1, 2, R - 1, R) if d >= 1} | {bw - 1}
    return sorted(u for u in us if 1 <= u < bw)


def motifs(kind, bw):
    """[(name, family, tags)]: tags = [(offset from A, count)], or "chunk16" """
    ns = SINGLE_N_COEF if kind == "coef" else SINGLE_N
    out = [(f"single{n}", "single", [(0, n)]) for n in ns]
    out.append(("chunk16", "single", "chunk16"))
    if bw >= 2:
        out.append(("pair", "pair", [(0, 2), (1, 2)]))
    for u in far_distances(bw):
        out.append((f"right{u}", "right", [(0, 2), (u, FAR)]))
    for u in far_distances(bw):
        out.append((f"left{u}", "left", [(-u, FAR), (0, 2)]))
    return out


def spread(kind, c):
    """[(strand, sample, count)] of c tags at one position"""
    if kind in ("one", "wide"):
        parts = [(0, 0, c)]
    elif kind == "pool":
        parts = [(0, 0, c // 2), (0, 2, c - c // 2)]
    elif kind == "coef":
        parts = [(0, 2, c)]
    else:
        parts = [(0, 0, c - c // 2), (1, 0, c // 2)]
    return [p for p in parts if p[2]]


def tags_at(tags, A, bw=0, length=None):
    if tags == "chunk16":
        # 16 tags on every position of A's chunk -- of the next one where that chunk
        # begins at a position <= bw, of the one before where it ends past the unit
        first = A - (A - 1) % CHUNK
        if first <= bw:
            first += CHUNK
        elif length is not None and first + CHUNK - 1 > length:
            first -= CHUNK
        return [(first + i, 16) for i in range(CHUNK)]
    return [(A + o, c) for o, c in tags]


@functools.lru_cache(maxsize=None)
def population(kind, bw, name):
    """one motif at every anchor where all of it lies in [bw + 1, len]:
    dict(units=[(length, pos, cf, cr)], copies=[(anchor, unit, A)], ...)"""
    par = KINDS[kind]
    S, nondir = par["S"], par["nondir"]
    family, tags = next((f, t) for n, f, t in motifs(kind, bw) if n == name)
    lens = unit_lengths()
    dense = [dict() for _ in lens]  # position -> counts [2][S]
    copies = []
    for aname, u, A in anchors(bw):
        placed = tags_at(tags, A, bw, lens[u])
        if any(p <= bw or p > lens[u] for p, _ in placed):
            continue
        copies.append((aname, u, A))
        for p, c in placed:
            row = dense[u].setdefault(p, np.zeros((2, S), np.uint32))
            for st, s, v in spread(kind, c):
                row[st, s] += v
        if par["control"]:
            dense[u].setdefault(A, np.zeros((2, S), np.uint32))[0, 1] += CONTROL
    units = []
    for u, length in enumerate(lens):
        pos = np.array(sorted(dense[u]), np.uint32)
        both = np.array([dense[u][int(p)] for p in pos], np.uint32).reshape(len(pos), 2, S)
        units.append((length, pos, both[:, 0].copy(), both[:, 1].copy() if nondir else None))
    return dict(kind=kind, bw=bw, name=name, family=family, tags=tags, units=units, copies=copies, **par)


def populations(kind, bw):
    return [population(kind, bw, n) for n, _, _ in motifs(kind, bw)]


def oracle_args(pop):
    return dict(nondir=pop["nondir"], control=pop["control"], coeffs=pop["coeffs"])


def oracle_profile(oracle, pop, u):
    length, pos, cf, cr = pop["units"][u]
    return oracle.profile(pop["bw"], BG, length, pos, cf, cr, **oracle_args(pop))


def oracle_run(oracle, pop, u, thr):
    """every candidate of unit u at region threshold thr (no kurtosis or hit filter)"""
    length, pos, cf, cr = pop["units"][u]
    return oracle.run_unit(pop["bw"], BG, pos, cf, cr, region_thr=float(thr), kurt_thr=0.0, hit_thr=0.0,
                           cap=1 << 10, **oracle_args(pop))


def score_positions(pop, u, A):
    """the positions whose largest score is the copy's marginal score"""
    if pop["tags"] == "chunk16":
        return [p for p, _ in tags_at("chunk16", A, pop["bw"], pop["units"][u][0])]
    return [A]


def marginal_scores(oracle, pop):
    """the marginal score of every copy, from the oracle's dense profile"""
    prof = {}
    out = []
    for _, u, A in pop["copies"]:
        if u not in prof:
            prof[u] = oracle_profile(oracle, pop, u)
        out.append(max(prof[u][p - 1] for p in score_positions(pop, u, A)))
    return np.array(out, np.float64)


def thresholds(s):
    """one ulp below the marginal score, the score, one ulp above"""
    return (float(np.nextafter(s, -np.inf)), float(s), float(np.nextafter(s, np.inf)))


# ---- the screen's parameters, restated from up_set_params (csrc/api.hip) ----

def screen_params(pop, thr):
    """(wskip, wscreen per non-control sample, fw[0 .. 32] FP32, fthr FP32)"""
    bw = pop["bw"]
    k = kernel(bw, BG)
    nnc = pop["S"] - (sum(pop["control"]) if pop["control"] else 0)
    w = [1] * nnc
    if pop["coeffs"]:
        w = [int(np.ceil(abs(c) + 1.0)) for c in pop["coeffs"]]
    kmax = k.max()
    wf = thr / (kmax * (1.0 + 1e-6))
    assert 0 < wf < K_BIG - 1
    wskip = int(np.ceil(wf)) - 1
    fw = np.zeros(K_SCR_HALO + 1, np.float32)
    for d in range(K_SCR_HALO + 1):
        u0 = 0 if d == 0 else CHUNK * (d - 1) + 1
        kd = max([abs(k[bw + u]) for u in range(u0, bw + 1)], default=0.0)
        want = kd * (1.0 + 1e-4)
        f = np.float32(want)
        if float(f) < want:
            f = np.nextafter(f, np.float32(np.inf))
        fw[d] = f
    return wskip, w, fw, np.float32(thr * (1.0 - 1e-6))


def weighted_chunks(pop, u, w):
    """the screen's weighted tag sum of every chunk of unit u (chunk (p - 1) // 16 of
    position p), over the non-control samples and both strands"""
    length, pos, cf, cr = pop["units"][u]
    nc = [s for s in range(pop["S"]) if not (pop["control"] and pop["control"][s])]
    tot = np.zeros(len(pos), np.int64)
    for i, s in enumerate(nc):
        tot += w[i] * cf[:, s].astype(np.int64)
        if cr is not None:
            tot += w[i] * cr[:, s].astype(np.int64)
    ch = np.zeros((length + 2 * 512) // CHUNK + 2 * K_SCR_HALO + 2, np.int64)
    np.add.at(ch, (pos.astype(np.int64) - 1) // CHUNK, tot)
    return ch


def window_sum(ch, A, bw):
    """weighted tags of the chunks within R = ceil(bw / 16) of A's chunk"""
    R = -(-bw // CHUNK)
    c = (A - 1) // CHUNK
    return int(ch[max(c - R, 0):c + R + 1].sum())


def fine_bound(ch, A, bw, fw):
    """screen_bits' FP32 bound of A's chunk: fw[0] f[c] + sum_d fw[d] (f[c - d] + f[c + d]),
    each step one fused multiply-add (the FP64 sum of an FP32 product and an
    FP32 term, rounded once)"""
    R = -(-bw // CHUNK)
    c = (A - 1) // CHUNK
    f = lambda i: np.float32(ch[i]) if i >= 0 else np.float32(0)
    b = np.float32(fw[0] * f(c))
    for d in range(1, R + 1):
        b = np.float32(float(fw[d]) * float(f(c - d) + f(c + d)) + float(b))
    return b


def tight_distance(pop, aname, A):
    """d when the copy's far cluster lies d chunks from A's chunk at the smallest
    distance two such chunks have, 16 (d - 1) + 1 -- else None"""
    if pop["family"] not in ("right", "left"):
        return None
    u = abs(pop["tags"][0][0] or pop["tags"][1][0])
    if (u - 1) % CHUNK:
        return None
    edge_last = A % CHUNK == 0       # A its chunk's last position
    edge_first = (A - 1) % CHUNK == 0  # A its chunk's first
    if (pop["family"] == "right" and edge_last) or (pop["family"] == "left" and edge_first):
        return (u - 1) // CHUNK + 1
    return None
