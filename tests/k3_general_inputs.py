"""Inputs of the branch-by-branch tests of the general K3 (stats_kernel<NH, POOL,
NONDIR>, csrc/kernels.hip) and their oracle results.

A case is a dict: the parameters and one unit (length, ascending positions,
forward counts [n][S], reverse counts [n][S] or None) plus `expect`, the
shape it was built for (region lengths, anchors, ...).  `oracle_run(oracle,
case)` is the reference.  tests/test_k3_general_oracle.py shows on the CPU
that every case holds its shape; tests/test_gpu_k3_general.py runs them on the
GPU.

The builders work on dense per-strand count arrays and place every block with
`Unit.region_at`, a numpy estimate of the score profile (a convolution of the
pooled counts with the kernel): region ends lie where the score crosses the
threshold, so an estimate good to 1e-12 finds them unless a score sits on the
threshold itself -- which only the single tall counts of `tall_regions` do,
and there the one product is exact.  Nothing here is trusted: the CPU test
asserts the exact lengths against the oracle.

Two threshold schemes:
  * thr 25 (the reference's default): a run of n consecutive positions holding
    small counts gives one region a little longer than the run;
  * TALL: the threshold is the score of a lone count of 10,000 at its own
    position, kernel[bw] * pooled(10,000): that lone count is a region of
    exactly one position, 10,010 gives three, 10,025 five, two neighbours of
    5,003 (5,009) two (four).  Runs then hold 1,200 per position in sample 0,
    which keeps the score above the threshold across a gap of 64 positions.
"""
import functools

import numpy as np

BW, BG, THR = 50, 0.004, 25.0
SHIFT = 7              # the reverse strand's run: SHIFT positions to the right
STRIP = 16_384         # kStrip (kernels.h): positions of one K1 strip
CACHE = 1_024          # kStatCache * 64: positions of pass-1 totals K3 keeps in LDS
CORR_CAP = 1_024       # StatParams::corr_cap: positions of a wave's correlation slab
TALL = 10_000
SOLID = 1_200


def kernel(bw, bg):
    """orc_kernel restated: 3 (1 - x^2) / 4 on x = i / bw, scaled to sum 1 / bg"""
    x = np.arange(-bw, bw + 1).astype(np.float64) / float(bw)
    w = 3 * (1 - x * x) / 4
    acc = 0.0
    for v in w:
        acc += v
    return w * ((1.0 / bg) / acc)


def lowcount(x, s, mod=3):
    """a small count 0 .. mod-1, a fixed function of (position, sample)"""
    x = np.asarray(x, np.uint64)
    h = (x * np.uint64(2654435761) + np.uint64(s) * np.uint64(2246822519) + np.uint64(12345)) >> np.uint64(9)
    return (h % np.uint64(mod)).astype(np.int64)


class Unit:
    """dense counts of one unit, positions 1 .. length, both strands"""

    def __init__(self, length, S, *, bw=BW, bg=BG, thr=THR, nondir=False, control=None, coeffs=None):
        self.length, self.S, self.bw, self.bg, self.thr, self.nondir = length, S, bw, bg, thr, nondir
        self.control = [0] * S if control is None else list(control)
        self.coeffs = None if coeffs is None else list(coeffs)
        self.F = np.zeros((length + 1, S), np.int64)
        self.R = np.zeros((length + 1, S), np.int64)
        self.k = kernel(bw, bg)
        # countSum weights (peakcall.cpp:186-200; with coefficients the second,
        # unscaled loop adds every pooled count once more, quirk Q5)
        w = np.zeros(S)
        nc = [s for s in range(S) if not self.control[s]]
        for i, s in enumerate(nc):
            w[s] = 1.0 if self.coeffs is None else self.coeffs[i] + 1.0
        self.w = w
        self.nc = nc
        self.bump = 0  # fit(): this much more of sample 0 at the middle position of every run

    def pooled(self, lo, hi):
        lo, hi = max(lo, 0), min(hi, self.length)
        q = self.F[lo:hi + 1] @ self.w
        if self.nondir:
            q = q + self.R[lo:hi + 1] @ self.w
        return lo, q

    def region_at(self, x):
        """estimated (left, right) of the region holding position x"""
        span = 4 * self.bw + 256
        while True:
            lo, q = self.pooled(x - span - self.bw, x + span + self.bw)
            sc = np.convolve(q, self.k)[self.bw:self.bw + q.size]
            ok = sc >= self.thr
            i = x - lo
            assert ok[i], f"position {x} is in no region"
            below = np.flatnonzero(~ok)
            lft, rgt = below[below < i], below[below > i]
            if lft.size and rgt.size and lft[-1] + lo > x - span and rgt[0] + lo < x + span:
                return int(lft[-1] + lo + 1), int(rgt[0] + lo - 1)
            span *= 4

    def fill(self, start, n, base, var=None, strands="f", shift=SHIFT):
        """a run of n positions from `start`: sample s holds base[s], and a small
        count below var[s] more (default: none) at the positions further than
        the bandwidth from both ends of the run -- the scores outside the run,
        and so the region's ends, move with the run; strand 'r' runs `shift` to
        the right"""
        x = np.arange(start, start + n)
        inner = (x > start + self.bw) & (x < start + n - 1 - self.bw)
        for st in strands:
            A, off = (self.F, 0) if st == "f" else (self.R, shift)
            for s in range(self.S):
                v = np.full(n, base[s], np.int64)
                if var is not None and var[s]:
                    v += np.where(inner, lowcount(x + off, s + (100 if st == "r" else 0), var[s]), 0)
                A[x + off, s] = v

    def clear(self, lo, hi):
        self.F[lo:hi + 1] = 0
        self.R[lo:hi + 1] = 0

    def _try(self, start, n, base, var, strands, more=0):
        self.clear(start - 4 * self.bw, start + n + 4 * self.bw + 2 * SHIFT)
        self.fill(start, n, base, var, strands)
        self.F[start + n - 1, 0] += more
        self.F[start + n // 2, 0] += self.bump
        try:
            return self.region_at(start + n // 2)
        except AssertionError:
            return None

    def _fit_len(self, start, length, base, var, strands):
        n = max(16, length - 2 * self.bw)
        for _ in range(6):
            g = self._try(start, n, base, var, strands)
            if g is not None and g[1] - g[0] + 1 == length:
                return g
            n = max(1, n + length - (g[1] - g[0] + 1 if g else 0))
        for div in (1, 2, 4, 8, 16):
            b = [v // div for v in base]
            for n in range(1, length + 1):
                for more in (0, 1, 2, 3):  # quarters of sample 0's count more at the run's last position
                    g = self._try(start, n, b, var, strands, more * (b[0] // 4))
                    if g is not None and g[1] - g[0] + 1 == length:
                        return g
        raise AssertionError(f"no run gives a region of {length} positions")

    def fit(self, start, length, base, var=None, strands=None, left=None, right=None):
        """a run whose region is exactly `length` positions long, starting near
        `start`, or with its region's left (right) end exactly at `left`
        (`right`) -> (left, right) as estimated.  A region much longer than the
        window grows by one position with the run; a short one grows in larger
        steps, so there every run length is tried, with the counts halved until
        one fits."""
        strands = strands or ("fr" if self.nondir else "f")
        for _ in range(8):
            l, r = self._fit_len(start, length, base, var, strands)
            dl = left - l if left is not None else right - r if right is not None else 0
            if dl == 0:
                return l, r
            self.clear(l - 4 * self.bw, r + 4 * self.bw)
            start += dl
        raise AssertionError("no run's region ends where it should")

    def sparse(self):
        m = self.F.any(axis=1) | self.R.any(axis=1)
        pos = np.flatnonzero(m).astype(np.uint32)
        assert pos.size == 0 or pos[0] > 2 * self.bw + 2, "a tag in the head (quirk Q1)"
        cf = self.F[m].astype(np.uint32)
        cr = self.R[m].astype(np.uint32) if self.nondir else None
        assert self.F.max() < 2**32 and self.R.max() < 2**32
        return pos, cf, cr


def _case(name, U, *, kurt_thr=50.0, corr_thr=-1.0, hit_thr=10.0, want_corr=False, **expect):
    pos, cf, cr = U.sparse()
    return dict(name=name, bw=U.bw, bg=U.bg, S=U.S, nondir=U.nondir, control=U.control if any(U.control) else None,
                coeffs=U.coeffs, thr=U.thr, kurt_thr=kurt_thr, corr_thr=corr_thr, hit_thr=hit_thr,
                want_corr=want_corr, length=U.length, pos=pos, cf=cf, cr=cr, expect=expect)


def oracle_run(oracle, case, **over):
    """(regions, exptSums) of every candidate region of the case's unit"""
    kw = dict(region_thr=case["thr"], kurt_thr=case["kurt_thr"], corr_thr=case["corr_thr"],
              hit_thr=case["hit_thr"], nondir=case["nondir"], control=case["control"], coeffs=case["coeffs"])
    kw.update(over)
    return oracle.run_unit(case["bw"], case["bg"], case["pos"], case["cf"], case["cr"], **kw)


def oracle_profile(oracle, case):
    return oracle.profile(case["bw"], case["bg"], case["length"], case["pos"], case["cf"], case["cr"],
                          nondir=case["nondir"], control=case["control"], coeffs=case["coeffs"])


def tall_thr(U):
    """the score of a lone count of TALL in sample 0 (the first pooled sample)
    at its own position, in the reference's operations: countSum = TALL *
    coefficient, then + TALL (Q5), and 0 + kernel[bw] * countSum"""
    cs = float(TALL)
    if U.coeffs is not None:
        cs = 0.0 + float(TALL) * U.coeffs[0]
        cs += float(TALL)
    return float(U.k[U.bw] * cs)


# lone counts of sample 0 (as neighbours at x, x + 1 where two are given) ->
# the region's length under the TALL threshold
TALL_MOTIFS = {1: (TALL,), 2: (5_003, 5_003), 3: (10_010,), 4: (5_009, 5_009), 5: (10_025,)}


def tall_regions(U, at, lengths=(1, 2, 3, 4, 5), step=400, sample=0, split=False):
    """one region per length, `step` apart from `at` -> {length: first tag position}
    (split: the second of two neighbours on the reverse strand -- the same
    scores, and both strands' scores vary over the region)"""
    out = {}
    for i, n in enumerate(lengths):
        for j, c in enumerate(TALL_MOTIFS[n]):
            (U.R if split and j else U.F)[at + step * i + j, sample] = c
        out[n] = at + step * i
    return out


# ---- A: length classes of pass 2 ------------------------------------------------

A_CONFIGS = {  # name -> S, nondir, control samples, coefficients
    "pool1": (3, False, (2,), None),
    "coeffs": (3, False, (2,), (0.37, 1.91)),
    "nondir2": (2, True, (), None),
    "s40": (40, False, (5, 38), None),
}
A_LENGTHS = (64, 65, 1_023, 1_024, 1_025)
A_LONG = 4_500
A_HOLES = {3: 1, 5: 0, 9: 63, 17: 0, 24: 1, 30: 63, 40: 0}  # block of the long region -> hit positions left in it


def _solid_base(S):
    base = [0] * S
    base[0] = SOLID
    var = [3] * S
    var[0] = 0
    return base, var


@functools.lru_cache(maxsize=None)
def ladder(config):
    """case A: regions of 1 .. 5, 64, 65, 1,023, 1,024, 1,025 and 4,500
    positions, in this order of position except the short ones, which come
    first; the 4,500 one holds blocks (64 positions from its left end) with 0,
    1, 63 and 64 hit positions, on both sides of its first 1,024 positions, and
    tags of the control samples alone in the emptied blocks"""
    S, nondir, ctl, coeffs = A_CONFIGS[config]
    control = [1 if s in ctl else 0 for s in range(S)]
    U = Unit(24_000, S, nondir=nondir, control=control, coeffs=coeffs)
    U.thr = tall_thr(U)
    base, var = _solid_base(S)
    short = tall_regions(U, 1_000)
    at, runs = 3_500, {}
    for n in A_LENGTHS + (A_LONG,):
        l, r = U.fit(at, n, base, var)
        runs[n] = (l, r)
        at = r + 600
    l, r = runs[A_LONG]
    for blk, keep in A_HOLES.items():
        x0 = l + 64 * blk
        if keep == 63:
            U.clear(x0 + 40, x0 + 40)
            continue
        U.clear(x0, x0 + 63)
        if keep == 1:
            U.F[x0 + 31, 0] = SOLID
        for s in ctl:  # control tags alone: no pooled count, so no stored hit vector
            U.F[x0 + 5:x0 + 60:9, s] = 2
            if nondir:
                U.R[x0 + 7:x0 + 60:11, s] = 1
    assert U.region_at(l + 2_000) == (l, r), "the holes split the long region"
    return _case(f"ladder-{config}", U, short=short, runs=runs, long=(l, r))


ONE_WAVES = 1_024  # waves of a context's first pass: region i + 1,024 follows region i in its wave
ONE_BUMP = 300
# regions 1,024 .. 1,031 and 2,048 .. 2,055: wave k takes a narrow region, then A[k], then B[k]
ONE_A = (1_024, 1_025, 1_023, 4_500, 64, 65, 1_025, 1_024)
ONE_B = (1_025, 1_024, 4_500, 1_023, 65, 64, 1_024, 1_025)
ONE_STEP = 72  # between the narrow regions' tags: two lone counts 72 apart stay below the threshold between them


@functools.lru_cache(maxsize=None)
def ladder_one():
    """case A with one directional sample, for the general kernel under
    UNIPEAK_K3_ONE=0.  That configuration has K1b's integer keys (Q keys) and,
    with a known peak and at most 1,024 positions, the cached count path, whose
    count bytes are fetched one region ahead within a wave.  So:
      * 2,056 regions: a context's first pass runs 1,024 waves, wave k takes
        regions k, k + 1,024 and k + 2,048.  Regions 0 .. 1,023 are narrow (1 ..
        5 positions, the TALL motifs); regions 1,024 + k and 2,048 + k, k < 8,
        are runs of ONE_A[k] and ONE_B[k] positions; the rest is narrow again.
        A wave thus meets 1,024 then 1,025 positions (the prefetch used, then
        refused), 1,025 then 1,024, 1,023 then 4,500, 64 then 65, ...
      * every run holds ONE_BUMP more at its middle position, so the largest
        key Q = sum of count x (bw^2 - d^2) is unique there: the key arrives
        unmarked, the peak is known and the run takes the cached path if it
        fits.  (A flat run's keys tie along its whole interior, which sends
        the region to K3's own KDE instead.)
    The 4,500 ones hold the emptied blocks of `ladder`."""
    U = Unit(171_000, 1)
    U.thr = tall_thr(U)
    U.bump = ONE_BUMP
    base, var = _solid_base(1)
    order = (3, 1, 5, 2, 4)
    at, idx, runs = 400, 0, {}

    def narrow(upto):
        nonlocal at, idx
        while idx < upto:
            for j, c in enumerate(TALL_MOTIFS[order[idx % 5]]):
                U.F[at + j, 0] = c
            at += ONE_STEP
            idx += 1

    def ladder_runs(lengths):
        nonlocal at, idx
        at += 150
        for n in lengths:
            l, r = U.fit(at + 60, n, base, var)
            if n == A_LONG:
                for blk, keep in A_HOLES.items():
                    x0 = l + 64 * blk
                    if keep == 63:
                        U.clear(x0 + 40, x0 + 40)
                        continue
                    U.clear(x0, x0 + 63)
                    if keep == 1:
                        U.F[x0 + 31, 0] = SOLID
                assert U.region_at(l + 2_000) == (l, r), "the holes split the long region"
            runs[idx] = (l, r)
            idx += 1
            at = r + 150

    narrow(ONE_WAVES)
    ladder_runs(ONE_A)
    narrow(2 * ONE_WAVES)
    ladder_runs(ONE_B)
    assert at < U.length - 200
    return _case("ladder-one", U, runs=runs, n_regions=idx)


# ---- B: a negative coefficient --------------------------------------------------

B_COEFFS = {"negative": (-1.0, 0.5), "positive": (0.37, 1.91)}


@functools.lru_cache(maxsize=None)
def cancelled(which):
    """case B: S = 3, sample 2 the control, coefficients (-1.0, 0.5): with the
    unscaled second loop (Q5) the pooled count is 1.5 x sample 1, so a position
    holding sample 0 alone pools to 0 and stores no hit vector.  A block of
    1,700 positions: every third holds 1 or 2 tags of sample 0 only, the others
    samples 1 and 2; seven of the others hold one tag of sample 0 too.  Sparse
    background of all three samples around it."""
    U = Unit(12_000, 3, control=[0, 0, 1], coeffs=B_COEFFS[which])
    first, n = 4_000, 1_700
    x = np.arange(first, first + n)
    third = (x - first) % 3 == 0
    U.F[x[third], 0] = 1 + lowcount(x[third], 0, 2)
    U.F[x[~third], 1] = 1 + lowcount(x[~third], 1, 2)
    U.F[x[~third], 2] = lowcount(x[~third], 2, 3)
    both = x[~third][40::150][:7]
    U.F[both, 0] = 1
    for s in range(3):
        bgx = 300 + 97 * np.arange(110) + 31 * s
        bgx = bgx[(bgx < first - 300) | (bgx > first + n + 300)]
        U.F[bgx, s] += 1
    return _case(f"cancelled-{which}", U, block=(first, first + n - 1), both=both)


# ---- C: the staged path's boundary (S x strands <= 32) --------------------------

C_CONFIGS = {"s32": (32, False), "s33": (33, False), "s16nd": (16, True), "s17nd": (17, True)}
C_LEFT_MOD = (0, 1, 2, 63)  # left mod 64; (left - 1) mod 64 = 0 starts a 16-byte piece of the track
C_ESCAPES = (3, 254, 255, 256, 70_000, 1 << 24)


@functools.lru_cache(maxsize=None)
def staged(config):
    """case C: one control (the last sample), thr 25; four regions of 300
    positions whose left ends take every class of `left mod 64` in C_LEFT_MOD,
    escaped counts on hit positions of several samples and both strands (the
    2^24 one in the first region only)"""
    S, nondir = C_CONFIGS[config]
    control = [0] * (S - 1) + [1]
    U = Unit(12_000, S, nondir=nondir, control=control)
    base, var = [0] * S, [3] * S
    base[0] = 1
    regions = []
    for i, m in enumerate(C_LEFT_MOD):
        want = 1_024 * (2 * i + 2) + (m if m else 64)
        l, r = U.fit(want + 45, 300, base, var, left=want)
        regions.append((l, r))
        for j, c in enumerate(C_ESCAPES):
            if c == 1 << 24 and i:
                continue
            x = l + 60 + 37 * j
            U.F[x, (3 * j + i) % S] = c
            if nondir:
                U.R[x + 1, (5 * j + i + 1) % S] = c
        # (the escapes raise the score inside the run only by more; the ends stay)
    return _case(f"staged-{config}", U, regions=regions, hit_thr=30.0)


# ---- D: range sums of the per-sample path ----------------------------------------

D_CONFIGS = {"s40": (40, False), "s20nd": (20, True)}
D_THR = 600.0


@functools.lru_cache(maxsize=None)
def range_sums(config):
    """case D: integer pooling beyond the staged path: the non-control exptSums
    are range sums over the tracks (track_range_sum).  thr 600, so that a run
    of low counts (a skirt: one tag per position, a count of 3 every fourth)
    stays below it and a region of a dense core ends inside the skirt: tags lie
    on both sides of both region ends, in the same 16-position chunk.
      32 regions   cores of 130 positions starting i = 0 .. 15 positions past a
                   multiple of 64, then cores of 146 .. 161 positions: the left
                   and the right ends take every residue mod 16
      chunk        a lone count of 162: 11 positions, inside one chunk
      sat          a core with one chunk of sample 1 holding exactly 255 tags
                   and one of sample 2 holding 320 (a saturated plane byte)
    Escapes (3) sit in the skirts, i.e. in the partial end chunks; positions of
    every core hold control tags where no pooled sample has one."""
    S, nondir = D_CONFIGS[config]
    control = [0] * S
    control[4] = control[S - 1] = 1
    U = Unit(40_000, S, nondir=nondir, control=control, thr=D_THR * (2 if nondir else 1))
    nc = U.nc
    strands = "fr" if nondir else "f"
    cores = []

    def block(start, n):
        sk = 70
        for st in strands:
            A, off = (U.F, 0) if st == "f" else (U.R, SHIFT)
            x = np.arange(start - sk, start + n + sk) + off
            for xi in x:  # skirt: one tag per position, sample by position; an escape every fourth
                A[xi, nc[xi % len(nc)]] = 1
                if xi % 4 == 1:
                    A[xi, nc[(xi // 4) % len(nc)]] = 3
            xc = np.arange(start, start + n) + off
            for s in nc[:12]:
                A[xc, s] += 1 + lowcount(xc, s, 2)
            # control tags alone at every 17th core position
            hole = xc[8::17]
            A[hole] = 0
            A[hole, control.index(1)] = 2
            A[hole[::2], S - 1] = 1
        return U.region_at(start + n // 2)

    at = 2_048
    for i in range(32):
        # 16 starts one position on each (every left residue), then 16 lengths
        cores.append(block(at + i, 130) if i < 16 else block(at, 130 + i))
        at += 704
    # a region inside one chunk: positions x - 5 .. x + 5 with (x - 6) mod 16 <= 5
    lone = at + 16 * 10 + 8
    U.F[lone, nc[3]] = 162 * (2 if nondir else 1)
    at += 704
    sat = block(at, 400)
    c255 = ((sat[0] + 120) // 16) * 16 + 1  # first position of a chunk: (x - 1) mod 16 == 0
    c320 = c255 + 160
    for x0, s, big in ((c255, nc[1], 255), (c320, nc[2], 320)):
        U.F[x0:x0 + 16, s] = 1
        U.F[x0 + 6, s] = big - 15
    sat = U.region_at(at + 200)
    return _case(f"range-{config}", U, cores=cores, lone=lone, sat=sat, c255=(c255, nc[1]), c320=(c320, nc[2]),
                 want_corr=nondir, corr_thr=0.3 if nondir else -1.0, hit_thr=30.0)


# ---- E: the correlation slab -----------------------------------------------------

E_LENGTHS = (961, 962, 1_024, 1_025, 3_000)


@functools.lru_cache(maxsize=None)
def slab_lengths():
    """case E, first unit: one pooled sample, both strands, the correlation
    wanted (corr_thr 0.3), the TALL threshold: regions of 3 and 4 positions
    (strandCorr NaN below four positions, and its rejection), of 961 and 962
    (the last length read back from the slab, the first recomputed), 1,024,
    1,025 and 3,000, and one of 500 positions on the forward strand alone (the
    reverse scores' deviation is 0: 0 / 0)"""
    U = Unit(16_000, 1, nondir=True)
    U.thr = tall_thr(U)
    short = tall_regions(U, 1_000, lengths=(3, 4), split=True)
    at, runs = 2_500, {}
    for n in E_LENGTHS:
        l, r = U.fit(at, n, [SOLID], [3])
        # a slope, so that neither strand's scores are flat
        U.F[l + 60:l + 60 + 300, 0] += np.arange(300) // 3
        assert U.region_at(l + 100) == (l, r)
        runs[n] = (l, r)
        at = r + 600
    runs["fwd"] = U.fit(at, 500, [SOLID], [3], strands="f")
    return _case("slab-lengths", U, short=short, runs=runs, want_corr=True, corr_thr=0.3)


E_WAVES = 1_024  # waves of the first pass (the estimate starts at 1,024 regions)


@functools.lru_cache(maxsize=None)
def slab_reuse():
    """case E, second unit: bw 5, more than 2,100 regions: narrow ones (a
    count of 50 on each strand, 13 apart) and long ones (runs of 962 .. 1,000
    positions, not read back from the slab) at the even indices 0 .. 38 and
    1,100 .. 1,138, so that over 1,024 waves 20 waves take a long region, then
    a narrow one, and 20 a narrow one, then a long one"""
    bw, bg = 5, 0.01
    n_regions = 2_200
    long_at = set(range(0, 40, 2)) | set(range(1_100, 1_140, 2))
    U = Unit(120_000, 1, bw=bw, bg=bg, nondir=True)
    at, k = 200, 0
    for i in range(n_regions):
        if i % 50 == 7:  # a middling one, read back from the slab
            n = 100 + (i * 37) % 800
            U.fill(at, n, [1], [3], "fr", shift=3)
            at += n + 30
        elif i in long_at:
            n = 962 + 2 * k
            k = (k + 1) % 20
            U.fill(at, n, [1], [2], "fr", shift=2)
            U.F[at + 100:at + 400, 0] += 1 + np.arange(300) // 100
            at += n + 30
        else:
            U.F[at, 0] = 50 + i % 3
            U.R[at + 1 + i % 2, 0] = 50
            at += 13
    return _case("slab-reuse", U, long_at=sorted(long_at), n_regions=n_regions, want_corr=True, corr_thr=0.3,
                 kurt_thr=0.0, hit_thr=1.0)


# ---- F: halo classes of K3's own KDE ---------------------------------------------

F_WIDTHS = (63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447, 448, 511)  # both sides of every NH step
F_POOLED = (64, 256, 511)
F_CASES = [(bw, "one") for bw in F_WIDTHS] + [(bw, m) for bw in F_POOLED for m in ("control", "coeffs")]
F_MODES = {"one": (1, None, None), "control": (3, [0, 0, 1], None), "coeffs": (3, [0, 0, 1], (0.37, 1.91))}


@functools.lru_cache(maxsize=None)
def halo(bw, mode):
    """case F: both strands with the correlation, so K3 runs its own KDE over
    2 NH + 1 window words, NH = bw / 64 + 1.  The background 0.2 / bw keeps a
    tag's own score at 3.75.  Three runs (bw / 2, 2 bw and 5 bw positions) and
    two tied-key motifs: equal counts at x and x + 1 with equal flanks at
    x - d and x + 1 + d -- K1b's integer key Q is the same at x and x + 1, so
    the key arrives marked and the FP64 first maximum decides."""
    S, control, coeffs = F_MODES[mode]
    U = Unit(16 * bw + 12_000, S, bw=bw, bg=0.2 / bw, nondir=True, control=control, coeffs=coeffs)
    base, var = [1] * S, [2] * S
    at = 3 * bw + 64
    runs = []
    for n in (bw // 2, 2 * bw, 5 * bw):
        U.fill(at, n, base, var, "fr")
        U.F[at + n // 3, 0] += 4  # an escape, and a peak away from the middle
        runs.append(at)
        at += n + 3 * bw + 100
    ties = []
    d = max(3, (3 * bw) // 5)
    for k in range(2):
        x = at + d + bw
        for dx, c in ((0, 10), (1, 10), (-d, 3), (1 + d, 3)):
            (U.F if k == 0 else U.R)[x + dx, 0] += c
        ties.append(x)
        at = x + 4 * bw + 100
    assert at + 2 * bw < U.length
    return _case(f"halo-{bw}-{mode}", U, runs=runs, ties=ties, want_corr=True, corr_thr=0.3, hit_thr=5.0)


# ---- G: peaks of runs that cross strip edges -------------------------------------

G_CONFIGS = {"pool1": (3, False, [0, 0, 1]), "nondir1": (1, True, None)}
G_D = 120  # > 2 bw: the two windows do not overlap


@functools.lru_cache(maxsize=None)
def strips(config):
    """case G: strips of 16,384 positions (strip k: 16,384 k + 1 .. 16,384 (k + 1)).
      over      a region over the edge of strips 0 | 1
      first     a region whose left end is strip 2's first position
      last      a region whose right end is strip 3's last position
      three     a region from strip 4 over strip 5 into strip 6
      twin      over the edge of strips 7 | 8: a count of 1 (per pooled sample
                and strand) at every position and 6 more of sample 0 at x1 =
                edge - 59 and x1 + 120: both windows see the same counts at the
                same offsets, so both scores are the same sum -- the region's
                largest score, bit for bit, in two strips.  The first wins.
    Every other region has one bump of 5 more near its right end, so that its
    peak lies in its last strip."""
    S, nondir, control = G_CONFIGS[config]
    U = Unit(9 * STRIP + 2_000, S, nondir=nondir, control=control)
    base = [1] * S
    regs = {}

    def bump(x):
        U.F[x, 0] += 5

    regs["over"] = U.fit(STRIP - 300, 700, base)
    bump(regs["over"][1] - 120)
    regs["first"] = U.fit(2 * STRIP + 60, 500, base, left=2 * STRIP + 1)
    bump(regs["first"][0] + 90)
    regs["last"] = U.fit(4 * STRIP - 450, 500, base, right=4 * STRIP)
    bump(regs["last"][1] - 90)
    regs["three"] = U.fit(5 * STRIP - 200, STRIP + 400, base)
    bump(regs["three"][0] + 130)  # in strip 4; equal counts elsewhere: later strips hold no larger score
    regs["twin"] = U.fit(8 * STRIP - 400, 800, base)
    x1 = 8 * STRIP - 59
    U.F[x1, 0] += 6
    U.F[x1 + G_D, 0] += 6
    for name, (l, r) in regs.items():
        assert U.region_at((l + r) // 2) == (l, r), name
    return _case(f"strips-{config}", U, regions=regs, twin=(x1, x1 + G_D))


# ---- H: wraps ----------------------------------------------------------------------

H_CONFIGS = {"s2": (2, False, [0, 1]), "nondir1": (1, True, None)}


@functools.lru_cache(maxsize=None)
def wraps(config):
    """case H: a region longer than 65,536 positions (the reference's UShort
    position index wraps in posMean and posKurtosis, and pc * index sums in
    uint32): a tag at every position of 70,000, two in sample 0 at every
    seventh, and a denser stretch past index 65,536 so that the wrapped
    kurtosis differs from the unwrapped one.  kurt_thr 50 decides on the
    wrapped value."""
    S, nondir, control = H_CONFIGS[config]
    U = Unit(90_000, S, nondir=nondir, control=control)
    first, n = 10_000, 70_000
    U.fill(first, n, [1] * S, None, "fr" if nondir else "f")
    x = np.arange(first, first + n)
    U.F[x[::7], 0] += 1
    U.F[first + 66_000:first + 69_000, 0] += 2 + lowcount(np.arange(3_000), 0, 3)
    return _case(f"wraps-{config}", U, block=(first, first + n - 1), want_corr=nondir,
                 corr_thr=0.3 if nondir else -1.0)


HUGE = 3_000_000_000


@functools.lru_cache(maxsize=None)
def huge_counts():
    """case H: S = 3, sample 2 the control; sample 0 holds 3,000,000,000 at two
    positions of one region: its exptSums, Region::sum and the non-control sum
    that meets hit_thr wrap at 2^32 (6e9 mod 2^32 = 1,705,032,704).  A second,
    ordinary region for comparison."""
    U = Unit(8_000, 3, control=[0, 0, 1])
    U.fill(2_000, 300, [1, 1, 1], [2, 2, 2])
    U.F[2_100, 0] = HUGE
    U.F[2_200, 0] = HUGE
    U.fill(5_000, 300, [1, 1, 1], [2, 2, 2])
    return _case("huge-counts", U, at=(2_100, 2_200), hit_thr=2.0e9)


# ---- I: many samples ---------------------------------------------------------------

I_CONFIGS = {"s300": (300, False), "s260nd": (260, True)}


@functools.lru_cache(maxsize=None)
def many(config):
    """case I: more than 256 samples (exptSums in an LDS row per wave), two
    controls, thr 25: one region of 1,025 positions (pass 2 recounts its last
    position) and one of 3,000; sample by position, one or two tags"""
    S, nondir = I_CONFIGS[config]
    control = [0] * S
    control[7] = control[S - 2] = 1
    U = Unit(8_000, S, nondir=nondir, control=control)
    runs = {}
    at = 1_000

    def scatter_samples(l, r):
        for st, A in (("f", U.F), ("r", U.R)):
            if st == "r" and not nondir:
                continue
            x = np.arange(l + 60, r - 60)
            A[x, (x * 7 + (3 if st == "r" else 0)) % S] += 1 + lowcount(x, 1, 2)
            A[x[::5], (x[::5] * 13 + 1) % S] += 1

    for n in (1_025, 3_000):
        l, r = U.fit(at, n, [1] + [0] * (S - 1))
        scatter_samples(l, r)
        assert U.region_at(l + 500) == (l, r)
        runs[n] = (l, r)
        at = r + 600
    return _case(f"many-{config}", U, runs=runs, want_corr=nondir, corr_thr=0.3 if nondir else -1.0,
                 hit_thr=30.0)
