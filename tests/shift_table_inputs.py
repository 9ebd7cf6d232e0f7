"""Inputs of the narrow-bandwidth K4 table tests (shift_kernel<NH, POOL>,
kernels.hip; bandwidths up to 511) and their oracle tables.

A case is a dict: the parameters, `max_shift` and a list of nondirectional
units (length, buffer, ascending positions, forward counts [n][S], reverse
counts [n][S]).  Every unit is small (<= 60,000 positions): a few solid blocks
of tags per strand, the reverse strand's block OFF positions to the right, so
that strandCorr(shift) peaks at shift OFF / 2 with a clear margin.

`oracle_tables(oracle, case)` is the reference: per unit the oracle's candidate
regions, exptSums and Region::strandCorr(0 .. max_shift) of each
(orc_run_unit_shifts).  tests/test_oracle_shift.py shows on the CPU that every
case holds the shape it was built for and that the best shift of every region
is clear of near ties; tests/test_gpu_shift_table.py runs them on the GPU.
"""
import functools

import numpy as np

BG = 0.003
OFF = 30          # reverse strand's blocks: OFF positions to the right (best shift OFF / 2)
LDS = 2048        # kShiftLds (kernels.hip): positions of f and r a block keeps in LDS
MARGIN = 1e-9     # every region's best correlation exceeds the others by more than this, relative

WIDTHS = [1, 63, 64, 127, 128, 191, 192, 255, 256, 319, 320, 383, 384, 447, 448, 511]  # both sides of every NH step


def _unit(length, pos, cf, cr, buffer=0):
    return dict(length=int(length), buffer=buffer, pos=np.asarray(pos, np.uint32),
                cf=np.asarray(cf, np.uint32), cr=np.asarray(cr, np.uint32))


def _case(name, bw, units, max_shift, *, S=1, thr=25.0, control=None, coeffs=None, kurt_thr=50.0,
          hit_thr=10.0):
    return dict(name=name, bw=bw, bg=BG, S=S, thr=thr, control=control, coeffs=coeffs, kurt_thr=kurt_thr,
                hit_thr=hit_thr, max_shift=max_shift, units=units)


def from_dense(df, dr, S=1):
    """{pos: counts[S]} per strand -> (pos, cf [n][S], cr [n][S]) over the union of positions"""
    allp = np.array(sorted(set(df) | set(dr)), np.uint32)
    zero = np.zeros(S, np.int64)
    cf = np.array([df.get(int(p), zero) for p in allp], np.int64).reshape(len(allp), S)
    cr = np.array([dr.get(int(p), zero) for p in allp], np.int64).reshape(len(allp), S)
    return allp, cf.astype(np.uint32), cr.astype(np.uint32)


def _block(rng, d, lo, hi, S=1, bump=6):
    """a tag at every position lo..hi of one strand: per sample a count of 1 or
    2 plus a bump of up to `bump` around the middle (counts >= 3 are escapes
    of the 2-bit track)"""
    mid, sd = (lo + hi) / 2.0, max(2.0, (hi - lo) / 6.0)
    for x in range(lo, hi + 1):
        v = d.setdefault(x, np.zeros(S, np.int64))
        v += rng.integers(1, 3, S) + int(np.rint(bump * np.exp(-0.5 * ((x - mid) / sd) ** 2)))


def _blocks_unit(rng, bw, S=1, n=4, small=True):
    """n blocks of max(45, bw) positions each side of their centre on both
    strands, the reverse ones OFF to the right, and a short one (20 each side)
    -> (length, pos, cf, cr); no tag at a position <= bw + 1"""
    hw = max(45, bw)
    step = 4 * (hw + bw) + 500
    df, dr = {}, {}
    for k in range(n):
        c = step * (k + 1)
        _block(rng, df, c - hw, c + hw, S)
        _block(rng, dr, c - hw + OFF, c + hw + OFF, S)
    if small:
        c = step * (n + 1)
        _block(rng, df, c - 20, c + 20, S)
        _block(rng, dr, c - 20 + OFF, c + 20 + OFF, S)
    return (step * (n + 2),) + from_dense(df, dr, S)


# ---- cases ------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def widths(bw):
    """one sample, max_shift 40, four long regions and a short one"""
    rng = np.random.default_rng(8000 + bw)
    return _case(f"width-{bw}", bw, [_unit(*_blocks_unit(rng, bw))], 40)


ESC_COUNTS = (3, 254, 255, 256, 70_000)
POOLING = ["one", "escapes", "control", "coeffs", "near_u32", "over_u32"]


@functools.lru_cache(maxsize=None)
def pooling(bw, mode):
    """api.hip pool_mode() from the inputs: it returns 2 with coefficients, 0
    with one pooled sample, else 1 while (largest count of any track, at least
    2) x (pooled samples) stays below 2^32, else 2.
      one       S = 1                                  -> POOL 0
      escapes   S = 1, counts 3, 254, 255, 256 and 70,000 on both strands at positions
                1024 k - 1 .. 1024 k + 2 (the overflow table's block edge)  -> POOL 0
      control   S = 3, one control: 2 pooled samples, counts <= 8      -> POOL 1
      coeffs    S = 3, coefficients                    -> POOL 2
      near_u32  S = 3, counts 1.4e9 / 1.3e9 / 1.2e9 at a few positions: 3 x 1.4e9 =
                4.2e9 < 2^32 = 4.295e9                 -> still POOL 1, sums of 3.9e9 in uint32 words
      over_u32  S = 3, counts 3e9 / 2e9 / 7: 3 x 3e9 >= 2^32  -> POOL 2 with zero coefficients"""
    rng = np.random.default_rng(8100 + 10 * bw + POOLING.index(mode))
    S = 1 if mode in ("one", "escapes") else 3
    hw = max(45, bw)
    step = 4096  # block centres at multiples of 1,024: the overflow blocks' edges lie inside the regions
    assert 2 * (hw + bw) + OFF < step
    df, dr = {}, {}
    for k in (1, 2, 3):
        _block(rng, df, step * k - hw, step * k + hw, S)
        _block(rng, dr, step * k - hw + OFF, step * k + hw + OFF, S)
    if mode == "escapes":
        for k, (d, e) in enumerate(((df, dr), (dr, df), (df, dr))):
            for i in range(4):
                d[step * (k + 1) - 1 + i][0] = ESC_COUNTS[(i + k) % 5]
                e[step * (k + 1) - 1 + i][0] = ESC_COUNTS[(i + k + 2) % 5]
    big = {"near_u32": (1_400_000_000, 1_300_000_000, 1_200_000_000),
           "over_u32": (3_000_000_000, 2_000_000_000, 7)}.get(mode)
    if big:
        for k in (1, 2, 3):
            for d, at in ((df, -17), (df, 9), (dr, -17 + OFF), (dr, 12 + OFF)):
                d[step * k + at][:] = np.roll(big, k)
    kw = dict(control=[0, 1, 0]) if mode == "control" else dict(coeffs=[0.37, 1.91, 0.7]) if mode == "coeffs" else {}
    return _case(f"pool-{mode}-{bw}", bw, [_unit(step * 4, *from_dense(df, dr, S))], 40, S=S, **kw)


LDS_BW, LDS_SHIFT = 50, 1100
LDS_LENGTHS = (2047, 2048, 2049, 4200)


def _solid(blocks):
    """count-1 tags at every position of [a, a + n) on the forward strand and
    of [a + OFF, a + OFF + n) on the reverse strand, per (a, n)"""
    one = np.ones(1, np.int64)
    df, dr = {}, {}
    for a, n in blocks:
        for x in range(a, a + n):
            df[x] = one
            dr[x + OFF] = one
    return from_dense(df, dr)


@functools.lru_cache(maxsize=None)
def _lds_case(oracle):
    # a solid block's region is the block plus what the kernel's tails add on
    # each side above the threshold: measured once on a probe, then each block
    # is sized for its region's length (the tests assert the lengths from the
    # oracle's regions)
    probe, _ = oracle.run_unit(LDS_BW, BG, *_solid([(1000, 1500)]), nondir=True)
    assert len(probe) == 1
    grow = int(probe["npos"][0]) - 1500
    blocks, a = [], 1000
    for want in LDS_LENGTHS:
        blocks.append((a, want - grow))
        a += want + 1000
    return _case("lds", LDS_BW, [_unit(a, *_solid(blocks))], LDS_SHIFT)


def lds(oracle):
    """regions of exactly 2,047, 2,048 and 2,049 positions (kShiftLds = 2048:
    the last one's scores go to the global slab) and one of 4,200, in one
    unit; max_shift 1,100: shifts past (len - 4) / 2 are NaN, a thread owns up
    to six shifts, and the four lengths minus an even 2 shift give every m & 3"""
    return _lds_case(oracle)


# mixed order, regions given several times: slab offsets for a mixture of LDS and slab regions.  More
# requests than the device has L2 domains (8 XCDs, blocks dealt to them in turn), with the 2,048-position
# region at requests 8 and 16 and slab regions at 0, 9 and 15: a block that took a slab where it
# has none would share it with a block whose writes it can see
LDS_IDX = np.array([3, 1, 0, 3, 2, 0, 2, 3, 1, 3, 0, 2, 1, 0, 2, 3, 1], np.uint64)


@functools.lru_cache(maxsize=None)
def shortest():
    """bw 1 (the kernel's only non-zero weight is its centre: a region is a run
    of tagged positions): runs of 1, 3, 4 and 5 positions, tags of both
    strands in each of the longer ones; max_shift 2"""
    runs = {100: ([3], [0]),
            200: ([2, 1, 0], [0, 3, 1]),
            300: ([2, 1, 0, 3], [1, 0, 2, 1]),
            400: ([1, 0, 2, 1, 4], [0, 3, 1, 2, 0])}
    df, dr = {}, {}
    for a, (f, r) in runs.items():
        for i, (x, y) in enumerate(zip(f, r)):
            assert x + y > 0
            if x:
                df[a + i] = np.array([x], np.int64)
            if y:
                dr[a + i] = np.array([y], np.int64)
    return _case("shortest", 1, [_unit(1000, *from_dense(df, dr))], 2, kurt_thr=0.0, hit_thr=0.0)


@functools.lru_cache(maxsize=None)
def degenerate():
    """bw 10: one region with forward tags only (every correlation 0 / 0), one
    whose reverse tags lie in its first 60 positions (r[2 shift ..] is
    constant from some shift on: NaN there, finite below)"""
    rng = np.random.default_rng(8300)
    df, dr = {}, {}
    _block(rng, df, 500, 800)
    _block(rng, df, 2000, 2400)
    for x in range(2000, 2050, 3):
        dr[x] = rng.integers(1, 6, 1)
    return _case("degenerate", 10, [_unit(4000, *from_dense(df, dr))], 80)


@functools.lru_cache(maxsize=None)
def contig_end():
    """tags up to the unit's last position: the last region's right end lies
    past the contig's length"""
    rng = np.random.default_rng(8400)
    length, bw = 8000, 50
    df, dr = {}, {}
    _block(rng, df, 3000, 3200)
    _block(rng, dr, 3000 + OFF, 3200 + OFF)
    _block(rng, df, 7700, length - OFF)
    _block(rng, dr, 7700 + OFF, length)
    return _case("contig-end", bw, [_unit(length, *from_dense(df, dr))], 40)


@functools.lru_cache(maxsize=None)
def several_units():
    """three units in two buffers"""
    rng = np.random.default_rng(8500)
    units = [_unit(*_blocks_unit(rng, 50, n=n, small=False), buffer=b) for n, b in ((2, 0), (3, 1), (2, 1))]
    return _case("three-units", 50, units, 40)


@functools.lru_cache(maxsize=None)
def heads(bw):
    """quirk Q1: forward tags at positions <= bw and a block of both strands
    that starts 2 bw in, so that the exact replay emits the first records;
    the blocks further on are the parallel scan's"""
    rng = np.random.default_rng(8600 + bw)
    length, pos, cf, cr = _blocks_unit(rng, bw, n=3, small=False)
    df = {int(p): c.astype(np.int64) for p, c in zip(pos, cf) if c.any()}
    dr = {int(p): c.astype(np.int64) for p, c in zip(pos, cr) if c.any()}
    for p in (3, bw // 2, bw):
        df[p] = rng.integers(5, 40, 1)
    _block(rng, df, 2 * bw, 2 * bw + 120)
    _block(rng, dr, 2 * bw + OFF, 2 * bw + 120 + OFF)
    return _case(f"heads-{bw}", bw, [_unit(length, *from_dense(df, dr))], 40)


Q11_BW = 64


@functools.lru_cache(maxsize=None)
def q11(with_heads):
    """region threshold 0 (quirk Q11, K1q): every run of processed positions is
    a region, reached by a leap, so the region stores the positions left - 1 ..
    right - 1 of its record; the unit's last run is never closed.  With heads:
    tags at positions 3, 20 and 40 (<= bw + 1: the unit processes position
    1 and K0 replays the chain from there)"""
    rng = np.random.default_rng(8700 + int(with_heads))
    length, pos, cf, cr = _blocks_unit(rng, Q11_BW, n=4, small=True)
    if with_heads:
        df = {int(p): c.astype(np.int64) for p, c in zip(pos, cf) if c.any()}
        dr = {int(p): c.astype(np.int64) for p, c in zip(pos, cr) if c.any()}
        df[3] = np.array([2], np.int64)
        df[40] = np.array([1], np.int64)
        dr[20] = np.array([2], np.int64)
        pos, cf, cr = from_dense(df, dr)
    return _case(f"q11-{'heads' if with_heads else 'plain'}", Q11_BW, [_unit(length, pos, cf, cr)], 40, thr=0.0)


# ---- the oracle's tables -------------------------------------------------------

_REF = {}


def oracle_tables(oracle, case):
    """per unit (regions, exptSums, table [n][max_shift + 1]) of the case's
    units, each on a buffer of its own (no unit of a multi-unit case has head
    tags, so no state passes between them); computed once, read-only"""
    if case["name"] in _REF:
        return _REF[case["name"]]
    assert len(case["units"]) == 1 or all(u["pos"].min() > case["bw"] + 1 for u in case["units"])
    out = []
    for u in case["units"]:
        ref = oracle.run_unit_shifts(case["bw"], case["bg"], u["pos"], u["cf"], u["cr"], max_shift=case["max_shift"],
                                     region_thr=case["thr"], kurt_thr=case["kurt_thr"], hit_thr=case["hit_thr"],
                                     buffer_forward=u["buffer"] == 0, nondir=True, control=case["control"],
                                     coeffs=case["coeffs"])
        for a in ref:
            a.setflags(write=False)
        out.append(ref)
    _REF[case["name"]] = out
    return out


def reference_best(tab):
    """src/strand_shift.cpp:209-217 per row of a table: shifts ascending, `corr >
    bestCorr` from -1 (NaN never wins) -> (best shift, best correlation)"""
    best = np.zeros(len(tab), np.uint16)
    corr = np.full(len(tab), -1.0)
    for k, row in enumerate(tab):
        for s, v in enumerate(row):
            if v > corr[k]:
                best[k], corr[k] = s, v
    return best, corr


def clear_of_ties(tab):
    """every row's maximum exceeds the value at every other shift by more than
    MARGIN relative (rows without a finite value above -1 have no contest)"""
    for row in tab:
        v = row[~np.isnan(row)]
        if v.size < 2 or v.max() <= -1.0:
            continue
        top = np.sort(v)[-2:]
        if not top[1] - top[0] > MARGIN * abs(top[1]):
            return False
    return True


# ---- what each case was built for, from the oracle's output alone ---------------

def lengths(regs):
    return regs["npos"].astype(np.int64)


def nan_cells_follow_length(regs, tab):
    """NaN exactly where the region is too short for the shift (len <= 2 shift + 3)"""
    s = np.arange(tab.shape[1])
    return bool(np.array_equal(np.isnan(tab), lengths(regs)[:, None] <= 2 * s[None, :] + 3))


def holds_widths(ref):
    regs, _, tab = ref
    s = np.arange(tab.shape[1])
    # (a short window of equal counts may add a 0 / 0 to the cells that are NaN for their length)
    assert len(regs) >= 3 and np.isnan(tab[lengths(regs)[:, None] <= 2 * s[None, :] + 3]).all()
    assert (~np.isnan(tab)).all(axis=1).sum() >= 3, "fewer than 3 regions long enough for every shift"


def holds_pooling(case, ref):
    regs, sums, tab = ref
    assert len(regs) >= 3 and nan_cells_follow_length(regs, tab) and not np.isnan(tab).any()
    u = case["units"][0]
    top = int(max(u["cf"].max(), u["cr"].max()))
    pooled = case["S"] - (sum(case["control"]) if case["control"] else 0)
    mode = 2 if case["coeffs"] else 0 if pooled == 1 else 1 if max(top, 2) * pooled < 2 ** 32 else 2  # pool_mode()
    want = {"one": 0, "escapes": 0, "control": 1, "coeffs": 2, "near_u32": 1, "over_u32": 2}
    assert mode == want[case["name"].split("-")[1]], (case["name"], mode)
    if "escapes" in case["name"]:
        for c in (u["cf"][:, 0], u["cr"][:, 0]):
            esc = np.isin(c, ESC_COUNTS[1:])  # (3 is also an ordinary count of the blocks)
            assert set(c[esc]) == set(ESC_COUNTS[1:]) and (c == 3).any()
            assert {int(p) % 1024 for p in u["pos"][esc]} == {1023, 0, 1, 2}  # both sides of the block edge
            assert all(((regs["left"] <= p) & (p <= regs["right"])).any() for p in u["pos"][esc])
    if "u32" in case["name"]:
        assert int(sums.astype(np.uint64).sum(axis=1).max()) > 2 ** 31  # the huge counts lie inside regions


def holds_lds(ref):
    regs, _, tab = ref
    assert [int(x) for x in lengths(regs)] == list(LDS_LENGTHS), lengths(regs)
    assert LDS_LENGTHS[0] < LDS == LDS_LENGTHS[1] < LDS_LENGTHS[2] and LDS_LENGTHS[3] > 2 * LDS
    assert nan_cells_follow_length(regs, tab)
    assert np.isnan(tab[:3]).any() and not np.isnan(tab[3]).any()  # shifts past (len - 4) / 2
    # m = len - 2 shift over the valid shifts: every residue of m & 3
    assert {(int(n) - 2 * s) & 3 for n in lengths(regs) for s in (0, 1)} == {0, 1, 2, 3}


def holds_shortest(ref):
    regs, _, tab = ref
    assert [int(x) for x in lengths(regs)] == [1, 3, 4, 5]
    finite = ~np.isnan(tab)
    assert finite.tolist() == [[False] * 3, [False] * 3, [True, False, False], [True, False, False]]


def holds_degenerate(ref):
    regs, sums, tab = ref
    assert len(regs) == 2 and lengths(regs).min() > 2 * (tab.shape[1] - 1) + 3  # no cell is NaN for its length
    assert np.isnan(tab[0]).all()
    nan = np.isnan(tab[1])
    k = int(np.argmax(nan))
    assert 0 < k < tab.shape[1] and not nan[:k].any() and nan[k:].all(), nan


def holds_contig_end(case, ref):
    regs, _, tab = ref
    assert int(regs["right"].max()) > case["units"][0]["length"] and not np.isnan(tab).any()


def holds_q11(ref):
    regs, _, tab = ref
    assert len(regs) >= 3 and nan_cells_follow_length(regs, tab)
