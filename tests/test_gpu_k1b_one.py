"""K1b for one directional sample (csrc/exact1.hip): the software-pipelined
exact kernel -- a wave's share of the work list as one stream of (item, exact
block) pairs, the next block's window bytes and the next items' headers in
flight while the current block is computed.

Every case is compared three ways: with the oracle (tests/test_gpu_unit.py's
`compare`, bit-exact), bit for bit with the generic K1b run in-process in a
context opened under UNIPEAK_K1B_ONE=0, and by up_last_exact_kind (1 or 0 as
intended), so a later change of the dispatch rule cannot turn these into
tests of the other kernel.  The cases aim at the lookahead: shares with
remainders, waves without an item, a last item with nothing after it
(UNIPEAK_K1B_BLOCKS=1: four waves), consecutive items in different units,
items of 1, 2 and 16 exact blocks, windows reaching into the neighbouring
strip, the padding before position 1 and past len + bw, escapes in a window
that was prefetched, record overflow, the keys' undecided band, every window
width, and pipelined passes.  Each case asserts the property of its input it
relies on (regions present, > 32 runs in a strip, ties), so an input that
stops exercising its branch fails.

A run that ends because the next visited word is not adjacent has a case of
its own (test_run_ends_where_the_next_visited_word_is_not_adjacent): its
input is built against the screen's own bound, so the word after the run is
dead."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

from tests.gen import random_unit
from tests.test_gpu_keys import motif_unit
from tests.test_gpu_unit import compare

pytestmark = pytest.mark.gpu

STRIP, BLOCK = 16384, 1024
BG = 0.003
FIELDS = ("unit", "left", "right", "peak", "sum", "nonctl_sum", "accepted", "close_pos")


@contextmanager
def knobs(**kw):
    """environment read per context in up_open"""
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def make_unit(length, centres, rng, tags=60, sd=25, bg_step=997, extra=()):
    """clusters of `tags` tags around each centre over single tags every
    bg_step positions (never two within a window: background strips are not
    listed), plus (pos, count) extras; vectorised"""
    d = np.zeros(length + 1, np.uint32)
    lo, hi = 110, length
    d[np.arange(200, length - 110, bg_step)] = 1
    if len(centres):
        c = np.repeat(np.asarray(centres, np.int64), tags)
        p = c + np.rint(rng.normal(0, sd, c.size)).astype(np.int64)
        p = p[(p >= lo) & (p <= hi)]
        np.add.at(d, p, 1)
    for p, v in extra:
        d[p] = v
    pos = np.flatnonzero(d).astype(np.uint32)
    return pos, d[pos].reshape(-1, 1)


def gpu_pass(capi, units, bw, one, blocks=None, **params):
    """one blocking pass over `units` [(length, pos, cnt)]: records, counts,
    the K1b and K3 kinds"""
    with knobs(UNIPEAK_K1B_ONE=1 if one else 0, UNIPEAK_K1B_BLOCKS=blocks):
        with capi.Lib(0) as g:
            g.set_params(bw, 1, BG, **params)
            for length, pos, cnt in units:
                u = g.add_unit(length)
                g.scatter(u, 0, 0, pos, cnt[:, 0])
            n = g.run()
            regs, c = g.regions(n)
            return regs, c, g.last_exact_kind(), g.last_k3_kind()


def same_bits(a, b):
    assert len(a) == len(b)
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), k
    for k in ("peak_score", "kurtosis", "corr"):
        assert a[k].tobytes() == b[k].tobytes(), k


def three_way(capi, oracle, units, bw, blocks=None, kind=1, min_regions=1, reverse=(), **params):
    """oracle == exact1_kernel == generic K1b, and the kinds that ran"""
    params.setdefault("kurt_thr", 0.0)
    new, cn, k_new, _ = gpu_pass(capi, units, bw, True, blocks, **params)
    old, co, k_old, _ = gpu_pass(capi, units, bw, False, blocks, **params)
    assert k_new == kind and k_old == 0
    same_bits(new, old)
    assert np.array_equal(cn, co)
    total = 0
    refs = []
    opar = {k: v for k, v in params.items() if k in ("region_thr", "kurt_thr", "hit_thr")}
    for u, (length, pos, cnt) in enumerate(units):
        if u in reverse:
            ref, sums = oracle.run_unit(bw, BG, pos, None, cnt, buffer_forward=False, **opar)
        else:
            ref, sums = oracle.run_unit(bw, BG, pos, cnt, **opar)
        m = new["unit"] == u
        compare(ref, sums, new[m], cn[m])
        total += len(ref)
        refs.append(ref)
    assert total >= min_regions
    return new, refs


def strips_unit(n, rng):
    """n strips, every one listed: a cluster in each, in a block that moves
    with the strip; every fourth a second exact block"""
    length = n * STRIP - 300
    centres = []
    for s in range(n):
        centres.append(s * STRIP + BLOCK * (s % 16) + 500)
        if s % 4 == 1:
            centres.append(s * STRIP + BLOCK * ((s + 7) % 16) + 300)
    centres = [c for c in centres if c < length - 200]
    return (length,) + make_unit(length, centres, rng)


@pytest.mark.parametrize("n,blocks", [(1, 1), (3, 1), (4, 1), (5, 1), (8, 1), (9, 1), (41, 1), (41, 2)])
def test_lookahead_across_items(gpu_lib, oracle, n, blocks):
    """four (eight) waves over n listed strips: shares with remainders, waves
    with no item, a last item with nothing after it"""
    rng = np.random.default_rng(700 + n)
    unit = strips_unit(n, rng)
    _, refs = three_way(gpu_lib, oracle, [unit], 50, blocks=blocks, min_regions=n)
    # every strip holds a region: every strip is listed
    assert np.unique((refs[0]["left"].astype(np.int64) - 1) // STRIP).size == n


def test_no_listed_strip(gpu_lib, oracle):
    """a pass whose work list is empty (sparse background only: no wave has
    an item), then the same unit shape with one listed strip (three of four
    waves have none)"""
    rng = np.random.default_rng(1)
    length = 5 * STRIP
    unit = (length,) + make_unit(length, [], rng)
    new, refs = three_way(gpu_lib, oracle, [unit], 50, blocks=1, min_regions=0)
    assert len(new) == 0 and len(refs[0]) == 0
    unit = (length,) + make_unit(length, [3 * STRIP + 500], rng)
    new, refs = three_way(gpu_lib, oracle, [unit], 50, blocks=1, min_regions=1)
    assert np.unique((refs[0]["left"].astype(np.int64) - 1) // STRIP).tolist() == [3]


def test_items_across_units(gpu_lib, oracle):
    """consecutive items of a wave in different units: the next item's track
    address and first position come from another descriptor"""
    rng = np.random.default_rng(2)
    lengths = [STRIP - 300, 3 * STRIP + 5000, 2 * STRIP - 200, 50_000, 6 * STRIP - 7000]
    units = []
    for length in lengths:
        last0 = ((length + 50) // STRIP) * STRIP  # first position of the last strip - 1
        centres = sorted({600, 9000, min(last0 + 900, length - 300), length - 300})
        units.append((length,) + make_unit(length, centres, rng))
    for blocks in (1, None):
        _, refs = three_way(gpu_lib, oracle, units, 50, blocks=blocks, min_regions=2 * len(units), reverse=(2,))
    # the listed strips (those holding a region) in global order, with their
    # units: every unit is listed in its first and its last strip, and with
    # four waves (blocks=1) a wave's next item lies four items on -- in another
    # unit for most of them, whichever way the list's two halves are split
    listed = []
    for u, (ref, length) in enumerate(zip(refs, lengths)):
        strips = np.unique((ref["left"].astype(np.int64) - 1) // STRIP)
        assert strips[0] == 0 and strips[-1] == (length + 50 - 1) // STRIP, u
        listed += [u] * strips.size
    listed = np.array(listed)
    assert listed.size > 8 and np.mean(listed[4:] != listed[:-4]) > 0.5


def test_block_shapes(gpu_lib, oracle):
    """items of 1, 2 and 16 exact blocks; blocks 0 and 15 (the window reaches
    into the neighbouring strip); the unit's first strip (padding before
    position 1) and last strip (past len + bw); runs across a strip edge and
    across block edges; spikes whose runs end at every offset of a word"""
    rng = np.random.default_rng(3)
    length = 7 * STRIP - 2000
    centres = [300]                                              # strip 0, block 0: one block
    centres += [STRIP + 400, STRIP + 15 * BLOCK + 600]           # strip 1: blocks 0 and 15
    centres += [2 * STRIP + j * BLOCK + 512 for j in range(16)]  # strip 2: 16 blocks
    centres += [3 * STRIP, 4 * STRIP + 1]                        # runs across strip edges
    centres += [4 * STRIP + 5 * BLOCK, 4 * STRIP + 9 * BLOCK + 1]  # runs across block edges
    centres += [length - 40]                                     # the window runs past len + bw
    # single spikes five words and one position apart: their runs end at 48 offsets of a word
    extra = [(5 * STRIP + 200 + 321 * k, 40) for k in range(48)]
    unit = (length,) + make_unit(length, centres, rng, extra=extra)
    for blocks in (1, None):
        new, refs = three_way(gpu_lib, oracle, [unit], 50, blocks=blocks, min_regions=20)
    ref = refs[0]
    left, right = ref["left"].astype(np.int64) - 1, ref["right"].astype(np.int64) - 1
    assert np.any(left // STRIP != right // STRIP)  # a run across a strip edge
    assert np.any((left // BLOCK != right // BLOCK) & (left // STRIP == right // STRIP))
    assert np.unique(left[left // STRIP == 2] // BLOCK).size >= 14  # the 16-block item
    assert np.unique(right[(left // STRIP == 5)] % 64).size > 32   # run ends spread over a word


def test_run_ends_where_the_next_visited_word_is_not_adjacent(gpu_lib, oracle):
    """A run whose last position is lane 63 of a visited word while the word
    after it is dead to the screen, so the run is closed by `open && g != last
    + 1` when a later word of the strip is visited, and by the strip's end
    (`last != kStripWords - 1`) when none is.

    Input: counts of 2 (no escape) at x - 48, x - 32, x - 16, x the last
    position of a word.  score(x) = score(x - 64) = 2 (k16 + k32 + k48), the
    largest of [x - 64, x]; score(x + 1) = 2 (k17 + k33 + k49).  The screen's
    bound of the first chunk after x (api.hip: fw[d] = the weight at the
    smallest distance of chunks d apart, 1, 17, 33, 49, times 1 + 1e-4) is
    that same 2 (k17 + k33 + k49) (1 + 1e-4), and smaller for the chunks
    further on.  With the threshold halfway between the two scores (2.5 %
    apart at bw 50) the run is [x - 64, x] and every chunk of the next word
    stays under the screen's bound: the word is dead."""
    bw = 50
    k = oracle.kernel(bw, 1.0 / BG)[bw:]  # k[d]
    s_in, s_out = 2 * (k[16] + k[32] + k[48]), 2 * (k[17] + k[33] + k[49])
    thr = 0.5 * (s_in + s_out)
    # the screen's FP32 test of the next word's first chunk (b > fthr: live)
    fw = [np.float32(k[u] * (1 + 1e-4)) for u in (17, 33, 49)]
    bound = np.float32(2) * (fw[0] + fw[1] + fw[2])
    assert float(bound) * (1 + 1e-5) < thr * (1 - 1e-6) and s_in > thr * (1 + 1e-6)
    length = 4 * STRIP
    ends = [64 * 40, 64 * 43,              # strip 0: the second run's word is visited two words later
            STRIP + 64 * 16,               # strip 1: the run ends with a block, nothing after it in the strip
            2 * STRIP + 64 * 100, 2 * STRIP + 64 * 140,  # strip 2: the next visited word is in another block
            3 * STRIP + 64 * 255]          # strip 3: last visited word 254, not the strip's last
    d = np.zeros(length + 1, np.uint32)
    for x in ends:
        d[[x - 48, x - 32, x - 16]] = 2
    pos = np.flatnonzero(d).astype(np.uint32)
    cnt = d[pos].reshape(-1, 1)
    for blocks in (1, None):
        _, refs = three_way(gpu_lib, oracle, [(length, pos, cnt)], bw, blocks=blocks, region_thr=float(thr),
                            min_regions=len(ends))
    ref = refs[0]
    assert ref["right"].tolist() == ends and ref["left"].tolist() == [x - 64 for x in ends]
    prof = oracle.profile(bw, BG, length, pos, cnt)
    for x in ends:  # position p at prof[p - 1]
        assert prof[x - 1] >= thr > prof[x] and prof[x - 65] >= thr > prof[x - 66]


def test_record_overflow(gpu_lib, oracle):
    """test_dense_unit_overflows_inline_records' input: more than 32 runs in a
    strip spill the strip's records to an overflow slot"""
    length, bw = 40_000, 5
    pos = np.arange(200, 30_000, 13, dtype=np.uint32)
    cnt = np.full((pos.size, 1), 50, np.uint32)
    _, refs = three_way(gpu_lib, oracle, [(length, pos, cnt)], bw, kurt_thr=0.0, hit_thr=1.0, min_regions=1000)
    assert np.bincount((refs[0]["left"].astype(np.int64) - 1) // STRIP).max() > 32


def escape_unit(rng, values):
    """clusters on block edges holding escaped counts at a block's last
    position, at the next block's first (the halo word of the block before)
    and in the first exact block of the next listed strip"""
    length = 6 * STRIP
    centres, extra = [], []
    for i, v in enumerate(values):
        s = i % 4
        edge = s * STRIP + (3 + 2 * i) * BLOCK  # last position of a block
        centres += [edge, edge - BLOCK + 20, (s + 1) * STRIP + 40]
        extra += [(edge, v), (edge + 1, v), (edge - BLOCK + 1, v), ((s + 1) * STRIP + 1, v),
                  ((s + 1) * STRIP + 64, v)]
    return (length,) + make_unit(length, centres, rng, extra=extra)


def test_escapes_in_a_prefetched_window(gpu_lib, oracle):
    """counts 3, 4, 255 and 3,000 (escapes of the 2-bit fields) at a block's
    first and last position, in the halo word of the following block and in
    the first block of the next item; the keys stay on"""
    rng = np.random.default_rng(4)
    unit = escape_unit(rng, (3, 4, 255, 3000))
    for blocks in (1, None):
        _, refs = three_way(gpu_lib, oracle, [unit], 50, blocks=blocks, min_regions=8)
    # every escaped count placed above lies inside a region (so in an exact
    # block that ran), the 3,000s among them
    ref = refs[0]
    length, pos, cnt = unit
    esc = pos[np.isin(cnt[:, 0], (3, 4, 255, 3000)) & (pos % BLOCK <= 64)]
    assert esc.size >= 16
    for p in esc:
        assert np.any((ref["left"] <= p) & (p <= ref["right"])), int(p)
    assert (ref["sum"] >= 3000).sum() >= 2


def test_count_beyond_the_keys(gpu_lib, oracle):
    """one count of 2,000,000: Q no longer fits uint32, the keys go off and
    the generic kernel runs (kind 0); the records still equal the oracle"""
    rng = np.random.default_rng(5)
    length, pos, cnt = escape_unit(rng, (3, 4, 255, 3000))
    cnt = cnt.copy()
    cnt[np.searchsorted(pos, 2 * STRIP + 40), 0] = 2_000_000
    three_way(gpu_lib, oracle, [(length, pos, cnt)], 50, blocks=1, kind=0, min_regions=8)


def q_profile(length, pos, cnt, bw):
    """the keys' exact integer Q(x) = sum c_h (bw^2 - (x - h)^2)"""
    d = np.zeros(length + 2 * bw + 2, np.int64)
    d[pos] = cnt[:, 0]
    k = bw * bw - np.arange(-bw, bw + 1, dtype=np.int64) ** 2
    return np.convolve(d, k, mode="same")


@pytest.mark.parametrize("bw", [50, 90])
def test_tied_peaks(gpu_lib, oracle, bw):
    """test_gpu_keys' motif_unit: the run's largest key at two positions,
    within a strip and across a strip edge (K3 orders them by FP64 score)"""
    rng = np.random.default_rng(31 + bw)
    length = 5 * STRIP
    centres, sep, count = [], [], []
    x = 2000
    while x < length - 2000:
        centres.append(x)
        sep.append(int(rng.choice([1, 3, 5, 11, 2 * (bw // 2) + 1])))
        count.append(int(rng.integers(8, 14)))
        x += int(rng.integers(700, 1500))
    for s in range(1, 5):
        centres.append(s * STRIP)  # a pair straddling a strip edge: the tie spans two strips
        sep.append(1)
        count.append(12)
    pos, cnt = motif_unit(rng, length, bw, centres, sep, count)
    # no background within reach of the edge pairs: their two keys stay equal
    d = pos.astype(np.int64)[:, None] - STRIP * np.arange(1, 5)[None, :]
    keep = ~np.any((np.abs(d) <= bw + 2) & (d != 0) & (d != 1), axis=1)
    pos, cnt = pos[keep], cnt[keep]
    _, refs = three_way(gpu_lib, oracle, [(length, pos, cnt)], bw, min_regions=20)
    q = q_profile(length, pos, cnt, bw)
    ties = edge_ties = 0
    for l, r in zip(refs[0]["left"].astype(np.int64), refs[0]["right"].astype(np.int64)):
        at = l + np.flatnonzero(q[l:r + 1] == q[l:r + 1].max())
        ties += at.size > 1
        edge_ties += at.size > 1 and (at[0] - 1) // STRIP != (at[-1] - 1) // STRIP
    assert ties > 10 and edge_ties > 0


def test_threshold_on_an_fp64_score(gpu_lib, oracle):
    """a region threshold equal to an FP64 score the oracle computed, and one
    ulp either side: Q cannot decide those lanes, the FP64 walk must"""
    rng = np.random.default_rng(500)
    length, bw = 60_000, 50
    pos, cnt = random_unit(rng, length, bw)
    prof = oracle.profile(bw, BG, length, pos, cnt)
    cand = prof[(prof > 5.0) & (prof < 60.0)]
    assert cand.size > 100
    thr = rng.choice(cand)
    for t in (thr, np.nextafter(thr, np.inf), np.nextafter(thr, -np.inf)):
        three_way(gpu_lib, oracle, [(length, pos, cnt)], bw, region_thr=float(t))


@pytest.mark.parametrize("bw", [20, 63, 64, 127, 128, 300])
def test_window_widths(gpu_lib, oracle, bw):
    """either side of every change of NH = ceil((bw + 1) / 64), and NH 5"""
    rng = np.random.default_rng(900 + bw)
    length = 5 * STRIP + 3000
    pos, cnt = random_unit(rng, length, bw, n_clusters=30)
    for blocks in (1, None):
        three_way(gpu_lib, oracle, [(length, pos, cnt)], bw, blocks=blocks, min_regions=10)


def test_pipelined_passes(gpu_lib, oracle):
    """five passes in flight on one context: every slot's records equal the
    blocking pass's; then one unit's track changes between passes and the
    next pass sees the new data, with the same kernels"""
    capi = gpu_lib
    rng = np.random.default_rng(6)
    bw = 50
    units = [strips_unit(n, rng) for n in (9, 3, 5)]
    with knobs(UNIPEAK_K1B_ONE=1, UNIPEAK_K1B_BLOCKS=None):
        with capi.Lib(0) as g:
            g.set_params(bw, 1, BG, kurt_thr=0.0)
            for length, pos, cnt in units:
                g.scatter(g.add_unit(length), 0, 0, pos, cnt[:, 0])
            n = g.run()
            ref, rcnt = g.regions(n)
            kinds = (g.last_exact_kind(), g.last_k3_kind())
            assert kinds == (1, 1) and n > 17
            for _ in range(2):
                for _ in range(5):
                    g.run_async()
                for _ in range(5):
                    m = g.run_wait()
                    regs, cnt_ = g.regions(m)
                    assert m == n and regs.tobytes() == ref.tobytes() and np.array_equal(cnt_, rcnt)
                    assert (g.last_exact_kind(), g.last_k3_kind()) == kinds
            # a new cluster in unit 1, in a strip edge's window
            length, pos, cnt = units[1]
            add = np.arange(2 * STRIP - 20, 2 * STRIP + 20, dtype=np.uint32)
            add = add[~np.isin(add, pos)]
            g.scatter(1, 0, 0, add, np.full(add.size, 2, np.uint32))
            pos2 = np.concatenate([pos, add])
            o = np.argsort(pos2)
            units[1] = (length, pos2[o], np.concatenate([cnt[:, 0], np.full(add.size, 2, np.uint32)])[o].reshape(-1, 1))
            g.run_async()
            g.run_async()
            for _ in range(2):
                m = g.run_wait()
                regs, cnt_ = g.regions(m)
                assert (g.last_exact_kind(), g.last_k3_kind()) == kinds
    assert m > n
    for u, (length, pos, cnt) in enumerate(units):
        r, sums = oracle.run_unit(bw, BG, pos, cnt, kurt_thr=0.0)
        sel = regs["unit"] == u
        compare(r, sums, regs[sel], cnt_[sel])
    old, co, k_old, _ = gpu_pass(capi, units, bw, False, kurt_thr=0.0)
    assert k_old == 0
    same_bits(regs, old)
    assert np.array_equal(cnt_, co)
