"""The per-dataset index byte for byte (csrc/kernels.h; csum_units_kernel,
pool_units_kernel, pct_units_kernel, unit_last_kernel): the packed tracks,
the chunk-sum planes, the pooled plane and the pooled count track of every unit, read
back through up_unit_index_read and compared over the whole array -- padding included --
with tests/index_ref.py.  A pass only shows a wrong index byte when a region happens to
sit on it; here every byte is a closed-form integer function of the scattered counts, so
the comparison is np.array_equal.

A chunk is 16 positions: chunk k of the contig holds positions 16k + 1 .. 16k + 16
(kPadPos is a multiple of 16), field f of it is position 16k + 1 + f.  In-place fields
hold at most 2, so 16 of them reach 32: the sums 254, 255 and 256 are built from
escapes only and from escapes mixed with in-place counts; the in-place-only chunks
cover 0 .. 32.
"""
import numpy as np
import pytest

from tests.index_ref import UnitModel, index_arrays, unit_stride
from tests.test_gpu_replay import compare

pytestmark = pytest.mark.gpu

BG = 0.003
GRID_CAP = 8192 * 256  # threads of an index launch at most (api.hip sync_index, `grid`)
NAMES = ("tracks", "csum", "pooled", "pct")  # UP_IDX_* in order


def open_ctx(capi, bw, S, policy=None, **kw):
    if capi.track_bits() != 2:
        pytest.skip("the 4-bit track build keeps no index")
    g = capi.Lib(0)
    g.set_index_policy(capi.INDEX_ALWAYS if policy is None else policy)
    g.set_params(bw, S, BG, **kw)
    return g


def put(g, m, u, strand, sample, pos, cnt):
    pos, cnt = np.asarray(pos, np.uint32), np.asarray(cnt, np.uint32)
    g.scatter(u, strand, sample, pos, cnt)
    m.scatter(strand, sample, pos, cnt)


def same(got, want, what):
    if got.shape == want.shape and np.array_equal(got, want):
        return
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    i = int(bad[0])
    raise AssertionError(f"{what}: {len(bad)} of {len(got)} bytes differ, first at byte {i}: "
                         f"got {int(got[i])}, want {int(want[i])}")


def check(capi, g, u, m, control=None, coeffs=None, *, pooled, pct):
    lay = g.unit_layout(u)
    assert (lay.len, lay.nstrands, lay.n_samples, lay.pad_pos, lay.track_bits, lay.index_on) == \
        (m.length, m.nstrands, m.S, 1024, 2, 1)
    assert lay.stride % 256 == 0 and 4 * lay.stride >= 2 * lay.pad_pos + m.length
    assert (lay.has_pooled, lay.has_pct) == (int(pooled), int(pct)), (lay.has_pooled, lay.has_pct)
    ref = index_arrays(m.sparse(), lay.stride, lay.pad_pos, m.nstrands, m.S, control, coeffs, want_pct=pct)
    for what, key in enumerate(NAMES):
        if (key == "pooled" and not pooled) or (key == "pct" and not pct):
            continue
        same(g.index_read(u, what), ref[key], f"unit {u} {key}")
    for kept, what in ((pooled, capi.IDX_POOLED), (pct, capi.IDX_PCT)):
        if not kept:
            with pytest.raises(capi.UpError) as e:
                g.index_read(u, what)
            assert e.value.code == capi.UP_E_STATE
    assert g.last_add(u) == ref["last_add"], "last_add"
    return lay


# ---- saturation and escapes ---------------------------------------------------------

E16 = list(range(16))
CHUNKS = [  # {field: count} per chunk, each in a chunk of its own
    # in place only: 0 .. 32
    dict.fromkeys(E16, 2), {0: 1}, {15: 2}, {0: 2, 7: 1, 15: 1}, {f: 1 + f % 2 for f in E16},
    # escapes only: 254, 255, 256 from sixteen, three and two escapes
    {**dict.fromkeys(E16, 16), 15: 14}, {**dict.fromkeys(E16, 16), 15: 15}, dict.fromkeys(E16, 16),
    {3: 85, 4: 85, 5: 84}, {3: 85, 4: 85, 5: 85}, {3: 86, 4: 85, 5: 85},
    {0: 127, 15: 127}, {0: 127, 15: 128}, {0: 128, 15: 128},
    # a single escape: 254 (its tile byte), 255, 256 and 70,000 (tile byte 255: the binary search)
    {5: 254}, {6: 255}, {7: 256}, {8: 70_000},
    # escapes and in-place counts: 254, 255, 256
    {0: 252, 9: 2}, {0: 252, 9: 2, 10: 1}, {0: 252, 9: 2, 10: 2},
    {15: 253, 0: 1}, {15: 254, 0: 1}, {15: 254, 0: 2}, {0: 254, 15: 2},
    {2: 255, 3: 1}, {2: 70_000, 3: 2, 4: 3}, {1: 255, 2: 5}, {1: 5, 2: 255, 3: 5},
    # the smallest escape, in field 0 and in field 15
    {0: 3}, {15: 3, 14: 2}, dict.fromkeys(E16, 3), {0: 4, 15: 4},
]
FIRST_CHUNK = 200  # positions 3201 ..: clear of the positions below
# escapes on the bounds: position 1, overflow block edges, strip 0's last and strip 1's first
EDGES = {1: 9, 1024: 5, 1025: 6, 2048: 7, 2049: 300, 16_384: 8, 16_385: 10}
# several entries >= 255 in one overflow block (positions 8193 .. 9216)
SEARCH = {8_200: 300, 8_201: 301, 8_217: 302, 8_700: 303, 9_215: 304, 9_216: 255}


def saturation_counts(length):
    d = dict(EDGES)
    d.update(SEARCH)
    d[length] = 11
    for i, spec in enumerate(CHUNKS):
        for f, c in spec.items():
            d[16 * (FIRST_CHUNK + 2 * i) + 1 + f] = c
    return d


def fill_saturation(g, m, u, S, rng):
    d = saturation_counts(m.length)
    pos = np.array(sorted(d), np.uint32)
    put(g, m, u, 0, 0, pos, [d[int(p)] for p in pos])
    if S > 1:  # a second sample: +1 on field 0 of every chunk above, a few tags elsewhere
        p1 = np.union1d(16 * (FIRST_CHUNK + 2 * np.arange(len(CHUNKS))) + 1,
                        rng.integers(20_000, m.length, 40)).astype(np.uint32)
        put(g, m, u, 0, 1, p1, np.where(p1 < 20_000, 1, rng.integers(1, 5, len(p1))))


def chunk_pos(i, f):
    return 16 * (FIRST_CHUNK + 2 * i) + 1 + f


@pytest.mark.parametrize("S", [1, 2])
def test_saturation_and_escapes(gpu_lib, S):
    length = 2 * 16_384 + 100
    rng = np.random.default_rng(40 + S)
    with open_ctx(gpu_lib, 50, S) as g:
        u = g.add_unit(length)
        m = UnitModel(length, 1, S)
        fill_saturation(g, m, u, S, rng)
        lay = check(gpu_lib, g, u, m, pooled=S > 1, pct=S > 1)
        csum = g.index_read(u, gpu_lib.IDX_CSUM)
        want = [min(255, sum(spec.values())) for spec in CHUNKS]
        got = [int(csum[lay.pad_pos // 16 + FIRST_CHUNK + 2 * i]) for i in range(len(CHUNKS))]
        assert got == want  # (the reference's bytes are the ones meant)
        assert {254, 255, 32, 3}.issubset(want)
        # counts dropped back from an escape to 2 and to 0, raised into one, the bounds cleared
        upd = {chunk_pos(14, 5): 2, chunk_pos(15, 6): 0, chunk_pos(17, 8): 1, 1: 2, length: 0,
               chunk_pos(0, 3): 400, chunk_pos(1, 0): 3, 16_384: 0, 16_385: 2, 8_217: 0, 2_048: 255}
        pos = np.array(sorted(upd), np.uint32)
        put(g, m, u, 0, 0, pos, [upd[int(p)] for p in pos])
        check(gpu_lib, g, u, m, pooled=S > 1, pct=S > 1)
        assert g.index_state() == (True, 2)


def test_regrown_unit_keeps_zero_padding(gpu_lib):
    """bw 50 -> 700 regrows the unit (regrow_unit: a longer stride): the arrays follow the
    new stride and every byte outside the counts is zero"""
    length, S = 31_668, 2
    rng = np.random.default_rng(43)
    with open_ctx(gpu_lib, 50, S) as g:
        u = g.add_unit(length)
        m = UnitModel(length, 1, S)
        fill_saturation(g, m, u, S, rng)
        a = check(gpu_lib, g, u, m, pooled=True, pct=True)
        g.set_params(700, S, BG)
        b = check(gpu_lib, g, u, m, pooled=True, pct=True)
        assert (a.stride, b.stride) == (unit_stride(length, 50), unit_stride(length, 700))
        assert b.stride > a.stride
        put(g, m, u, 0, 1, [length, 7], [2, 90])
        check(gpu_lib, g, u, m, pooled=True, pct=True)


# ---- pooling ------------------------------------------------------------------------

COEFFS = [0.37, 1.91, 4094.2]  # screen weights 2, 3, 4096


def pooling_unit(g, m, u, rng):
    length = m.length
    d = {(st, s): {} for st in range(2) for s in range(4)}
    for key in d:  # background on every track
        for p in rng.integers(1, 14_000, 150).tolist():
            d[key][p] = int(rng.choice([1, 1, 2, 3, 5]))
    # samples 0 and 3 (each the control sample of some settings) carry large counts in
    # chunks of their own, beside small counts of the others
    for k, s in enumerate((0, 3)):
        for i in range(6):
            p = 14_001 + 16 * (12 * k + 2 * i)
            d[(i % 2, s)][p + 3] = 5_000 + i
            d[(i % 2, s)][p + 4] = 2
            d[((i + 1) % 2, 1)][p + 5] = 1
            d[(i % 2, 2)][p + 9] = 3
    # chunks where x + y (no coefficients) and 2x + 3y (COEFFS) are exactly 254, 255, 256;
    # x on the forward strand, y on the reverse strand, for the samples weighted (2, 3)
    # under either control sample: (1, 2) with sample 0 as control, (0, 1) with sample 3
    k = 16_001
    for a, b in ((1, 2), (0, 1)):
        for x, y in ((127, 127), (127, 128), (128, 128), (100, 18), (99, 19), (98, 20)):
            d[(0, a)][k + 2] = x
            d[(1, b)][k + 13] = y
            k += 32
    # a chunk byte of 1 under the weight 4096: samples 3 and 2 alone in a chunk
    d[(1, 3)][k + 7] = 1
    d[(0, 2)][k + 32 + 7] = 1
    d[(1, 0)][length] = 4
    for (st, s), t in d.items():
        pos = np.array(sorted(t), np.uint32)
        put(g, m, u, st, s, pos, [t[int(p)] for p in pos])


def test_pooling_follows_control_set_and_coefficients(gpu_lib):
    length, S, bw = 20_000, 4, 50
    settings = [dict(control=[1, 0, 0, 0]), dict(control=[0, 0, 0, 1]),
                dict(control=[1, 0, 0, 0], coeffs=COEFFS), dict(control=[0, 0, 0, 1], coeffs=COEFFS),
                dict(control=[0, 0, 0, 0]), dict(control=[0, 0, 0, 1], coeffs=[1.0, 0.0, 2.5])]
    rng = np.random.default_rng(44)
    with open_ctx(gpu_lib, bw, S, nondir=True, **settings[0]) as g:
        u = g.add_unit(length)
        m = UnitModel(length, 2, S)
        pooling_unit(g, m, u, rng)
        for i, kw in enumerate(settings):
            g.set_params(bw, S, BG, nondir=True, **kw)
            # with coefficients the exact kernels pool in FP64 (POOL 2): no pooled count track
            check(gpu_lib, g, u, m, kw["control"], kw.get("coeffs"), pooled=True, pct="coeffs" not in kw)
            assert g.index_state() == (True, i + 1)
        pooled = g.index_read(u, gpu_lib.IDX_POOLED)
        assert 0 < np.count_nonzero(pooled % 255)


# ---- the pooled count track ---------------------------------------------------------

PCT_STACKS = [(30_000, [40] * 8),                              # 320
              (30_001, [31, 32, 32, 32, 32, 32, 32, 32]),      # 255
              (30_002, [30, 32, 32, 32, 32, 32, 32, 32]),      # 254
              (30_003, [32] * 8),                              # 256
              (30_004, [2, 2, 2, 2, 2, 2, 2, 2]),              # 16, no escape
              (30_005, [0, 0, 0, 0, 0, 0, 0, 255]),            # one sample alone at 255
              (30_006, [300, 0, 0, 0, 0, 0, 0, 0]),            # ... above it
              (30_007, [3, 0, 0, 0, 0, 0, 0, 250]),            # 253 from two escapes
              (30_008, [2, 1, 0, 2, 1, 0, 2, 246]),            # 254 from one escape and fields
              (16_384, [1, 2, 3, 4, 5, 6, 7, 8]), (16_385, [8, 7, 6, 5, 4, 3, 2, 1])]
POOL1_MAX = (1 << 32) // 8 - 1  # 8 pooled samples: the largest count with count * 8 < 2^32 (pool_mode)


def test_pooled_count_track_and_its_bound(gpu_lib, oracle):
    length, S, bw = 40_000, 9, 50
    control = [0, 0, 1, 0, 0, 0, 0, 0, 0]  # sample 2: large counts, not pooled
    nc = [s for s in range(S) if not control[s]]
    rng = np.random.default_rng(45)
    with open_ctx(gpu_lib, bw, S, control=control) as g:
        u = g.add_unit(length)
        m = UnitModel(length, 1, S)
        for k, s in enumerate(nc):
            pos = np.unique(np.concatenate([rng.integers(200, 29_000, 120),
                                            [p for p, c in PCT_STACKS if c[k]]])).astype(np.uint32)
            cnt = rng.integers(1, 4, len(pos))
            for p, c in PCT_STACKS:
                cnt[pos == p] = c[k]
            put(g, m, u, 0, s, pos, cnt)
        pos = np.unique(np.concatenate([rng.integers(200, length, 60), np.arange(30_000, 30_009)])).astype(np.uint32)
        put(g, m, u, 0, 2, pos, np.full(len(pos), 1_000))
        check(gpu_lib, g, u, m, control, pooled=True, pct=True)
        pct = g.index_read(u, gpu_lib.IDX_PCT)
        assert pct[1024 + 30_000 - 1:1024 + 30_009 - 1].tolist() == [255, 255, 254, 255, 16, 255, 255, 253, 254]
        # just under the bound of POOL 1: the pooled count track stays
        put(g, m, u, 0, 5, [35_000], [POOL1_MAX])
        check(gpu_lib, g, u, m, control, pooled=True, pct=True)
        # just over it: the exact kernels pool in FP64, the context holds no pooled count track
        put(g, m, u, 0, 5, [35_000], [POOL1_MAX + 1])
        check(gpu_lib, g, u, m, control, pooled=True, pct=False)
        n = g.run()
        regs, k = g.regions(n)
        regs, k = regs.copy(), k.copy()
    sp = m.sparse()
    allp = np.unique(np.concatenate([sp[(0, s)][0] for s in range(S)]))
    cnt = np.zeros((len(allp), S), np.uint32)
    for s in range(S):
        cnt[np.searchsorted(allp, sp[(0, s)][0]), s] = sp[(0, s)][1]
    ref, ref_sums = oracle.run_unit(bw, BG, allp.astype(np.uint32), cnt, control=control)
    compare(ref, ref_sums, regs, k)
    assert any(r["left"] <= 35_000 <= r["right"] for r in ref)


# ---- many units in one build --------------------------------------------------------

LENGTHS = [1, 15, 16, 17, 1023, 1024, 1025, 16_383, 16_384, 16_385, 40_000]


def random_track(rng, length):
    n = min(length, 30)
    pos = np.unique(np.concatenate([rng.integers(1, length + 1, n), [1, length]])).astype(np.uint32)
    return pos, rng.choice([1, 1, 2, 2, 3, 7, 255, 300], len(pos)).astype(np.uint32)


@pytest.mark.parametrize("nondir", [False, True])
def test_many_units_in_one_build(gpu_lib, nondir):
    """the launches' list_entry: every unit of a 70-unit build, then a rebuild of three"""
    S, nst = 2, 2 if nondir else 1
    rng = np.random.default_rng(46 + nondir)
    lens = [LENGTHS[i % len(LENGTHS)] for i in rng.permutation(70)]
    with open_ctx(gpu_lib, 50, S, nondir=nondir) as g:
        units = []
        for length in lens:
            u, m = g.add_unit(length), UnitModel(length, nst, S)
            for st in range(nst):
                for s in range(S):
                    put(g, m, u, st, s, *random_track(rng, length))
            units.append((u, m))
        for u, m in units:
            check(gpu_lib, g, u, m, pooled=True, pct=True)
        assert g.index_state() == (True, 1)  # one build (one launch per kind) served them all
        # three stale units among them; one track cleared by zero counts
        for i in (0, 33, 69):
            u, m = units[i]
            put(g, m, u, nst - 1, 1, *random_track(rng, m.length))
        u, m = units[33]
        old = np.array(sorted(m.t[(0, 0)]), np.uint32)
        put(g, m, u, 0, 0, old, np.zeros(len(old), np.uint32))
        assert not m.t[(0, 0)]
        for u, m in units:
            check(gpu_lib, g, u, m, pooled=True, pct=True)
        assert g.index_state() == (True, 2)


# ---- more items than the launch has threads -----------------------------------------

def sparse_tracks(g, m, u, rng, n):
    for st in range(m.nstrands):
        for s in range(m.S):
            pos = np.unique(np.concatenate([rng.integers(1, m.length + 1, n // (m.nstrands * m.S)),
                                            np.arange(m.length - 999, m.length + 1, 37), [1]])).astype(np.uint32)
            put(g, m, u, st, s, pos, rng.choice([1, 2, 3, 9, 260], len(pos)))


def grid_stride_units(g, rng, nst, S, long_len):
    """one small unit, the long one, then small units of mixed lengths: a launch over them
    has about 1.5 times the items it has threads, so a third of the threads take a second
    item, and that item lies in the long unit's last third (the tags are spread over all
    of it) or in one of the units behind it -- list_entry's advance then steps from the
    first item's entry over one or several entry bounds"""
    units = []
    for length in [17, long_len, 1, 16_385, 40_000, 15, 1024]:
        u, m = g.add_unit(length), UnitModel(length, nst, S)
        if length == long_len:
            sparse_tracks(g, m, u, rng, 24_000)
        else:
            for st in range(nst):
                for s in range(S):
                    put(g, m, u, st, s, *random_track(rng, length))
        units.append((u, m))
    return units


def test_grid_stride_csum_and_pct(gpu_lib):
    """chunk-sum and pooled-count-track builds with more items than the launch has threads,
    over several units: the kernels' grid-stride branch and list_entry's advance"""
    S = 4
    rng = np.random.default_rng(48)
    with open_ctx(gpu_lib, 50, S, nondir=True) as g:
        units = grid_stride_units(g, rng, 2, S, 25_000_000)
        lays = [check(gpu_lib, g, u, m, pooled=True, pct=True) for u, m in units]
        assert g.index_state() == (True, 1)
        first = lays[0].stride + lays[1].stride  # up to the long unit's end: the rest is second items
        assert GRID_CAP < first // 16 * 2 * S < 2 * GRID_CAP  # csum_units_kernel's items
        assert GRID_CAP < first // 4 * 2 < 2 * GRID_CAP       # pct_units_kernel's items
        assert first // 16 * 2 * S > GRID_CAP * 4 // 3


def test_grid_stride_pooled_plane(gpu_lib):
    """the same for pool_units_kernel (one item per 16 bytes of a track)"""
    rng = np.random.default_rng(49)
    with open_ctx(gpu_lib, 50, 1, nondir=True) as g:
        units = grid_stride_units(g, rng, 2, 1, 200_000_000)
        lays = [check(gpu_lib, g, u, m, pooled=True, pct=False) for u, m in units]
        assert g.index_state() == (True, 1)
        first = lays[0].stride + lays[1].stride
        assert GRID_CAP * 4 // 3 < first // 16 < 2 * GRID_CAP


# ---- last_add -----------------------------------------------------------------------

def test_last_add(gpu_lib):
    length, S = 40_000, 2
    control = [0, 1]
    cases = {  # name: [(strand, sample, pos, count)]
        "control_only": [(0, 0, 30_000, 1), (0, 1, 39_000, 5), (1, 1, 39_500, 400)],
        "reverse_only": [(0, 0, 100, 2), (1, 0, 31_111, 1)],
        "escape": [(0, 0, 200, 1), (0, 0, 33_333, 500), (1, 0, 33_000, 2)],
        "strip_last": [(0, 0, 5, 1), (1, 0, 16_384, 1)],
        "strip_first": [(0, 0, 16_384, 2), (0, 0, 16_385, 1)],
        "second_strip_last": [(1, 0, 32_768, 3), (0, 0, 32_767, 1)],
        "contig_end": [(0, 0, length, 1)],
        "none": [(0, 1, 77, 3)],
    }
    with open_ctx(gpu_lib, 50, S, nondir=True, control=control) as g:
        units = {}
        for name, tags in cases.items():
            u, m = g.add_unit(length), UnitModel(length, 2, S)
            for st, s, p, c in tags:
                put(g, m, u, st, s, [p], [c])
            units[name] = (u, m)
        want = {"control_only": 30_000, "reverse_only": 31_111, "escape": 33_333, "strip_last": 16_384,
                "strip_first": 16_385, "second_strip_last": 32_768, "contig_end": length, "none": 0}
        for name, (u, m) in units.items():
            check(gpu_lib, g, u, m, control, pooled=True, pct=False)
            assert g.last_add(u) == want[name], name
        # the last tag cleared by a zero count: the one before it, also an escape's
        for name, st, p, then in (("escape", 0, 33_333, 33_000), ("strip_first", 0, 16_385, 16_384),
                                  ("reverse_only", 1, 31_111, 100), ("contig_end", 0, length, 0)):
            u, m = units[name]
            put(g, m, u, st, 0, [p], [0])
            check(gpu_lib, g, u, m, control, pooled=True, pct=False)
            assert g.last_add(u) == then, name


# ---- the accessor's own checks ------------------------------------------------------

def test_index_read_argument_and_state_checks(gpu_lib):
    import ctypes
    L = gpu_lib.load_library()
    E_ARG = gpu_lib.UP_E_ARG
    with open_ctx(gpu_lib, 50, 2, policy=gpu_lib.INDEX_AUTO) as g:
        u = g.add_unit(5_000)
        g.scatter(u, 0, 0, np.array([10, 4_000], np.uint32), np.array([1, 9], np.uint32))
        buf = np.zeros(1 << 16, np.uint8)
        n = ctypes.c_uint64(0)
        lay = gpu_lib.UnitLayout()

        def read(unit, what, cap=buf.size, dst=buf.ctypes.data):
            return L.up_unit_index_read(g.ctx, unit, what, dst, cap, ctypes.byref(n))
        # UP_INDEX_AUTO: the first pass runs without the index, so there is none to read
        assert read(u, gpu_lib.IDX_TRACKS) == gpu_lib.UP_E_STATE
        assert g.unit_layout(u).index_on == 0 and g.index_state() == (False, 0)
        g.run()
        assert read(u, gpu_lib.IDX_TRACKS) == gpu_lib.UP_OK and g.index_state() == (True, 1)
        stride = g.unit_layout(u).stride
        assert n.value == 2 * stride
        for what, size in ((gpu_lib.IDX_CSUM, 2 * stride // 4), (gpu_lib.IDX_POOLED, stride // 4),
                           (gpu_lib.IDX_PCT, 4 * stride)):
            assert read(u, what, cap=size - 1) == E_ARG and n.value == size
            assert read(u, what, cap=size) == gpu_lib.UP_OK
        assert g.index_state() == (True, 1)  # reads of a current index build nothing
        assert read(u + 1, gpu_lib.IDX_TRACKS) == E_ARG
        assert read(u, -1) == E_ARG and read(u, 4) == E_ARG
        assert read(u, gpu_lib.IDX_TRACKS, dst=None) == E_ARG
        assert L.up_unit_layout(g.ctx, u + 1, ctypes.byref(lay)) == E_ARG
        assert L.up_unit_layout(g.ctx, u, None) == E_ARG
        assert L.up_unit_layout(None, u, ctypes.byref(lay)) == E_ARG
        assert L.up_unit_index_read(None, u, 0, buf.ctypes.data, buf.size, None) == E_ARG
        g.set_index_policy(gpu_lib.INDEX_NEVER)
        assert read(u, gpu_lib.IDX_CSUM) == gpu_lib.UP_E_STATE
        with pytest.raises(gpu_lib.UpError):
            g.index_read(u, gpu_lib.IDX_CSUM)
    with gpu_lib.Lib(0) as g:  # no parameters, no units
        assert L.up_unit_layout(g.ctx, 0, ctypes.byref(lay)) == E_ARG
