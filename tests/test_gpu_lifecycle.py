"""Lifetime of what a context owns (csrc/devmem.h): the unit buffers, the
per-pass buffers, events, streams and cached graphs free themselves, so the
hazards are a moved-from owner that frees live memory and a destructor that
runs too early.  Units that survive the growth of the unit vector, a regrown
unit that keeps its tracks, reset and reuse, two contexts closed in crossed
order, a close after the index and the escape tables were built, and a close
with graphs cached and a record target set -- every record against the oracle
(or, where stated, a fresh context).  One directional sample, bw 50, units of
20,000 bp."""
import numpy as np
import pytest

from tests.gen import random_unit
from tests.test_gpu_pipeline import _parse, _target
from tests.test_gpu_replay import compare

pytestmark = pytest.mark.gpu

BW, BG, LEN = 50, 0.003, 20_000
WIDE = 600  # the margins the inputs keep clear of tags: test_regrow_unit_keeps_data rescans them up to this bw
NUNITS = 12


def _escaped(pos, cnt):
    """the same unit with one count far above any escape value (3 or 15)"""
    cnt = cnt.copy()
    cnt[len(pos) // 2, 0] = 40
    return pos, cnt


@pytest.fixture(scope="module")
def units():
    """[(pos, counts)] of NUNITS units; unit 0 holds an escaped count"""
    rng = np.random.default_rng(2024)
    out = [random_unit(rng, LEN, WIDE, n_clusters=6) for _ in range(NUNITS)]
    out[0] = _escaped(*out[0])
    return out


@pytest.fixture(scope="module")
def refs(oracle, units):
    """the oracle's (records, counts) of every unit at bw 50"""
    return [oracle.run_unit(BW, BG, pos, cnt) for pos, cnt in units]


def _add(g, pos, cnt):
    u = g.add_unit(LEN)
    g.scatter(u, 0, 0, pos, cnt[:, 0])
    return u


def _check_units(regs, gcnt, refs):
    """records of unit k of the context against refs[k]"""
    assert len(regs) == sum(len(r) for r, _ in refs)
    for u, (ref, ref_sums) in enumerate(refs):
        m = regs["unit"] == u
        compare(ref, ref_sums, regs[m], gcnt[m])


def test_units_survive_vector_growth(gpu_lib, units, refs):
    with gpu_lib.Lib(0) as g:
        g.set_params(BW, 1, BG)
        _add(g, *units[0])
        total = g.tag_total(0, 0, 0)
        assert total == int(units[0][1].sum())
        assert g.run() == len(refs[0][0])  # (the escape tables of unit 0 exist from here on)
        for k in range(1, 9):  # one at a time: the unit vector reallocates several times
            _add(g, *units[k])
        n = g.run()
        regs, gcnt = g.regions(n)
        assert sum(len(r) for r, _ in refs[:9]) > 9
        _check_units(regs, gcnt, refs[:9])
        assert g.tag_total(0, 0, 0) == total


@pytest.mark.parametrize("bw", [511, WIDE])
def test_regrow_unit_keeps_data(gpu_lib, oracle, units, refs, bw):
    """tracks written at bw 50, then a wider bandwidth: 511, the widest the
    first padding still covers, and 600, past it, which copies every unit's
    tracks into a larger allocation (regrow_unit)"""
    with gpu_lib.Lib(0) as g:
        g.set_params(BW, 1, BG)
        for k in range(3):
            _add(g, *units[k])
        n = g.run()
        _check_units(*g.regions(n), refs[:3])
        g.set_params(bw, 1, BG)
        n = g.run()
        regs, gcnt = g.regions(n)
        wide = [oracle.run_unit(bw, BG, pos, cnt) for pos, cnt in units[:3]]
        assert sum(len(r) for r, _ in wide) > 0
        _check_units(regs, gcnt, wide)
        assert g.tag_total(0, 0, 0) == int(units[0][1].sum())


def test_reset_and_reuse(gpu_lib, units, refs):
    capi = gpu_lib
    with capi.Lib(0) as fresh:
        fresh.set_params(BW, 1, BG)
        for k in (9, 10, 11):
            _add(fresh, *units[k])
        n = fresh.run()
        want, want_cnt = fresh.regions(n)
    with capi.Lib(0) as g:
        g.set_params(BW, 1, BG)
        for k in range(4):
            _add(g, *units[k])
        n = g.run()
        _check_units(*g.regions(n), refs[:4])
        g.reset_units()
        for k in (9, 10, 11):
            _add(g, *units[k])
        n = g.run()
        regs, gcnt = g.regions(n)
    assert len(want) > 0
    assert regs.tobytes() == want.tobytes()
    assert np.array_equal(gcnt, want_cnt)
    _check_units(regs, gcnt, refs[9:12])


def test_two_contexts_crossed_close(gpu_lib, units, refs):
    capi = gpu_lib
    a, b = capi.Lib(0), capi.Lib(0)
    try:
        for g, ks in ((a, (0, 1, 2)), (b, (3, 4))):
            g.set_params(BW, 1, BG)
            for k in ks:
                _add(g, *units[k])
        na = a.run()
        nb = b.run()
        _check_units(*a.regions(na), refs[0:3])
        before, before_cnt = b.regions(nb)
        _check_units(before, before_cnt, refs[3:5])
        a.close()
        assert b.run() == nb
        after, after_cnt = b.regions(nb)
        assert after.tobytes() == before.tobytes()
        assert np.array_equal(after_cnt, before_cnt)
    finally:
        a.close()
        b.close()


def test_index_on_then_close(gpu_lib, units, refs):
    """the index lists and the escape bitmap are built, then freed by the
    close; a fresh context in the same process still runs right"""
    capi = gpu_lib
    with capi.Lib(0) as g:
        g.set_params(BW, 1, BG)
        g.set_index_policy(capi.INDEX_ALWAYS)
        for k in range(3):
            _add(g, *units[k])
        for _ in range(2):
            n = g.run()
            _check_units(*g.regions(n), refs[:3])
        assert g.index_state() == (True, 1)
    with capi.Lib(0) as g:
        g.set_params(BW, 1, BG)
        for k in range(3):
            _add(g, *units[k])
        n = g.run()
        _check_units(*g.regions(n), refs[:3])


def test_pipelined_targets_then_close(gpu_lib, monkeypatch, units, refs):
    """UP_MAX_IN_FLIGHT passes at a time into rotating record targets, nine
    per pass slot and then the first again: past the eight graphs a slot
    caches, so graphs are evicted and captured anew (passes go out as graphs
    when this thread launches them, UNIPEAK_LAUNCHER=0).  The context closes
    with the graphs cached, the targets registered and one still set."""
    capi = gpu_lib
    monkeypatch.setenv("UNIPEAK_LAUNCHER", "0")  # up_open reads it
    depth = capi.MAX_IN_FLIGHT
    with capi.Lib(0) as g:
        g.set_params(BW, 1, BG)
        for k in range(4):
            _add(g, *units[k])
        n = g.run()
        ref, rcnt = g.regions(n)
        _check_units(ref, rcnt, refs[:4])
        cap = n + 16
        bufs = [_target(cap, 1, capi.REGION_DTYPE.itemsize) for _ in range(9 * depth)]
        for b, off in bufs:
            g.host_register(b[off:].ctypes.data, len(b) - off)
        g.set_timing(1)  # (a pass timed phase by phase is not a graph)
        for rnd in range(10):
            mine = [bufs[(rnd * depth + i) % len(bufs)] for i in range(depth)]
            for b, off in mine:
                b[off:off + 8] = 0  # (the record count of the buffer's previous pass)
                g.set_record_target(b[off:].ctypes.data, cap)
                g.run_async()
            for b, off in mine:
                assert g.run_wait() == n
                recs, cnt = _parse(b, off, cap, 1, capi.REGION_DTYPE)
                assert recs.tobytes() == ref.tobytes(), rnd
                assert np.array_equal(cnt, rcnt), rnd
