"""Inputs of the head-place tests (up_set_head_place: quirk-Q1 head units
replayed and merged on the device, inside the pass) and their oracle lists.

A case is a dict: the parameters and a list of units (length, buffer,
ascending positions, forward counts [n][S], reverse counts or None).  Every
case has head tags (pooled tags at positions <= bw) and tags just past bw, so
that the exact replay emits records, resyncs inside the unit and replaces
records of the parallel scan.  `headless(case)` is the same case without the
tags at positions <= bw: the list the parallel scan alone would stand for.

test_head_place_oracle.py shows on the CPU that every case exercises the
merge; test_gpu_head_place.py runs them with the mode off and on.
"""
import ctypes
import functools

import numpy as np

from tests.gen import random_unit

BG = 0.003


def _dense_unit(rng, length, bw, S, head_tags, near, clusters):
    """one strand: random background and clusters (gen.random_unit, from
    position 1), `head_tags` tags of count 5..39 at positions <= bw and, with
    `near`, a cluster of 80 tags around `near` (sd bw / 2)"""
    pos, cnt = random_unit(rng, length, bw, S=S, lo=1, n_clusters=clusters)
    dense = {int(p): c.astype(np.int64) for p, c in zip(pos, cnt)}
    for p in rng.integers(1, bw + 1, head_tags):
        v = dense.setdefault(int(p), np.zeros(S, np.int64))
        v[int(rng.integers(0, S))] += int(rng.integers(5, 40))
    if near:
        for o in np.rint(rng.normal(near, bw / 2, 80)).astype(int):
            if 1 <= o <= length:
                v = dense.setdefault(int(o), np.zeros(S, np.int64))
                v[int(rng.integers(0, S))] += 1
    p = np.array(sorted(dense), np.uint32)
    c = np.array([dense[int(x)] for x in p], np.uint32).reshape(len(p), S)
    return p, c


def _case(name, bw, units, *, S=1, thr=5.0, nondir=False, control=None, coeffs=None, corr_thr=-1.0,
          want_corr=False, hit_thr=10.0):
    return dict(name=name, bw=bw, bg=BG, S=S, thr=thr, nondir=nondir, control=control, coeffs=coeffs,
                corr_thr=corr_thr, want_corr=want_corr, kurt_thr=0.0, hit_thr=hit_thr, units=units)


def _unit(length, pos, cf, cr=None, buffer=0):
    return dict(length=int(length), buffer=buffer, pos=np.asarray(pos, np.uint32),
                cf=np.asarray(cf, np.uint32), cr=None if cr is None else np.asarray(cr, np.uint32))


def _both_strands(pf, cf, pr, cr, S):
    allp = np.union1d(pf, pr).astype(np.uint32)
    f = np.zeros((allp.size, S), np.uint32)
    r = np.zeros((allp.size, S), np.uint32)
    f[np.searchsorted(allp, pf)] = cf
    r[np.searchsorted(allp, pr)] = cr
    return allp, f, r


@functools.lru_cache(maxsize=None)
def directional(bw, seed):
    """S = 1, thresholds 5 (seeds 0, 1) and 25 (seeds 2, 3); odd seeds put the
    cluster around bw, so that a region is open across the resync horizon,
    even seeds at 3 bw (its region starts before the resync position)"""
    rng = np.random.default_rng(7000 + 10 * bw + seed)
    length = int(rng.integers(3_000, 60_000))
    near = bw if seed % 2 else 3 * bw
    pos, cnt = _dense_unit(rng, length, bw, 1, int(rng.integers(1, 6)), near, int(rng.integers(1, 6)))
    return _case(f"dir-bw{bw}-s{seed}", bw, [_unit(length, pos, cnt)], thr=(5.0, 25.0)[(seed // 2) % 2])


DIRECTIONAL = [(bw, seed) for bw in (13, 50, 120) for seed in range(4)]


def _nondir_unit(rng, length, bw, S=1):
    pf, cf = _dense_unit(rng, length, bw, S, 3, 2 * bw, 4)
    pr, cr = _dense_unit(rng, length, bw, S, 1, 2 * bw + 7, 4)
    return _both_strands(pf, cf, pr, cr, S)


@functools.lru_cache(maxsize=None)
def nondirectional():
    rng = np.random.default_rng(7100)
    length, bw = 20_000, 50
    p, f, r = _nondir_unit(rng, length, bw)
    return _case("nondir-bw50", bw, [_unit(length, p, f, r)], nondir=True, corr_thr=0.1, want_corr=True)


@functools.lru_cache(maxsize=None)
def chains():
    """one context, two buffers, seven units (every record accepted: the
    oracle's chain reports accepted regions only)"""
    rng = np.random.default_rng(7200)
    bw = 50
    units = []
    # buffer 0: no heads
    p, c = random_unit(rng, 12_000, bw, lo=2 * bw + 2, n_clusters=3)
    units.append(_unit(12_000, p, c))
    # a head unit that resyncs mid-unit
    p, c = _dense_unit(rng, 15_000, bw, 1, 3, 2 * bw, 3)
    units.append(_unit(15_000, p, c))
    # every add at <= bw: replayed to its end, its state leaks on
    p = np.array([7, 19, 23, 41, 50], np.uint32)
    units.append(_unit(9_000, p, np.array([[9], [14], [30], [11], [6]], np.uint32)))
    # the next unit: starts with the leaked window, then tags of its own
    p, c = random_unit(rng, 10_000, bw, lo=20, n_clusters=3)
    units.append(_unit(10_000, p, c))
    # no tags at all
    units.append(_unit(5_000, np.zeros(0, np.uint32), np.zeros((0, 1), np.uint32)))
    # buffer 1: a head unit, then a clean one
    p, c = _dense_unit(rng, 11_000, bw, 1, 4, bw, 2)
    units.append(_unit(11_000, p, c, buffer=1))
    p, c = random_unit(rng, 8_000, bw, lo=2 * bw + 2, n_clusters=2)
    units.append(_unit(8_000, p, c, buffer=1))
    return _case("chains-7", bw, units, hit_thr=0.0)


@functools.lru_cache(maxsize=None)
def three_samples():
    """S = 3, one control, -z coefficients (quirk Q5)"""
    rng = np.random.default_rng(7300)
    length, bw = 20_000, 50
    p, c = _dense_unit(rng, length, bw, 3, 4, 2 * bw, 4)
    return _case("s3-ctl-z", bw, [_unit(length, p, c)], S=3, control=[0, 1, 0], coeffs=[0.37, 1.91])


@functools.lru_cache(maxsize=None)
def wide(nondir):
    """K1w: bw 600, length 40,000"""
    rng = np.random.default_rng(7400 + int(nondir))
    length, bw = 40_000, 600
    if nondir:
        p, f, r = _nondir_unit(rng, length, bw)
        return _case("wide-nd-bw600", bw, [_unit(length, p, f, r)], nondir=True, corr_thr=0.1, want_corr=True)
    p, c = _dense_unit(rng, length, bw, 1, 4, 2 * bw, 5)
    return _case("wide-dir-bw600", bw, [_unit(length, p, c)])


@functools.lru_cache(maxsize=None)
def long_region():
    """one head unit whose first region (300,000 positions) is longer than the
    in-pass open-region capacity (262,144): a tag of count 5 every 20 positions
    from position 1"""
    length, bw = 400_000, 50
    p = np.arange(1, 300_000, 20, dtype=np.uint32)
    tail = np.array([350_000, 350_010, 350_020], np.uint32)
    pos = np.concatenate([p, tail])
    cnt = np.full((pos.size, 1), 5, np.uint32)
    return _case("long-region", bw, [_unit(length, pos, cnt)])


@functools.lru_cache(maxsize=None)
def no_heads():
    rng = np.random.default_rng(7500)
    length, bw = 30_000, 50
    p, c = random_unit(rng, length, bw, n_clusters=5)
    return _case("no-heads", bw, [_unit(length, p, c)])


def merge_cases():
    """every case whose merge drops and adds records"""
    return ([directional(bw, s) for bw, s in DIRECTIONAL] +
            [nondirectional(), chains(), three_samples(), wide(False), wide(True)])


def headless(case):
    """the same case without the tags at positions <= bw"""
    units = []
    for u in case["units"]:
        m = u["pos"] > case["bw"]
        units.append(dict(u, pos=u["pos"][m], cf=u["cf"][m], cr=None if u["cr"] is None else u["cr"][m]))
    return dict(case, name=case["name"] + "-headless", units=units)


# ---- the oracle's lists --------------------------------------------------

REF_DTYPE = np.dtype([("unit", "<u4"), ("left", "<u4"), ("right", "<u4"), ("peak", "<u4"), ("sum", "<u4"),
                      ("accepted", "<i4"), ("peak_score", "<f8"), ("kurtosis", "<f8"), ("corr", "<f8")])


def _chain_api(L):
    c, vp = ctypes, ctypes.c_void_p
    if getattr(L, "_head_place_api", False):
        return
    L.orc_buf_new.restype = vp
    L.orc_buf_new.argtypes = [vp, c.c_uint32, c.c_double, c.c_double, c.c_double, c.c_double, c.c_int,
                              c.c_uint16, vp, vp, c.c_uint32, vp, vp, vp, vp]
    L.orc_buf_free.restype = None
    L.orc_buf_free.argtypes = [vp]
    L.orc_buf_add.restype = None
    L.orc_buf_add.argtypes = [vp, vp, c.c_uint32, c.c_uint32, c.c_int]
    L.orc_buf_flush.restype = c.c_uint64
    L.orc_buf_flush.argtypes = [vp]
    for name, res in (("orc_region_contig", c.c_uint32), ("orc_region_left", c.c_uint32),
                      ("orc_region_npos", c.c_uint32), ("orc_region_peak", c.c_uint32),
                      ("orc_region_sum", c.c_uint32), ("orc_region_peak_score", c.c_double),
                      ("orc_region_kurtosis", c.c_double)):
        getattr(L, name).restype = res
        getattr(L, name).argtypes = [vp]
    L.orc_region_corr.restype = c.c_double
    L.orc_region_corr.argtypes = [vp, c.c_uint16]
    L.orc_region_expt_sums.restype = None
    L.orc_region_expt_sums.argtypes = [vp, vp]
    L.orc_region_free.restype = None
    L.orc_region_free.argtypes = [vp]
    L._head_place_api = True


_REGION_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_void_p)


def _oracle_chain(oracle, case):
    """the buffers as chains (orc_buf_*): each buffer's units in order, the
    contig switch flushing the previous unit (contig = unit + 1).  The sink
    sees accepted regions only, so chain cases accept every candidate."""
    assert case["kurt_thr"] == 0.0 and case["hit_thr"] == 0.0 and case["corr_thr"] <= -1.0
    L = oracle.L
    _chain_api(L)
    S = case["S"]
    k = oracle.kernel(case["bw"], 1.0 / case["bg"])
    ctl = np.zeros(S, np.uint8) if case["control"] is None else np.asarray(case["control"], np.uint8)
    rows = []

    def sink(_user, reg):
        sums = np.zeros(S, np.uint32)
        L.orc_region_expt_sums(reg, sums.ctypes.data)
        left, n = L.orc_region_left(reg), L.orc_region_npos(reg)
        rows.append(((L.orc_region_contig(reg) - 1, left, left + n - 1, L.orc_region_peak(reg),
                      L.orc_region_sum(reg), 1, L.orc_region_peak_score(reg), L.orc_region_kurtosis(reg),
                      L.orc_region_corr(reg, 0)), sums))
        L.orc_region_free(reg)

    cb = _REGION_CB(sink)
    for b in (0, 1):
        buf = L.orc_buf_new(k.ctypes.data, k.size, case["thr"], 0.0, -1.0, 0.0, int(b == 0), S, ctl.ctypes.data,
                            None, 0, ctypes.cast(cb, ctypes.c_void_p), None, None, None)
        for ui, u in enumerate(case["units"]):
            if u["buffer"] != b:
                continue
            cnt = np.ascontiguousarray(u["cf"], np.uint32)
            for i, p in enumerate(u["pos"]):
                L.orc_buf_add(buf, cnt[i].ctypes.data, ui + 1, int(p), int(b == 0))
        L.orc_buf_flush(buf)
        L.orc_buf_free(buf)
    order = sorted(range(len(rows)), key=lambda i: rows[i][0][0])  # unit-major, emission order kept
    ref = np.array([rows[i][0] for i in order], REF_DTYPE)
    sums = np.array([rows[i][1] for i in order], np.uint32).reshape(len(order), S)
    return ref, sums


_REF = {}


def oracle_list(oracle, case):
    """(records, exptSums) of the case, unit-major; computed once per case"""
    if case["name"] in _REF:
        return _REF[case["name"]]
    if len(case["units"]) > 1:
        out = _oracle_chain(oracle, case)
    else:
        u = case["units"][0]
        r, sums = oracle.run_unit(case["bw"], case["bg"], u["pos"], u["cf"], u["cr"], region_thr=case["thr"],
                                  kurt_thr=case["kurt_thr"], corr_thr=case["corr_thr"], hit_thr=case["hit_thr"],
                                  buffer_forward=u["buffer"] == 0, nondir=case["nondir"],
                                  control=case["control"], coeffs=case["coeffs"])
        ref = np.zeros(len(r), REF_DTYPE)
        for f in ("left", "right", "peak", "sum", "accepted", "peak_score", "kurtosis", "corr"):
            ref[f] = r[f]
        out = (ref, sums)
    for a in out:
        a.setflags(write=False)
    _REF[case["name"]] = out
    return out


def keys(recs):
    """one hashable key per record: what identifies a region and its peak"""
    return [(int(r["unit"]), int(r["left"]), int(r["right"]), int(r["peak"]), int(r["sum"]),
             r["peak_score"].tobytes()) for r in recs]
