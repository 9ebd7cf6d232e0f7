"""The route of a context (csrc/route.h) through the real entry points: which
scan the blocking up_run takes, and whether up_run_async and the dense profile
are admitted or refused with UP_E_UNSUPPORTED.  Default environment, 2-bit
tracks; tests/test_route.py holds the whole table on the CPU."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UP_E_UNSUPPORTED = -5  # (include/unipeak_hip.h)
K1, K1W, K1Q, REPLAY = 0, 1, 2, 3  # up_last_scan_kind


def expected(bw, thr, nondir, capture, wide_nd_full, wide_q11_nd):
    """(scan kind, up_run_async admitted, dense profile admitted)"""
    wide = bw > 511
    if thr > 0:
        if not wide:
            return K1, True, True
        if not nondir:
            return K1W, True, True
        if capture and not wide_nd_full:
            return REPLAY, False, False
        return K1W, wide_nd_full, wide_nd_full
    if wide and (capture or (nondir and not wide_q11_nd)):
        return REPLAY, False, False
    return K1Q, False, True


def admitted(capi, call):
    try:
        call()
        return True
    except capi.UpError as e:
        assert e.code == UP_E_UNSUPPORTED, e
        return False


@pytest.mark.parametrize("nondir", [False, True])
@pytest.mark.parametrize("thr", [25.0, 0.0])
@pytest.mark.parametrize("bw", [50, 600])
def test_route_through_the_entry_points(gpu_lib, bw, thr, nondir):
    capi = gpu_lib
    for capture, full, q11nd in itertools.product([False, True], repeat=3):
        row = (bw, thr, nondir, capture, full, q11nd)
        kind, async_ok, profile_ok = expected(*row)
        with capi.Lib(0) as g:
            g.set_params(bw, 1, 0.003, region_thr=thr, nondir=nondir)
            g.set_profile_capture(capture)
            g.set_wide_nd_full(full)
            g.set_wide_q11_nd(q11nd)
            # one tag past bw: no head unit, none of the data-dependent fallbacks
            u = g.add_unit(10_000)
            g.scatter(u, 0, 0, np.array([5000], np.uint32), np.array([3], np.uint32))
            assert g.run() >= 0
            assert g.last_scan_kind() == kind, row
            enqueued = admitted(capi, g.run_async)
            if enqueued:
                assert g.run_wait() >= 0
            assert enqueued == async_ok, row
            assert admitted(capi, lambda: g.profile_range(u, 1, 100)) == profile_ok, row
