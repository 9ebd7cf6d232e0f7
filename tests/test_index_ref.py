"""tests/index_ref.py (the vectorised reference the GPU byte tests compare with) against
a per-field pure-Python loop written from the sentences of csrc/kernels.h: no GPU."""
import numpy as np
import pytest

from tests.index_ref import UnitModel, index_arrays, screen_weights, unit_stride

PAD = 1024  # kPadPos of the 2-bit tracks


def loop_reference(model, stride, control, coeffs):
    S, nstrands = model.S, model.nstrands
    nc, w = screen_weights(control, coeffs)
    nfields = 4 * stride
    nd = stride // 4
    ntracks = nstrands * S
    trk = [0] * (ntracks * stride)
    csum = [0] * (ntracks * nd)
    pooled_sum = [0] * nd
    pct = [0] * (nstrands * nfields)
    last = 0
    for st in range(nstrands):
        for s in range(S):
            t = st * S + s
            dense = [0] * nfields
            for p, c in model.t[(st, s)].items():
                dense[PAD + p - 1] = c          # position p is field kPadPos + p - 1
                if s in nc and c:
                    last = max(last, p)
            for n in range(nfields):
                # bits 2 * (n % 4) .. + 1 of byte n / 4; a count >= 3 is stored as 3
                trk[t * stride + n // 4] |= min(dense[n], 3) << (2 * (n % 4))
            for j in range(nd):
                # byte j = the tag sum of fields 16j .. 16j + 15, saturated at 255
                csum[t * nd + j] = min(255, sum(dense[16 * j:16 * j + 16]))
                if s in nc:
                    pooled_sum[j] += w[nc.index(s)] * csum[t * nd + j]
            if s in nc:
                for n in range(nfields):
                    pct[st * nfields + n] += dense[n]
    u8 = lambda a: np.array([min(255, v) for v in a], np.uint8)  # noqa: E731
    return {"tracks": u8(trk), "csum": u8(csum), "pooled": u8(pooled_sum), "pct": u8(pct), "last_add": last}


CASES = [
    # length, stride, nstrands, S, control, coeffs
    (900, 768, 1, 1, None, None),
    (1500, 1024, 2, 3, [0, 1, 0], None),
    (3000, unit_stride(3000, 50), 2, 4, [1, 0, 0, 0], [0.37, 1.91, 4094.2]),
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_vectorised_reference_matches_loop(case):
    length, stride, nstrands, S, control, coeffs = CASES[case]
    rng = np.random.default_rng(500 + case)
    m = UnitModel(length, nstrands, S)
    palette = np.array([1, 1, 2, 2, 3, 4, 17, 120, 254, 255, 256, 70_000], np.uint32)
    for st in range(nstrands):
        for s in range(S):
            # dense clusters (several counts per chunk, sums around 255) and the bounds
            pos = np.unique(np.concatenate([rng.integers(1, length + 1, length // 12),
                                            np.arange(33, 49), [1, length]]))
            m.scatter(st, s, pos, palette[rng.integers(0, len(palette), len(pos))])
            # written twice: raised, dropped back from an escape, cleared
            again = pos[rng.integers(0, len(pos), 20)]
            again = np.unique(again)
            m.scatter(st, s, again, rng.integers(0, 4, len(again)))
    ctl = [0] * S if control is None else control
    got = index_arrays(m.sparse(), stride, PAD, nstrands, S, control, coeffs)
    want = loop_reference(m, stride, ctl, coeffs)
    for k in ("tracks", "csum", "pooled", "pct"):
        assert got[k].dtype == np.uint8 and np.array_equal(got[k], want[k]), k
    assert got["last_add"] == want["last_add"] > 0
    assert got["csum"].max() == 255 and got["pct"].max() == 255  # the saturation is exercised
    assert got["pooled"].max() == 255
    if coeffs is None:
        assert np.count_nonzero(got["pooled"] % 255)  # unsaturated pooled bytes as well


def test_screen_weights():
    assert screen_weights([0, 1, 0], None) == ([0, 2], [1, 1])
    assert screen_weights([1, 0, 0, 0], [0.37, -1.91, 4094.2]) == ([1, 2, 3], [2, 3, 4096])
    assert screen_weights([0], [2.0]) == ([0], [3])  # ceil(|coef| + 1), not ceil(|coef|) + ...
    assert screen_weights([0], [0.0]) == ([0], [1])


def test_unit_stride():
    assert unit_stride(1, 50) == 512 + 4096
    assert unit_stride(16384 - 1024, 50) == 512 + 4096
    assert unit_stride(16384 - 1023, 50) == 512 + 2 * 4096
    assert unit_stride(31_668, 50) == 512 + 2 * 4096 and unit_stride(31_668, 700) == 512 + 3 * 4096
