"""Plain reference of the per-dataset index (csrc/kernels.h; csum_units_kernel,
pool_units_kernel, pct_units_kernel, unit_last_kernel): every byte of the packed tracks,
the chunk-sum planes, the pooled plane and the pooled count track is a closed-form
integer function of the scattered counts.  numpy only, no GPU; the sums are carried in
uint64, so the reference itself cannot wrap (counts are uint32, weights <= 4096).

Position p (1-based) is field n = pad + p - 1 of its track; track (strand, sample) has
index strand * S + sample.  The arrays are built sparsely (only the touched bytes are
computed), so a unit of 10^8 positions costs its array sizes and no more.
"""
import math

import numpy as np

STRIP = 16384       # kStrip
PAD_BYTES = 256     # kPadBytes
MAX_BW = 511        # kMaxBw


def unit_stride(length, bw):
    """bytes per 2-bit track of a unit added at bandwidth bw (api.hip unit_stride)"""
    dom = length + 2 * max(bw, MAX_BW) + 2
    return PAD_BYTES + -(-dom // STRIP) * (STRIP // 4) + PAD_BYTES


def screen_weights(control, coeffs):
    """(indices of the non-control samples, their integer screen weights): 1 without
    coefficients, else ceil(|coef| + 1) (up_set_params; |coef| <= 4095 keeps the
    weights in the range where it does not switch the screen off)"""
    nc = [k for k, c in enumerate(control) if not c]
    if coeffs is None or len(coeffs) == 0:
        return nc, [1] * len(nc)
    assert len(coeffs) == len(nc)
    assert all(abs(q) <= 4095 for q in coeffs)
    return nc, [int(math.ceil(abs(float(q)) + 1.0)) for q in coeffs]


class UnitModel:
    """the counts of one unit as the scatters left them: {(strand, sample): {pos: count}}"""

    def __init__(self, length, nstrands, S):
        self.length, self.nstrands, self.S = length, nstrands, S
        self.t = {(st, s): {} for st in range(nstrands) for s in range(S)}

    def scatter(self, strand, sample, pos, cnt):
        d = self.t[(strand, sample)]
        for p, c in zip(np.asarray(pos).tolist(), np.asarray(cnt).tolist()):
            assert 1 <= p <= self.length
            if c:
                d[p] = c
            else:
                d.pop(p, None)

    def sparse(self):
        out = {}
        for key, d in self.t.items():
            p = np.array(sorted(d), np.int64)
            out[key] = (p, np.array([d[q] for q in p.tolist()], np.uint64))
        return out


def _sum_by(idx, val):
    """(unique idx, uint64 sum of val per idx)"""
    if len(idx) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.uint64)
    u, inv = np.unique(idx, return_inverse=True)
    s = np.zeros(len(u), np.uint64)
    np.add.at(s, inv.reshape(-1), val.astype(np.uint64))
    return u, s


def index_arrays(tracks, stride, pad, nstrands, S, control=None, coeffs=None, want_pct=True):
    """tracks: {(strand, sample): (pos int array, count array)}, positions unique per
    track -> dict of uint8 arrays "tracks", "csum", "pooled", "pct" laid out as on the
    device, and "last_add" (0: no pooled tag); want_pct False leaves "pct" out (four
    bytes per track byte: the largest of the arrays)"""
    control = [0] * S if control is None else list(control)
    nc, w = screen_weights(control, coeffs)
    ntracks = nstrands * S
    nd = stride // 4                       # plane bytes per track
    trk = np.zeros(ntracks * stride, np.uint8)
    csum = np.zeros(ntracks * nd, np.uint8)
    pooled = np.zeros(nd, np.uint8)
    pct = np.zeros(nstrands * 4 * stride if want_pct else 0, np.uint8)
    pool_idx, pool_val = [], []
    last = 0
    for st in range(nstrands):
        pct_idx, pct_val = [], []
        for s in range(S):
            pos, cnt = tracks.get((st, s), (np.zeros(0, np.int64), np.zeros(0, np.uint64)))
            pos = np.asarray(pos, np.int64)
            cnt = np.asarray(cnt, np.uint64)
            keep = cnt != 0
            pos, cnt = pos[keep], cnt[keep]
            assert len(np.unique(pos)) == len(pos)
            t = st * S + s
            n = pad + pos - 1                                  # the field index
            assert len(n) == 0 or (n.min() >= 0 and n.max() < 4 * stride)
            fld = np.minimum(cnt, 3).astype(np.uint8)          # min(count, 3), LSB first
            np.bitwise_or.at(trk, t * stride + n // 4, fld << (2 * (n % 4)).astype(np.uint8))
            j, sm = _sum_by(n // 16, cnt)                      # chunk sums
            byte = np.minimum(sm, 255)
            csum[t * nd + j] = byte.astype(np.uint8)
            if s in nc:
                pool_idx.append(j)
                pool_val.append(byte * np.uint64(w[nc.index(s)]))
                pct_idx.append(n)
                pct_val.append(cnt)
                if len(pos):
                    last = max(last, int(pos.max()))
        if pct_idx and want_pct:
            n, sm = _sum_by(np.concatenate(pct_idx), np.concatenate(pct_val))
            pct[st * 4 * stride + n] = np.minimum(sm, 255).astype(np.uint8)
    if pool_idx:
        j, sm = _sum_by(np.concatenate(pool_idx), np.concatenate(pool_val))
        pooled[j] = np.minimum(sm, 255).astype(np.uint8)
    return {"tracks": trk, "csum": csum, "pooled": pooled, "pct": pct, "last_add": last}
