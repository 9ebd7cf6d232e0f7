"""Time the head-unit work of one pass (up_set_head_place) on one chr21-sized
nondirectional unit whose tags were moved by -s 75, as `regions -D -s 75`
sees it: the reverse strand's tags land at positions <= bw, so the unit is a
head unit (quirk Q1).

Prints one JSON line: per mode the blocking pass's wall time (up_timings [3],
which includes the host merge when the mode is off) and K1..K3's device
times, and for the mode on the device times of K0 and of the two placement
kernels alone (HIP events around those launches: up_timings [6], [7]).
Medians and ranges over --reps passes after --warmup.

  python tools/head_place_time.py [--reps 20] [--warmup 3] [--bw 50] [--shift 75]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHR21 = 48_129_895


def stats(v):
    v = np.asarray(v, float)
    return dict(median=round(float(np.median(v)), 4), min=round(float(v.min()), 4), max=round(float(v.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bw", type=int, default=50)
    ap.add_argument("--shift", type=int, default=75)
    ap.add_argument("--length", type=int, default=CHR21)
    a = ap.parse_args()
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()  # torch's HIP runtime first (capi.py)
    from unipeak_amd import capi
    out = dict(length=a.length, bw=a.bw, shift=a.shift, reps=a.reps)
    with capi.Lib(0) as g:
        g.set_params(a.bw, 1, 0.003, region_thr=25.0, kurt_thr=50.0, corr_thr=0.3, nondir=True, want_corr=True)
        u = g.add_unit(a.length)
        for strand, off in ((0, a.shift), (1, -a.shift)):
            g.synth(u, strand, 0, 1000, 20, strand, nondir=True, peaks=True, offset=off)
        # (this seed's chr21 has no background tag within the first bw positions after
        # the shift; two reverse tags there make it the head unit the genome's contigs are)
        g.scatter(u, 1, 0, [7, 31], [2, 1])
        g.set_timing(2)
        for on in (False, True):
            g.set_head_place(on)
            wall, k123, k0, place = [], [], [], []
            for i in range(a.warmup + a.reps):
                n = g.run()
                t = np.zeros(8, np.float64)
                capi._ck(g.L.up_timings(g.ctx, t.ctypes.data, 8))
                if i >= a.warmup:
                    wall.append(t[3])
                    k123.append(t[0] + t[1] + t[2])
                    k0.append(t[6])
                    place.append(t[7])
            mode = dict(regions=int(n), head_kind=g.last_head_kind(), resync=g.unit_resync(u),
                        wall_ms=stats(wall), k1_k2_k3_ms=stats(k123))
            if on:
                mode["k0_ms"] = stats(k0)
                mode["placement_ms"] = stats(place)
            out["on" if on else "off"] = mode
            if mode["head_kind"] != int(on):
                raise SystemExit(f"expected head kind {int(on)}: {json.dumps(mode)}")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
