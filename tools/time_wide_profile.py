#!/usr/bin/env python3
"""Time `-w` at a wide bandwidth through the C-ABI: one contig of the
synthetic genome as a directional unit pair (up_unit_synth, both buffers),
the -w capture on, then up_run plus the whole profile of both units -- the
way bin/regions' write_profile collects it: up_unit_replay_profile for what
the exact replay retired, up_unit_profile_range (chunks of 4 Mi positions up
to len + bw) for the rest.  A library from before wide_profile_kernel replays
every unit with the capture on and hands the whole profile over as replay
entries; this one runs K1w and the dense profile kernel.

One JSON line per bandwidth: wall ms of up_run, of the profile calls and
their sum (C-ABI calls only, host post-processing excluded), the dense
profile kernel's own time from HIP events (up_timings [5]; 0 where the
library has none) with the positions per second it reaches, a K1w pass
without the capture, and the SHA-256 of the profile's nonzero (position,
score) pairs, so two libraries can be compared byte for byte.

  UNIPEAK_LIB=<library> python tools/time_wide_profile.py --out new.jsonl
  UNIPEAK_WIDE_PROFILE_LIST=0 ... --out direct.jsonl   (the direct window walk)
  python tools/time_wide_profile.py --check parent.jsonl new.jsonl

  --nondir: the contig as ONE nondirectional synthetic unit (both strands in
  one buffer, the unit tools/wide_nd_time.py builds, `-D -y` thresholds), the
  capture on and, where the library has it, up_set_wide_nd_full on: a library
  without it replays the whole buffer with the capture on; this one runs K1w
  and wide_profile_kernel<POOL, true>.  The profile is f + r.  `--warmup`
  passes (up_run + profile) go untimed, then `--reps` timed ones: the row
  holds their median, minimum and maximum.

Run each library in a process of its own, every step under its own
`timeout`, the steps chained with `&&`."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLUSH = 0xFFFFFFFF  # UP_FLUSH_EVENT
CHUNK = 1 << 22


def collect(g, u, length, bw, clock, nondir=False):
    """nonzero (pos, score) of unit u in position order; adds the C-ABI time
    to clock["profile"] and the dense kernel's to clock["kernel"]"""
    t0 = time.perf_counter()
    resync, _, pos, score = g.replay_profile(u)
    clock["profile"] += time.perf_counter() - t0
    ps, ss = [pos.astype(np.uint32)], [score]
    clock["replayed"] += int(pos.size)
    if resync != FLUSH:
        first, end = (resync if resync else 1), length + bw
        while first <= end:
            n = min(CHUNK, end - first + 1)
            t0 = time.perf_counter()
            f, r = g.profile_range(u, first, n)
            clock["profile"] += time.perf_counter() - t0
            if nondir:
                f = f + r
            clock["kernel"] += g.profile_kernel_ms()
            clock["dense"] += n
            nz = np.flatnonzero(f)
            ps.append((nz + first).astype(np.uint32))
            ss.append(f[nz])
            first += n
    return np.concatenate(ps), np.concatenate(ss)


def measure(capi, name, ci, length, bw, reps):
    with capi.Lib(0) as g:
        g.set_params(bw, 1, 0.0029)
        units = []
        for buf in (0, 1):
            u = g.add_unit(length, buffer_id=buf)
            g.synth(u, 0, 0, 1000, ci, buf, nondir=False, peaks=True)
            units.append(u)
        g.run()  # warm-up: allocations, the index
        t0 = time.perf_counter()
        n = g.run()
        k1w = time.perf_counter() - t0
        g.set_profile_capture(True)
        best = None
        for _ in range(reps):
            clock = {"profile": 0.0, "kernel": 0.0, "dense": 0, "replayed": 0}
            t0 = time.perf_counter()
            n = g.run()
            run_s = time.perf_counter() - t0
            h = hashlib.sha256()
            nonzero = 0
            for u in units:
                p, s = collect(g, u, length, bw, clock)
                h.update(p.tobytes())
                h.update(s.tobytes())
                nonzero += int(p.size)
            row = {"contig": name, "bp": length, "bw": bw, "lib": os.path.basename(capi.LIB_PATH),
                   "list": os.environ.get("UNIPEAK_WIDE_PROFILE_LIST", "1") != "0",
                   "candidates": int(n), "k1w_pass_ms": round(k1w * 1e3, 3),
                   "run_ms": round(run_s * 1e3, 3), "profile_ms": round(clock["profile"] * 1e3, 3),
                   "total_ms": round((run_s + clock["profile"]) * 1e3, 3),
                   "kernel_ms": round(clock["kernel"], 3), "dense_positions": clock["dense"],
                   "replayed_entries": clock["replayed"],
                   "kernel_positions_per_s": (round(clock["dense"] / (clock["kernel"] * 1e-3))
                                              if clock["kernel"] > 0 else None),
                   "nonzero": nonzero, "sha256": h.hexdigest()}
            if best is None or row["total_ms"] < best["total_ms"]:
                best = row
        return best


def measure_nondir(capi, name, ci, length, bw, reps, warmup):
    with capi.Lib(0) as g:
        g.set_params(bw, 1, 0.0029, nondir=True)
        u = g.add_unit(length)
        tags = 0
        for st in (0, 1):
            g.synth(u, st, 0, 1, ci, st, nondir=True, peaks=True)
            tags += g.tag_total(u, st, 0)
        g.set_params(bw, 1, tags / length, region_thr=25.0, kurt_thr=0.0, corr_thr=0.3, hit_thr=10.0,
                     nondir=True, want_corr=True)
        full = hasattr(g.L, "up_set_wide_nd_full")
        if full:
            g.set_wide_nd_full(True)
        g.set_profile_capture(True)
        rows = []
        for i in range(warmup + reps):
            clock = {"profile": 0.0, "kernel": 0.0, "dense": 0, "replayed": 0}
            t0 = time.perf_counter()
            n = g.run()
            run_s = time.perf_counter() - t0
            kind = g.last_scan_kind()
            p, s = collect(g, u, length, bw, clock, nondir=True)
            if i >= warmup:
                rows.append((run_s * 1e3, clock["profile"] * 1e3, clock["kernel"], clock))
        h = hashlib.sha256()
        h.update(p.tobytes())
        h.update(s.tobytes())
        tot = [a + b for a, b, _, _ in rows]
        ker = [k for _, _, k, _ in rows]
        clock = rows[-1][3]
        med = lambda v: round(statistics.median(v), 3)
        return {"contig": name, "bp": length, "bw": bw, "nondir": True, "wide_nd_full": full, "scan_kind": kind,
                "lib": os.path.basename(capi.LIB_PATH), "tags": int(tags), "candidates": int(n),
                "warmup": warmup, "reps": reps,
                "run_ms": med([a for a, _, _, _ in rows]), "profile_ms": med([b for _, b, _, _ in rows]),
                "total_ms": med(tot), "total_ms_min": round(min(tot), 3), "total_ms_max": round(max(tot), 3),
                "kernel_ms": med(ker), "kernel_ms_min": round(min(ker), 3), "kernel_ms_max": round(max(ker), 3),
                "dense_positions": clock["dense"], "replayed_entries": clock["replayed"],
                "kernel_positions_per_s": (round(clock["dense"] / (statistics.median(ker) * 1e-3))
                                           if min(ker) > 0 else None),
                "nonzero": int(p.size), "sha256": h.hexdigest()}


def check(a_path, b_path):
    """same profiles, and b faster than a, at every bandwidth"""
    def rows(p):
        return {r["bw"]: r for r in map(json.loads, open(p)) if "bw" in r}
    a, b = rows(a_path), rows(b_path)
    ok = True
    for bw in sorted(a):
        same = a[bw]["sha256"] == b[bw]["sha256"] and a[bw]["nonzero"] == b[bw]["nonzero"]
        ratio = a[bw]["total_ms"] / b[bw]["total_ms"]
        print(json.dumps({"bw": bw, "identical": same, "a_total_ms": a[bw]["total_ms"],
                          "b_total_ms": b[bw]["total_ms"], "a_over_b": round(ratio, 2)}), flush=True)
        ok &= same and ratio > 1
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig", default="chr21")
    ap.add_argument("--bw", type=int, nargs="+", default=[600, 2000])
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--nondir", action="store_true", help="one nondirectional unit (see above)")
    ap.add_argument("--warmup", type=int, default=1, help="untimed passes (--nondir)")
    ap.add_argument("--out")
    ap.add_argument("--check", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.check:
        sys.exit(check(*a.check))
    from unipeak_amd import capi
    rows = [l.split() for l in open(os.path.join(ROOT, "unipeak_amd", "data", "hg19.txt"))
            if l.strip() and not l.startswith("#")]
    ci = [r[0] for r in rows].index(a.contig)
    length = int(rows[ci][1])
    out = open(a.out, "w") if a.out else None
    for bw in a.bw:
        line = json.dumps(measure_nondir(capi, a.contig, ci, length, bw, a.reps, a.warmup) if a.nondir
                          else measure(capi, a.contig, ci, length, bw, a.reps))
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
