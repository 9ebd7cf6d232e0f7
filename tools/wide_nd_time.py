"""Time one blocking up_run of a chr21-sized nondirectional synthetic unit at
a wide bandwidth: K1w over both strands (csrc/wide.hip) against the exact
replay of the same build (UNIPEAK_WIDE_ND=0, read at up_open).

  python tools/wide_nd_time.py                 # -b 700 and 2000, both paths
  python tools/wide_nd_time.py --bw 700 --reps 7
  python tools/wide_nd_time.py --bw 2000 --no-replay --reps 10    # K1w alone

Every (bandwidth, path) measurement runs in a fresh child process, the two
paths alternating, `--rounds` times; a child builds the unit, runs `--warmup`
untimed passes (index build, first launches) and then `--reps` timed ones.
up_run is blocking, so the host clock around it ends after the device is
done.  Prints one JSON line per child and a summary: the median over all
timed passes, the spread (min .. max) and the ratio of the two medians.  The
two paths must report the same number of regions and the same checksum of
the records."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHR21 = 48_129_895  # hg19
# the record fields both paths give bit for bit (kurtosis and the correlation
# agree within 1e-12: tests/test_gpu_wide_nondir.py)
EXACT = ("left", "right", "peak", "sum", "accepted", "peak_score")


def child(args):
    sys.path.insert(0, ROOT)
    from unipeak_amd import capi
    with capi.Lib(0) as g:
        g.set_params(args.bw, 1, 0.0029, nondir=True)
        u = g.add_unit(args.length)
        tags = 0
        for st in (0, 1):
            g.synth(u, st, 0, args.seed, 20, st, nondir=True, peaks=True)
            tags += g.tag_total(u, st, 0)
        g.set_params(args.bw, 1, tags / args.length, region_thr=args.thr, kurt_thr=0.0, corr_thr=0.3,
                     hit_thr=10.0, nondir=True, want_corr=True)
        for _ in range(args.warmup):
            n = g.run()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            n = g.run()
            ms.append((time.perf_counter() - t0) * 1e3)
        regs, cnt = g.regions(n)
        print(json.dumps({"bw": args.bw, "wide_nd": os.environ.get("UNIPEAK_WIDE_ND", "1"),
                          "scan_kind": g.last_scan_kind(), "tags": tags, "regions": int(n),
                          "accepted": int(regs["accepted"].sum()),
                          "crc": zlib.crc32(b"".join(regs[k].tobytes() for k in EXACT) + cnt.tobytes()),
                          "ms": ms,
                          # the last pass by phase (up_timings: K1, K2, K3 with the
                          # wide correlation, wall, K1b), zeros for the replay
                          "phases_ms": [round(float(x), 3) for x in g.timings()]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bw", type=int, action="append")
    ap.add_argument("--length", type=int, default=CHR21)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--thr", type=float, default=25.0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-replay", action="store_true", help="time K1w only (a replay pass at -b 2000 takes 25 s)")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        args.bw = args.bw[0]
        return child(args)
    out = {}
    for bw in args.bw or [700, 2000]:
        for rnd in range(args.rounds):
            for nd in ("1",) if args.no_replay else ("1", "0"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--bw", str(bw), "--length",
                       str(args.length), "--seed", str(args.seed), "--thr", str(args.thr), "--warmup",
                       str(args.warmup), "--reps", str(args.reps)]
                r = subprocess.run(cmd, env=dict(os.environ, UNIPEAK_WIDE_ND=nd), capture_output=True, text=True)
                if r.returncode != 0:
                    sys.exit(f"child failed ({r.returncode}):\n{r.stderr[-2000:]}")
                line = r.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                out.setdefault((bw, nd), []).append(json.loads(line))
    for bw in args.bw or [700, 2000]:
        if args.no_replay:
            t = [x for d in out[(bw, "1")] for x in d["ms"]]
            print(f"bw {bw}: K1w median {statistics.median(t):.2f} ms ({min(t):.2f} .. {max(t):.2f})")
            continue
        new, old = out[(bw, "1")], out[(bw, "0")]
        assert {d["scan_kind"] for d in new} == {1} and {d["scan_kind"] for d in old} == {3}
        assert len({(d["regions"], d["crc"]) for d in new + old}) == 1, "the two paths' records differ"
        t = {k: [x for d in v for x in d["ms"]] for k, v in (("k1w", new), ("replay", old))}
        med = {k: statistics.median(v) for k, v in t.items()}
        print(f"bw {bw}: {new[0]['regions']} regions ({new[0]['accepted']} accepted); "
              f"K1w median {med['k1w']:.2f} ms ({min(t['k1w']):.2f} .. {max(t['k1w']):.2f}), "
              f"replay median {med['replay']:.2f} ms ({min(t['replay']):.2f} .. {max(t['replay']):.2f}), "
              f"ratio {med['replay'] / med['k1w']:.2f}x")


if __name__ == "__main__":
    main()
