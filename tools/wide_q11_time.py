"""Time one blocking up_run at `-r 0` and a wide bandwidth: chr21 of the
synthetic genome as a directional unit pair (one unit per buffer), this
build's library -- wide K1q, csrc/wide.hip -- against another library, the
parent commit's, which takes the segmented replay for this combination.

  python tools/wide_q11_time.py --parent-lib <parent's libunipeak_hip.so>
  python tools/wide_q11_time.py --parent-lib ... --bw 600 --rounds 3
  python tools/wide_q11_time.py --bw 2000 --reps 10            # this build alone

Every (bandwidth, library) measurement runs in a fresh child process
(UNIPEAK_LIB picks the library), the two libraries alternating, the parent
first, `--rounds` times; a child builds the units, runs its warm-up passes
untimed (index build, first launches, the growth of the record areas) and then
its timed ones.  The parent's pass at -b 2000 takes tens of seconds, so it
runs `--parent-warmup` (1) and `--parent-reps` (1) passes per process.
up_run is blocking, so the host clock around it ends after the device is done.

Prints one JSON line per child (its passes in ms, the last pass by phase from
up_timings, the scan kind, the region count and a CRC over the bit-exact record
fields) and a summary per bandwidth: median (min .. max) per library and the
ratio of the medians.  Acceptance, checked here: in every round this build's
median is below the parent's minimum, the parent reports scan kind 3 and this
build 2, and both deliver the same records."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHR21, CHR21_INDEX = 48_129_895, 20  # hg19; its index in the synthetic genome
# the record fields both paths give bit for bit (kurtosis agrees within 1e-12:
# tests/test_gpu_wide_q11.py)
EXACT = ("left", "right", "peak", "sum", "accepted", "peak_score")


def child(args):
    sys.path.insert(0, ROOT)
    from unipeak_amd import capi
    with capi.Lib(0) as g:
        g.set_params(args.bw, 1, 0.0029, region_thr=0.0)
        tags = 0
        for buf in (0, 1):
            u = g.add_unit(args.length, buffer_id=buf)
            g.synth(u, 0, 0, args.seed, CHR21_INDEX, buf, nondir=False, peaks=True)
            tags += g.tag_total(u, 0, 0)
        g.set_timing(2)
        for _ in range(args.warmup):
            n = g.run()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            n = g.run()
            ms.append((time.perf_counter() - t0) * 1e3)
        regs, cnt = g.regions(n)
        print(json.dumps({"bw": args.bw, "lib": args.tag, "scan_kind": g.last_scan_kind(),
                          "k3_kind": g.last_k3_kind(), "tags": tags, "regions": int(n),
                          "longest": int((regs["right"] - regs["left"]).max()) + 1 if n else 0,
                          "crc": zlib.crc32(b"".join(regs[k].tobytes() for k in EXACT) + cnt.tobytes()),
                          "ms": [round(x, 3) for x in ms],
                          # the last pass by phase (up_timings: K1 = the run kernel, K2, K3 with
                          # the peak kernels, wall, K1b), device phases zero for the replay
                          "phases_ms": [round(float(x), 3) for x in g.timings()]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bw", type=int, action="append")
    ap.add_argument("--length", type=int, default=CHR21)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parent-warmup", type=int, default=1)
    ap.add_argument("--parent-reps", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", help="the other library; without it this build is timed alone")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tag", default="new")
    args = ap.parse_args()
    if args.child:
        args.bw = args.bw[0]
        return child(args)
    bws = args.bw or [600, 2000]
    out = {}
    for bw in bws:
        for rnd in range(args.rounds):
            for tag in (("parent", "new") if args.parent_lib else ("new",)):
                old = tag == "parent"
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tag", tag, "--bw", str(bw),
                       "--length", str(args.length), "--seed", str(args.seed),
                       "--warmup", str(args.parent_warmup if old else args.warmup),
                       "--reps", str(args.parent_reps if old else args.reps)]
                env = dict(os.environ)
                env.pop("UNIPEAK_LIB", None)
                if old:
                    env["UNIPEAK_LIB"] = os.path.abspath(args.parent_lib)
                if old and (bw, "parent-failed") in out:
                    continue
                r = subprocess.run(cmd, env=env, capture_output=True, text=True)
                if r.returncode != 0 and old:
                    # (the parent's replay gives up where one region outgrows its
                    # scratch: report it and go on with this build alone)
                    why = (r.stderr.strip().splitlines() or ["?"])[-1]
                    print(json.dumps({"bw": bw, "lib": tag, "failed": why}), flush=True)
                    out[(bw, "parent-failed")] = why
                    continue
                if r.returncode != 0:
                    sys.exit(f"child failed ({r.returncode}):\n{r.stderr[-2000:]}")
                line = r.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                out.setdefault((bw, tag), []).append(json.loads(line))
    ok = True
    for bw in bws:
        new = out[(bw, "new")]
        t_new = [x for d in new for x in d["ms"]]
        if not args.parent_lib or (bw, "parent-failed") in out:
            why = out.get((bw, "parent-failed"))
            print(f"bw {bw}: {new[0]['regions']} regions (the longest {new[0]['longest']} positions); "
                  f"median {statistics.median(t_new):.2f} ms "
                  f"({min(t_new):.2f} .. {max(t_new):.2f}); phases of the last pass {new[-1]['phases_ms']}"
                  + (f"; the parent's pass failed: {why}" if why else ""))
            ok = ok and not why
            continue
        old = out[(bw, "parent")]
        t_old = [x for d in old for x in d["ms"]]
        kinds = {d["scan_kind"] for d in new} == {2} and {d["scan_kind"] for d in old} == {3}
        same = len({(d["regions"], d["crc"]) for d in new + old}) == 1
        faster = all(statistics.median(n["ms"]) < min(o["ms"]) for n, o in zip(new, old))
        ok = ok and kinds and same and faster
        print(f"bw {bw}: {new[0]['regions']} regions (the longest {new[0]['longest']} positions); "
              f"this build median {statistics.median(t_new):.2f} ms ({min(t_new):.2f} .. {max(t_new):.2f}), "
              f"parent median {statistics.median(t_old):.2f} ms ({min(t_old):.2f} .. {max(t_old):.2f}), "
              f"ratio {statistics.median(t_old) / statistics.median(t_new):.1f}x; "
              f"phases of this build's last pass {new[-1]['phases_ms']}; "
              f"scan kinds {'ok' if kinds else 'WRONG'}, records {'identical' if same else 'DIFFER'}, "
              f"every round faster: {'yes' if faster else 'NO'}")
    if not ok:
        sys.exit("acceptance not met")


if __name__ == "__main__":
    main()
