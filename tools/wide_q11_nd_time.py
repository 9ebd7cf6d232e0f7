"""Time one blocking up_run at `-r 0` and a wide bandwidth on a nondirectional
unit: chr21 of the synthetic genome with both strands in one buffer, the
strand correlation evaluated -- this build's library with up_set_wide_q11_nd on
(wide K1q: csrc/wide.hip, with the stage and chain kernels for long regions)
against another library, the parent commit's, which takes the segmented
replay for this combination.

  python tools/wide_q11_nd_time.py --parent-lib <parent's libunipeak_hip.so>
  python tools/wide_q11_nd_time.py --parent-lib ... --row b600 --rounds 3
  python tools/wide_q11_nd_time.py --row b2000_whole            # this build alone

Rows: b600 (the whole contig at -b 600), b2000_6m (-b 2000 on the contig's
first 6 Mbp), b2000_whole (-b 2000 on the whole contig: this build only -- on
directional units the parent needed about 150 s there and then failed).

Every (row, library) measurement runs in a fresh child process (UNIPEAK_LIB
picks the library), the two libraries alternating, the parent first,
`--rounds` times; a child builds the unit, runs its warm-up passes untimed and
then its timed ones (the parent `--parent-warmup` and `--parent-reps`).
up_run is blocking, so the host clock around it ends after the device is done.

Prints one JSON line per child (its passes in ms, the last pass by phase from
up_timings, the scan kind, the region count, the longest region and a CRC over
the bit-exact record fields, the correlation's bits included) and a summary per
row.  Acceptance, checked here for the A/B rows: in every round this build's
median is below the parent's minimum, the parent reports scan kind 3 and this
build 2, and both deliver the same records (at -b 2000 both lists may be
empty: one run spans the unit and the last run of a buffer is never closed)."""
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
ROWS = {"b600": (600, CHR21, True), "b2000_6m": (2000, 6_000_000, True), "b2000_whole": (2000, CHR21, False)}
# the record fields both paths give bit for bit (kurtosis agrees within 1e-12:
# tests/test_gpu_wide_q11_nd.py)
EXACT = ("left", "right", "peak", "sum", "accepted", "peak_score", "corr")


def child(args):
    sys.path.insert(0, ROOT)
    from unipeak_amd import capi
    with capi.Lib(0) as g:
        g.set_params(args.bw, 1, 0.0029, nondir=True)
        u = g.add_unit(args.length)
        tags = 0
        for st in (0, 1):
            g.synth(u, st, 0, args.seed, CHR21_INDEX, st, nondir=True, peaks=True)
            tags += g.tag_total(u, st, 0)
        g.set_params(args.bw, 1, tags / args.length, region_thr=0.0, kurt_thr=0.0, corr_thr=0.3, hit_thr=10.0,
                     nondir=True, want_corr=True)
        if hasattr(g.L, "up_set_wide_q11_nd"):
            g.set_wide_q11_nd(True)
        g.set_timing(2)
        for _ in range(args.warmup):
            n = g.run()
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            n = g.run()
            ms.append((time.perf_counter() - t0) * 1e3)
        regs, cnt = g.regions(n)
        print(json.dumps({"row": args.row, "bw": args.bw, "bp": args.length, "lib": args.tag,
                          "scan_kind": g.last_scan_kind(), "tags": tags, "regions": int(n),
                          "accepted": int(regs["accepted"].sum()),
                          "longest": int((regs["right"] - regs["left"]).max()) + 1 if n else 0,
                          "crc": zlib.crc32(b"".join(regs[k].tobytes() for k in EXACT) + cnt.tobytes()),
                          "ms": [round(x, 3) for x in ms],
                          # the last pass by phase (up_timings: K1 = the run kernel, K2, K3 with the
                          # peak and correlation kernels, wall, K1b), device phases zero for the replay
                          "phases_ms": [round(float(x), 3) for x in g.timings()]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--row", action="append", choices=sorted(ROWS))
    ap.add_argument("--bw", type=int)
    ap.add_argument("--length", type=int)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-warmup", type=int, default=1)
    ap.add_argument("--parent-reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", help="the other library; without it this build is timed alone")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tag", default="new")
    args = ap.parse_args()
    if args.child:
        args.row = args.row[0]
        return child(args)
    rows = args.row or sorted(ROWS)
    out = {}
    for row in rows:
        bw, length, ab = ROWS[row]
        ab = ab and bool(args.parent_lib)
        for rnd in range(args.rounds):
            for tag in (("parent", "new") if ab else ("new",)):
                old = tag == "parent"
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tag", tag, "--row", row,
                       "--bw", str(bw), "--length", str(length), "--seed", str(args.seed),
                       "--warmup", str(args.parent_warmup if old else args.warmup),
                       "--reps", str(args.parent_reps if old else args.reps)]
                env = dict(os.environ)
                env.pop("UNIPEAK_LIB", None)
                if old:
                    env["UNIPEAK_LIB"] = os.path.abspath(args.parent_lib)
                if old and (row, "parent-failed") in out:
                    continue
                r = subprocess.run(cmd, env=env, capture_output=True, text=True)
                if r.returncode != 0 and old:
                    # (the parent's replay gives up where one region outgrows its
                    # scratch: report it and go on with this build alone)
                    why = (r.stderr.strip().splitlines() or ["?"])[-1]
                    print(json.dumps({"row": row, "lib": tag, "failed": why}), flush=True)
                    out[(row, "parent-failed")] = why
                    continue
                if r.returncode != 0:
                    sys.exit(f"child failed ({r.returncode}):\n{r.stderr[-2000:]}")
                line = r.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                out.setdefault((row, tag), []).append(json.loads(line))
    ok = True
    for row in rows:
        new = out[(row, "new")]
        t_new = [x for d in new for x in d["ms"]]
        head = (f"{row}: {new[0]['regions']} regions (the longest {new[0]['longest']} positions); this build "
                f"median {statistics.median(t_new):.2f} ms ({min(t_new):.2f} .. {max(t_new):.2f}), phases of its "
                f"last pass {new[-1]['phases_ms']}")
        if (row, "parent-failed") in out:
            print(f"{head}; the parent's pass failed: {out[(row, 'parent-failed')]}")
            ok = False
            continue
        if (row, "parent") not in out:
            print(head)
            continue
        old = out[(row, "parent")]
        t_old = [x for d in old for x in d["ms"]]
        kinds = {d["scan_kind"] for d in new} == {2} and {d["scan_kind"] for d in old} == {3}
        same = len({(d["regions"], d["crc"]) for d in new + old}) == 1
        faster = all(statistics.median(n["ms"]) < min(o["ms"]) for n, o in zip(new, old))
        ok = ok and kinds and same and faster
        print(f"{head}; parent median {statistics.median(t_old):.2f} ms ({min(t_old):.2f} .. {max(t_old):.2f}), "
              f"ratio {statistics.median(t_old) / statistics.median(t_new):.1f}x; "
              f"scan kinds {'ok' if kinds else 'WRONG'}, records {'identical' if same else 'DIFFER'}"
              f"{' (both lists empty)' if same and not new[0]['regions'] else ''}, "
              f"every round faster: {'yes' if faster else 'NO'}")
    if not ok:
        sys.exit("acceptance not met")


if __name__ == "__main__":
    main()
