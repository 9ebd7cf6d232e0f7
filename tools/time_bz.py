#!/usr/bin/env python3
"""Time the ways of reading one wiggle sample into bin/regions end to end
(DESIGN.md §17), the forms alternating in one command:

  wig         bin/regions s0.wig                               the floor
  gz          bin/regions s0.wig.gz                            zlib on the host
  bz2_device  bin/regions s0.wig.bz2, UNIPEAK_BZ_DEVICE=1      the device decoder
  bz2_host    bin/regions s0.wig.bz2, UNIPEAK_BZ_DEVICE=0      its host twin
  pipe        bunzip2 -c s0.wig.bz2 | bin/regions ... stdin    how a build without the
                                                               decoder reads the file

  python tools/time_bz.py OUTDIR [--contig chr21,chr22] [--pairs 2] [--parent-bin DIR]

--parent-bin names the bin/ directory of a build without the decoder for the
"pipe" form (this build's own regions reads stdin with the same code).  After
the pairs, two more children decode the .bz2 alone through capi.Bunzip, one with
the default number of inverse-BWT walk starts and one with UNIPEAK_BZ_STARTS=1,
and print the per-kernel device times of up_bz_timings ("kernels_many",
"kernels_one": the second decode of each child, the first one warms up).

The sample is the bench generator's (seed 1000), compressed with gzip and
bzip2 -9.  Every run is a child process of its own with UNIPEAK_TIMING=1.
OUTDIR/<stage>_<pair>.err keep the children's stderr, OUTDIR/summary.json the
table, the file sizes and whether every form gave the plain run's table."""
import argparse
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def decode_alone(path):
    """child mode: per-kernel device ms of the second decode of one .bz2 file"""
    import time
    from unipeak_amd import capi
    data = open(path, "rb").read()
    with capi.Bunzip(0) as bz:
        bz.decode(data)
        t0 = bz.timings()
        w0 = time.perf_counter()
        out, info = bz.decode(data)
        wall = time.perf_counter() - w0
        t = bz.timings() - t0
    names = ("scan", "entropy", "rank", "walks", "rle_crc")
    print(json.dumps(dict(file=os.path.basename(path), bytes_in=len(data), bytes_out=len(out),
                          blocks=int(info.blocks), starts=os.environ.get("UNIPEAK_BZ_STARTS", "default"),
                          wall_ms=round(wall * 1e3, 3), **{n: round(float(v), 3) for n, v in zip(names, t)})),
          flush=True)
    return 0


def table_body(path):
    return [l for l in open(path, "rb").read().split(b"\n") if not l.startswith(b"# align_file=")]


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--decode":
        return decode_alone(sys.argv[2])
    from tools.time_bigwig import child
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--contig", default="chr21,chr22")
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--work", default=None)
    ap.add_argument("--parent-bin", default=None)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds per child")
    a = ap.parse_args()
    out = os.path.abspath(a.outdir)
    work = os.path.abspath(a.work or os.path.join(out, "work"))
    os.makedirs(out, exist_ok=True)
    os.makedirs(work, exist_ok=True)
    from tests.conftest import _ensure_oracle
    from tests.make_wig import contig_table, write_sample
    from tests.oracle_binding import Oracle
    _ensure_oracle()
    table = contig_table("hg19")
    idx = [i for i, (c, _) in enumerate(table) if c in a.contig.split(",")]
    contigs = [table[i] for i in idx]
    with open(os.path.join(work, "contigs.txt"), "w") as f:
        for c, size in contigs:
            f.write(f"{c}\t{size}\n")
    tags = write_sample(os.path.join(work, "s0.wig"), "s0", Oracle(), contigs, 1000, False, True, index=idx)
    subprocess.run("gzip -c s0.wig > s0.wig.gz && bzip2 -9 -c s0.wig > s0.wig.bz2", shell=True, cwd=work, check=True)
    with open(os.path.join(out, "make.log"), "w") as f:
        f.write(f"s0: {tags} tags on {contigs}\n")
    here = [os.path.join(ROOT, "bin", "regions"), "-q", "-f", "-c", "contigs.txt"]
    pipe_bin = os.path.join(os.path.abspath(a.parent_bin), "regions") if a.parent_bin else here[0]
    pipe = f"set -o pipefail; bunzip2 -c s0.wig.bz2 | {pipe_bin} -q -f -c contigs.txt -o r4.txt stdin"
    stages = [("wig", here + ["-o", "r0.txt", "s0.wig"], {}),
              ("gz", here + ["-o", "r1.txt", "s0.wig.gz"], {}),
              ("bz2_device", here + ["-o", "r2.txt", "s0.wig.bz2"], {"UNIPEAK_BZ_DEVICE": "1"}),
              ("bz2_host", here + ["-o", "r3.txt", "s0.wig.bz2"], {"UNIPEAK_BZ_DEVICE": "0"}),
              ("pipe", ["bash", "-c", pipe], {})]
    me = [sys.executable, os.path.abspath(__file__), "--decode", "s0.wig.bz2"]
    rows, ok = [], True

    def one(name, cmd, env, tag):
        for k in ("UNIPEAK_BZ_DEVICE", "UNIPEAK_BZ_STARTS"):
            os.environ.pop(k, None)
        os.environ.update(env)
        wall, rss, rc = child(cmd, work, os.path.join(out, f"{name}_{tag}.err"), a.limit)
        rows.append(dict(stage=name, pair=tag, wall_s=round(wall, 3), peak_rss_mib=round(rss, 1), rc=rc))
        print(json.dumps(rows[-1]), flush=True)
        return rc == 0

    for pair in range(1, a.pairs + 1):
        for name, cmd, env in stages:
            ok = ok and one(name, cmd, env, pair)
            if not ok:
                break  # nothing more is started after a child that failed
        if not ok:
            break
    kernels = {}
    for name, env in (("kernels_many", {}), ("kernels_one", {"UNIPEAK_BZ_STARTS": "1"})):
        if not ok:
            break
        for k in ("UNIPEAK_BZ_DEVICE", "UNIPEAK_BZ_STARTS"):
            os.environ.pop(k, None)
        os.environ.update(env)
        r = subprocess.run(["timeout", "-k", "10", str(int(a.limit))] + me, cwd=work, capture_output=True, text=True)
        open(os.path.join(out, f"{name}.txt"), "w").write(r.stdout + r.stderr)
        ok = r.returncode == 0
        if ok:
            kernels[name] = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps({name: kernels[name]}), flush=True)
    result = dict(tags=tags, contigs=contigs, runs=rows, kernels=kernels)
    if ok:
        result["bytes"] = {n: os.path.getsize(os.path.join(work, n)) for n in sorted(os.listdir(work))
                           if n.startswith("s0.wig")}
        ref = table_body(os.path.join(work, "r0.txt"))
        result["same_table"] = {n: table_body(os.path.join(work, n)) == ref
                                for n in ("r1.txt", "r2.txt", "r3.txt", "r4.txt")}
        ok = all(v for n, v in result["same_table"].items() if n != "r4.txt")  # stdin names itself differently
    with open(os.path.join(out, "summary.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
