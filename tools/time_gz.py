#!/usr/bin/env python3
"""Time the compressed ways of writing a -w density profile end to end on one
synthetic sample, the paths alternating in one command:

  wig        bin/regions -f -w x.wig                          the floor
  gz_zlib    bin/regions -f -w a.wig.gz, UNIPEAK_GZ_DEVICE=0  host zlib, one thread
  gz_device  bin/regions -f -w b.wig.gz                       the device's encoder
  bw_zlib    bin/regions -f -W y                              compress2 on the pool
  bw_device  bin/regions -f -W z, UNIPEAK_BIGWIG_DEFLATE=device

  python tools/time_gz.py OUTDIR [--contig chr21,chr22] [--pairs 2] [--parent-bin DIR]

--parent-bin names a bin/ directory of another build (with the library beside
it as that build lays it out); its regions then writes one more .wig.gz per
pair ("gz_parent"), to show that the zlib path here is that build's.  The
sample is the bench generator's (seed 1000).  Every run is a child process of
its own with UNIPEAK_TIMING=1; wall time and peak RSS come from wait4.
OUTDIR/<stage>_<pair>.err keep the children's stderr, OUTDIR/summary.json the
table, the file sizes and whether the .gz files inflate to the plain profile
(checked with `gzip -dc | cmp`).  Work files are removed at the end."""
import argparse
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.time_bigwig import child  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--contig", default="chr21,chr22")
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--work", default=None)
    ap.add_argument("--parent-bin", default=None)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds per child")
    ap.add_argument("--skip", default="", help="comma-separated stages to leave out")
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
    with open(os.path.join(out, "make.log"), "w") as f:
        f.write(f"s0: {tags} tags on {contigs}\n")
    # (-n: a track is named after its file otherwise, and the profiles would differ in that)
    here = [os.path.join(ROOT, "bin", "regions"), "-q", "-f", "-n", "trk", "-c", "contigs.txt"]
    stages = [("wig", here + ["-w", "x.wig", "-o", "r0.txt", "s0.wig"], {}),
              ("gz_zlib", here + ["-w", "a.wig.gz", "-o", "r1.txt", "s0.wig"], {"UNIPEAK_GZ_DEVICE": "0"}),
              ("gz_device", here + ["-w", "b.wig.gz", "-o", "r2.txt", "s0.wig"], {}),
              ("bw_zlib", here + ["-W", "y", "-o", "r3.txt", "s0.wig"], {}),
              ("bw_device", here + ["-W", "z", "-o", "r4.txt", "s0.wig"], {"UNIPEAK_BIGWIG_DEFLATE": "device"})]
    if a.parent_bin:
        parent = [os.path.join(os.path.abspath(a.parent_bin), "regions"), "-q", "-f", "-n", "trk", "-c", "contigs.txt"]
        stages.insert(2, ("gz_parent", parent + ["-w", "p.wig.gz", "-o", "r5.txt", "s0.wig"], {}))
    stages = [s for s in stages if s[0] not in a.skip.split(",")]
    rows, ok = [], True
    for pair in range(1, a.pairs + 1):
        for name, cmd, env in stages:
            for k in ("UNIPEAK_GZ_DEVICE", "UNIPEAK_BIGWIG_DEFLATE", "UNIPEAK_GZ_BATCH"):
                os.environ.pop(k, None)
            os.environ.update(env)
            wall, rss, rc = child(cmd, work, os.path.join(out, f"{name}_{pair}.err"), a.limit)
            rows.append(dict(stage=name, pair=pair, wall_s=round(wall, 3), peak_rss_mib=round(rss, 1), rc=rc))
            print(json.dumps(rows[-1]), flush=True)
            ok = ok and rc == 0
            if rc != 0:
                break  # nothing more is started after a child that failed
        if not ok:
            break
    result = dict(tags=tags, contigs=contigs, runs=rows)
    if ok:
        result["bytes"] = {n: os.path.getsize(os.path.join(work, n)) for n in sorted(os.listdir(work))
                           if n.endswith((".bw", ".wig", ".gz"))}
        same = {}
        for n in sorted(os.listdir(work)):
            if n.endswith(".wig.gz") and os.path.exists(os.path.join(work, "x.wig")):
                r = subprocess.run(f"gzip -dc {n} | cmp -s - x.wig", shell=True, cwd=work)
                same[n] = r.returncode == 0
        result["inflates_to_plain"] = same
    with open(os.path.join(out, "summary.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
