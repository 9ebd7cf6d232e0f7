#!/usr/bin/env python3
"""Time the profile-to-bigWig paths end to end on one synthetic sample
(DESIGN.md §15): the two-stage pipeline `bin/regions -f -w x.wig` followed by
`bin/wigs2bigwigs`, against `bin/regions -f -W x`, alternating in one command.

  python tools/time_bigwig.py OUTDIR [--contig chr1|chr21] [--pairs 2] [--skip-two-stage]

The sample is the bench generator's (seed 1000) on one contig of the hg19
table.  Every run is a child process of its own with UNIPEAK_TIMING=1; its
wall time and peak RSS (ru_maxrss of the child) and its stderr are kept:
OUTDIR/<stage>_<pair>.err, OUTDIR/summary.json, and OUTDIR/identical.txt with
the comparison of the two paths' bigWig files (name several contigs, as in
`--contig chr21,chr22`: with one contig the -w file repeats its track lines for
the flush and wigs2bigwigs keeps each file's last track only): the SHA-256 of every item
(chromosome id, start, float bits) in file order, the chromosome tree's bytes,
and the total summaries (counts, min and max equal, sums to 1e-9).
Work files go to --work (default OUTDIR/work) and are removed at the end."""
import argparse
import json
import os
import shutil
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(cmd, cwd, err_path, limit):
    """(wall s, peak RSS MiB, return code) of one child, run under `timeout`; stderr to
    err_path.  The RSS is wait4's for that child (the largest process below it)."""
    t0 = time.perf_counter()
    with open(err_path, "w") as e:
        p = subprocess.Popen(["timeout", "-k", "10", str(int(limit))] + cmd, cwd=cwd, stdout=subprocess.DEVNULL,
                             stderr=e, env=dict(os.environ, UNIPEAK_TIMING="1"))
        _, status, ru = os.wait4(p.pid, 0)
    p.returncode = os.waitstatus_to_exitcode(status)
    wall = time.perf_counter() - t0
    return wall, ru.ru_maxrss / 1024.0, p.returncode


def digest(path):
    """(items, SHA-256 of every section's chromosome id and item bytes in R-tree order,
    chromosome tree bytes, total summary) -- section boundaries do not enter"""
    import hashlib
    import zlib
    b = open(path, "rb").read()
    zooms, ctree, data, index = struct.unpack_from("<HQQQ", b, 6)
    tsum, = struct.unpack_from("<Q", b, 44)
    ksize, = struct.unpack_from("<I", b, ctree + 8)
    nchrom, = struct.unpack_from("<Q", b, ctree + 16)
    tree = b[ctree:ctree + 36 + nchrom * (ksize + 8)]
    h = hashlib.sha256()
    n = 0
    last = None  # the chromosome id enters the hash where it changes, not once per section

    def walk(off):
        nonlocal n, last
        leaf, _, cnt = struct.unpack_from("<BBH", b, off)
        off += 4
        for _ in range(cnt):
            if leaf:
                _, _, _, _, doff, dsize = struct.unpack_from("<IIIIQQ", b, off)
                raw = zlib.decompress(b[doff:doff + dsize])
                if raw[:4] != last:
                    last = raw[:4]
                    h.update(last)
                h.update(raw[24:])
                n += (len(raw) - 24) // 8
                off += 32
            else:
                walk(struct.unpack_from("<IIIIQ", b, off)[4])
                off += 24
    walk(index + 48)
    red = [struct.unpack_from("<I", b, 64 + 24 * z)[0] for z in range(zooms)]
    return n, h.hexdigest(), tree, struct.unpack_from("<Qdddd", b, tsum), red


def compare(old, new):
    na, ha, ta, sa, _ = digest(old)
    nb, hb, tb, sb, red = digest(new)
    sums = all(abs(x - y) <= 1e-9 * abs(x) for x, y in zip(sa[3:], sb[3:]))
    return dict(items=nb, items_equal=(na, ha) == (nb, hb), tree_equal=ta == tb,
                summary_equal=sa[:3] == sb[:3] and sums, zoom_reductions=red, sha256=hb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("outdir")
    ap.add_argument("--contig", default="chr1")
    ap.add_argument("--pairs", type=int, default=2)
    ap.add_argument("--work", default=None)
    ap.add_argument("--skip-two-stage", action="store_true")
    ap.add_argument("--limit", type=float, default=420.0, help="seconds per child")
    ap.add_argument("--no-compare", action="store_true", help="skip the Python decode of the files")
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
    regions = [os.path.join(ROOT, "bin", "regions"), "-q", "-f", "-c", "contigs.txt"]
    rows = []
    ok = True
    for pair in range(1, a.pairs + 1):
        stages = []
        if not a.skip_two_stage:
            stages += [("wig", regions + ["-w", "x.wig", "-o", "r_wig.txt", "s0.wig"]),
                       ("wigs2bigwigs", [os.path.join(ROOT, "bin", "wigs2bigwigs"), "--sizes", "contigs.txt", "x.wig"])]
        for name, cmd in stages + [("bigwig", regions + ["-W", "y", "-o", "r_bw.txt", "s0.wig"])]:
            wall, rss, rc = child(cmd, work, os.path.join(out, f"{name}_{pair}.err"), a.limit)
            rows.append(dict(stage=name, pair=pair, wall_s=round(wall, 3), peak_rss_mib=rss and round(rss, 1), rc=rc))
            print(json.dumps(rows[-1]), flush=True)
            if rc != 0:
                ok = False
                if name != "bigwig":  # the two-stage path does not finish here: time the rest without it
                    a.skip_two_stage = True
                    break
    result = dict(tags=tags, contigs=contigs, runs=rows)
    if ok and not a.skip_two_stage and not a.no_compare:
        cmp_ = {t: compare(os.path.join(work, f"x{t}.bw"), os.path.join(work, f"y{t}.bw")) for t in "+-"}
        result["compare"] = cmp_
        with open(os.path.join(out, "identical.txt"), "w") as f:
            for t, c in cmp_.items():
                f.write(f"track {t}: {json.dumps(c)}\n")
        same_table = open(os.path.join(work, "r_wig.txt"), "rb").read() == open(os.path.join(work, "r_bw.txt"), "rb").read()
        result["region_tables_equal"] = same_table
    if ok:
        result["bytes"] = {n: os.path.getsize(os.path.join(work, n)) for n in sorted(os.listdir(work))
                           if n.endswith((".bw", ".wig"))}
    with open(os.path.join(out, "summary.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}), flush=True)
    shutil.rmtree(work, ignore_errors=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
