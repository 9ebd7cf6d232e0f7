"""The -w profile as bigWig from the device (csrc/bigwig.hip behind
up_unit_profile_bigwig) and bin/regions -W through it.

The reference is always built here from Lib.profile_range's scores: an item is
(pos - 1, numpy.float32(float('%g' % (f + r)))) for every position whose f + r
is not 0 ('%g' and float() are pinned to libc's in test_format_g6.py and
test_g6_float.py), a '-' in front of the text for the reverse buffer -- never
anything the new path made.  The CLI tests compare bin/regions -W with the
pipeline it replaces, bin/regions -w and then bin/wigs2bigwigs.

All scores of a track have one sign (no negative coefficient is used), so any
summation order of n <= 2^22 terms is within (n - 1) * 2^-53 < 5e-10 of the
exact sum: sums in double are compared at relative 1e-9, and the float sums of
zoom records, rounded once from such doubles, within one float ulp."""
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests.gen import random_unit
from tests.test_bigwig import read_bigwig
from tests.test_cli import BIN, HG_LIKE, gen_sample, make_inputs, run
from tests.test_gpu_profile_text import BG, fused_case, load, scatter, with_tag
from tests.wig import write_contigs, write_wig

pytestmark = pytest.mark.gpu

UP_E_ARG = -1


def fbits(v):
    return np.ascontiguousarray(v, np.float32).view(np.uint32)


def ref_items(f, r, first, negate=False, clip_end=None):
    """(starts uint32[], values float32[]) of the scores f, r of [first, first + len(f))"""
    s = f + r
    idx = np.flatnonzero(s)
    if clip_end is not None:
        idx = idx[first + idx <= clip_end]
    sign = "-" if negate else ""
    vals = np.array([float(sign + "%g" % x) for x in s[idx].tolist()], np.float64).astype(np.float32)
    return (first + idx - 1).astype(np.uint32), vals


def check_sums(got, want, what):
    assert abs(got - want) <= 1e-9 * abs(want), (what, got, want)


def check_sections(sec, starts, vals):
    n = len(starts)
    assert len(sec) == (n + 1023) // 1024
    v = vals.astype(np.float64)
    for k, s in enumerate(sec):
        a, b = 1024 * k, min(n, 1024 * (k + 1))
        assert (s["start"], s["end"], s["count"]) == (starts[a], starts[b - 1] + 1, b - a), k
        assert fbits(s["vmin"]) == fbits(vals[a:b].min()) and fbits(s["vmax"]) == fbits(vals[a:b].max()), k
        check_sums(s["sum"], v[a:b].sum(), ("section sum", k))
        check_sums(s["sumsq"], (v[a:b] * v[a:b]).sum(), ("section sumsq", k))


def ref_zoom(starts, vals, red, clip_end):
    """per non-empty bin [j * red, (j + 1) * red) of the fixed grid: start, end, valid,
    min, max, and the sums in double"""
    bins = starts.astype(np.int64) // red
    edge = np.flatnonzero(np.diff(bins, prepend=-1))
    v = vals.astype(np.float64)
    st = bins[edge] * red
    return (st, np.minimum(st + red, clip_end), np.diff(np.append(edge, len(bins))),
            np.minimum.reduceat(vals, edge), np.maximum.reduceat(vals, edge),
            np.add.reduceat(v, edge), np.add.reduceat(v * v, edge))


def check_zoom(rec, starts, vals, red, clip_end, chrom):
    """rec: records with the fields of capi.BW_ZOOM_DTYPE, of one chromosome"""
    if len(starts) == 0:
        assert len(rec) == 0
        return
    st, en, valid, lo, hi, sm, sq = ref_zoom(starts, vals, red, clip_end)
    assert len(rec) == len(st), (red, len(rec), len(st))
    assert np.all(rec["chrom"] == chrom)
    assert np.array_equal(rec["start"], st) and np.array_equal(rec["end"], en), red
    assert np.array_equal(rec["valid"], valid), red
    assert np.array_equal(fbits(rec["vmin"]), fbits(lo)) and np.array_equal(fbits(rec["vmax"]), fbits(hi)), red
    for got, want in ((rec["sum"], sm), (rec["sumsq"], sq)):
        w32 = want.astype(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - w32.astype(np.float64)) <= np.spacing(np.abs(w32))), red


def check_call(g, u, f, r, first, count, negate, clip_end, red0=10, n_levels=0, chrom=0):
    """one profile_bigwig call against the scores f, r of positions 1 .. len(f)"""
    starts, vals = ref_items(f[first - 1:first - 1 + count], r[first - 1:first - 1 + count], first, negate, clip_end)
    items, sec, zoom, exact = g.profile_bigwig(u, first, count, negate=negate, clip_end=clip_end, reduction0=red0,
                                               n_levels=n_levels, chrom_id=chrom)
    assert exact
    assert np.array_equal(items["start"], starts)
    assert np.array_equal(fbits(items["value"]), fbits(vals)), "value bits differ at item %d" % next(
        iter(np.flatnonzero(fbits(items["value"]) != fbits(vals))), -1)
    check_sections(sec, starts, vals)
    assert len(zoom) == n_levels
    for z in range(n_levels):
        check_zoom(zoom[z], starts, vals, red0 * 4 ** z, clip_end, chrom)
    return starts, vals, sec, zoom


def test_bigwig_fused_k1(gpu_lib):
    c = fused_case()
    length, bw = c["length"], c["bw"]
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, c["pos"], c["cnt"])
        f, r = g.profile_range(u, 1, length + bw)
        assert (f + r)[length:].any()  # scores past the contig's end: clip_end has something to drop
        for negate in (False, True):
            starts, vals, sec, zoom = check_call(g, u, f, r, 1, length + bw, negate, length, n_levels=10, chrom=3)
            assert len(starts) > 20_000 and len(sec) > 20
            assert starts[-1] == length - 1  # the tag at the last position
            assert (vals < 0).all() if negate else (vals > 0).all()
            assert len(zoom[9]) == 1 and zoom[9]["valid"][0] == len(starts)
        assert g.profile_bigwig_ms() > 0
        # the value is the text's, not the score's
        s = (f + r)[starts.astype(np.int64)]
        assert np.count_nonzero(fbits(s.astype(np.float32)) != fbits(-vals)) > 1000
        # a range that starts at 160 * k + 1, three levels; workgroup and strip edges inside it
        check_call(g, u, f, r, 160 * 100 + 1, 30_000, False, length, n_levels=3, chrom=1)
        check_call(g, u, f, r, 160 * 431 + 1, length + bw - 160 * 431, True, length, n_levels=3)
        # no clipping inside the range, no zoom; a range without any item
        check_call(g, u, f, r, 1234, 5000, False, None)
        z = np.flatnonzero(f + r == 0)
        runs = np.split(z, np.flatnonzero(np.diff(z) != 1) + 1)
        run0 = max(runs, key=len)
        items, sec, zoom, exact = g.profile_bigwig(u, int(run0[0]) + 1, len(run0))
        assert exact and len(items) == 0 and len(sec) == 0


def test_bigwig_misaligned_first(gpu_lib):
    capi = gpu_lib
    c = fused_case()
    with capi.Lib(0) as g:
        g.set_params(c["bw"], 1, BG)
        u = load(g, c["length"], c["pos"], c["cnt"])
        for first, levels in ((11, 2), (41, 3), (2, 1), (161, 4)):
            with pytest.raises(capi.UpError) as e:
                g.profile_bigwig(u, first, 1000, n_levels=levels)
            assert e.value.code == UP_E_ARG, (first, levels)
        for bad in (dict(first=0, count=10), dict(first=1, count=0), dict(first=1, count=10, n_levels=11),
                    dict(first=1, count=10, n_levels=1, reduction0=0)):
            with pytest.raises(capi.UpError):
                g.profile_bigwig(u, **bad)
        # the same firsts with fewer levels are fine
        for first, levels in ((11, 1), (41, 2), (2, 0), (161, 3)):
            assert g.profile_bigwig(u, first, 1000, n_levels=levels)[3]


def test_bigwig_wide_profile_one_strand(gpu_lib):
    rng = np.random.default_rng(5102)
    length, bw = 40_000, 700
    pos, cnt = random_unit(rng, length, bw, lo=bw + 1, hi=length)
    pos, cnt = with_tag(pos, cnt, length, 1)
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, pos, cnt)
        f, r = g.profile_range(u, 1, length + bw)
        assert not r.any() and f[length:].any()
        for negate in (False, True):
            starts, _, _, _ = check_call(g, u, f, r, 1, length + bw, negate, length, n_levels=5)
            assert starts[-1] == length - 1 and len(starts) > 10_000


def test_bigwig_wide_profile_two_strands(gpu_lib):
    rng = np.random.default_rng(5103)
    length, bw = 40_000, 700
    pf, cf = random_unit(rng, length, bw, lo=bw + 1, hi=length)
    pr, cr = random_unit(rng, length, bw, lo=bw + 1, hi=length)
    pr, cr = with_tag(pr, cr, length, 1)
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG, nondir=True)
        g.set_wide_nd_full(True)
        u = load(g, length, pf, cf, 0)
        scatter(g, u, pr, cr, 1)
        f, r = g.profile_range(u, 1, length + bw)
        assert f.any() and r.any()
        check_call(g, u, f, r, 1, length + bw, False, length, n_levels=5)
        check_call(g, u, f, r, 2561, 20_000, False, length, n_levels=5)


def test_bigwig_refusal_by_limit(gpu_lib, monkeypatch):
    c = fused_case()
    bw, length = c["bw"], c["length"]
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, c["pos"], c["cnt"])
        f, r = g.profile_range(u, 1, length + bw)
    s = f + r
    limit = float(s.max())
    assert np.count_nonzero(s >= limit) == 1  # exactly one score crosses it
    at = int(np.argmax(s)) + 1
    monkeypatch.setenv("UNIPEAK_PROFILE_TEXT_LIMIT", repr(limit))
    with gpu_lib.Lib(0) as g:  # (read at up_open)
        g.set_params(bw, 1, BG)
        u = load(g, length, c["pos"], c["cnt"])
        items, sec, zoom, exact = g.profile_bigwig(u, 1, length + bw, n_levels=3)
        assert not exact and items is None and sec is None and zoom is None
        assert not g.profile_bigwig(u, at, 1)[3]
        check_call(g, u, f, r, 1, at - 1, False, length, n_levels=2)  # the ranges on both sides of it
        first = (at // 160 + 1) * 160 + 1
        assert 1 < at and first <= length
        check_call(g, u, f, r, first, length + bw - first + 1, False, length, n_levels=3)


def test_bigwig_scores_below_1e_17(gpu_lib):
    """scores the digit routine formats but whose text is below 1e-17: refused"""
    c = fused_case()
    with gpu_lib.Lib(0) as g:
        g.set_params(c["bw"], 1, 1.5e16)
        u = load(g, c["length"], c["pos"], c["cnt"])
        f, r = g.profile_range(u, 1, 20_000)
        s = (f + r)[f + r != 0]
        assert s.size > 1000 and s.min() >= 2.0 ** -67 and s.min() < 9e-18
        text, _, _, exact_text = g.profile_text(u, 1, 20_000)
        assert exact_text  # the text path formats them
        assert not g.profile_bigwig(u, 1, 20_000)[3]


# ---- bin/regions -W against bin/regions -w | bin/wigs2bigwigs

TIMING = re.compile(r"\[timing\] bigwig: device (\d+) items, host (\d+) items, fallback chunks (\d+) of (\d+), "
                    r"sections (\d+)")


def total_summary(path):
    b = open(path, "rb").read()
    off, = struct.unpack_from("<Q", b, 44)
    return struct.unpack_from("<Qdddd", b, off)


def sections_of(path):
    """[(chrom id, start, end, item starts)] of every data section, in R-tree order, after
    checking that its leaf covers it"""
    b = open(path, "rb").read()
    index, = struct.unpack_from("<Q", b, 24)
    out = []

    def walk(off):
        leaf, _, cnt = struct.unpack_from("<BBH", b, off)
        off += 4
        for _ in range(cnt):
            if leaf:
                c0, s0, c1, s1, doff, dsize = struct.unpack_from("<IIIIQQ", b, off)
                raw = zlib.decompress(b[doff:doff + dsize])
                cid, cs, ce, step, span, typ, _, n = struct.unpack_from("<IIIIIBBH", raw, 0)
                assert typ == 2 and span == 1 and len(raw) == 24 + 8 * n
                st = np.frombuffer(raw, "<u4", offset=24).reshape(n, 2)[:, 0]
                assert c0 == c1 == cid and s0 <= cs == st[0] and st[-1] + 1 == ce <= s1
                out.append((cid, cs, ce, st))
                off += 32
            else:
                walk(struct.unpack_from("<IIIIQ", b, off)[4])
                off += 24
    walk(index + 48)
    return out


def keyed(items):
    return [(s, e, struct.pack("<f", v)) for s, e, v in items]


def compare_track(old, new, max_levels=10):
    """new: a file of regions -W; old: wigs2bigwigs's of the same track"""
    a, ca, _ = read_bigwig(old)
    b, cb, zl = read_bigwig(new)
    assert ca == cb  # the chromosome tree: ids, names, sizes
    assert list(a) == list(b)
    n = 0
    for c in a:
        assert keyed(a[c]) == keyed(b[c]), c
        n += len(a[c])
    assert n > 1000
    ta, tb = total_summary(old), total_summary(new)
    assert ta[:3] == tb[:3] and ta[0] == n
    check_sums(tb[3], ta[3], "total sum")
    check_sums(tb[4], ta[4], "total sumsq")
    # sections: at most 1,024 items, sorted, in (chromosome, start) order without overlap
    last = (-1, 0)
    for cid, cs, ce, st in sections_of(new):
        assert len(st) <= 1024 and np.all(np.diff(st.astype(np.int64)) >= 0)
        assert (cid, cs) >= last
        last = (cid, ce)
    # zoom levels on the fixed grid, each with fewer records than the one before
    cid = {name: i for i, (name, _) in cb.items()}
    assert 1 <= len(zl) <= max_levels
    prev = n
    for k, (red, recs) in enumerate(zl):
        assert red == 10 * 4 ** k
        assert len(recs) < prev
        prev = len(recs)
        rec = np.array(recs, dtype=[("chrom", "<u4"), ("start", "<u4"), ("end", "<u4"), ("valid", "<u4"),
                                    ("vmin", "<f4"), ("vmax", "<f4"), ("sum", "<f4"), ("sumsq", "<f4")])
        assert np.all(np.diff(rec["chrom"].astype(np.int64)) >= 0)
        for c in b:
            it = b[c]
            starts = np.array([s for s, _, _ in it], np.uint32)
            vals = np.array([v for _, _, v in it], np.float32)
            check_zoom(rec[rec["chrom"] == cid[c]], starts, vals, red, cb[cid[c]][1], cid[c])
    return n, len(zl)


def regions_pair(tmp_path, monkeypatch, args, files, ct, tracks, env=None, max_levels=10):
    """bin/regions -w then bin/wigs2bigwigs in old/, bin/regions -W in new/ (with env);
    every track compared; the -W run's [timing] bigwig figures"""
    common = ["-q", "-c", ct] + args
    for d in ("old", "new"):
        (tmp_path / d).mkdir()
    run([os.path.join(BIN, "regions")] + common + ["-w", "old/p.wig", "-o", "old/r.txt"] + files, tmp_path)
    run([os.path.join(BIN, "wigs2bigwigs"), "--sizes", ct, "old/p.wig"], tmp_path)
    monkeypatch.setenv("UNIPEAK_TIMING", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    r = run([os.path.join(BIN, "regions")] + common + ["-W", "new/p", "-o", "new/r.txt"] + files, tmp_path)
    assert (tmp_path / "old/r.txt").read_bytes() == (tmp_path / "new/r.txt").read_bytes()
    assert sorted(p.name for p in (tmp_path / "new").glob("*.bw")) == sorted(f"p{t}.bw" for t in tracks)
    got = [compare_track(tmp_path / f"old/p{t}.bw", tmp_path / f"new/p{t}.bw", max_levels) for t in tracks]
    return [int(v) for v in TIMING.search(r.stderr).groups()], got


NAME_ORDER = [("chr2", 60_000), ("chr10", 45_000)]  # chr10 comes first in a bigWig

CLI_CASES = [
    ("directional_name_order", NAME_ORDER, 1, ["-f"], {}, ["+", "-"], {}),
    ("nondir_two_samples", HG_LIKE, 2, ["-D", "-y"], {"shift_rev": 100}, [""], {}),
    ("bw_700", [("chrA", 200_000), ("chrB", 90_000)], 1, ["-f", "-b", "700", "-k", "0"],
     {"lo": 2500, "n_cl": 12, "sd": 200}, ["+", "-"], {}),
    ("small_chunks", NAME_ORDER, 1, ["-f"], {}, ["+", "-"], {"UNIPEAK_BIGWIG_CHUNK": "10240"}),
]


@pytest.mark.parametrize("case", CLI_CASES, ids=lambda c: c[0])
def test_regions_cli_bigwig(gpu_lib, tmp_path, monkeypatch, case):
    name, contigs, ns, args, kw, tracks, env = case
    ct, files = make_inputs(tmp_path, 5200 + len(name), contigs, ns, **kw)
    st, got = regions_pair(tmp_path, monkeypatch, args, files, ct, tracks, env, 6 if env else 10)
    assert st[0] > 0 and st[1] == 0 and st[2] == 0  # every item from the device
    assert st[0] == sum(n for n, _ in got)
    if env:  # 10,240 positions a chunk: six levels at most, several chunks per unit
        assert st[3] >= sum(-(-size // 10240) for _, size in contigs) * len(tracks)
    if name == "directional_name_order":
        _, chroms, _ = read_bigwig(tmp_path / "new/p+.bw")
        assert chroms == {0: ("chr10", 45_000), 1: ("chr2", 60_000)}


def test_regions_cli_bigwig_shift_75_heads(gpu_lib, tmp_path, monkeypatch):
    """tags at positions <= bw after the shift: every unit is a head unit (quirk Q1), its
    replayed entries are the first sections and the resync chunk is cut on the host"""
    rng = np.random.default_rng(5300)
    write_contigs(tmp_path / "contigs.txt", HG_LIKE)
    fwd, rev = gen_sample(rng, HG_LIKE)
    for c, _ in HG_LIKE:
        fwd[c] = sorted(fwd[c] + [(5, 2), (30, 1)])
        rev[c] = sorted(rev[c] + [(80, 2), (100, 1), (120, 3)])
    write_wig(tmp_path / "s0.wig", "s0", fwd, rev)
    st, _ = regions_pair(tmp_path, monkeypatch, ["-D", "-s", "75"], ["s0.wig"], str(tmp_path / "contigs.txt"), [""],
                         {"UNIPEAK_BIGWIG_CHUNK": "10240"}, 6)
    assert st[1] > 0 and st[0] > 0 and st[2] == 0


def test_regions_cli_bigwig_fallback_chunk(gpu_lib, tmp_path, monkeypatch):
    ct, files = make_inputs(tmp_path, 5301, HG_LIKE, 1)
    # a limit between the two largest scores of a first -w run: a text is within 5e-7 of its
    # score, so texts 1e-5 apart have the midpoint strictly between their scores
    run([os.path.join(BIN, "regions"), "-q", "-c", ct, "-f", "-w", "first.wig", "-o", "first.txt"] + files, tmp_path)
    v = sorted({abs(float(l.split()[1])) for l in open(tmp_path / "first.wig") if l[:1].isdigit()})
    assert v[-2] * (1 + 1e-5) < v[-1]
    env = {"UNIPEAK_BIGWIG_CHUNK": "10240", "UNIPEAK_PROFILE_TEXT_LIMIT": repr((v[-2] + v[-1]) / 2)}
    st, _ = regions_pair(tmp_path, monkeypatch, ["-f"], files, ct, ["+", "-"], env, 6)
    assert 1 <= st[2] <= 2 and st[2] < st[3]
    assert st[0] > 0 and st[1] > 0


def test_regions_cli_bigwig_with_wig_in_one_pass(gpu_lib, tmp_path):
    ct, files = make_inputs(tmp_path, 5302, NAME_ORDER, 1)
    common = [os.path.join(BIN, "regions"), "-q", "-c", ct, "-f"]
    for d in ("a", "b", "c"):
        (tmp_path / d).mkdir()
    run(common + ["-w", "a/p.wig", "-o", "a/r.txt"] + files, tmp_path)
    run(common + ["-W", "b/p", "-o", "b/r.txt"] + files, tmp_path)
    run(common + ["-w", "c/p.wig", "--bigwig", "c/p", "-o", "c/r.txt"] + files, tmp_path)
    assert (tmp_path / "a/p.wig").read_bytes() == (tmp_path / "c/p.wig").read_bytes()
    assert (tmp_path / "a/r.txt").read_bytes() == (tmp_path / "b/r.txt").read_bytes() == \
        (tmp_path / "c/r.txt").read_bytes()
    for t in "+-":
        assert (tmp_path / f"b/p{t}.bw").read_bytes() == (tmp_path / f"c/p{t}.bw").read_bytes()
    assert not list((tmp_path / "a").glob("*.bw")) and not (tmp_path / "b/p.wig").exists()


def test_regions_cli_bigwig_repeated_contig(gpu_lib, tmp_path):
    """chrA's forward records come in two runs with chrB's between them: two units of
    the forward track hold chrA"""
    write_contigs(tmp_path / "contigs.txt", [("chrA", 50_000), ("chrB", 40_000)])
    rng = np.random.default_rng(5303)
    with open(tmp_path / "s0.wig", "w") as f:
        lines = []
        for c, lo, hi in (("chrA", 1000, 20_000), ("chrB", 1000, 30_000), ("chrA", 25_000, 45_000)):
            lines.append(f"variableStep chrom={c}\n")
            for p in np.unique(rng.integers(lo, hi, 300)):
                lines.append(f"{p} {int(rng.integers(1, 4))}\n")
        f.write("# original_file=synthetic\n# tags=%d\n" % sum(int(l.split()[1]) for l in lines if l[0].isdigit()))
        f.write('track name="s0 +" description="s0" priority=3 visibility=full type=wiggle_0 alwaysZero=on '
                'color=0,0,255\n')
        f.writelines(lines)
    cmd = [os.path.join(BIN, "regions"), "-q", "-c", "contigs.txt", "-f", "-o", "r.txt", "s0.wig"]
    run(cmd, tmp_path)  # fine without -W
    r = subprocess.run(cmd + ["-W", "q"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 1
    assert any(l.startswith("error: ") and "chrA" in l for l in r.stderr.split("\n")), r.stderr
