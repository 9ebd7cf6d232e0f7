"""The -w lines formatted on the device (csrc/proftext.hip behind
up_unit_profile_text) and bin/regions -w through them.

The reference is always the text built here from Lib.profile_range's scores:
"<pos> <'%g' % (f + r)>\\n" for every position whose f + r is not 0 ('%g' is
pinned to libc's in test_format_g6.py) -- never anything the text path made.
A text workgroup owns 1,024 positions, a K1 strip 16,384."""
import gzip
import os
import re

import numpy as np
import pytest

from tests.gen import random_unit
from tests.test_cli import BIN, HG_LIKE, gen_sample, make_inputs, run
from tests.wig import write_contigs, write_wig

pytestmark = pytest.mark.gpu

BG = 0.003
UP_E_UNSUPPORTED = -5


def ref_text(f, r, first, negate=False):
    s = f + r
    sign = b"-" if negate else b""
    return b"".join(b"%d %s%s\n" % (first + int(i), sign, b"%g" % float(s[i])) for i in np.flatnonzero(s))


def ref_offsets(f, r, first, negate, cuts):
    """bytes of the reference lines at positions < each cut"""
    s = f + r
    sign = 1 if negate else 0
    lens = np.zeros(len(s) + 1, np.int64)
    for i in np.flatnonzero(s):
        lens[i + 1] = len(b"%d " % (first + int(i))) + sign + len(b"%g" % float(s[i])) + 1
    pre = np.cumsum(lens)
    return np.array([pre[int(c) - first] for c in cuts], np.uint64)


def with_tag(pos, cnt, p, c=1):
    """the unit with c more tags of sample 0 at position p"""
    d = {int(a): b.copy() for a, b in zip(pos, cnt)}
    d.setdefault(p, np.zeros(cnt.shape[1], np.uint32))[0] += c
    ks = sorted(d)
    return np.array(ks, np.uint32), np.array([d[k] for k in ks], np.uint32).reshape(len(ks), cnt.shape[1])


def load(g, length, pos, cnt, strand=0):
    u = g.add_unit(length)
    scatter(g, u, pos, cnt, strand)
    return u


def scatter(g, u, pos, cnt, strand=0):
    for s in range(cnt.shape[1]):
        m = cnt[:, s] != 0
        if m.any():
            g.scatter(u, strand, s, pos[m], cnt[m, s])


_fused = {}


def fused_case():
    """bw 50, one directional sample, 70,000 positions (more than 4 strips), a
    tag at 10,000 so that lines sit on both sides of the 4 -> 5 digit change,
    one at the contig's end"""
    if not _fused:
        rng = np.random.default_rng(4100)
        length, bw = 70_000, 50
        pos, cnt = random_unit(rng, length, bw, lo=bw + 1, hi=length)
        pos, cnt = with_tag(pos, cnt, 10_000, 2)
        pos, cnt = with_tag(pos, cnt, length, 1)  # the flush's positions up to len + bw hold scores
        _fused.update(length=length, bw=bw, pos=pos, cnt=cnt)
    return _fused


def check_whole(g, u, n, must):
    """both signs over [1, n] against the dense scores; `must`: byte strings the
    reference text has to contain for the case to test what it is for"""
    f, r = g.profile_range(u, 1, n)
    for negate in (False, True):
        want = ref_text(f, r, 1, negate)
        for m in must:
            assert negate or m in want, m
        got, _, nl, exact = g.profile_text(u, 1, n, negate=negate)
        assert exact
        assert nl == np.count_nonzero(f + r)
        assert got == want, "differs at byte %d" % next(
            (i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    assert g.profile_text_ms() > 0
    return f, r


def test_text_fused_k1(gpu_lib):
    c = fused_case()
    with gpu_lib.Lib(0) as g:
        g.set_params(c["bw"], 1, BG)
        u = load(g, c["length"], c["pos"], c["cnt"])
        f, _ = check_whole(g, u, c["length"] + c["bw"], [b"\n9999 ", b"\n10000 ", b"\n70049 "])
        assert np.count_nonzero(f) > 20_000


def test_text_two_strands_coefficients(gpu_lib):
    rng = np.random.default_rng(4101)
    length, bw = 40_000, 50
    pf, cf = random_unit(rng, length, bw, S=2, lo=bw + 1, hi=length)
    pr, cr = random_unit(rng, length, bw, S=2, lo=bw + 1, hi=length)
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 2, BG, nondir=True, coeffs=[0.6, 1.7])
        u = load(g, length, pf, cf, 0)
        scatter(g, u, pr, cr, 1)
        f, r = check_whole(g, u, length + bw, [b"\n30000 ", b"."])
        assert np.count_nonzero(f) > 1000 and np.count_nonzero(r) > 1000
        assert np.count_nonzero((f != 0) & (r != 0)) > 1000  # lines that are a sum of both


def test_text_wide_profile_one_strand(gpu_lib):
    rng = np.random.default_rng(4102)
    length, bw = 40_000, 600
    pos, cnt = random_unit(rng, length, bw, lo=bw + 1, hi=length)
    pos, cnt = with_tag(pos, cnt, length, 1)  # scores up to len + bw - 1
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, pos, cnt)
        _, r = check_whole(g, u, length + bw, [b"\n40599 "])
        assert not r.any()


def test_text_wide_profile_two_strands(gpu_lib):
    rng = np.random.default_rng(4103)
    length, bw = 40_000, 600
    pf, cf = random_unit(rng, length, bw, lo=bw + 1, hi=length)
    pr, cr = random_unit(rng, length, bw, lo=bw + 1, hi=length)
    pr, cr = with_tag(pr, cr, length, 1)  # scores up to len + bw - 1
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG, nondir=True)
        g.set_wide_nd_full(True)
        u = load(g, length, pf, cf, 0)
        scatter(g, u, pr, cr, 1)
        f, r = check_whole(g, u, length + bw, [b"\n40599 "])
        assert f.any() and r.any()


def test_text_scientific_small(gpu_lib):
    """bw 6000: the weights next to the kernel's edge are below 1e-4 of its
    centre's, so lone tags give scores that print as e-05 and smaller"""
    length, bw = 80_000, 6000
    pos = np.array([7000, 7001, 30_000, 55_000, 79_990], np.uint32)
    cnt = np.array([[1], [2], [1], [3], [1]], np.uint32)
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, 0.05)
        u = load(g, length, pos, cnt)
        f, _ = check_whole(g, u, length + bw, [b"e-05\n", b"e-06\n", b"e-07\n", b" 0.0", b"\n85989 "])
        assert np.count_nonzero(f) > 40_000


def test_text_scientific_large(gpu_lib):
    """counts of 100,000 (the overflow table) side by side: scores of 1e6 and more"""
    rng = np.random.default_rng(4105)
    length, bw = 40_000, 50
    pos, cnt = random_unit(rng, length, bw, lo=bw + 1, hi=length)
    for p in (20_000, 20_001, 20_002, 20_003, 33_333):
        pos, cnt = with_tag(pos, cnt, p, 100_000)
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, pos, cnt)
        check_whole(g, u, length + bw, [b"e+06\n", b"\n20000 ", b"."])


def test_cuts(gpu_lib):
    c = fused_case()
    first, count = 1, c["length"] + c["bw"]
    rng = np.random.default_rng(4106)
    with gpu_lib.Lib(0) as g:
        g.set_params(c["bw"], 1, BG)
        u = load(g, c["length"], c["pos"], c["cnt"])
        f, r = g.profile_range(u, first, count)
        s = f + r
        zeros = rng.choice(np.flatnonzero(s == 0), 40, replace=False) + first  # positions without a line
        rnd = rng.integers(first, first + count + 1, 146)
        cuts = np.sort(np.concatenate([[first, first, first + count, first + count, 1024, 1025, 16_384, 16_385],
                                       zeros, rnd, rnd[:6]])).astype(np.uint64)  # (repeats)
        assert cuts.size == 200 and cuts[0] == first and cuts[-1] == first + count
        for negate in (False, True):
            text, off, _, exact = g.profile_text(u, first, count, negate=negate, cuts=cuts)
            assert exact and text == ref_text(f, r, first, negate)
            assert np.array_equal(off, ref_offsets(f, r, first, negate, cuts))
            assert off[-1] == len(text)


def test_ranges(gpu_lib):
    c = fused_case()
    length, bw = c["length"], c["bw"]
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, c["pos"], c["cnt"])
        f, r = g.profile_range(u, 1, length + bw)
        s = f + r

        def one(first, count, cuts=None):
            got = g.profile_text(u, first, count, cuts=cuts)
            assert got[3]
            assert got[0] == ref_text(f[first - 1:first - 1 + count], r[first - 1:first - 1 + count], first)
            return got

        nz = int(np.flatnonzero(s)[777]) + 1  # a position with a line
        first = nz if nz % 64 else nz + 1
        assert first % 64 and s[first - 1] != 0
        text, _, nl, _ = one(first, 1)
        assert nl == 1 and text.count(b"\n") == 1
        # inside an all-zero stretch
        z = np.flatnonzero(s == 0)
        runs = np.split(z, np.flatnonzero(np.diff(z) != 1) + 1)
        run0 = max(runs, key=len)
        assert len(run0) > 100
        text, off, nl, exact = g.profile_text(u, int(run0[3]) + 1, len(run0) - 6, cuts=[int(run0[10]) + 1])
        assert exact and nl == 0 and off[0] == 0 and not text
        # ending at len + bw, across a workgroup and a strip edge
        assert c["pos"][-1] == length and s[length:].any()
        one(length - 3000, bw + 3001)
        one(16_000, 1_500)
        # two calls that meet, at a position off every boundary
        a = one(20_001, 4_567)[0]
        b = one(24_568, 3_333)[0]
        assert a + b == one(20_001, 7_900)[0] and a and b


def test_range_over_six_digit_positions(gpu_lib):
    rng = np.random.default_rng(4108)
    length, bw = 120_000, 50
    pos, cnt = random_unit(rng, length, bw, lo=90_000, hi=length)
    pos, cnt = with_tag(pos, cnt, 100_000, 3)
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, pos, cnt)
        first, count = 99_000, 2_000
        f, r = g.profile_range(u, first, count)
        want = ref_text(f, r, first)
        assert b"\n99999 " in want and b"\n100000 " in want
        cuts = [99_999, 100_000, 100_001]
        text, off, _, exact = g.profile_text(u, first, count, cuts=cuts)
        assert exact and text == want
        assert np.array_equal(off, ref_offsets(f, r, first, False, cuts))


def test_scores_below_the_range(gpu_lib):
    c = fused_case()
    with gpu_lib.Lib(0) as g:
        g.set_params(c["bw"], 1, 1e30)
        u = load(g, c["length"], c["pos"], c["cnt"])
        f, r = g.profile_range(u, 1, 20_000)
        s = (f + r)[f + r != 0]
        assert s.size > 1000 and np.abs(s).max() < 2.0 ** -67
        text, _, nl, exact = g.profile_text(u, 1, 20_000)
        assert not exact and text is None and nl == 0


def test_limit_flags_only_ranges_above_it(gpu_lib, monkeypatch):
    c = fused_case()
    bw, length = c["bw"], c["length"]
    with gpu_lib.Lib(0) as g:
        g.set_params(bw, 1, BG)
        u = load(g, length, c["pos"], c["cnt"])
        f, r = g.profile_range(u, 1, length + bw)
    s = f + r
    limit = float(np.sort(s[s != 0])[-200])  # between the smallest and the largest nonzero score
    big = np.flatnonzero(s >= limit)
    gaps = np.flatnonzero(np.diff(big) > 3000)
    assert gaps.size, "needs a stretch of 3,000 positions without a score at the limit"
    lo = int(big[gaps[0]]) + 2  # positions lo .. lo + 2,999 hold no score >= limit
    assert s[lo - 1:lo + 2999].any() and s[lo - 1:lo + 2999].max() < limit
    monkeypatch.setenv("UNIPEAK_PROFILE_TEXT_LIMIT", repr(limit))
    with gpu_lib.Lib(0) as g:  # (read at up_open)
        g.set_params(bw, 1, BG)
        u = load(g, length, c["pos"], c["cnt"])
        text, _, _, exact = g.profile_text(u, lo, 3000)
        assert exact and text == ref_text(f[lo - 1:lo + 2999], r[lo - 1:lo + 2999], lo)
        # one position further down: the score equal to the limit is inside
        text, _, _, exact = g.profile_text(u, lo - 1, 3000)
        assert not exact and text is None
        text, _, _, exact = g.profile_text(u, 1, length + bw)
        assert not exact and text is None


def test_refusals(gpu_lib):
    capi = gpu_lib
    c = fused_case()
    with capi.Lib(0) as g:
        g.set_params(40_000, 1, BG)  # the replay of every unit
        u = load(g, c["length"], c["pos"], c["cnt"])
        with pytest.raises(capi.UpError) as e1:
            g.profile_range(u, 1, 100)
        with pytest.raises(capi.UpError) as e2:
            g.profile_text(u, 1, 100)
        assert e1.value.code == e2.value.code == UP_E_UNSUPPORTED
    with capi.Lib(0) as g:
        g.set_params(600, 1, BG, nondir=True)  # without set_wide_nd_full
        u = load(g, c["length"], c["pos"], c["cnt"])
        with pytest.raises(capi.UpError) as e1:
            g.profile_range(u, 1, 100)
        with pytest.raises(capi.UpError) as e2:
            g.profile_text(u, 1, 100)
        assert e1.value.code == e2.value.code
    with capi.Lib(0) as g:
        g.set_params(50, 1, BG)
        u = load(g, c["length"], c["pos"], c["cnt"])
        for bad in (dict(first=0, count=10), dict(first=1, count=0), dict(first=1, count=10, cuts=[12]),
                    dict(first=5, count=10, cuts=[4]), dict(first=1, count=10, cuts=[3, 2])):
            with pytest.raises(capi.UpError):
                g.profile_text(u, **bad)


# ---- bin/regions -w through the text path, byte for byte against the oracle CLI

TIMING = re.compile(r"\[timing\] profile text: device (\d+) bytes (\d+) lines, host (\d+) lines, "
                    r"fallback chunks (\d+) of (\d+)")


def write_alternating_wig(path, name, fwd, rev):
    """both strands of every contig merged by position, a track header at every
    change of strand: the driver's adds alternate between the two buffers"""
    total = sum(c for d in (fwd, rev) for v in d.values() for _, c in v)
    hdr = {True: f'track name="{name} +" description="{name}" priority=3 visibility=full '
                 'type=wiggle_0 alwaysZero=on color=0,0,255\n',
           False: f'track name="{name} -" description=" " priority=3 visibility=full '
                  'type=wiggle_0 alwaysZero=on color=255,0,0 altColor=255,0,0\n'}
    with open(path, "w") as f:
        f.write("# original_file=synthetic\n")
        f.write(f"# tags={total}\n")
        for c in fwd:
            recs = sorted([(p, 0, k) for p, k in fwd[c]] + [(p, 1, k) for p, k in rev.get(c, [])])
            last = None
            for p, st, k in recs:
                if st != last:
                    f.write(hdr[st == 0])
                    f.write(f"variableStep chrom={c}\n")
                    last = st
                f.write(f"{p} {'-' if st else ''}{k}\n")


def regions_w(orc_bin, tmp_path, monkeypatch, args, files, ct, out="p.wig", limit_from_ref=False):
    """oracle, default path and UNIPEAK_PROFILE_TEXT=0: (reference bytes, stats of
    the default run); every file compared whole"""
    common = ["-q", "-c", ct] + args
    for d in ("ref", "got", "host"):
        (tmp_path / d).mkdir()
    monkeypatch.setenv("UNIPEAK_PROFILE_TEXT_CHUNK", "16384")
    monkeypatch.setenv("UNIPEAK_TIMING", "1")
    run([orc_bin, "regions"] + common + ["-w", f"ref/{out}", "-o", "ref/r.txt"] + files, tmp_path)
    a = (tmp_path / "ref" / out).read_bytes()
    if limit_from_ref:  # a limit that some chunks' scores reach and some do not
        peak, key = {}, None
        for line in a.decode().split("\n"):
            if line.startswith("track"):
                strand = line.split('"')[1][-1]
            elif line.startswith("variableStep"):
                key = (strand, line.split("chrom=")[1])
            elif line and not line.startswith("#"):
                p, v = line.split(" ")
                k = key + ((int(p) - 1) // 16384,)
                peak[k] = max(peak.get(k, 0.0), abs(float(v.replace("--", "-"))))
        m = sorted(peak.values())
        assert len(m) >= 4 and m[len(m) // 2 - 1] * 1.01 < m[len(m) // 2]
        monkeypatch.setenv("UNIPEAK_PROFILE_TEXT_LIMIT", repr((m[len(m) // 2 - 1] + m[len(m) // 2]) / 2))
    r = run([os.path.join(BIN, "regions")] + common + ["-w", f"got/{out}", "-o", "got/r.txt"] + files, tmp_path)
    monkeypatch.setenv("UNIPEAK_PROFILE_TEXT", "0")
    r0 = run([os.path.join(BIN, "regions")] + common + ["-w", f"host/{out}", "-o", "host/r.txt"] + files, tmp_path)
    table = (tmp_path / "ref/r.txt").read_bytes()
    assert table == (tmp_path / "got/r.txt").read_bytes() == (tmp_path / "host/r.txt").read_bytes()
    b, h = (tmp_path / "got" / out).read_bytes(), (tmp_path / "host" / out).read_bytes()
    if out.endswith(".gz"):
        a, b, h = gzip.decompress(a), gzip.decompress(b), gzip.decompress(h)
    assert a.count(b"\n") > 1000
    for name, x in (("device text", b), ("host", h)):
        assert a == x, "%s profile differs at byte %d" % (name, next(
            (i for i, (p, q) in enumerate(zip(a, x)) if p != q), min(len(a), len(x))))
    st = [int(v) for v in TIMING.search(r.stderr).groups()]
    st0 = [int(v) for v in TIMING.search(r0.stderr).groups()]
    assert st[1] > 0 and st[0] > 0  # the device formatted lines
    assert st0[0] == 0 and st0[1] == 0 and st0[2] == sum(
        1 for l in a.split(b"\n") if l[:1].isdigit())  # UNIPEAK_PROFILE_TEXT=0: every line on the host
    # (the device formats whole chunks: lines below a head unit's resync point are counted
    # there although the replayed entries are what is written for them)
    assert st[1] + st[2] >= st0[2]
    return a, st


CLI_CASES = [
    ("strand_sorted", HG_LIKE, 1, ["-f"], {}, "p.wig"),
    ("nondir_two_samples", HG_LIKE, 2, ["-D", "-y"], {"shift_rev": 100}, "p.wig"),
    ("nondir_shift_75_heads", HG_LIKE, 1, ["-D", "-s", "75"], {"low": True}, "p.wig"),
    ("bw_600", [("chrA", 200_000), ("chrB", 90_000)], 1, ["-f", "-b", "600", "-k", "0"],
     {"lo": 2100, "n_cl": 12, "sd": 200}, "p.wig"),
    ("gz", HG_LIKE, 1, ["-f"], {}, "p.wig.gz"),
]


@pytest.mark.parametrize("case", CLI_CASES, ids=lambda c: c[0])
def test_regions_cli_text_path(orc_bin, gpu_lib, tmp_path, monkeypatch, case):
    name, contigs, ns, args, kw, out = case
    if kw.get("low"):  # tags at positions <= bw after the shift: every unit is a head unit (quirk Q1)
        rng = np.random.default_rng(4200 + len(name))
        write_contigs(tmp_path / "contigs.txt", contigs)
        fwd, rev = gen_sample(rng, contigs)
        for c, _ in contigs:
            fwd[c] = sorted(fwd[c] + [(5, 2), (30, 1)])
            rev[c] = sorted(rev[c] + [(80, 2), (100, 1), (120, 3)])
        write_wig(tmp_path / "s0.wig", "s0", fwd, rev)
        ct, files = str(tmp_path / "contigs.txt"), ["s0.wig"]
    else:
        ct, files = make_inputs(tmp_path, 4200 + len(name), contigs, ns, **kw)
    a, st = regions_w(orc_bin, tmp_path, monkeypatch, args, files, ct, out)
    assert st[3] == 0 and st[4] > 3  # several chunks, none fell back
    if name == "nondir_shift_75_heads":
        assert st[2] > 0  # replayed entries between the slices


def test_regions_cli_text_path_alternating_strands(orc_bin, gpu_lib, tmp_path, monkeypatch):
    contigs = [("chrX", 80_000)]
    rng = np.random.default_rng(4300)
    ct = tmp_path / "contigs.txt"
    write_contigs(ct, contigs)
    fwd, rev = gen_sample(rng, contigs)
    write_alternating_wig(tmp_path / "s0.wig", "s0", fwd, rev)
    a, st = regions_w(orc_bin, tmp_path, monkeypatch, ["-f"], ["s0.wig"], str(ct))
    assert a.count(b"track") > 100  # a header at every switch of buffer: one slice per add
    assert st[3] == 0


def test_regions_cli_text_path_with_fallback_chunks(orc_bin, gpu_lib, tmp_path, monkeypatch):
    ct, files = make_inputs(tmp_path, 4301, HG_LIKE, 1)
    a, st = regions_w(orc_bin, tmp_path, monkeypatch, ["-f"], files, ct, limit_from_ref=True)
    assert 1 <= st[3] <= st[4] - 1
    assert st[1] > 0 and st[2] > 0
