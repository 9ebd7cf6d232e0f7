"""".gz" outputs of the CLIs through the device's DEFLATE encoder (host/gzdev.cpp), and
regions -W with UNIPEAK_BIGWIG_DEFLATE=device: what inflates from the files must be
the bytes the plain outputs hold; only the framing (members, which path wrote them) is
looked at beyond that."""
import gzip
import os
import re
import struct
import zlib

import numpy as np
import pytest

from tests.test_bigwig import read_bigwig
from tests.test_cli import BIN, HG_LIKE, gen_sample, make_inputs, run
from tests.test_gpu_bigwig import keyed, sections_of, total_summary
from tests.test_gpu_convert import rand_aligns, write_bed
from tests.wig import write_contigs, write_wig

pytestmark = pytest.mark.gpu

GZ_LINE = re.compile(r"\[timing\] gz (\S+) in (\d+) B out (\d+) B members (\d+) device ([0-9.]+) ms path (\w+)")
BLOCK = 65536


def members(path):
    """the decompressed pieces of a multi-member gzip file, one per member"""
    raw, out = open(path, "rb").read(), []
    while raw:
        d = zlib.decompressobj(wbits=31)
        out.append(d.decompress(raw))
        assert d.eof
        raw = d.unused_data
    return out


def gz_lines(stderr):
    return {os.path.basename(m.group(1)): (int(m.group(2)), int(m.group(3)), int(m.group(4)), float(m.group(5)),
                                          m.group(6)) for m in GZ_LINE.finditer(stderr)}


def env_with(monkeypatch, **kw):
    monkeypatch.setenv("UNIPEAK_TIMING", "1")
    for k in ("UNIPEAK_GZ_BATCH", "UNIPEAK_GZ_DEVICE", "UNIPEAK_BIGWIG_DEFLATE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in kw.items():
        monkeypatch.setenv(k, str(v))


def head_inputs(tmp_path):
    """tags at positions <= bw after -s 75: head units, whose lines the host replays"""
    rng = np.random.default_rng(5300)
    write_contigs(tmp_path / "contigs.txt", HG_LIKE)
    fwd, rev = gen_sample(rng, HG_LIKE)
    for c, _ in HG_LIKE:
        fwd[c] = sorted(fwd[c] + [(5, 2), (30, 1)])
        rev[c] = sorted(rev[c] + [(80, 2), (100, 1), (120, 3)])
    write_wig(tmp_path / "s0.wig", "s0", fwd, rev)
    return str(tmp_path / "contigs.txt"), [str(tmp_path / "s0.wig")]


PROFILE_CASES = [("directional", ["-f"]), ("nondir", ["-f", "-D"]), ("shift_75_heads", ["-f", "-D", "-s", "75"])]


@pytest.mark.parametrize("case", PROFILE_CASES, ids=lambda c: c[0])
def test_regions_profile_gz(gpu_lib, tmp_path, monkeypatch, case):
    name, args = case
    if name == "shift_75_heads":
        ct, files = head_inputs(tmp_path)
    else:
        ct, files = make_inputs(tmp_path, 6100 + len(name), HG_LIKE, 1)
    regions = os.path.join(BIN, "regions")
    common = [regions, "-q", "-c", ct, "-n", "trk"] + args  # (a track is named after its file otherwise)
    env_with(monkeypatch)
    run(common + ["-w", "p.wig", "-o", "r.txt"] + files, tmp_path)
    plain = (tmp_path / "p.wig").read_bytes()
    table = (tmp_path / "r.txt").read_bytes()
    assert len(plain) > 3 * BLOCK + 1000, len(plain)  # more than three blocks of text
    for tag, env in (("b1", {"UNIPEAK_GZ_BATCH": BLOCK}), ("b3", {"UNIPEAK_GZ_BATCH": 3 * BLOCK}), ("def", {}),
                     ("zlib", {"UNIPEAK_GZ_DEVICE": 0})):
        env_with(monkeypatch, **env)
        out = f"p_{tag}.wig.gz"
        r = run(common + ["-w", out, "-o", f"r_{tag}.txt"] + files, tmp_path)
        assert (tmp_path / f"r_{tag}.txt").read_bytes() == table
        assert gzip.decompress((tmp_path / out).read_bytes()) == plain
        n_in, n_out, n_mem, ms, path = gz_lines(r.stderr)[out]
        assert n_in == len(plain) and n_out == (tmp_path / out).stat().st_size
        parts = members(tmp_path / out)
        assert b"".join(parts) == plain and len(parts) == n_mem
        if tag in ("b1", "b3"):
            batch = int(env["UNIPEAK_GZ_BATCH"])
            assert path == "device" and ms > 0
            assert [len(p) for p in parts] == [batch] * (len(plain) // batch) + (
                [len(plain) % batch] if len(plain) % batch else [])
            assert len(parts) > 1
        elif tag == "def":  # one batch: the device from 1 MiB on, zlib below
            assert path == ("device" if len(plain) >= (1 << 20) else "zlib") and n_mem == 1
        else:
            assert path == "zlib" and n_mem == 1 and ms == 0


def test_small_table_stays_zlib(gpu_lib, tmp_path, monkeypatch):
    ct, files = make_inputs(tmp_path, 6200, HG_LIKE, 1)
    regions = os.path.join(BIN, "regions")
    env_with(monkeypatch)
    run([regions, "-q", "-c", ct, "-f", "-o", "r.txt"] + files, tmp_path)
    r = run([regions, "-q", "-c", ct, "-f", "-o", "r.txt.gz"] + files, tmp_path)
    plain = (tmp_path / "r.txt").read_bytes()
    assert 0 < len(plain) < (1 << 20)
    got = (tmp_path / "r.txt.gz").read_bytes()
    assert gzip.decompress(got) == plain
    assert gz_lines(r.stderr)["r.txt.gz"][4] == "zlib"
    # and the bytes are the ones the zlib-only writer leaves
    env_with(monkeypatch, UNIPEAK_GZ_DEVICE=0)
    run([regions, "-q", "-c", ct, "-f", "-o", "r0.txt.gz"] + files, tmp_path)
    assert (tmp_path / "r0.txt.gz").read_bytes() == got


def test_convert_align_gz(gpu_lib, tmp_path, monkeypatch):
    table = [("chrA", 30_000), ("chrB", 20_000), ("chrC", 5_000)]
    write_contigs(tmp_path / "ct.txt", table)
    rng = np.random.default_rng(6300)
    write_bed(tmp_path / "a.bed", rand_aligns(rng, 40_000, names=("chrA", "chrB", "chrC")))
    conv = os.path.join(BIN, "convert_align")
    env_with(monkeypatch, UNIPEAK_GZ_BATCH=BLOCK)
    run([conv, "-q", "-c", "ct.txt", "-o", "s.wig", "a.bed"], tmp_path)
    r = run([conv, "-q", "-c", "ct.txt", "-o", "s.wig.gz", "a.bed"], tmp_path)
    plain = (tmp_path / "s.wig").read_bytes()
    assert len(plain) > 2 * BLOCK
    assert gzip.decompress((tmp_path / "s.wig.gz").read_bytes()) == plain
    line = gz_lines(r.stderr)["s.wig.gz"]
    assert line[4] == "device" and line[2] == len(members(tmp_path / "s.wig.gz")) > 1


def test_regions_reads_device_written_gz(gpu_lib, tmp_path, monkeypatch):
    """a multi-member .wig.gz written by the device path is an input like any other"""
    contigs = [("chrA", 400_000), ("chrB", 300_000)]
    ct, files = make_inputs(tmp_path, 6400, contigs, 1)
    conv, regions = os.path.join(BIN, "convert_align"), os.path.join(BIN, "regions")
    env_with(monkeypatch, UNIPEAK_GZ_BATCH=BLOCK)
    run([conv, "-q", "-c", ct, "-o", "s.wig"] + files, tmp_path)
    run([conv, "-q", "-c", ct, "-o", "s.wig.gz"] + files, tmp_path)
    assert len(members(tmp_path / "s.wig.gz")) > 1
    run([regions, "-q", "-c", ct, "-f", "-o", "a.txt", "s.wig"], tmp_path)
    run([regions, "-q", "-c", ct, "-f", "-o", "b.txt", "s.wig.gz"], tmp_path)

    def rows(name):  # (the header names the input file)
        return [ln for ln in (tmp_path / name).read_bytes().split(b"\n") if not ln.startswith(b"#")]
    assert rows("a.txt") == rows("b.txt") and len(rows("a.txt")) > 10


@pytest.mark.parametrize("case", [("directional", ["-f"], ["+", "-"]), ("nondir", ["-D", "-y"], [""])],
                         ids=lambda c: c[0])
def test_bigwig_device_deflate(gpu_lib, tmp_path, monkeypatch, case):
    name, args, tracks = case
    ct, files = make_inputs(tmp_path, 6500 + len(name), HG_LIKE, 1, shift_rev=100)
    regions = os.path.join(BIN, "regions")
    for d in ("host", "dev"):
        (tmp_path / d).mkdir()
    env_with(monkeypatch)
    r0 = run([regions, "-q", "-c", ct] + args + ["-W", "host/q", "-o", "host/r.txt"] + files, tmp_path)
    env_with(monkeypatch, UNIPEAK_BIGWIG_DEFLATE="device")
    r1 = run([regions, "-q", "-c", ct] + args + ["-W", "dev/q", "-o", "dev/r.txt"] + files, tmp_path)
    assert "deflate zlib" in r0.stderr and "deflate device" in r1.stderr
    assert (tmp_path / "host/r.txt").read_bytes() == (tmp_path / "dev/r.txt").read_bytes()
    for t in tracks:
        a, b = tmp_path / f"host/q{t}.bw", tmp_path / f"dev/q{t}.bw"
        ia, ca, za = read_bigwig(a)
        ib, cb, zb = read_bigwig(b)
        assert ca == cb and list(ia) == list(ib)
        for c in ia:
            assert keyed(ia[c]) == keyed(ib[c]), c  # items with their float bits
        assert sum(len(v) for v in ia.values()) > 1000
        assert total_summary(a) == total_summary(b)
        assert len(za) == len(zb) >= 1
        for (ra, xa), (rb, xb) in zip(za, zb):
            assert ra == rb
            pack = lambda recs: [struct.pack("<IIIIffff", *x) for x in recs]
            assert pack(xa) == pack(xb)
        sa, sb = sections_of(a), sections_of(b)
        assert len(sa) == len(sb)
        for x, y in zip(sa, sb):
            assert x[:3] == y[:3] and np.array_equal(x[3], y[3])
        print(name, t, "bytes host", a.stat().st_size, "device", b.stat().st_size)
