"""The CLIs read ".bz2" inputs wherever they read ".gz" ones (host/gzio.cpp:
the bzip2 decoder's host twin, or the device decoder with
UNIPEAK_BZ_DEVICE=1): every output equals the plain file's run byte for byte,
on both routes.  The
oracle is never given a .bz2 name."""
import bz2
import os
import subprocess

import numpy as np
import pytest

from tests.test_cli import gen_sample
from tests.wig import write_contigs, write_wig

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
CONTIGS = [("chrA", 60_000), ("chrB", 45_000), ("chrC", 30_000)]
DEVICE = {"UNIPEAK_BZ_DEVICE": "1"}


def _bz(path):
    with open(path, "rb") as f:
        data = f.read()
    with open(str(path) + ".bz2", "wb") as f:
        f.write(bz2.compress(data))


def _inputs(tmp_path, seed=3, shift_rev=0):
    rng = np.random.default_rng(seed)
    write_contigs(tmp_path / "ct.txt", CONTIGS)
    fwd, rev = gen_sample(rng, CONTIGS, shift_rev=shift_rev)
    write_wig(tmp_path / "s.wig", "s", fwd, rev)
    _bz(tmp_path / "s.wig")
    _bz(tmp_path / "ct.txt")


def _body(path):
    # "# align_file=<name>" carries the input's file name; everything else must agree
    return b"\n".join(l for l in open(path, "rb").read().split(b"\n") if not l.startswith(b"# align_file="))


def _run(cmd, cwd, env=None):
    r = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, f"{cmd[0]} failed ({r.returncode}):\n{r.stderr[-2000:]}"
    return r


@pytest.mark.parametrize("env", [{}, DEVICE, {"UNIPEAK_BZ_DEVICE": "0"}, dict(DEVICE, UNIPEAK_NO_LEX="1"),
                                 {"UNIPEAK_NO_LEX": "1"}],
                         ids=["default", "device", "host", "device-nolex", "nolex"])
def test_regions_reads_bz2(gpu_lib, tmp_path, env):
    """bin/regions -w on s.wig.bz2: the table and the profile of the run on s.wig"""
    _inputs(tmp_path)
    for who, name in (("plain", "s.wig"), ("bz", "s.wig.bz2")):
        (tmp_path / who).mkdir()  # the profile's track name is its file name's prefix
        r = _run([os.path.join(BIN, "regions"), "-q", "-f", "-c", "../ct.txt", "-w", "p.wig", "-o", "t.txt",
                  "../" + name], tmp_path / who, dict(env, UNIPEAK_TIMING="1") if who == "bz" else None)
    assert _body(tmp_path / "plain" / "t.txt") == _body(tmp_path / "bz" / "t.txt")
    assert sum(1 for l in _body(tmp_path / "bz" / "t.txt").split(b"\n") if l.startswith(b"chr")) > 10
    prof = _body(tmp_path / "bz" / "p.wig")  # (the profile names its input in the same comment line)
    assert prof == _body(tmp_path / "plain" / "p.wig") and len(prof) > 1000
    line = [l for l in r.stderr.splitlines() if l.startswith("[timing] bz2 ")]
    assert line and "s.wig.bz2" in line[0], r.stderr[-500:]
    assert line[0].endswith("path device" if env.get("UNIPEAK_BZ_DEVICE") == "1" else "path host")


def test_contig_table_bz2(gpu_lib, tmp_path):
    _inputs(tmp_path)
    reg = os.path.join(BIN, "regions")
    _run([reg, "-q", "-c", "ct.txt", "-o", "a.txt", "s.wig"], tmp_path)
    _run([reg, "-q", "-c", "ct.txt.bz2", "-o", "b.txt", "s.wig"], tmp_path, DEVICE)
    _run([reg, "-q", "-c", "ct.txt.bz2", "-o", "c.txt", "s.wig.bz2"], tmp_path)
    # (the table's comment lines name the contig file and the input)
    assert (tmp_path / "a.txt").read_bytes() == (tmp_path / "b.txt").read_bytes().replace(b"ct.txt.bz2", b"ct.txt")
    assert _body(tmp_path / "a.txt") == _body(tmp_path / "c.txt").replace(b"ct.txt.bz2", b"ct.txt")
    assert b"ct.txt.bz2" in (tmp_path / "b.txt").read_bytes()


def test_strand_shift_and_tags_in_regions_bz2(gpu_lib, tmp_path):
    _inputs(tmp_path, shift_rev=150)
    ss = os.path.join(BIN, "strand_shift")
    _run([ss, "-x", "100", "-c", "ct.txt", "-o", "a.txt", "s.wig"], tmp_path)
    _run([ss, "-x", "100", "-c", "ct.txt", "-o", "b.txt", "s.wig.bz2"], tmp_path, DEVICE)
    assert _body(tmp_path / "a.txt") == _body(tmp_path / "b.txt")
    assert b"# best_shift=" in (tmp_path / "b.txt").read_bytes()
    _run([os.path.join(BIN, "regions"), "-q", "-c", "ct.txt", "-o", "reg.txt", "s.wig"], tmp_path)
    _bz(tmp_path / "reg.txt")
    tir = os.path.join(BIN, "tags_in_regions")
    _run([tir, "-c", "ct.txt", "-f", "reg.txt", "-o", "ta.txt", "s.wig"], tmp_path)
    _run([tir, "-c", "ct.txt", "-f", "reg.txt.bz2", "-o", "tb.txt", "s.wig"], tmp_path, DEVICE)
    _run([tir, "-c", "ct.txt", "-f", "reg.txt.bz2", "-o", "tc.txt", "s.wig.bz2"], tmp_path)
    a = (tmp_path / "ta.txt").read_bytes()
    assert len(a) > 200
    for other in ("tb.txt", "tc.txt"):
        got = (tmp_path / other).read_bytes()
        assert got.replace(b"reg.txt.bz2", b"reg.txt").replace(b"s.wig.bz2", b"s.wig") == a, other


def test_convert_align_bz2(gpu_lib, tmp_path):
    rng = np.random.default_rng(5)
    write_contigs(tmp_path / "ct.txt", CONTIGS)
    with open(tmp_path / "a.bed", "w") as f:
        for _ in range(20_000):
            c, L = CONTIGS[int(rng.integers(0, 3))]
            s = int(rng.integers(0, L - 40))
            f.write(f"{c}\t{s}\t{s + 36}\tr\t0\t{'+-'[int(rng.integers(0, 2))]}\n")
    _bz(tmp_path / "a.bed")
    ca = os.path.join(BIN, "convert_align")
    for who, name, env in (("plain", "a.bed", None), ("bz", "a.bed.bz2", DEVICE), ("bzh", "a.bed.bz2", None)):
        (tmp_path / who).mkdir()
        _run([ca, "-q", "-c", "../ct.txt", "-o", "x.wig", "../" + name], tmp_path / who, env)
    a = (tmp_path / "plain" / "x.wig").read_bytes()
    assert len(a) > 10_000
    for who in ("bz", "bzh"):
        assert (tmp_path / who / "x.wig").read_bytes().replace(b"a.bed.bz2", b"a.bed") == a, who


def test_wigs2bigwigs_bz2(gpu_lib, tmp_path):
    """x.wig.bz2 gives x+.bw / x-.bw like x.wig (the script strips .bz2, then .wig)"""
    _inputs(tmp_path)
    (tmp_path / "s.sizes").write_text("".join(f"{c}\t{L}\n" for c, L in CONTIGS))
    reg = os.path.join(BIN, "regions")
    _run([reg, "-q", "-f", "-c", "ct.txt", "-w", "x.wig", "-o", "t.txt", "s.wig"], tmp_path)
    _bz(tmp_path / "x.wig")
    out = {}
    for who, name, env in (("plain", "x.wig", None), ("bz", "x.wig.bz2", DEVICE), ("bzh", "x.wig.bz2", None)):
        (tmp_path / who).mkdir()
        os.link(tmp_path / name, tmp_path / who / name)
        r = _run([os.path.join(BIN, "wigs2bigwigs"), "--sizes", "../s.sizes", "--prefix", "http://h/", name],
                 tmp_path / who, env)
        out[who] = (r.stdout, (tmp_path / who / "x+.bw").read_bytes(), (tmp_path / who / "x-.bw").read_bytes())
    assert len(out["plain"][1]) > 1000
    assert out["bz"] == out["plain"] and out["bzh"] == out["plain"]


@pytest.mark.parametrize("env", [{}, DEVICE], ids=["host", "device"])
@pytest.mark.parametrize("tool", ["regions", "wigs2bigwigs"])
def test_corrupt_bz2_is_refused(gpu_lib, tmp_path, tool, env):
    """exit 1, an "error:" line with the file's name, and no output file"""
    _inputs(tmp_path)
    z = (tmp_path / "s.wig.bz2").read_bytes()
    (tmp_path / "bad.wig.bz2").write_bytes(z[:len(z) // 2] + bytes([z[len(z) // 2] ^ 0x10]) + z[len(z) // 2 + 1:])
    (tmp_path / "s.sizes").write_text("".join(f"{c}\t{L}\n" for c, L in CONTIGS))
    cmd = ([os.path.join(BIN, "regions"), "-q", "-c", "ct.txt", "-w", "p.wig", "-o", "o.txt", "bad.wig.bz2"]
           if tool == "regions" else [os.path.join(BIN, "wigs2bigwigs"), "--sizes", "s.sizes", "bad.wig.bz2"])
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, env=dict(os.environ, **env))
    assert r.returncode == 1, r.stderr[-500:]
    assert any(l.startswith("error: could not read bad.wig.bz2: ") for l in r.stderr.splitlines()), r.stderr[-500:]
    for name in ("o.txt", "p.wig", "bad+.bw", "bad-.bw"):
        assert not (tmp_path / name).exists(), name
