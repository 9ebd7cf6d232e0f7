"""csrc/route.h on the CPU: the route of every context, against the predicates
it replaced (tests/route_table.cpp keeps them as its reference) and against
the named rows below, which are the policy in readable form."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "route_table.cpp")


def _build(out, *flags):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, SRC], check=True)
    return out


@pytest.fixture(scope="module")
def route_table(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("route") / "route_table"))


def test_route_equals_the_replaced_predicates(route_table):
    """Every combination of bw in {1, 511, 512, 32767, 32768, 65535}, the sign
    of the threshold, the coefficients' sign, strandedness, the capture, both
    context switches, six environment switches and the track bits: scan,
    async-ok and profile-ok row by row."""
    r = subprocess.run([route_table], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.split()[0]) == 6 * 2 * 2 ** 12


def test_route_table_under_sanitizers(tmp_path):
    exe = _build(str(tmp_path / "route_table_san"), "-g", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=undefined")
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe, "bw=512,thr=0,nondir=1,wide_q11_nd=1"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split() == ["K1qWide", "0", "1"], r.stdout + r.stderr


# (row, scan, up_run_async allowed, dense profile allowed); thr=1: a threshold
# > 0, thr=0: <= 0; unnamed inputs: a fresh library context, no variable set,
# no negative coefficient
NAMED = [
    ("bw=511,thr=1", "K1", 1, 1),
    ("bw=511,thr=0", "K1q", 0, 1),
    ("bw=511,thr=0,capture=1", "K1q", 0, 1),
    ("bw=511,thr=0,neg=1", "Replay", 0, 0),
    ("bw=512,thr=1", "K1w", 1, 1),
    ("bw=512,thr=1,nondir=1", "K1w", 0, 0),
    ("bw=512,thr=1,nondir=1,wide_nd_full=1", "K1w", 1, 1),
    ("bw=512,thr=1,nondir=1,wide_nd_full=1,capture=1", "K1w", 1, 1),
    ("bw=512,thr=1,nondir=1,capture=1", "Replay", 0, 0),
    ("bw=512,thr=0", "K1qWide", 0, 1),
    ("bw=512,thr=0,capture=1", "Replay", 0, 0),
    ("bw=512,thr=0,nondir=1", "Replay", 0, 0),
    ("bw=512,thr=0,nondir=1,wide_q11_nd=1", "K1qWide", 0, 1),
    ("bw=512,thr=0,nondir=1,wide_q11_nd=1,WIDE_Q11_ND=0", "Replay", 0, 0),
    ("bw=32767,thr=1", "K1w", 1, 1),
    ("bw=32768,thr=1", "Replay", 0, 0),
    ("bw=512,thr=1,WIDE=0", "Replay", 0, 0),
    ("bw=512,thr=1,nondir=1,wide_nd_full=1,WIDE_ND=0", "Replay", 0, 0),
    ("bits=4,bw=1,thr=0", "Replay", 0, 0),
    ("bits=4,bw=512,thr=1", "Replay", 0, 0),
]


def test_named_rows(route_table):
    r = subprocess.run([route_table] + [row for row, *_ in NAMED], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [line.split() for line in r.stdout.splitlines()]
    want = [[scan, str(a), str(p)] for _, scan, a, p in NAMED]
    assert len(got) == len(want)
    for (row, *_), g, w in zip(NAMED, got, want):
        assert g == w, (row, g, w)
