"""bench.py --dump-outputs (CPU): the writer of the last step's records --
one float64 array per record field plus the counts, exact and finite (what
a double field held where it was not finite goes into <field>_nonfinite),
and above the size limit the same fixed rows in every array.  bench.py is
imported in a child process (importing it sets the process's hardware-queue
count)."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import sys
import numpy as np
import bench
from unipeak_amd import capi
n, S, out = int(sys.argv[1]), 3, sys.argv[2]
bench.DUMP_LIMIT_BYTES = int(sys.argv[3])
rng = np.random.default_rng(5)
recs = np.zeros(n, capi.REGION_DTYPE)
for f in recs.dtype.names:
    if recs.dtype[f].kind == "f":
        recs[f] = rng.standard_normal(n)
    else:
        recs[f] = rng.integers(0, 2**31 - 1, n)
recs["left"][0] = 2**32 - 1
recs["corr"][::2] = np.nan
recs["kurtosis"][1], recs["kurtosis"][2] = np.inf, -np.inf
counts = rng.integers(0, 2**32, (n, S), dtype=np.uint64).astype(np.uint32)
np.savez(out + "_in.npz", recs=recs, counts=counts)
bench.dump_outputs(out, recs, counts, {"n_regions": n})
"""


def dump(tmp_path, name, n, limit):
    out = str(tmp_path / name)
    subprocess.run([sys.executable, "-c", CHILD, str(n), out, str(limit)], cwd=ROOT, check=True,
                   timeout=120)
    src = np.load(out + "_in.npz")
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    return src["recs"], src["counts"], got


def restored(got, f):
    """the record's field from <f>.npy and, for a double field, <f>_nonfinite.npy"""
    a = got[f].copy()
    if f + "_nonfinite" in got:
        k = got[f + "_nonfinite"]
        assert np.all(a[k != 0] == 0.0) and set(np.unique(k)) <= {0.0, 1.0, 2.0, 3.0}
        a[k == 1], a[k == 2], a[k == 3] = np.nan, np.inf, -np.inf
    return a


def test_dump_is_exact_float64(tmp_path):
    recs, counts, got = dump(tmp_path, "a", 1000, 64 * 1000 * 1000)
    doubles = {"peak_score", "kurtosis", "corr"}
    assert set(got) == set(recs.dtype.names) | {d + "_nonfinite" for d in doubles} | {"counts", "n_regions"}
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a)) for a in got.values())
    assert got["corr_nonfinite"][:4].tolist() == [1.0, 0.0, 1.0, 0.0]
    assert got["kurtosis_nonfinite"][:4].tolist() == [0.0, 2.0, 3.0, 0.0]
    for f in recs.dtype.names:
        assert got[f].dtype == np.float64 and got[f].shape == (1000,)
        assert np.array_equal(restored(got, f).astype(recs.dtype[f]), recs[f], equal_nan=True), f
    assert got["left"][0] == 2.0**32 - 1
    assert got["counts"].dtype == np.float64
    assert np.array_equal(got["counts"].astype(np.uint32), counts)
    assert got["n_regions"].tolist() == [1000.0]


def test_dump_above_the_limit_is_a_fixed_sample(tmp_path):
    limit = 20_000
    recs, counts, got = dump(tmp_path, "a", 1000, limit)
    _, _, again = dump(tmp_path, "b", 1000, limit)
    rows = got["rows"].astype(np.int64)
    assert 0 < len(rows) < 1000 and np.all(np.diff(rows) > 0)
    out = str(tmp_path / "a")
    assert sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out)) <= limit
    for f in recs.dtype.names:
        assert np.array_equal(restored(got, f).astype(recs.dtype[f]), recs[f][rows], equal_nan=True), f
    assert np.array_equal(got["counts"].astype(np.uint32), counts[rows])
    assert got["n_regions"].tolist() == [1000.0]  # the whole step's count, not the sample's
    for k in got:
        assert np.all(np.isfinite(got[k])) and np.array_equal(got[k], again[k]), k
