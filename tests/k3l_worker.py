"""Not a test: the child process of tests/test_gpu_k3_lane.py.

UNIPEAK_K3_LANE, UNIPEAK_K3L_HEAVY and UNIPEAK_K3L_W2 are read once per
process, so each setting needs a fresh one.  Runs the named cases (or a group,
"all" / "c123") of test_gpu_k3_lane through capi.Lib and writes every case's
records, per-sample counts and K3 kind to OUTDIR/cases.npz.

    python tests/k3l_worker.py OUTDIR CASE [CASE ...]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv):
    from tests import test_gpu_k3_lane as t
    from tests.oracle_binding import Oracle
    from unipeak_amd import capi

    outdir, names = argv[0], []
    for a in argv[1:]:
        names += t.case_names(a) if a in ("all", "c123") else [a]
    capi.load_library()
    if capi.device_count() < 1:
        raise SystemExit("k3l_worker: no HIP device visible")
    oracle = Oracle()  # (thr_* take their thresholds from the oracle's medians)
    out = {}
    for n in names:
        regs, cnt, kind = t.run_case(capi, t.build_case(n, oracle))
        out[n + "__regs"], out[n + "__cnt"], out[n + "__kind"] = regs, cnt, np.int32(kind)
    np.savez(os.path.join(outdir, "cases.npz"), **out)
    print(f"k3l_worker: {len(names)} cases")


if __name__ == "__main__":
    main(sys.argv[1:])
