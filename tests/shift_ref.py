"""Host restatement of Region::strandCorr(shift) (src/strand_shift.cpp:205-217,
misc/data.cpp:22-58, 184-193) over the oracle's dense profile of each strand
alone: the second reference behind up_shift_scan's table, independent of the
oracle's own orc_run_unit_shifts (tests/test_oracle_shift.py holds the two
against each other on the CPU)."""
import numpy as np


def strand_corr(f, r, shift):
    """Region::strandCorr(shift) (src/strand_shift.cpp:205-217, misc/data.cpp:
    22-58, 184-193): sequential sums (np.cumsum adds in index order)"""
    n = f.size
    if not n > 2 * shift + 3:
        return np.nan
    m = n - 2 * shift
    a, b = f[:m], r[2 * shift:2 * shift + m]
    seq = lambda v: np.cumsum(v)[-1]
    m1, m2 = seq(a) / m, seq(b) / m
    with np.errstate(invalid="ignore", divide="ignore"):
        sd1 = np.sqrt(seq((a - m1) * (a - m1)) / (m - 1.0))
        sd2 = np.sqrt(seq((b - m2) * (b - m2)) / (m - 1.0))
        return seq((a - m1) * (b - m2)) / ((m - 1.0) * sd1 * sd2)


def host_shift_table(oracle, bw, bg, pos, cf, cr, regs, max_shift, control=None, coeffs=None):
    """strandCorr(0 .. max_shift) of the given regions of one unit over f =
    the oracle's dense profile of the forward counts alone and r = that of the
    reverse counts alone (regions the K0 head chain did not emit); a position
    is an add of a strand when any sample's count there is non-zero"""
    span = int(regs["right"].max())
    mf, mr = (cf != 0).any(axis=1), (cr != 0).any(axis=1)
    f = oracle.profile(bw, bg, span, pos[mf], cf[mf], control=control, coeffs=coeffs)
    r = oracle.profile(bw, bg, span, pos[mr], cr[mr], control=control, coeffs=coeffs)
    return np.array([[strand_corr(f[q["left"] - 1:q["right"]], r[q["left"] - 1:q["right"]], s)
                      for s in range(max_shift + 1)] for q in regs]).reshape(len(regs), max_shift + 1)
