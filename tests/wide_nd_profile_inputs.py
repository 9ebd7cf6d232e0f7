"""Seeded inputs and oracle references of the nondirectional dense-profile
tests (bw 512..32767, both strands in one buffer, up_set_wide_nd_full on):
shared by tests/test_wide_nd_profile_oracle.py (CPU: the oracle alone shows
that each input has the properties its GPU case relies on) and
tests/test_gpu_wide_nd_profile.py (GPU: every score bit for bit)."""
import numpy as np

from tests import wide_nd_inputs as W

LENGTH = 60_000         # 3.7 strips, 14.6 stretches
STRETCH = 4_096         # positions of one wave's stretch in wide_profile_kernel
PARITY_SEEDS = {512: 5121, 700: 7001, 2000: 20001}
RANGE_BW = 700
POOL_CONTROL = [0, 1, 0]
POOL_COEFFS = [None, [0.6, 1.7]]


def strand_refs(oracle, bw, bg, length, pos, cf, cr, **kw):
    """(f, r, f + r as the oracle's nondirectional profile): f the oracle's
    profile of the forward counts alone, r that of the reverse counts alone
    (host_shift_table's idiom in tests/shift_ref.py); read-only"""
    mf, mr = cf.any(axis=1), cr.any(axis=1)
    f = oracle.profile(bw, bg, length, pos[mf], cf[mf], **kw)
    r = oracle.profile(bw, bg, length, pos[mr], cr[mr], **kw)
    both = oracle.profile(bw, bg, length, pos, cf, cr, nondir=True, **kw)
    for a in (f, r, both):
        a.setflags(write=False)
    return f, r, both


def parity_unit(bw):
    return W.parity_unit(bw, length=LENGTH, seed=PARITY_SEEDS[bw])


def pooled_unit():
    return W.parity_unit(700, S=3, length=LENGTH, seed=7003)


def tail_unit():
    """the bw 700 parity body plus tags on both strands in the last 300
    positions (one at len itself), so the scores of len + 1 .. len + bw, which
    the flush retires, are nonzero on both strands"""
    length, pos, cf, cr = W.parity_unit(RANGE_BW, length=LENGTH, seed=7002)
    df = {int(p): int(c) for p, c in zip(pos, cf[:, 0]) if c}
    dr = {int(p): int(c) for p, c in zip(pos, cr[:, 0]) if c}
    rng = np.random.default_rng(7012)
    for d, last in ((df, length), (dr, length - 7)):
        for p in rng.integers(length - 300, last, 12):
            d[int(p)] = d.get(int(p), 0) + int(rng.integers(1, 4))
        d[last] = d.get(last, 0) + 5
    return (length,) + W.from_dense(df, dr)


HEAD_BW = 700
HEAD_GAP = (651, 4_000)  # no tag on either strand: longer than 2 bw + 1


def head_gap_unit():
    """tags at 3, 40 and 650 on the reverse strand only (a head unit: tags at
    positions <= bw), nothing on either strand in 651 .. 4,000 -- a gap longer
    than 2 bw + 1, so the head replay's window drains and it can resync --
    then a parity_unit-style body to the contig end"""
    length, pos, cf, cr = W.parity_unit(HEAD_BW, length=LENGTH, seed=7004)
    df = {int(p): int(c) for p, c in zip(pos, cf[:, 0]) if c and p > HEAD_GAP[1]}
    dr = {int(p): int(c) for p, c in zip(pos, cr[:, 0]) if c and p > HEAD_GAP[1]}
    for p in (3, 40, 650):
        dr[p] = 9
    return (length,) + W.from_dense(df, dr)


def stretch_hits(p, bw, x):
    """hits of strand positions p inside the windows of the stretch that holds x
    (whole-profile call: stretches start at 1 + 4,096 k)"""
    x_lo = 1 + (x - 1) // STRETCH * STRETCH
    return int(np.sum((p >= x_lo - bw) & (p <= x_lo + STRETCH - 1 + bw)))
