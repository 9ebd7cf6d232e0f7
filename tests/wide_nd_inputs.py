"""Seeded inputs of the nondirectional wide-bandwidth tests (bw 512..32767
on both strands of one buffer): shared by tests/test_wide_nd_oracle.py (CPU:
the oracle alone shows that each input has the properties its GPU case relies
on) and tests/test_gpu_wide_nondir.py (GPU: parity with the oracle)."""
import numpy as np

from tests.gen import random_unit

STRIP = 16_384          # positions of one K1w strip
SLAB = 4_096            # wide_corr_kernel's per-wave (f, r) slab, positions
LIST = 512              # hits one LDS list of the dense scores holds
BG = 0.003


def merge(pos_f, cnt_f, pos_r, cnt_r):
    """two strands' sparse units -> (positions, forward counts, reverse counts)"""
    S = cnt_f.shape[1]
    allp = np.union1d(pos_f, pos_r).astype(np.uint32)
    cf = np.zeros((allp.size, S), np.uint32)
    cr = np.zeros((allp.size, S), np.uint32)
    cf[np.searchsorted(allp, pos_f)] = cnt_f
    cr[np.searchsorted(allp, pos_r)] = cnt_r
    return allp, cf, cr


def from_dense(df, dr, S=1):
    """{pos: count} per strand -> merged sparse arrays (sample 0 only)"""
    def arr(d):
        p = np.array(sorted(d), np.uint32)
        c = np.zeros((p.size, S), np.uint32)
        c[:, 0] = [d[int(x)] for x in p]
        return p, c
    return merge(*arr(df), *arr(dr))


# ---- case 1: parity, one sample -------------------------------------------
PARITY_SEEDS = {512: 5120, 700: 7000, 2000: 20000}
PARITY_LEN = 200_000


def parity_unit(bw, S=1, length=PARITY_LEN, seed=None):
    """two independent random_unit strands, no tag at a position <= bw"""
    rng = np.random.default_rng(PARITY_SEEDS[bw] if seed is None else seed)
    pos_f, cnt_f = random_unit(rng, length, bw, S=S, lo=bw + 1, sd=200)
    pos_r, cnt_r = random_unit(rng, length, bw, S=S, lo=bw + 1, sd=200)
    return (length,) + merge(pos_f, cnt_f, pos_r, cnt_r)


def crosses_strip(ref):
    return (ref["left"] - 1) // STRIP != (ref["right"] - 1) // STRIP


# ---- case 4: a head unit --------------------------------------------------------
HEAD_BW = 700


def head_unit():
    """tags at positions <= bw on the reverse strand only, a forward cluster
    around 900 whose region starts inside the first bw positions (quirk Q1: the
    K0 head chain emits it), a cluster at the contig end and a tag at len"""
    bw = HEAD_BW
    rng = np.random.default_rng(41)
    length, pos, cf, cr = parity_unit(bw, length=60_000, seed=411)
    df = {int(p): int(c) for p, c in zip(pos, cf[:, 0]) if c}
    dr = {int(p): int(c) for p, c in zip(pos, cr[:, 0]) if c}
    for p in (3, 40, 650):
        dr[p] = dr.get(p, 0) + 9
    for o in np.rint(rng.normal(0, 60, 80)).astype(int):
        p = min(length, length - 150 + int(o))
        df[p] = df.get(p, 0) + 1
    df[length] = df.get(length, 0) + 12
    for o in np.rint(rng.normal(0, 120, 100)).astype(int):
        p = max(bw + 1, 900 + int(o))
        df[p] = df.get(p, 0) + 1
    return (length,) + from_dense(df, dr)


# ---- case 6: the widest kernel K1w takes --------------------------------------------
LIMIT_BW = 32_767
LIMIT_LEN = 120_000
LIMIT_BG = 0.002
LIMIT_KW = dict(region_thr=0.3, kurt_thr=0.0, hit_thr=1.0, corr_thr=0.3)


def limit_unit():
    """a few hundred tags in two clusters per strand, every one above position
    bw: no head unit, so K1w and the wide correlation produce the records"""
    rng = np.random.default_rng(LIMIT_BW)
    df, dr = {}, {}
    for d, shift in ((df, 0), (dr, 300)):
        for c, n in ((60_000, 150), (95_000, 120)):
            for o in np.rint(rng.normal(0, 400, n)).astype(int):
                p = int(np.clip(c + shift + o, LIMIT_BW + 1, LIMIT_LEN))
                d[p] = d.get(p, 0) + 1
    return (LIMIT_LEN,) + from_dense(df, dr)


# ---- case 3: one-strand regions ---------------------------------------------
ONE_STRAND_BW = 700
ONE_STRAND_LEN = 60_000


def one_strand_unit():
    """a forward-only and a reverse-only cluster more than 2 bw apart"""
    rng = np.random.default_rng(31)
    df, dr = {}, {}
    for d, centre in ((df, 15_000), (dr, 40_000)):
        for o in np.rint(rng.normal(0, 150, 150)).astype(int):
            d[centre + int(o)] = d.get(centre + int(o), 0) + 1
    return (ONE_STRAND_LEN,) + from_dense(df, dr)


# ---- case 5: stress of the dense-score kernels' branches --------------------
STRESS_BW = 600
STRESS_LEN = 80_000


def stress_unit():
    """* positions 20,000..20,999 hold a forward tag each (1,000 hits inside
         one stretch's windows: more than the LDS list, the fallback walk) with
         counts 3..9 among them (escape table);
       * the reverse chunk 30,001..30,016 holds 16 x 20 = 320 tags (a saturated
         plane entry);
       * a chain of clusters 45,000..56,000 on both strands keeps the score
         above the threshold for more than SLAB positions."""
    rng = np.random.default_rng(55)
    df, dr = {}, {}
    for p in range(20_000, 21_000):
        df[p] = 1 + (int(rng.integers(2, 9)) if p % 50 == 0 else 0)
    for p in range(20_300, 20_700, 7):
        dr[p] = 2
    for p in range(30_001, 30_017):
        dr[p] = 20
    for p in range(29_800, 30_300, 5):
        df[p] = df.get(p, 0) + 1
    for centre in range(45_000, 56_001, 500):
        for d in (df, dr):
            for o in np.rint(rng.normal(0, 200, 120)).astype(int):
                d[centre + int(o)] = d.get(centre + int(o), 0) + 1
    return (STRESS_LEN,) + from_dense(df, dr)
