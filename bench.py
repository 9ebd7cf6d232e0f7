#!/usr/bin/env python3
"""Headline benchmark: genome Gbp/s for KDE smoothing + region scan on hg19.

Default workload (BASELINE.json configs[1], the metric's config): hg19 full
genome (25 contigs, 3,095,693,983 bp), one directional sample (3SEQ-style),
default parameters (bw 50, -r 25, -k 50, -t 10), synthetic hg19-shaped tag
counts generated on the device, packed to 2-bit tracks and
resident in HBM before timing.  Other BASELINE configs are available with
--workload for our own measurements (the default line is the headline):

  hg19-dir1    configs[1]  1 directional sample                      (default)
  hg19-nondir1 configs[2]  regions pass of C3: -D -y, 1 sample, both strands
  hg19-shift   configs[2]  the whole C3 pipeline: strand_shift, then regions -D -y -s <best>
  hg19-8s1c    configs[3]  8 samples + 1 negative control (-e 9), directional
  hg19mm9-32s  configs[4]  hg19+mm9, 32 samples, -D -k 50 -u 0.3 -y (8 GPUs): the survey's
                           generator (independent peak centres per sample: no region
                           reaches -r 25 once 32 samples are pooled)
  hg19mm9-32rep configs[4] the same table and flags on 32 replicates (shared peak
                           centres), read with -s 75: the filters decide

One step = the whole hot path over the genome: the tag totals summed over
the ranks (node-shared StepBoard on one node; RCCL across nodes) ->
background -> up_run_async (K1a stream+screen on a high-priority
stream -> K1b exact blocks -> K2 segmentation -> K3 region statistics +
filters on a chain stream, records written straight into pinned host memory;
up to five passes in flight) -> rank 0 reads every rank's records from the
node's shared memory in global unit order.

Multi-GPU: one process per GPU (torchrun); units are LPT-assigned to ranks by
unipeak_amd/shard.py (strong scaling: the genome is fixed), so there is no
data-path collective besides the RCCL background all-reduce and the record
gather.  UNIPEAK_BENCH_DIST=1 takes the distributed path at N=1 too (to
exercise RCCL on a one-GPU box).

Prints ONE JSON line on rank 0 (contract in the task statement), including
the roofline of the dominant kernel (K1a) as its events in the timed steps
give it.

A plain run does what the headline needs and no more: set-up, warm-up, the
--steps timed steps of the headline leg, the result line.  --full adds every
measurement that takes passes of its own: the warm leg, the isolated
per-kernel passes, the single cold passes, the HBM copy rate and the oracle
CPU baseline (--no-cpu-baseline leaves that one out of a --full run).

--dump-outputs DIR writes what the last timed step of the headline leg
delivered to rank 0 -- the region records in global unit order, one
DIR/<field>.npy per record field, and the per-sample counts, DIR/counts.npy --
as float64 (every field is a 32-bit integer or a double: exact).  Every array
is finite: where a double field holds NaN (a statistic not computed in this
configuration, or undefined for the region) <field>.npy carries 0 and
DIR/<field>_nonfinite.npy marks the row.  The inputs are generated from --seed, so two builds run with the same arguments can be
compared array for array.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# the library's five streams (context, K1a, three chains) plus torch's and
# RCCL's: more hardware queues than HIP's default 4, so no stream of a pass
# shares an in-order queue with another (read at HIP initialisation)
# (the configs[2] pipeline holds two contexts: twice the streams)
# Set explicitly (a box that exports HIP's default 4 would otherwise keep it,
# and the five streams would share four in-order queues); UNIPEAK_HWQ
# overrides; both values go into the bench line (hw_queues)
HWQ_INHERITED = os.environ.get("GPU_MAX_HW_QUEUES")
os.environ["GPU_MAX_HW_QUEUES"] = os.environ.get("UNIPEAK_HWQ") or ("12" if "hg19-shift" in sys.argv else "8")

from unipeak_amd import capi, shard  # noqa: E402

METRIC = "genome Gbp/s for KDE smoothing + region scan on hg19, at 1/2/4/8 MI355X"
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s (spec)

WORKLOADS = {
    "hg19-dir1": dict(tables=["hg19"], nondir=False, samples=1, controls=0, kurt=50.0, corr=-1.0,
                      want_corr=False, baseline="configs[1]",
                      desc="hg19 full genome, 1 directional sample (3SEQ-style), bw 50, "
                           "-r 25 -k 50 -t 10 (BASELINE configs[1])"),
    "hg19-nondir1": dict(tables=["hg19"], nondir=True, samples=1, controls=0, kurt=50.0, corr=-1.0,
                         want_corr=True, baseline="configs[2]",
                         desc="hg19, 1 nondirectional sample, regions -D -y pass of C3, bw 50, "
                              "-r 25 -k 50 -t 10 (BASELINE configs[2])"),
    "hg19-8s1c": dict(tables=["hg19"], nondir=False, samples=9, controls=1, kurt=50.0, corr=-1.0,
                      want_corr=False, baseline="configs[3]",
                      desc="hg19, 8 pooled directional samples + 1 negative control (-e 9), bw 50, "
                           "-r 25 -k 50 -t 10 (BASELINE configs[3])"),
    "hg19-shift": dict(tables=["hg19"], nondir=True, samples=1, controls=0, kurt=50.0, corr=0.3,
                       want_corr=True, baseline="configs[2]", shift_pipeline=True,
                       desc="hg19, 1 nondirectional sample, the whole configs[2] pipeline per step: "
                            "strand_shift (KDE pass, sort by sum, strandCorr(0..150) table, shift "
                            "histogram) then regions -D -y -s <best> (BASELINE configs[2])"),
    "hg19mm9-32s": dict(tables=["hg19", "mm9"], nondir=True, samples=32, controls=0, kurt=50.0,
                        corr=0.3, want_corr=True, baseline="configs[4]",
                        desc="hg19+mm9 (names prefixed), 32 nondirectional samples, -D -k 50 -u 0.3 -y, "
                             "bw 50 (BASELINE configs[4])"),
    # configs[4] as a ChIP experiment of 32 replicates: shared peak centres
    # (per-sample heights and jitter; artifact, spike and weak peaks the
    # filters reject), read with -s 75 as strand_shift finds it
    "hg19mm9-32rep": dict(tables=["hg19", "mm9"], nondir=True, samples=32, controls=0, kurt=50.0,
                          corr=0.3, want_corr=True, baseline="configs[4]", peak_seed=7, shift=75,
                          desc="hg19+mm9 (names prefixed), 32 nondirectional replicate samples "
                               "(shared peak centres), -D -k 50 -u 0.3 -y -s 75, bw 50 "
                               "(BASELINE configs[4])"),
}


def read_contigs(path):
    out = []
    for line in open(path):
        f = line.split()
        if len(f) >= 2 and not line.startswith("#"):
            out.append((f[0], int(f[1])))
    return out


def load_table(names):
    contigs = []
    for t in names:
        rows = read_contigs(os.path.join(ROOT, "unipeak_amd", "data", f"{t}.txt"))
        contigs += [((f"{t}_{n}" if len(names) > 1 else n), L) for n, L in rows]
    return contigs


def pmc_traffic(bytes_per_launch):
    """HBM bytes per K1a launch from the committed rocprofv3 PMC passes
    (tools/pmc_traffic.py) when they were taken on this exact workload."""
    for rnd in ("r06",):  # (earlier rounds' files measured other K1a builds)
        p = os.path.join(ROOT, "profiles", rnd, "k1a_pmc_traffic.json")
        try:
            d = json.load(open(p))
        except (OSError, ValueError):
            continue
        if int(d.get("algorithmic_bytes_per_launch", -1)) == int(bytes_per_launch):
            return round(d["traffic_bytes_per_launch"] / 1e9, 3), os.path.relpath(p, ROOT)
    return None, None


DUMP_LIMIT_BYTES = 64 * 1000 * 1000


def dump_outputs(path, recs, counts, extra=None):
    """--dump-outputs: one float64 .npy per record field, counts.npy and the
    scalars in extra (name -> value).  Every array is finite: a double field
    (peak_score, kurtosis, corr) may hold NaN -- a statistic the pass did not
    compute or that is undefined for the region -- so <field>.npy carries 0
    there and <field>_nonfinite.npy says what the record held (0 finite,
    1 NaN, 2 +inf, 3 -inf).  Above DUMP_LIMIT_BYTES in all, the same fixed,
    seeded sample of the rows (ascending) goes into every array."""
    os.makedirs(path, exist_ok=True)
    n = len(recs)
    extra = extra or {}
    # every array's rows, the row numbers themselves, and 256 B per file for its header and a scalar
    doubles = [f for f in recs.dtype.names if recs.dtype[f].kind == "f"]
    row_bytes = 8 * (len(recs.dtype.names) + len(doubles) + counts.shape[1] + 1)
    budget = DUMP_LIMIT_BYTES - 256 * (len(recs.dtype.names) + len(doubles) + 2 + len(extra))
    if n * row_bytes > budget:
        rows = np.sort(np.random.default_rng(0).choice(n, max(budget // row_bytes, 1), replace=False))
        recs, counts = recs[rows], counts[rows]
        np.save(os.path.join(path, "rows.npy"), rows.astype(np.float64))
    for f in recs.dtype.names:
        a = np.ascontiguousarray(recs[f]).astype(np.float64)
        if f in doubles:
            kind = np.where(np.isnan(a), 1.0, np.where(np.isposinf(a), 2.0, np.where(np.isneginf(a), 3.0, 0.0)))
            np.save(os.path.join(path, f + "_nonfinite.npy"), kind)
            a[kind != 0] = 0.0
        np.save(os.path.join(path, f + ".npy"), a)
    np.save(os.path.join(path, "counts.npy"), counts.astype(np.float64))
    for k, v in extra.items():
        np.save(os.path.join(path, k + ".npy"), np.array([v], np.float64))


def free_port():
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(n, argv):
    """`bench.py --gpus N` started without torchrun: run the N ranks as
    children of this process (torch.distributed.run, one process per GPU on
    this node) and return their exit status.  Called before anything touches
    the GPU; this process only waits (nothing is exec'd).  Rank 0's JSON
    line reaches stdout through the inherited descriptor."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("MASTER_ADDR", "127.0.0.1")
    port = env.get("UNIPEAK_BENCH_PORT") or str(free_port())
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", f"--master-port={port}", os.path.abspath(__file__)] + argv
    print(f"[bench] --gpus {n}: launching {n} ranks: {' '.join(cmd[1:])}", file=sys.stderr, flush=True)
    r = subprocess.run(cmd, env=env)
    if r.returncode != 0:
        print(f"[bench] rank processes failed (exit {r.returncode})", file=sys.stderr, flush=True)
    return r.returncode


def check_world(args):
    """--gpus against the launcher's world size.  Returns the world size
    this process belongs to, or None when this process must launch the
    ranks itself; raises SystemExit (status 2) on a mismatch."""
    ws = os.environ.get("WORLD_SIZE")
    if args.gpus < 1:
        raise SystemExit(f"--gpus {args.gpus}: must be >= 1")
    if ws is None:
        return None if args.gpus > 1 else 1
    if int(ws) != args.gpus:
        print(f"error: --gpus {args.gpus} but WORLD_SIZE={ws} (launch N ranks with --gpus N)",
              file=sys.stderr, flush=True)
        raise SystemExit(2)
    return int(ws)


def launch_probe():
    """UNIPEAK_BENCH_LAUNCH_PROBE=<rc> (tests/test_bench_launch.py, CPU): each
    rank joins a gloo world, all-reduces its rank, rank 0 prints the world it
    saw; rank world-1 exits with <rc> -- the launcher's plumbing without a GPU."""
    import torch
    import torch.distributed as dist
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    t = torch.tensor([rank], dtype=torch.int64)
    dist.all_reduce(t)
    dist.destroy_process_group()
    if rank == 0:
        print(json.dumps({"n_gpus": world, "rank_sum": int(t.item()),
                          "local_world": int(os.environ.get("LOCAL_WORLD_SIZE", "0"))}), flush=True)
    rc = int(os.environ["UNIPEAK_BENCH_LAUNCH_PROBE"])
    return rc if rank == world - 1 else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bw", type=int, default=50)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--workload", default="hg19-dir1", choices=sorted(WORKLOADS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample", default="all")
    ap.add_argument("--full", action="store_true",
                    help="also the measurements that take passes of their own: warm leg, isolated "
                         "per-kernel passes, single cold passes, HBM copy rate, oracle CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the records and counts of the last timed step as DIR/<name>.npy (float64)")
    args = ap.parse_args()
    W = WORKLOADS[args.workload]
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")

    if W.get("shift_pipeline") and args.gpus != 1:
        raise SystemExit("hg19-shift runs on one GPU (--gpus 1)")
    if check_world(args) is None:  # --gpus N > 1 without a launcher
        return launch_ranks(args.gpus, sys.argv[1:])
    if os.environ.get("UNIPEAK_BENCH_LAUNCH_PROBE") is not None:
        return launch_probe()
    if W.get("shift_pipeline"):
        return shift_pipeline(args, W)
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    comm = None
    # UNIPEAK_SHARE_GPU=1 (rehearsal on a one-GPU box, with
    # UNIPEAK_DIST_BACKEND=gloo: RCCL refuses two ranks on one GPU): every
    # rank runs on device 0, so the N-rank path -- StepBoard, node-shared
    # record slots, rank 0's merge -- runs end to end on real hardware
    dev = 0 if os.environ.get("UNIPEAK_SHARE_GPU") == "1" else local
    if world > 1 or os.environ.get("UNIPEAK_BENCH_DIST") == "1":
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(dev)  # torch's HIP runtime first (tools/mix_probe.py)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29577")
        os.environ.setdefault("RANK", str(rank))
        os.environ.setdefault("WORLD_SIZE", str(world))
        backend = os.environ.get("UNIPEAK_DIST_BACKEND", "nccl")  # "nccl" = RCCL over xGMI
        dist.init_process_group(backend)
        comm = shard.Comm(dist, rank, world, f"cuda:{dev}" if backend == "nccl" else "cpu")

    contigs = load_table(W["tables"])
    genome = sum(L for _, L in contigs)
    mappable = genome & 0xFFFFFFFF  # ContigTable::genomeSize_ is uint32 (quirk Q10)
    lens = [L for _, L in contigs]
    S, n_ctl, nondir = W["samples"], W["controls"], W["nondir"]
    s_nc = S - n_ctl
    nstr = 2 if nondir else 1
    # UNIPEAK_SIM_WORLD=N UNIPEAK_SIM_RANK=r (single process, measurement aid
    # only): plan for N ranks and run rank r's shard alone, no collectives --
    # the compute side of one rank of an N-GPU run on a one-GPU box
    sim_world = int(os.environ.get("UNIPEAK_SIM_WORLD", "0"))
    sim_rank = int(os.environ.get("UNIPEAK_SIM_RANK", "0"))
    if sim_world > 1 and comm is not None:
        raise SystemExit("UNIPEAK_SIM_WORLD is for single-process runs")
    units, owner, mine_all = shard.plan(lens, nondir=nondir, world=sim_world or world, n_samples=S)
    mine = mine_all[sim_rank if sim_world > 1 else rank]
    # resident track bytes: TB-bit counts
    TB = capi.track_bits()
    need = sum(lens[units[k][0]] * nstr * S for k in mine) * TB / 8
    if need > 250e9:
        raise SystemExit(f"workload {args.workload} needs {need / 1e9:.0f} GB of tracks per GPU at "
                         f"N={world}; run it on more GPUs")

    control = [0] * s_nc + [1] * n_ctl
    g = capi.Lib(dev)
    g.set_params(args.bw, S, 0.0029, nondir=nondir, control=control)  # background set per step
    t_gen = time.time()
    pseed, shift = W.get("peak_seed", 0), W.get("shift", 0)

    def offset(synth_strand):  # -s: forward +s, reverse -s (misc/format.cpp:693-705)
        return shift if synth_strand == 0 else -shift

    for k in mine:  # ascending global order: records come back unit-major
        ci, buf = units[k]
        u = g.add_unit(lens[ci], buffer_id=buf)
        for st in range(nstr):
            synth_strand = st if nondir else buf
            for smp in range(S):
                seed = args.seed + smp if smp < s_nc else 2000 + (smp - s_nc)
                g.synth(u, st, smp, seed, ci, synth_strand, nondir=nondir, peaks=smp < s_nc,
                        offset=offset(synth_strand), peak_seed=pseed)
    local_tags = sum(g.tag_total(i, st, smp) for i in range(len(mine)) for st in range(nstr)
                     for smp in range(s_nc))
    if sim_world > 1:  # the background needs the genome-wide total: generate the other units too
        g2 = capi.Lib(dev)
        g2.set_params(args.bw, S, 0.0029, nondir=nondir, control=control)
        for k in range(len(units)):
            if k in mine:
                continue
            ci, buf = units[k]
            g2.reset_units()
            u = g2.add_unit(lens[ci], buffer_id=buf)
            for st in range(nstr):
                for smp in range(s_nc):
                    sst = st if nondir else buf
                    g2.synth(u, st, smp, args.seed + smp, ci, sst, nondir=nondir, peaks=True,
                             offset=offset(sst), peak_seed=pseed)
                    local_tags += g2.tag_total(u, st, smp)
        g2.close()
    gen_s = time.time() - t_gen
    mine_bp = sum(lens[units[k][0]] for k in mine)
    copy_gbps = g.hbm_copy_gbps(1 << 30, 5) if args.full else None
    # legs (DESIGN.md §3 "Index policy", §7): "cold" -- every pass reads only
    # the packed 2-bit tracks, no derived index survives between passes
    # (UP_INDEX_NEVER): the reference's one pass per run, the headline value;
    # "warm" -- the chunk-sum plane / pooled planes / pooled count tracks are
    # built once (untimed) and reused, a parameter sweep's re-scan (value_warm);
    # a run without --full times the first leg only
    legs = os.environ.get("UNIPEAK_BENCH_LEGS", "cold,warm").split(",")
    policy_of = {"cold": capi.INDEX_NEVER, "warm": capi.INDEX_ALWAYS}
    if not legs or any(x not in policy_of for x in legs):
        raise SystemExit(f"UNIPEAK_BENCH_LEGS={os.environ.get('UNIPEAK_BENCH_LEGS')}: cold and/or warm")
    if not args.full:
        legs = legs[:1]
    g.set_index_policy(policy_of[legs[0]])

    phase = {"allreduce": 0.0, "launch": 0.0, "wait": 0.0, "gather_merge": 0.0}
    sub = {"submit": 0.0, "target": 0.0, "run_async": 0.0}  # parts of "launch"
    # one node (torchrun --nnodes=1): records meet in node-shared host memory
    gather_mode = os.environ.get("UNIPEAK_GATHER") or (
        "shm" if int(os.environ.get("LOCAL_WORLD_SIZE", world)) == world else "rccl")
    bg_set = [None]
    nr = rbuf = cap = None
    pool = None
    # size the record slots once (the data are the same every step): one
    # untimed pass with host delivery, then K3 writes every later pass
    # straight into the slots
    g.set_params(args.bw, S, (comm.global_tags(local_tags) if comm else local_tags) / mappable /
                 (1 if nondir else 2), region_thr=25.0, kurt_thr=W["kurt"], corr_thr=W["corr"],
                 hit_thr=10.0 * s_nc, nondir=nondir, control=control, want_corr=W["want_corr"])
    n0 = g.run()
    cap = int((comm.max_over_ranks(n0) if comm else n0) * 1.25) + 64
    # shm delivery: passes are pipelined -- step i launches pass i and then
    # completes pass i-DEPTH+1 (up_run_async / up_run_wait), so the GPU never
    # waits for the host between passes and consecutive passes overlap on the
    # device (a pass's streaming K1a beside the previous passes' exact and
    # statistics kernels); NSLOT rotating record slots per rank
    # (NSLOT a multiple of the library's pass slots: each pass slot then cycles
    # through two record targets, i.e. two cached graphs)
    DEPTH = int(os.environ.get("UNIPEAK_BENCH_DEPTH", str(capi.MAX_IN_FLIGHT)))
    NSLOT = 2 * capi.MAX_IN_FLIGHT
    # at most MAX_IN_FLIGHT passes in flight (up_run_async), and rank 0's
    # reads trail by DEPTH steps while a slot is reused after NSLOT steps
    if not 1 <= DEPTH <= capi.MAX_IN_FLIGHT or NSLOT < 2 * DEPTH:
        raise SystemExit(f"UNIPEAK_BENCH_DEPTH={DEPTH}: must be 1..{capi.MAX_IN_FLIGHT}")
    pipelined = comm is None or gather_mode == "shm"
    if pipelined:
        tag = f"{os.environ.get('TORCHELASTIC_RUN_ID', 'run')}_{os.environ.get('MASTER_PORT', '0')}"
        nr = shard.NodeRecords(comm, cap, S, capi.REGION_DTYPE.itemsize, tag, nslots=NSLOT)
        g.host_register(*nr.my_range())
        board = shard.StepBoard(comm, tag) if comm is not None else None
        if rank == 0:
            from concurrent.futures import ThreadPoolExecutor
            pool = ThreadPoolExecutor(1)
    else:
        board = None
        rbuf = comm.target_buffer(cap, S, capi.REGION_DTYPE.itemsize)
        comm.torch.cuda.synchronize()
        g.set_record_target(rbuf.data_ptr(), cap)
    it = [0]           # steps launched
    bbase = [0]        # board index of this phase's step 0 (the board never rewinds)
    timed = [False]    # inside the timed region
    # timed passes with HIP events around K1a (the roofline sample): every
    # pass -- consecutive passes overlap and alternate between a K1a that runs
    # beside one earlier pass's kernels and one beside two, so a sparser
    # sample would see one phase only
    K1A_EVERY = int(os.environ.get("UNIPEAK_K1A_EVERY", "1"))
    reads = []         # rank 0: (step, future) of record reads in flight
    done_times = []    # per completed pass: library timings

    border = shard.BlockOrder([mine_all[sim_rank]] if sim_world > 1 else mine_all)

    def consume(parts):
        """rank 0: every rank's records in global unit order (zero-copy
        spans; the accepted count is taken once, after the timed region)"""
        spans, n = border.spans(parts)
        return n, parts

    read_s = [0.0, 0]  # host time of the rank-0 record reads (helper thread)

    def timed_read(j):
        if board is not None:  # every rank has completed pass j
            board.wait_done(bbase[0] + j)
        t = time.perf_counter()
        r = consume(nr.read(capi.REGION_DTYPE, j))
        read_s[0] += time.perf_counter() - t
        read_s[1] += 1
        if board is not None:
            board.post_read(bbase[0] + j)
        return r

    def read_step(j):
        return pool.submit(timed_read, j)

    def set_background(tags):
        # regions.cpp:205-213: tags / mappable, per strand when directional
        background = tags / mappable / (1 if nondir else 2)
        if bg_set[0] != background:
            while it[0] > len(done_times):  # parameters change only between passes
                g.run_wait()
                done_times.append(g.timings())
                if board is not None:
                    board.post_done(bbase[0] + len(done_times) - 1)
            g.set_params(args.bw, S, background, region_thr=25.0, kurt_thr=W["kurt"],
                         corr_thr=W["corr"], hit_thr=10.0 * s_nc, nondir=nondir, control=control,
                         want_corr=W["want_corr"])
            bg_set[0] = background

    def step():
        i = it[0]
        t0 = time.perf_counter()
        if not pipelined:  # multi-node: blocking pass + RCCL gather of device record buffers
            set_background(comm.global_tags(local_tags))
            t1 = time.perf_counter()
            g.run()
            done_times.append(g.timings())
            t2 = time.perf_counter()
            raw = comm.gather_target(rbuf)
            if raw is not None:
                consume([shard.parse_target(raw[k], cap, S, capi.REGION_DTYPE) for k in range(world)])
            it[0] += 1
            t3 = time.perf_counter()
            phase["allreduce"] += t1 - t0
            phase["launch"] += t2 - t1
            phase["gather_merge"] += t3 - t2
            return
        # slot i % NSLOT held step i-NSLOT: rank 0's read of it must be over
        # before this rank launches a pass into it
        while reads and reads[0][0] <= i - NSLOT:
            reads.pop(0)[1].result()
        if board is not None:
            b = bbase[0] + i
            if i >= NSLOT:
                board.wait_read(b - NSLOT)
            # the background's all-reduce of this step through the board
            board.post_tags(b, local_tags)
            tags = board.tags(b)
        else:
            tags = local_tags
        set_background(tags)
        t1 = time.perf_counter()
        # rank 0 reads pass i-DEPTH while later passes run (its helper thread
        # first waits until every rank has completed that pass)
        if rank == 0 and i >= DEPTH:
            reads.append((i - DEPTH, read_step(i - DEPTH)))
        ta = time.perf_counter()
        g.set_record_target(nr.my_slot_address(i), cap)
        if timed[0]:  # K1a events on every K1A_EVERY-th timed pass only (an event pair idles the GPU)
            g.set_timing(1 if i % K1A_EVERY == 0 else 0)
        tb = time.perf_counter()
        g.run_async()
        it[0] += 1
        t2 = time.perf_counter()
        sub["submit"] += ta - t1
        sub["target"] += tb - ta
        sub["run_async"] += t2 - tb
        if i >= DEPTH - 1:
            g.run_wait()
            done_times.append(g.timings())
            if board is not None:
                board.post_done(bbase[0] + len(done_times) - 1)
        t3 = time.perf_counter()
        phase["allreduce"] += t1 - t0
        phase["launch"] += t2 - t1
        phase["wait"] += t3 - t2

    def drain():
        """complete every pass; rank 0 reads the records of the steps not yet
        read (after every rank finished them)"""
        while it[0] > len(done_times):
            g.run_wait()
            done_times.append(g.timings())
            if board is not None:
                board.post_done(bbase[0] + len(done_times) - 1)
        if not pipelined:
            return None
        if comm is not None:
            comm.dist.barrier()
        res = None
        if rank == 0:
            last = it[0] - 1
            pend = [f for j, f in reads]
            reads.clear()
            for f in pend:
                res = f.result()
            for j in range(max(0, last - DEPTH + 1), last + 1):  # steps not read during the loop
                res = consume(nr.read(capi.REGION_DTYPE, j))
                if board is not None:
                    board.post_read(bbase[0] + j)
        return res

    def barrier():
        if comm is not None:
            comm.dist.barrier()

    def run_leg(name):
        """warm-up passes, then exactly args.steps timed steps under the leg's
        index policy (barrier + sync on both sides, max over ranks), then
        (--full) three blocking passes for the isolated per-kernel breakdown"""
        barrier()
        g.set_index_policy(policy_of[name])
        g.set_timing(2)  # warm-up passes report every phase
        for _ in range(args.warmup):
            step()
        drain()
        warm = [float(x) for x in done_times[-1]] if done_times else [0.0] * 5
        if rank == 0 and done_times:
            tt = done_times[-1]
            print(f"[bench] {name} warmup: K1 {tt[0]:.3f} ms (exact part {tt[4]:.3f}), K2 {tt[1]:.3f} ms, "
                  f"K3 {tt[2]:.3f} ms, pass wall {tt[3]:.3f} ms", file=sys.stderr, flush=True)
        # K1a algorithmic bytes per bp per strand per non-control sample: what
        # its stream reads -- the chunk-sum plane (1 byte per 16 bp) for one
        # directional track with the index on, else the TB-bit counts
        dens = g.scan_density()  # bytes per 1,024 positions of a unit
        alg_bytes = mine_bp * dens // 1024
        builds0 = g.index_state()[1]
        g.set_timing(1)  # timed passes: HIP events around K1a only
        timed[0] = True
        for k in phase:
            phase[k] = 0.0
        for k in sub:
            sub[k] = 0.0
        read_s[0], read_s[1] = 0.0, 0
        done_times.clear()
        bbase[0] += it[0]
        it[0] = 0
        barrier()
        if comm is not None:
            comm.torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        final = drain()  # inside the timed region: the last step's records reach rank 0
        barrier()
        if comm is not None:
            comm.torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        timed[0] = False
        builds = g.index_state()[1] - builds0  # index builds inside the timed steps
        dump = os.environ.get("UNIPEAK_BENCH_DUMP")
        if args.dump_outputs and rank == 0 and final is None:
            raise SystemExit("--dump-outputs: the records of a step reach rank 0 whole only on one node")
        # the merged records of the last step (rehearsals: UNIPEAK_BENCH_DUMP, one .npz)
        if final is not None and (dump or args.dump_outputs) and name == legs[0]:
            blocks, _, _ = border.blocks(final[1])
            recs = [b.copy() for _, b, _ in blocks]
            for (gunit, _, _), r in zip(blocks, recs):
                r["unit"] = gunit  # rank-local unit id -> global unit id
            recs = np.concatenate(recs) if recs else np.zeros(0, capi.REGION_DTYPE)
            counts = np.concatenate([c for _, _, c in blocks]) if blocks else np.zeros((0, S), np.uint32)
            if dump:
                np.savez(dump, recs=recs, counts=counts)
            if args.dump_outputs:
                dump_outputs(args.dump_outputs, recs, counts, {"n_regions": len(recs)})
        if final is not None:  # the last step's records: accepted count (outside the timing)
            final = (final[0], sum(int(np.count_nonzero(r["accepted"])) for r, _ in final[1] if len(r)))
        # after the timed region: blocking passes (nothing overlapping) for the
        # per-kernel breakdown of one pass on an otherwise idle GPU (--full)
        iso = None
        if args.full:
            iso = []
            if pipelined:
                g.set_record_target(nr.my_slot_address(it[0]), cap)
            g.set_timing(2)
            for _ in range(3):
                g.run()
                iso.append(g.timings())
            iso = [float(np.median([t[k] for t in iso])) for k in range(5)]
        # K1a = K1 minus its exact part (timing level 1: K1b = 0); level-0 passes carry no events
        k1a = [t[0] - t[4] for t in done_times if t[0] > 0] or [t[0] for t in done_times]
        k1a_ms = float(np.mean(k1a))
        my_achieved = alg_bytes / (k1a_ms * 1e-3) / 1e9
        if comm is not None:
            dt = comm.max_over_ranks(dt)
            achieved = comm.sum_over_ranks(my_achieved) / world  # mean per-GPU K1a GB/s
            k1a_max = comm.max_over_ranks(k1a_ms)
        else:
            achieved, k1a_max = my_achieved, k1a_ms
        if rank == 0:
            print(f"[bench] {name}: {dt * 1e3:.4f} ms/step, K1a {k1a_ms:.4f} ms ({alg_bytes / 1e6:.1f} MB), "
                  f"index builds {builds}; per-step phases (ms): " + ", ".join(
                      f"{k} {v / args.steps * 1e3:.3f}" for k, v in phase.items()) +
                  f"; record read {read_s[0] / max(read_s[1], 1) * 1e3:.3f} ms x{read_s[1]} (helper thread)"
                  "; launch = " + ", ".join(f"{k} {v / args.steps * 1e3:.3f}" for k, v in sub.items()),
                  file=sys.stderr, flush=True)
        return dict(dt=dt, k1a_ms=k1a_ms, k1a_max=k1a_max, achieved=achieved, alg_bytes=alg_bytes, dens=dens,
                    iso=iso, warm=warm, final=final, index_builds=builds)

    res_leg = {}
    for name in legs:
        res_leg[name] = run_leg(name)
    L0 = res_leg[legs[0]]
    dt, k1a_ms, k1a_max, achieved = L0["dt"], L0["k1a_ms"], L0["k1a_max"], L0["achieved"]
    alg_bytes, dens, iso, warm = L0["alg_bytes"], L0["dens"], L0["iso"], L0["warm"]
    final = L0["final"]
    last = (None, final if final is not None else (n0, 0), None)
    k1_ms = k1a_ms
    # one cold pass as a user's single run pays it (blocking up_run: first
    # launch -> records in host memory), median of 5: without the index
    # (the headline's pass), and with the index built inside it (--full)
    single = {}
    if pipelined:
        g.set_record_target(nr.my_slot_address(it[0]), cap)
    g.set_timing(0)
    for tag, pol in ((("no_index", capi.INDEX_NEVER), ("index_built_in_pass", capi.INDEX_ALWAYS))
                     if args.full and os.environ.get("UNIPEAK_BENCH_SINGLE", "1") != "0" else ()):
        g.set_index_policy(pol)
        ts = []
        for _ in range(5):
            g.invalidate_index()
            t = time.perf_counter()
            g.run()
            ts.append((time.perf_counter() - t) * 1e3)
        single[tag] = ts
    if rank == 0:
        value = genome / dt / 1e9
        if sim_world > 1:  # not a headline line: one rank's shard of an N-GPU plan
            print(json.dumps({"sim_world": sim_world, "sim_rank": sim_rank, "leg": legs[0],
                              "ms_per_step": round(dt * 1e3, 4),
                              "legs_ms_per_step": {k: round(v["dt"] * 1e3, 4) for k, v in res_leg.items()},
                              "shard_bp": int(sum(lens[units[k][0]] * nstr for k in mine)), "k1a_ms": round(k1a_ms, 4),
                              "k1_ms": round(k1_ms, 4), "warmup_timings_ms": [round(x, 4) for x in warm],
                              "isolated_ms": iso and [round(x, 4) for x in iso]}), flush=True)
            g.set_record_target(0, 0)
            g.close()
            if pool is not None:
                pool.shutdown()
            return
        traffic, traffic_src = (pmc_traffic(alg_bytes) if (world == 1 and args.workload == "hg19-dir1")
                                else (None, None))
        res = {
            "metric": METRIC,
            "value": round(value, 3),
            "unit": "Gbp/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt * 1e3, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f64",
            "data": "synthetic (device-generated hg19-shaped tag counts, DESIGN.md §8)",
            "config": {"workload": W["desc"], "baseline_config": W["baseline"],
                       "genome_bp": genome, "units": len(units), "samples": S,
                       "parallelism": f"contig{'' if nondir else '-strand'} units LPT over {world} GPU(s)"},
            "regions": {"candidates": int(last[1][0]), "accepted": int(last[1][1])},
            "index": ({"cold": "none: every pass reads only the packed 2-bit tracks (+ their overflow "
                               "table); nothing derived from them survives between passes "
                               "(UP_INDEX_NEVER, DESIGN.md §3) -- the reference's one pass per run",
                       "warm": "chunk-sum plane / pooled planes / pooled count tracks built once before "
                               "the timed steps and reused (UP_INDEX_ALWAYS): a re-scan of the same "
                               "tracks"}[legs[0]]),
            "index_builds_in_timed_steps": int(L0["index_builds"]),
            "roofline": {"bound": "hbm", "achieved": round(achieved, 1),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "traffic": traffic,
                         "traffic_unit": "GB per launch (rocprofv3 PMC FETCH_SIZE+WRITE_SIZE, gfx950-corrected)",
                         "traffic_source": traffic_src,
                         "kernel": (("k1a_fields_kernel" if (S - n_ctl == 1 and not nondir and args.bw <= 255)
                                     else "scan_kernel<..., kModeScreenF>") +
                                    " (K1a: stream of the 2-bit fields + screen)"
                                    if legs[0] == "cold" else
                                    "scan_kernel<..., kModeScreen> (K1a: stream + integer screen)"),
                         "kernel_ms": round(k1a_ms, 4), "kernel_ms_max_rank": round(k1a_max, 4),
                         "bytes_per_launch": int(alg_bytes),
                         "bytes_rule": (f"{dens / 1024} B per bp of a unit (" +
                                        ("chunk-sum plane: 1 byte per 16 positions of the pooled track"
                                         if dens == 64 else f"{TB}-bit counts of every pooled track") + ")"),
                         "kernel_note": "mean K1a duration over the timed passes (HIP events on the pass "
                                        "stream); passes overlap, so K1a shares the GPU with earlier "
                                        "passes' K1b/K2/K3"},
            "setup_s": round(gen_s, 2),
        }
        if args.full:  # the figures of the passes taken beside the timed steps
            res["roofline"].update({
                "isolated_ms": {"k1a": round(iso[0] - iso[4], 4), "k1b_k1x": round(iso[4], 4),
                                "k2": round(iso[1], 4), "k3": round(iso[2], 4),
                                "pass_wall": round(iso[3], 4)},
                "frac_isolated": round(alg_bytes / ((iso[0] - iso[4]) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                "hbm_copy_GBps": round(copy_gbps, 1),
                "frac_of_copy_rate": round(achieved / copy_gbps, 4)})
        # SURVEY §8(d)'s pricing: one uint32 count per bp per strand per
        # non-control sample (8 * S_nc B/bp over both strands), beside the
        # layout's algorithmic bytes the kernel actually reads
        survey_bytes = sum(lens[units[k][0]] * nstr * s_nc for k in mine_all[0]) * 4 if world == 1 else None
        rf = res["roofline"]
        rf["frac_step"] = round(alg_bytes / dt / 1e9 / HBM_PEAK_GBS, 4)  # whole pass at the step rate
        rf["step_note"] = ("frac_step = K1a's algorithmic bytes / ms_per_step (the whole step: K1a plus the "
                           "exact, segmentation and statistics kernels it overlaps, and rank 0's record read)")
        if survey_bytes:
            rf["bytes_rule_survey"] = "8 * S_nc B/bp (SURVEY 8(d): uint32 counts, both strands)"
            rf["bytes_per_launch_survey"] = int(survey_bytes)
            rf["frac_survey_rule"] = round(survey_bytes / (k1a_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)
            rf["survey_rule_note"] = ("above 1: the kernel does not read SURVEY's uint32 bytes -- the tracks are "
                                      f"{TB}-bit counts with an exact overflow table and a chunk-sum plane "
                                      "(DESIGN.md §3)")
        for name, Lg in res_leg.items():
            if name == legs[0]:
                continue
            res["value_" + name] = round(genome / Lg["dt"] / 1e9, 3)
            res[name] = {"ms_per_step": round(Lg["dt"] * 1e3, 4), "value": round(genome / Lg["dt"] / 1e9, 3),
                         "index_builds": int(Lg["index_builds"]),
                         "roofline": {"achieved": round(Lg["achieved"], 1),
                                      "frac": round(Lg["achieved"] / HBM_PEAK_GBS, 4),
                                      "kernel_ms": round(Lg["k1a_ms"], 4), "bytes_per_launch": int(Lg["alg_bytes"]),
                                      "bytes_rule": f"{Lg['dens'] / 1024} B per bp of a unit",
                                      "isolated_ms": {"k1a": round(Lg["iso"][0] - Lg["iso"][4], 4),
                                                      "k1b_k1x": round(Lg["iso"][4], 4), "k2": round(Lg["iso"][1], 4),
                                                      "k3": round(Lg["iso"][2], 4), "pass_wall": round(Lg["iso"][3], 4)}},
                         "regions": {"candidates": int((Lg["final"] or (0, 0))[0]),
                                     "accepted": int((Lg["final"] or (0, 0))[1])}}
        if args.full:
            res["single_pass_ms"] = {k: {"median": round(float(np.median(v)), 4), "runs": [round(x, 4) for x in v]}
                                     for k, v in single.items()} or None
            res["single_pass_note"] = ("one blocking up_run on an idle GPU, first launch -> records in host memory, "
                                       "median of 5; no_index: the headline's cold pass; index_built_in_pass: "
                                       "up_invalidate_index, then a pass that builds the planes/pooled tracks first")
        res["hw_queues"] = {"GPU_MAX_HW_QUEUES": os.environ.get("GPU_MAX_HW_QUEUES"),
                            "inherited": HWQ_INHERITED, "library_streams": 5,
                            "note": "set by bench.py before HIP initialisation; library streams: context "
                                    "(high priority), K1a (high priority), three chain streams"}
        if args.full and world == 1 and not args.no_cpu_baseline and args.workload == "hg19-dir1":
            res["cpu_baseline"] = cpu_baseline(contigs, args, value, bg_set[0], last[1])
        print(json.dumps(res), flush=True)
    g.set_record_target(0, 0)
    g.close()
    if pool is not None:
        pool.shutdown()
    if comm is not None:
        comm.dist.barrier()
        if nr is not None:
            nr.close()
        if board is not None:
            board.close()
        comm.dist.destroy_process_group()


def shift_pipeline(args, W):
    """configs[2] end to end on the device-resident genome, one step =
      strand_shift (src/strand_shift.cpp:133-259): one nondirectional pass
        (corr off, unscaled -t, Q13), the regions sorted by Region::sum()
        descending, strandCorr(0..150) of every region longer than 303
        positions (K4, up_shift_scan), the first 1000 with corr >= -u into
        the shift histogram, smoothed with Kernel(5), argmax over
        [minShift, maxShift+1-5);
      regions -D -y -s <best> (src/regions.cpp): one nondirectional pass
        over the tracks moved by the shift (forward +s, reverse -s, as the
        wiggle reader applies -s), strand correlation per region.
    Tracks of both passes are resident before timing (two contexts: the
    -s tracks are the spec's tracks moved by the shift the first pass
    finds, 75 for this generator; checked every step).  N = 1 only.
    The host sort is numpy's stable argsort (the CLI's std::sort order of
    equal sums, quirk Q15, only changes which tie is tested; tests cover it)."""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        raise SystemExit("hg19-shift runs on one GPU")
    contigs = load_table(W["tables"])
    genome = sum(L for _, L in contigs)
    mappable = genome & 0xFFFFFFFF
    lens = [L for _, L in contigs]
    bw, max_shift, min_shift, n_test, u_thr = args.bw, 150, 25, 1000, 0.3
    shift = 75  # the generator's strand shift; verified below
    ctx = []
    for off in (0, shift):
        g = capi.Lib(0)
        g.set_index_policy(capi.INDEX_NEVER)  # one pass per tool run, as the reference's (no index)
        g.set_params(bw, 1, 0.0029, nondir=True)
        tags = 0
        for ci, L in enumerate(lens):
            u = g.add_unit(L)
            for st in (0, 1):
                g.synth(u, st, 0, args.seed, ci, st, nondir=True, peaks=True,
                        offset=(off if st == 0 else -off))
                tags += g.tag_total(u, st, 0)
        ctx.append((g, tags))
    (ga, tags_a), (gb, tags_b) = ctx
    # strand_shift.cpp:131-142: background per position over both strands,
    # corr off, -t not scaled by the sample count (Q13)
    ga.set_params(bw, 1, tags_a / mappable, region_thr=25.0, kurt_thr=W["kurt"], corr_thr=-1.0,
                  hit_thr=10.0, nondir=True)
    gb.set_params(bw, 1, tags_b / mappable, region_thr=25.0, kurt_thr=W["kurt"], corr_thr=W["corr"],
                  hit_thr=10.0, nondir=True, want_corr=True)
    mk = capi.kernel_weights(5, 1.0)
    ph = {k: 0.0 for k in ("shift_pass", "sort_select", "shift_scan", "histogram", "regions_pass",
                           "shift_pass_up_run", "regions_pass_up_run")}
    info = {}
    delivered = []  # the last step's regions -s records and counts

    def step(timed):
        t0 = time.perf_counter()
        n = ga.run()
        tr = time.perf_counter()
        regs, _ = ga.regions_view()
        t1 = time.perf_counter()
        # the regions long enough to be tested, in the order of a stable sort
        # by sum descending -- only as far as the loop below reaches: the
        # top m by (sum desc, index asc) are selected in O(n) and sorted, and
        # the selection widens if more are needed (same order as a full
        # stable argsort)
        long_ = np.flatnonzero((regs["right"].astype(np.int64) - regs["left"] + 1) > 2 * max_shift + 3)
        key = (regs["sum"][long_].astype(np.uint64) << np.uint64(32)) | \
            (np.uint64(0xFFFFFFFF) - long_.astype(np.uint64))

        def top(m):
            if m >= len(key):
                return long_[np.argsort(key)[::-1]]
            part = np.argpartition(key, len(key) - m)[len(key) - m:]
            return long_[part[np.argsort(key[part])[::-1]]]
        elig = top(min(len(key), n_test + n_test // 4 + 16))
        t2 = time.perf_counter()
        # strand_shift.cpp:205-228: per region the first shift of the largest
        # correlation above -1 (K4 + a device reduction), then the first
        # n_test qualifying regions
        # (in chunks, as bin/strand_shift: the reference's loop stops at the
        # n_test-th qualifying region, so only the regions it reaches are
        # correlated)
        best_l, done, tested = [], 0, 0
        while tested < n_test and done < len(key):
            m = min(n_test + n_test // 4 + 16 if done == 0 else 2 * (n_test - tested) + 16, len(key) - done)
            if done + m > len(elig):
                elig = top(min(len(key), max(done + m, 2 * len(elig))))
            b_, c_ = ga.shift_best(elig[done:done + m], max_shift)
            q = np.flatnonzero(c_ >= u_thr)[:n_test - tested]
            best_l.append(b_[q])
            tested += len(q)
            done += m
        t3 = time.perf_counter()
        best = np.concatenate(best_l) if best_l else np.zeros(0, np.int64)
        ok = np.arange(len(best))
        freq = np.bincount(best[ok], minlength=max_shift + 1).astype(np.float64)
        # strand_shift.cpp:241-248: dens[i - 5 + j] += freq[i] * k5[j]; every
        # dens[k] receives its terms in ascending i, as in the reference loop
        dens = np.zeros(max_shift + 1)
        for d in range(-5, 6):
            lo, hi = max(0, -d), min(max_shift + 1, max_shift + 1 - d)
            dens[lo:hi] += freq[lo + d:hi + d] * mk[5 - d]
        cand = dens[min_shift:max_shift + 1 - 5]
        bs = int(min_shift + np.argmax(cand)) if cand.max() > 0 else 0
        t4 = time.perf_counter()
        if bs != shift:
            raise SystemExit(f"strand_shift found {bs}, the -s tracks were moved by {shift}")
        t4b = time.perf_counter()
        nb = gb.run()
        t4c = time.perf_counter()
        regs_b, cnt_b = gb.regions_view()
        acc = int(np.count_nonzero(regs_b["accepted"]))
        t5 = time.perf_counter()
        delivered[:] = [regs_b, cnt_b]  # views, valid until gb's next pass
        if timed:
            for k, v in zip(ph, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4, tr - t0, t4c - t4b)):
                ph[k] += v
        info.update(shift_candidates=int(n), eligible=int(len(key)), correlated=int(done), tested=int(len(ok)),
                    best_shift=bs,
                    regions_candidates=int(nb), regions_accepted=acc)

    for g, _ in ctx:
        g.set_timing(1)
    for _ in range(args.warmup):
        step(False)
    ka = []
    kb = []
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step(True)
        ka.append(ga.timings()[0])
        kb.append(gb.timings()[0])
    dt = (time.perf_counter() - t0) / args.steps
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, delivered[0], delivered[1],
                     {"n_regions": len(delivered[0]), "best_shift": info["best_shift"]})
    alg = genome * ga.scan_density() // 1024  # K1a of each pass
    k1a = float(np.mean(ka + kb))
    res = {
        "metric": METRIC, "value": round(genome / dt / 1e9, 3), "unit": "Gbp/s", "n_gpus": 1,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(dt * 1e3, 4),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64",
        "data": "synthetic (device-generated hg19-shaped tag counts, DESIGN.md §8)",
        "config": {"workload": W["desc"], "baseline_config": W["baseline"], "genome_bp": genome,
                   "units": len(lens), "samples": 1, "parallelism": "one GPU"},
        "pipeline": info,
        "phases_ms": {k: round(v / args.steps * 1e3, 4) for k, v in ph.items()},
        "roofline": {"bound": "hbm", "achieved": round(alg / (k1a * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(alg / (k1a * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                     "traffic": None, "kernel": "scan_kernel<..., kModeScreen> (K1a), both passes",
                     "kernel_ms": round(k1a, 4), "bytes_per_launch": int(alg),
                     "bytes_rule": f"{ga.scan_density() / 1024} B per bp (K1a's stream)"},
    }
    print(json.dumps(res), flush=True)
    for g, _ in ctx:
        g.close()


def cpu_baseline(contigs, args, gpu_value, background, gpu_regions):
    """The oracle (plain-C restatement of ProfileBuffer, oracle/) on the host
    cores, over the same synthetic genome with the GPU pass's background:
      value      1 core, hot path only (hits pre-generated, untimed), the
                 reference's own single-threaded mode (README:60-61);
      all_cores  the reference's contig-subset method (README:37): every
                 (contig, strand) unit on its own buffer, P threads;
      end_to_end the oracle CLI restatement of bin/regions on the synthetic
                 genome written as a wiggle file, beside this build's
                 bin/regions on the same file (tables compared).
    The candidate / accepted counts of the 1-core run are checked against
    the GPU pass's."""
    import shutil
    import subprocess
    import tempfile
    from concurrent.futures import ThreadPoolExecutor
    from tests.oracle_binding import Oracle
    orc = Oracle()
    names = [n for n, _ in contigs] if args.cpu_sample == "all" else args.cpu_sample.split(",")
    idx = [i for i, (n, _) in enumerate(contigs) if n in names]
    # the sample's contigs keep their hg19 contig indices for the generator:
    # pass lengths padded with zeros for skipped contigs
    lens = np.zeros(max(idx) + 1, np.uint32)
    for i in idx:
        lens[i] = contigs[i][1]
    npass, nrej, sec = orc.baseline(lens, args.seed, args.bw, 25.0, 50.0, 10.0, background)
    bp = int(lens.sum())
    out = {"value": round(bp / sec / 1e9, 4), "unit": "Gbp/s", "cores": 1, "kind": "port",
           "seconds": round(sec, 2),
           "sample": f"hg19 {'full genome' if args.cpu_sample == 'all' else args.cpu_sample} synthetic, "
                     f"directional, 1 sample, both strands ({bp} bp), oracle ProfileBuffer restatement, "
                     f"hits pre-parsed, same background as the GPU pass",
           "gpu_over_cpu": round(gpu_value / (bp / sec / 1e9), 1)}
    if args.cpu_sample == "all":
        out["regions_match_gpu"] = bool(npass + nrej == gpu_regions[0] and npass == gpu_regions[1])
        out["regions"] = {"candidates": int(npass + nrej), "accepted": int(npass)}
    # all cores: (contig, strand) units on P threads -- P = the box's CPU
    # share (16 per GPU) and, when more CPUs are visible, P = every visible
    # CPU up to the unit count (the reference's contig-subset method cannot
    # use more processes than units)
    try:
        ncpu = len(os.sched_getaffinity(0))
    except AttributeError:
        ncpu = os.cpu_count() or 1
    jobs = sorted(((int(lens[c]), c, st) for c in idx for st in (0, 1)), reverse=True)
    with ThreadPoolExecutor(max(1, min(16, ncpu))) as ex:  # generation untimed
        hits = list(ex.map(lambda j: orc.synth_track(args.seed, j[1], j[2], False, j[0], args.bw, True),
                           jobs))

    def unit(a):
        t = time.perf_counter()
        r = orc.baseline_unit(a[1][0], a[1][1], a[0][1], a[0][2], args.bw, 25.0, 50.0, 10.0, background)
        return r, time.perf_counter() - t

    def run_p(P):
        with ThreadPoolExecutor(P) as ex:  # ctypes releases the GIL
            t0 = time.perf_counter()
            rs = list(ex.map(unit, zip(jobs, hits)))
            wall = time.perf_counter() - t0
        return rs, wall

    for key, P in (("all_cores", max(1, min(16, ncpu))), ("all_cores_visible", min(ncpu, len(jobs)))):
        if key == "all_cores_visible" and P <= 16:
            break
        rs, wall = run_p(P)
        ut = [t for _, t in rs]
        out[key] = {"value": round(bp / wall / 1e9, 4), "unit": "Gbp/s", "cores": P,
                    "host_cpus_visible": ncpu, "wall_s": round(wall, 3),
                    # the unit-level bound on the speed-up: total unit time over the
                    # longest unit (chr1's strand), whatever the core count
                    "unit_bound_speedup": round(sum(ut) / max(ut), 2),
                    "regions": {"candidates": int(sum(a + b for (a, b), _ in rs)),
                                "accepted": int(sum(a for (a, _), _ in rs))},
                    "note": "(contig, strand) units on P threads, largest first; hits pre-generated"}
    del hits
    if args.cpu_sample != "all" or os.environ.get("UNIPEAK_BENCH_E2E", "1") == "0":
        return out
    # end to end through the CLIs on the same synthetic genome
    from tests.make_wig import write_sample
    d = tempfile.mkdtemp(prefix="unipeak_e2e_", dir="/tmp")
    try:
        with open(os.path.join(d, "contigs.txt"), "w") as f:
            for n, L in contigs:
                f.write(f"{n}\t{L}\n")
        write_sample(os.path.join(d, "s0.wig"), "s0", orc, contigs, args.seed, False, True, args.bw,
                     workers=P)
        e2e = {}
        for tag, exe in (("oracle_cli", [os.path.join(ROOT, "oracle", "_build", "orc"), "regions"]),
                         ("bin_regions", [os.path.join(ROOT, "bin", "regions")])):
            t0 = time.perf_counter()
            r = subprocess.run(exe + ["-q", "-f", "-c", "contigs.txt", "-o", f"{tag}.txt", "s0.wig"],
                               cwd=d, capture_output=True, timeout=300)
            e2e[tag + "_s"] = round(time.perf_counter() - t0, 3)
            if r.returncode != 0:
                e2e[tag + "_error"] = r.stderr.decode()[-300:]
        e2e["oracle_cli_gbps"] = round(bp / e2e["oracle_cli_s"] / 1e9, 4)
        e2e["bin_regions_gbps"] = round(bp / e2e["bin_regions_s"] / 1e9, 4)
        a, b = (os.path.join(d, f"{t}.txt") for t in ("oracle_cli", "bin_regions"))
        e2e["tables_identical"] = bool(os.path.exists(a) and os.path.exists(b) and
                                       open(a, "rb").read() == open(b, "rb").read())
        e2e["note"] = ("wall time of each CLI process on the synthetic hg19 wiggle file (parse + hot path + "
                       "write; bin/regions includes HIP initialisation); oracle_cli is 1 core")
        out["end_to_end"] = e2e
    finally:
        shutil.rmtree(d, ignore_errors=True)
    return out


if __name__ == "__main__":
    sys.exit(main() or 0)
