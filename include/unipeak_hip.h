/*
 * include/unipeak_hip.h -- the drop-in C-ABI boundary of unipeak-mi355x.
 *
 * The reference's hot path is an in-process C++ class driven position by
 * position (misc/peakcall.hpp:57-77):
 *
 *   Kernel(bw, 1/background)                         misc/kernel.hpp:16
 *   ProfileBuffer(kernel, r, k, u, t, fwd, control,
 *                 coeffs, contigs, regionsOut, prof) misc/peakcall.hpp:57-69
 *   ProfileBuffer::add(counts, contig, pos, fwd)     misc/peakcall.hpp:76
 *   ProfileBuffer::flushContig()                     misc/peakcall.hpp:75
 *   nRegions()/nRegionRejects()/nTagsInRegions()     misc/peakcall.hpp:71-74
 *   Region::exptSums/posKurtosis/strandCorr          misc/data.hpp:66-72
 *
 * On MI355X the same work is done in batches: every add() that one buffer
 * receives between two flushes (one "unit" = one buffer x one contig pass)
 * is a dense per-position count track resident in HBM, and up_run()
 * performs, for all units at once, what the sequence of add()/flushContig()
 * calls computes: pooled counts, the Epanechnikov KDE, the threshold scan,
 * region segmentation and processRegion()'s statistics and filters.
 * Mapping of entry points to the reference interface:
 *
 *   up_kernel_weights   <- Kernel::Kernel            misc/kernel.cpp:16-35
 *   up_open/up_set_params <- ProfileBuffer ctor      misc/peakcall.cpp:88-135
 *   up_add_unit + up_unit_scatter (or up_unit_pack)
 *                        <- the add() calls of one unit misc/peakcall.cpp:161-222
 *   up_run              <- add()'s window scatter + processPosition +
 *                          processRegion + flushContig  misc/peakcall.cpp:33-86,224-231
 *   up_get_regions      <- regionsOut vector + Region statistics
 *                          misc/peakcall.cpp:45, misc/data.cpp:104-193
 *   up_shift_scan       <- Region::strandCorr(shift) loop src/strand_shift.cpp:205-228
 *   up_unit_profile_text <- FormatOutStream::write(PosScore), the -w lines
 *                          misc/format.cpp:1091-1132
 *   up_unit_profile_bigwig <- the same lines through extras/wigs2bigwigs.pl
 *                          (wigToBigWig -clip): items, sections, zoom records
 *
 * Conventions: plain C types only; the caller owns host buffers, the library
 * owns device memory; one context per GPU, driven by one host thread (not
 * re-entrant, like ProfileBuffer).  Every entry point returns UP_OK (0) or a
 * negative UP_E_* code (up_strerror); nothing exits the process.
 */
#ifndef UNIPEAK_HIP_H
#define UNIPEAK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UP_OK 0
#define UP_E_ARG (-1)         /* bad argument */
#define UP_E_HIP (-2)         /* HIP runtime error */
#define UP_E_NOMEM (-3)       /* device allocation failed */
#define UP_E_STATE (-4)       /* call out of order (e.g. no params) */
#define UP_E_UNSUPPORTED (-5) /* configuration outside the GPU path */
#define UP_E_NODEV (-6)       /* no HIP device */
#define UP_E_INTERNAL (-7)    /* internal consistency check failed */

typedef struct up_ctx up_ctx;

/* Parameters of one ProfileBuffer pair (misc/peakcall.hpp:57-69) as the
 * CLI computes them (src/regions.cpp:152-232, src/strand_shift.cpp:131-142). */
typedef struct {
    uint16_t bw;              /* kernel bandwidth (-b) */
    uint16_t n_samples;       /* S = all samples, controls included */
    int32_t nondir;           /* 0: one strand per unit; 1: both strands in one unit */
    double background;        /* kernel sums to 1/background */
    double region_thr;        /* -r */
    double kurt_thr;          /* -k (0 disables) */
    double corr_thr;          /* -u (<= -1 disables) */
    double hit_thr;           /* already multiplied by S_nc where the CLI does */
    const uint8_t *is_control;/* [S] or NULL */
    const double *coeffs;     /* NULL or [n_coeffs] = normalised -z coefficients */
    uint32_t n_coeffs;
    int32_t want_corr;        /* evaluate strandCorr(0) for every region */
} up_params;

#define UP_CLOSE_RULE 0xFFFFFFFFu
/* region threshold <= 0 (quirk Q11, run in parallel): closed by the add
 * after the unit's first add at pos >= right + bw + 1 (the first add at a
 * larger position), else by the unit's flush */
#define UP_CLOSE_Q11 0xFFFFFFFEu
/* region threshold <= 0: the region the buffer's previous unit left open
 * after its flush, relabelled to this unit (misc/peakcall.cpp:164-168) and
 * closed by this unit's first add at a position above its first add's, else
 * by its flush; left/right/peak are positions of the previous unit */
#define UP_CLOSE_Q11_HEAD 0xFFFFFFFDu

/* One candidate region (accepted or rejected by processRegion). */
typedef struct {
    uint32_t unit;            /* unit the region was closed in */
    uint32_t left, right;     /* inclusive positions (right may exceed the contig, Q16) */
    uint32_t peak;            /* first position of the maximal f+r */
    uint32_t sum;             /* Region::sum() (uint32, wraps) */
    uint32_t nonctl_sum;      /* sum over non-control samples of exptSums */
    int32_t accepted;         /* passed the hit/kurtosis/correlation filters */
    uint32_t close_pos;       /* UP_CLOSE_RULE: closed by the unit's first add at
                                 pos >= right + bw + 2, else by its flush;
                                 UP_CLOSE_Q11 / UP_CLOSE_Q11_HEAD: threshold
                                 <= 0, see above;
                                 0: closed by the unit's flush; otherwise the
                                 position of the add whose retirement closed it
                                 (head-hit units replayed by the emulator, Q1) */
    double peak_score;        /* f+r at peak */
    double kurtosis;          /* Region::posKurtosis() */
    double corr;              /* Region::strandCorr(0) or NaN when not evaluated */
} up_region;

/* library / device */
int up_version(void);
/* bits per stored count in a device track: the K1a stream
 * reads bits/8 bytes per position per strand per non-control sample */
int up_track_bits(void);
const char *up_strerror(int code);
int up_device_count(int *n);

/* Kernel::Kernel(bw, sum) -- 2*bw+1 weights into w (host computation). */
int up_kernel_weights(uint16_t bw, double sum, double *w);

#define UP_G6_MAX 16
/* printf("%g", v) into out (no terminator, at most UP_G6_MAX bytes), host
 * computation, the routine the device formatter runs (csrc/fmt_g6.h: six
 * digits correctly rounded from the exact binary value in integer arithmetic);
 * *n = bytes written, 0 when v is outside the range that routine formats
 * itself: it formats every finite v with 2^-67 <= |v| < 2^60 (which contains
 * 1e-20 <= |v| < 1e18) and nothing else -- not 0, subnormals, NaN, infinities */
int up_format_g6(double v, char *out, int *n);
/* (float)strtod of that text without making it, host computation, the routine
 * the device's bigWig kernels run (csrc/fmt_g6.h: the six digits D and their
 * exponent give the text's value D * 10^k; for |k| <= 22 one IEEE multiply or
 * divide of two exact doubles is strtod's double, and the cast rounds it to
 * float).  *ok = 0 (and *out = 0): v is outside up_format_g6's range, or its
 * text is below 1e-17 (k < -22). */
int up_g6_to_float(double v, float *out, int *ok);

int up_open(int hip_device, up_ctx **out);
void up_close(up_ctx *ctx);
int up_set_params(up_ctx *ctx, const up_params *p);

/* Units.  A unit is one ProfileBuffer (buffer_id 0 = forward buffer, 1 =
 * reverse buffer) over one contig pass; units of one buffer must be added in
 * the order the buffer sees them.  nstrands is 1 (directional) or 2
 * (nondirectional: strand 0 forward, 1 reverse).  Tracks start zeroed and
 * cover positions 1..contig_len; in device memory they are up_track_bits()-bit
 * counts (2: four positions per byte) whose largest value is an escape into
 * an exact per-unit overflow table, so any uint32 count can
 * be written.
 * Quirk Q1 (misc/peakcall.cpp:177-183): a unit with pooled tags at a position
 * <= bw is replayed by the exact state machine; if all of its adds sit at
 * positions <= bw its leftover state leaks into the buffer's NEXT unit, which
 * must then be in the same context (the reference driver's chain). */
int up_add_unit(up_ctx *ctx, uint32_t contig_len, int32_t nstrands,
                int32_t buffer_id, uint32_t *unit_id);
int up_unit_count(up_ctx *ctx, uint32_t *n);
/* replace a track from DEVICE-resident dense uint32 counts: position p
 * (1-based) at dev_counts[p-1], contig_len elements (same device) */
int up_unit_pack(up_ctx *ctx, uint32_t unit, int32_t strand, uint16_t sample,
                 const uint32_t *dev_counts);
/* write n (pos, count) host pairs into a track: positions 1..len, each at
 * most once per call (UP_E_ARG otherwise: one nibble written twice would OR
 * two counts together); a count of 0 clears the position */
int up_unit_scatter(up_ctx *ctx, uint32_t unit, int32_t strand, uint16_t sample,
                    size_t n, const uint32_t *pos, const uint32_t *counts);
/* fill a track with the synthetic hg19-shaped spec */
int up_unit_synth(up_ctx *ctx, uint32_t unit, int32_t strand, uint16_t sample,
                  uint64_t seed, uint32_t contig_index, int32_t synth_strand,
                  int32_t nondir, int32_t with_peaks);
/* the same track moved by `offset` positions, as the wiggle reader's -s
 * shift moves it (forward strand +s, reverse -s, misc/format.cpp:693-705):
 * position p holds the spec's count at p - offset; counts that leave
 * [1, contig_len] are dropped */
int up_unit_synth_offset(up_ctx *ctx, uint32_t unit, int32_t strand, uint16_t sample,
                         uint64_t seed, uint32_t contig_index, int32_t synth_strand,
                         int32_t nondir, int32_t with_peaks, int32_t offset);
/* the same with peak_seed != 0: replicate samples -- peak
 * centres drawn from peak_seed and shared by every sample generated with it,
 * per-sample heights, centre jitter (-20..+20) and tag offsets from `seed`;
 * peak_seed 0 is up_unit_synth_offset */
int up_unit_synth_ex(up_ctx *ctx, uint32_t unit, int32_t strand, uint16_t sample,
                     uint64_t seed, uint32_t contig_index, int32_t synth_strand,
                     int32_t nondir, int32_t with_peaks, int32_t offset, uint64_t peak_seed);
/* total tags of one track (sum of its counts, uint64) */
int up_unit_tag_total(up_ctx *ctx, uint32_t unit, int32_t strand, uint16_t sample,
                      uint64_t *total);
/* override the last add position of a unit (host knows control-only adds) */
int up_unit_set_last_add(up_ctx *ctx, uint32_t unit, uint32_t last_add);
int up_unit_last_add(up_ctx *ctx, uint32_t unit, uint32_t *last_add);
int up_reset_units(up_ctx *ctx);

/* Run K1..K3 over every unit (stream-ordered, blocking).  A region
 * threshold <= 0 makes the leap branch of processPosition live (quirk Q11):
 * with non-negative scores every run of processed positions is a region,
 * found in parallel (K1q; records as UP_CLOSE_Q11 / UP_CLOSE_Q11_HEAD
 * describe).  A unit that processes position 1 (an add at <= bw + 1) adds a
 * short exact replay (K0) around it, from the start of the buffer's
 * previous unit's last run to the first clean leap past it; those records
 * name their closing add in close_pos like the whole-buffer replay's.
 * bw > UP_MAX_PARALLEL_BW (511: K1's register-resident halo of NH <= 8
 * 64-position words) with a threshold > 0 runs K1w, the parallel scan for
 * wide kernels (up to 32767, a window of 65535 cells).  On directional units
 * it is pipelined like K1, with or without the -w capture, and its dense
 * profile comes from wide_profile_kernel.  On nondirectional units it scores
 * both strands (forwardScore + reverseScore), the strand correlation comes
 * from wide_corr_kernel between K2 and K3 and up_shift_scan / up_shift_best
 * form the regions' dense scores with the same sums; those passes run inside
 * this blocking call only -- up_run_async and up_unit_profile* still refuse
 * such a context (UP_E_UNSUPPORTED), and with the -w capture on, or under
 * UNIPEAK_WIDE_ND=0 (read at up_open, for A/B runs), it takes the replay
 * below.  Wider kernels (32768..65535, where
 * the reference's UShort retirement count wraps, misc/peakcall.cpp:172-177)
 * take the whole-buffer replay.  bw > 511 (up to 32767) with a threshold
 * <= 0 on directional units with the -w capture off and no coefficient below
 * 0 runs wide K1q: the runs of processed positions and their peaks from
 * parallel kernels (wide_runs_kernel, wide_peak_kernel), K2 / K3, the
 * placement and the head chains as for K1q, inside this blocking call only
 * (UNIPEAK_WIDE_Q11=0, read at up_open, keeps the replay for A/B runs).
 * Nondirectional units take wide K1q under the same conditions once
 * up_set_wide_q11_nd is on: peaks of forwardScore + reverseScore, the strand
 * correlation of regions up to 65536 stored positions from wide_corr_kernel
 * and of longer ones from wide_corr_stage_kernel / wide_corr_chain_kernel.
 * A negative coefficient at a threshold <= 0,
 * the -w capture with a head unit at a threshold <= 0, and bw > 511 at a
 * threshold <= 0 on nondirectional units without up_set_wide_q11_nd or with the -w capture on, bw from
 * 32768 on, or nondirectional units above 511 with the -w
 * capture on run the exact
 * state machine over every unit instead (K0, as independent chains from
 * every run start, one chain per buffer with the -w capture on: exact, far
 * slower than the scans); up_run_async and up_unit_profile* refuse those
 * (UP_E_UNSUPPORTED).  up_shift_scan correlates a
 * replayed region's stored scores (Region::scores), as strandCorr does.
 * UNIPEAK_WIDE, UNIPEAK_Q11_REPLAY and UNIPEAK_Q11_HEADS are read at up_open
 * like the other switches that pick a scan (csrc/route.h holds the policy).
 * With a threshold <= 0 the last region of a unit is still open after its
 * flush and is closed in the buffer's next unit (UP_CLOSE_Q11_HEAD); the
 * last region of a buffer's last unit in the context is never closed (the
 * reference never writes it).  So every unit of one buffer must be in ONE
 * context at -r <= 0: a caller that splits a buffer's units over contexts
 * or ranks loses the region that crosses the split (bin/regions' multi-device
 * split keeps buffers whole for this reason). */
#define UP_MAX_PARALLEL_BW 511
int up_run(up_ctx *ctx, uint64_t *n_regions);
/* Pipelined form of up_run: up_run_async enqueues one pass and returns
 * (at most UP_MAX_IN_FLIGHT passes in flight); up_run_wait completes the OLDEST pass in
 * flight and makes its records current (as up_run would).  Passes in flight
 * overlap on the device: a pass's streaming K1a starts when the previous
 * pass's K1a has ended, beside that pass's exact/segmentation/statistics
 * kernels.  Each pass delivers into the record target that was set when it
 * was launched, so a caller rotates targets; with host delivery the view of
 * a pass stays valid until the UP_MAX_IN_FLIGHT-th following launch.  Units and
 * parameters cannot change while a pass is in flight (UP_E_STATE).  The HIP
 * calls of an async pass run on the context's own launcher thread
 * (UNIPEAK_LAUNCHER=0: on the caller's); a launch failure is returned by the
 * up_run_wait of that pass.  The context is still driven by one caller thread. */
#define UP_MAX_IN_FLIGHT 5
int up_run_async(up_ctx *ctx);
int up_run_wait(up_ctx *ctx, uint64_t *n_regions);
/* device timing of passes launched from now on (passes in flight keep
 * theirs): 0 = wall time only, 1 = + K1a (HIP events around the streaming
 * kernel), 2 = every phase (default).  Each event pair costs a few
 * microseconds of idle GPU between kernels. */
int up_set_timing(up_ctx *ctx, int level);
/* Copy region records (unit-major, left-ascending) and optionally the
 * per-sample exptSums [n][S]. */
int up_get_regions(up_ctx *ctx, up_region *out, uint32_t *counts, size_t cap);
/* Zero-copy view of the same records: host memory owned by the context
 * (pinned), valid until the next up_run / up_reset_units / up_close. */
int up_regions_view(up_ctx *ctx, const up_region **regions, const uint32_t **counts,
                    uint64_t *n);

/* Multi-GPU delivery: make up_run write the records into a caller-owned
 * buffer laid out as
 *   [uint64 n][cap x up_region][cap x n_samples x uint32 exptSums]
 * either DEVICE memory of this context's GPU (hand it to RCCL without a host
 * round trip) or HOST memory, e.g. a node-shared segment rank 0 reads
 * directly (the library pins it and K3 writes through the mapping).
 * up_run fails with UP_E_NOMEM if a pass yields more than cap records.
 * buf = NULL restores host delivery (up_get_regions / up_regions_view). */
int up_set_record_target(up_ctx *ctx, void *buf, uint64_t cap);
/* pin + map a host range once (e.g. every record slot of a node-shared
 * segment), so switching record targets inside it costs nothing; released
 * by up_close */
int up_host_register(up_ctx *ctx, void *ptr, uint64_t bytes);

/* strandCorr(shift) for shift = 0..max_shift of the given regions
 * (indices into up_get_regions order); out is [n][max_shift+1]. */
int up_shift_scan(up_ctx *ctx, const uint64_t *region_idx, size_t n,
                  uint16_t max_shift, double *out);
/* the same regions reduced on the device to strand_shift's per-region
 * choice (src/strand_shift.cpp:209-217): best_shift = the first shift whose
 * strandCorr is the largest value above -1 (0 if none), best_corr = that
 * value (-1 if none) */
int up_shift_best(up_ctx *ctx, const uint64_t *region_idx, size_t n,
                  uint16_t max_shift, uint16_t *best_shift, double *best_corr);

/* The per-dataset index (DESIGN.md §3 "Index policy"): data derived from
 * the packed tracks that repeated passes over the same tracks may reuse --
 * per track a chunk-sum plane (1 byte per 16 positions), per unit a pooled
 * plane and, with several pooled samples, a pooled count track (1 byte per
 * position and strand).  The reference makes ONE pass per run
 * (src/regions.cpp:311-391): a pass without the index reads only the packed
 * tracks and pays no build.  Policies:
 *   UP_INDEX_AUTO   (default) the first pass after a track or pooling change
 *                   runs without it; the index is built (one launch per
 *                   kind over every stale unit) before the second;
 *   UP_INDEX_NEVER  no pass uses it: every pass costs what one cold pass
 *                   costs (bw > UP_MAX_PARALLEL_BW still builds it: K1w
 *                   screens on the planes);
 *   UP_INDEX_ALWAYS built before the first pass.
 * Refused while a pass is in flight (UP_E_STATE).  up_invalidate_index drops
 * what was built (the next pass that wants it rebuilds it; AUTO counts
 * passes anew).  up_index_state: *on = the next pass uses the index now,
 * *builds = index builds so far in this context. */
#define UP_INDEX_AUTO 0
#define UP_INDEX_NEVER 1
#define UP_INDEX_ALWAYS 2
int up_set_index_policy(up_ctx *ctx, int policy);
int up_invalidate_index(up_ctx *ctx);
int up_index_state(up_ctx *ctx, int *on, uint64_t *builds);
/* Read-only view of one unit's index, for tests and tools; on no pass's
 * path.  Both calls first settle the passes in flight and bring the unit
 * table and the index up to date exactly as the next pass would (so under
 * UP_INDEX_ALWAYS, or where the next pass is a wide one, a stale index is
 * built and counted in up_index_state's builds); they change nothing else.
 * up_unit_layout: the geometry of the unit's arrays -- stride = bytes per
 * track (a multiple of 256), pad_pos = zero positions in front of position 1
 * (position p is field pad_pos + p - 1), track_bits = up_track_bits(),
 * index_on as up_index_state reports it, has_pooled = the pooled plane is
 * kept (nondirectional units, several pooled samples or coefficients; no
 * kernel reads it otherwise), has_pct = the unit holds a pooled count track.
 * up_unit_index_read copies one array to host memory as it lies on the
 * device (csrc/kernels.h describes the bytes), ntracks = nstrands * n_samples,
 * track (strand, sample) at index strand * n_samples + sample:
 *   UP_IDX_TRACKS  the packed tracks, ntracks * stride bytes
 *   UP_IDX_CSUM    the chunk-sum planes, ntracks * stride / 4 bytes
 *   UP_IDX_POOLED  the unit's pooled plane, stride / 4 bytes
 *   UP_IDX_PCT     the pooled count track, nstrands * 4 * stride bytes
 * *n (optional) = the array's size, also when cap is too small.  UP_E_STATE:
 * no parameters yet, the index is not on after the sync (UP_INDEX_NEVER, the
 * first pass under UP_INDEX_AUTO, 4-bit tracks), UP_IDX_POOLED without
 * has_pooled, or UP_IDX_PCT without has_pct; UP_E_ARG: unit out of range, an unknown
 * `what`, dst = NULL, or cap below the array's size. */
typedef struct up_unit_layout_t {
    uint64_t stride;
    uint32_t len;
    int32_t nstrands;
    int32_t n_samples;
    int32_t pad_pos;
    int32_t track_bits;
    int32_t index_on;
    int32_t has_pooled;
    int32_t has_pct;
} up_unit_layout_t;
#define UP_IDX_TRACKS 0
#define UP_IDX_CSUM 1
#define UP_IDX_POOLED 2
#define UP_IDX_PCT 3
int up_unit_layout(up_ctx *ctx, uint32_t unit, up_unit_layout_t *out);
int up_unit_index_read(up_ctx *ctx, uint32_t unit, int what, void *dst, uint64_t cap, uint64_t *n);
/* which statistics kernel (K3) the pass completed last (up_run, up_run_wait)
 * was launched with: 0 the general kernel, 1 the batched kernel for one
 * directional sample with a wave per region, 2 the same with a lane per
 * region (picked when the pass before it produced >= 16,384 regions;
 * DESIGN.md §4 "Round 6"); -1 when that pass launched no K3 (no units, the
 * K0 replay) or no pass has completed.  For tests and A/B runs: the records
 * do not depend on it. */
int up_last_stats_kind(up_ctx *ctx);
/* which exact kernel (K1b) the pass completed last was launched with: 0 the
 * generic scan kernel's exact mode, 1 the pipelined kernel for one pooled
 * directional sample with the Q keys on (DESIGN.md §4 "K1b for one
 * directional sample"; UNIPEAK_K1B_ONE=0 at up_open keeps the generic one);
 * -1 when that pass launched no K1b (no units, a threshold <= 0, a bandwidth
 * above 511, the K0 replay) or no pass has completed.  For tests and A/B
 * runs: the records do not depend on it. */
int up_last_exact_kind(up_ctx *ctx);
/* how the pass completed last found its regions: 0 K1 (K1a + K1b), 1 K1w
 * (bw above 511), 2 K1q (a threshold <= 0; above bw 511 its wide form, up to
 * 32767: on directional units, and on nondirectional ones with
 * up_set_wide_q11_nd on), 3 the exact replay of every unit
 * (K0); -1 when no pass has completed or it had no units.  The K0 chains of
 * head units inside a K1 / K1w / K1q pass do not change the value.  For
 * tests and A/B runs: the records do not depend on it. */
int up_last_scan_kind(up_ctx *ctx);
/* bytes the streaming scan (K1a) reads per 1,024 positions of a unit in the
 * index state of the moment (its algorithmic bytes): 64 when
 * it streams a chunk-sum plane (index on and bw <= 255: the pooled track's
 * own plane, or the unit's pooled plane of several samples / both strands),
 * else 1024 * up_track_bits() / 8 per pooled track and strand */
int up_scan_density(up_ctx *ctx, uint32_t *bytes_per_1024);
/* device-side timings of the last up_run in ms: [0]=K1 scan, [1]=K2
 * segment, [2]=K3 stats (with wide_corr_kernel, the strand correlation of a
 * nondirectional K1w or wide K1q pass -- behind wide K1q with the stage and
 * chain kernels of its long regions --, or wide K1q's peak kernels, which run
 * just before K3; wide K1q's run kernel counts under [0]), [3]=whole up_run wall, [4]=K1 launches; with n > 5
 * also [5]=the dense-profile kernel of the last up_unit_profile* call (HIP
 * events around it); with n > 6 also [6]=K0 and [7]=the placement kernels of
 * the last pass that placed its head units itself (up_set_head_place) at
 * timing level 2, else 0; with n > 8 also [8]=the text kernels of the last
 * up_unit_profile_text call (HIP events around them; [5] is then that call's
 * dense-profile kernel); with n > 9 also [9]=the bigWig kernels of the last
 * up_unit_profile_bigwig call (likewise) */
/* achievable HBM rate: a float4 streaming copy kernel of `bytes` (a multiple
 * of 16; best of reps),
 * GB/s counting read + write (the bench's copy-rate reference) */
int up_hbm_copy_gbps(up_ctx *ctx, uint64_t bytes, int reps, double *gbps);
int up_timings(up_ctx *ctx, double *ms, int n);
/* dense per-position score f+r of one unit (testing/-w): out[len].  K1's
 * fused profile path up to UP_MAX_PARALLEL_BW; wider kernels where K1w runs
 * (directional units, a threshold > 0, bw up to 32767): wide_profile_kernel,
 * every score the ascending sum K1w forms, out_r all zero; the same kernel
 * where wide K1q runs (a threshold <= 0, the -w capture
 * off: it does not look at the threshold).  Nondirectional
 * units above UP_MAX_PARALLEL_BW: refused by default; with
 * up_set_wide_nd_full on (a threshold > 0) or up_set_wide_q11_nd on (a
 * threshold <= 0 where wide K1q runs), the kernel's two-strand form fills
 * out_f with forwardScore and out_r with reverseScore, each its own ascending
 * sum (the caller adds them; out_r = NULL is UP_E_ARG there).  Refused
 * (UP_E_UNSUPPORTED) wherever up_run takes the exact replay of every unit. */
int up_unit_profile(up_ctx *ctx, uint32_t unit, double *out_f, double *out_r,
                    uint32_t len);
/* -w for units the exact replay produced (K0: quirk Q1 head hits, -r <= 0
 * with a unit processing position 1 or a negative coefficient,
 * bw > UP_MAX_PARALLEL_BW outside K1w), whose retirements the dense KDE does not
 * reproduce.  (A K1w pass keeps running K1w with the capture on: units without
 * head hits report resync = 0 and no entries, head units the K0 head replay's
 * entries and its resync point, as K1 passes do.  Nondirectional units above
 * UP_MAX_PARALLEL_BW: by default the capture sends them to the replay of
 * every unit; with up_set_wide_nd_full on they keep K1w like the rest.)  With the
 * capture on before up_run, the replay records every processPosition() with
 * a nonzero score (misc/peakcall.cpp:80-83: profileOut_->write), and
 * up_unit_replay_profile returns them for one unit in emission order:
 * event[i] = index of the unit's add() whose retirement loop wrote it
 * (UP_FLUSH_EVENT: the unit's flushContig()), pos[i], score[i] = f + r.
 * resync = 0: the unit was not replayed (up_unit_profile_range gives its
 * profile); X: the entries cover positions < X and the dense KDE the rest;
 * UP_FLUSH_EVENT (0xFFFFFFFF): the whole unit was replayed.  Call with
 * event/pos/score NULL to get n. */
#define UP_FLUSH_EVENT 0xFFFFFFFFu
int up_set_profile_capture(up_ctx *ctx, int on);
int up_unit_replay_profile(up_ctx *ctx, uint32_t unit, uint32_t *resync, uint64_t *n,
                           uint32_t *event, uint32_t *pos, double *score, uint64_t cap);
/* the same for positions [first, first + count) (first >= 1; the range may
 * run past the contig end into the scan domain, quirk Q16); out_r may be
 * NULL for directional units */
int up_unit_profile_range(up_ctx *ctx, uint32_t unit, uint64_t first, uint32_t count,
                          double *out_f, double *out_r);
/* -w as text: the lines FormatOutStream::write(PosScore) writes for positions
 * [first, first + count) of one unit -- "<pos> <score>\n" for every position
 * whose f + r is not 0, ascending, score as printf("%g") (negate != 0: "-"
 * before the score, the reverse buffer of a directional run) -- formatted on
 * the device (csrc/proftext.hip) from the same dense scores
 * up_unit_profile_range returns; f + r is one IEEE add.
 * cut_pos[n_cuts] (non-decreasing, each in [first, first + count]) asks for
 * cut_off[i] = the bytes of the lines at positions < cut_pos[i].
 * *text: host memory owned by the context (pinned), valid until the next
 * call that runs a pass, formats text, resets the units or closes it; NULL
 * when the range has no line (*n_bytes = 0, *exact = 1).
 * *exact = 0: the range holds a score outside up_format_g6's range (or NaN /
 * infinity; or |score| >= UNIPEAK_PROFILE_TEXT_LIMIT, a test-only variable
 * read at up_open); *text is NULL, *n_bytes and *n_lines 0, cut_off untouched,
 * and the caller formats this range from up_unit_profile_range.
 * Arguments, states and refusals as up_unit_profile_range's (both strands are
 * always summed, so there is no out_r rule). */
int up_unit_profile_text(up_ctx *ctx, uint32_t unit, uint64_t first, uint32_t count,
                         int32_t negate, uint32_t n_cuts, const uint64_t *cut_pos,
                         uint64_t *cut_off, const char **text, uint64_t *n_bytes,
                         uint64_t *n_lines, int32_t *exact);
/* -w as bigWig: what wigs2bigwigs (wigToBigWig -clip) makes of those lines,
 * without the text.  An item is (start = pos - 1, value) of every position in
 * [first, first + count) and <= clip_end (the contig's size) whose f + r is
 * not 0; value = (float)strtod("<%g of f + r>"), negated for negate != 0 --
 * up_g6_to_float's rule, not (float)(f + r).  Made on the device
 * (csrc/bigwig.hip) from the dense scores of up_unit_profile_range:
 *  items      ascending, the body of varStep sections of span 1;
 *  sections   one record per 1,024 consecutive items of the call (the last
 *             one shorter): extent [start, end), item count, min, max, and the
 *             sums of v and v * v in double (a fixed order);
 *  zoom[z]    the on-disk summary records (bbiSummaryOnDisk, 32 bytes) of
 *             level z = 0 .. n_levels - 1 for the bins [j * R, (j + 1) * R) of
 *             0-based starts that hold an item, R = reduction0 * 4^z, end
 *             clipped at clip_end, chromId = chrom_id; sums are added in double
 *             (level z + 1 from level z) and rounded to float once.
 * (first - 1) must be a multiple of reduction0 * 4^(n_levels - 1) -- every bin
 * of every level then lies inside the call -- else UP_E_ARG; n_levels <=
 * UP_BW_MAX_LEVELS (0: no zoom, zoom and n_zoom may be NULL).
 * The pointers are host memory owned by the context (pinned), valid until the
 * next call that runs a pass, formats a profile, resets the units or closes it;
 * NULL where the count is 0.
 * *exact = 0: the range holds a score up_g6_to_float refuses (or |score| >=
 * UNIPEAK_PROFILE_TEXT_LIMIT, the test-only variable of up_unit_profile_text);
 * no outputs, and the caller converts the range from up_unit_profile_range.
 * Arguments, states and refusals otherwise as up_unit_profile_range's.
 * up_timings [9] = these kernels ([5] the call's dense-profile kernel). */
#define UP_BW_MAX_LEVELS 10
typedef struct {
    uint32_t start; /* 0-based */
    float value;
} up_bw_item;
typedef struct {
    uint32_t start, end; /* first item's start, last item's start + 1 */
    uint32_t count, pad;
    float vmin, vmax;
    double sum, sumsq;
} up_bw_section;
typedef struct {
    uint32_t chrom, start, end, valid;
    float vmin, vmax, sum, sumsq;
} up_bw_zoom;
int up_unit_profile_bigwig(up_ctx *ctx, uint32_t unit, uint64_t first, uint32_t count,
                           int32_t negate, uint64_t clip_end, uint32_t reduction0,
                           uint32_t n_levels, uint32_t chrom_id, const up_bw_item **items,
                           uint64_t *n_items, const up_bw_section **sections,
                           uint64_t *n_sections, const up_bw_zoom **zoom, uint64_t *n_zoom,
                           int32_t *exact);
/* nondirectional units above UP_MAX_PARALLEL_BW (bw 512..32767, threshold > 0):
 * 0 (default): K1w only inside the blocking up_run with the -w capture off;
 *    up_run_async and up_unit_profile* refused, the capture keeps the replay.
 * 1: K1w also with the capture on, up_unit_profile* served by the profile
 *    kernel, up_run_async admitted (each pass slot in flight then holds its own
 *    64 MB of strand-correlation slabs when the correlation is evaluated).
 * UP_E_STATE while a pass is in flight. UNIPEAK_WIDE_ND=0 still forces the
 * replay whatever this says; a threshold <= 0 (up_set_wide_q11_nd below is
 * the switch of that case) and bw >= 32768 keep the replay
 * and the refusals as well.  The records and the -w profile do not depend on
 * it; bin/regions sets it.  Making 1 the default is a later change. */
int up_set_wide_nd_full(up_ctx *ctx, int on);
/* nondirectional units above UP_MAX_PARALLEL_BW at a threshold <= 0 (bw
 * 512..32767, the -w capture off, no coefficient below 0):
 * 0 (default): the exact replay of every unit, up_unit_profile* refused.
 * 1: wide K1q as on directional units, inside the blocking up_run only
 *    (up_run_async stays refused; up_last_scan_kind 2): peaks of forwardScore +
 *    reverseScore, the strand correlation (when it is evaluated) of regions
 *    of more than 65536 stored positions staged by many waves and chained by
 *    one through a staging area of at most 1 GiB; up_unit_profile* served by
 *    the profile kernel's two-strand form; up_shift_scan / up_shift_best form
 *    the regions' dense scores as behind K1w (2 * length doubles per region).
 * UP_E_STATE while a pass is in flight.  UNIPEAK_WIDE_Q11_ND=0 (read at
 * up_open, for A/B runs and tests) forces the replay whatever this says, as
 * do UNIPEAK_WIDE_Q11=0 and UNIPEAK_WIDE=0; the -w capture, a negative
 * coefficient and bw >= 32768 keep the replay and the refusals as well.
 * UNIPEAK_WIDE_CORR_LONG=<positions> and UNIPEAK_WIDE_CORR_TILE=<positions>
 * (read at up_open) override the long-region limit and the staging area's
 * size: test-only, to reach round boundaries with small inputs.  The records
 * do not depend on any of it; bin/regions -D and bin/strand_shift set the
 * switch.  Making 1 the default is a later change. */
int up_set_wide_q11_nd(up_ctx *ctx, int on);
/* Head units (quirk Q1) replayed and merged on the device, inside the pass.
 * 0 (default): after a pass with head units up_run / up_run_wait run K0 on
 *    the context stream, copy its records and the pass's K1-K3 records to the
 *    host and merge them there, in the caller's thread (with a device record
 *    target the merged list is copied up again): such passes do not overlap.
 * 1: the pass runs K0 on its own stream into areas of its slot, K3 writes to
 *    a device stage, and two kernels place both lists where the pass delivers
 *    (the pinned host records or the record target, its header included) --
 *    all stream-ordered before the pass's completion, no host round trip.
 *    Scope: a threshold > 0, K1 and K1w passes, any units and samples, the -w
 *    capture off.  With the capture on (its entries are gathered on the host),
 *    at a threshold <= 0 and in the whole-context replay nothing changes; a
 *    pass without head units launches nothing new.  When K0 runs out of an
 *    in-pass capacity (an open region longer than its area, its record area
 *    or its score slab) that pass is finished as with 0 -- which grows the
 *    capacities for the passes after it.
 * The initial value is 1 when UNIPEAK_HEAD_PLACE=1 is set at up_open.
 * UP_E_STATE while a pass is in flight.  The records, up_shift_scan /
 * up_shift_best and up_unit_replay_profile's resync do not depend on it;
 * bin/regions and bin/strand_shift set it. */
int up_set_head_place(up_ctx *ctx, int on);
/* what the pass completed last did with its head units: 0 merged on the host,
 * 1 replayed and placed inside the pass; -1 when no pass has completed, it
 * had no head unit, or it took a whole-context path (K1q at a threshold <= 0,
 * the replay of every unit).  For tests and A/B runs: the records do not
 * depend on it. */
int up_last_head_kind(up_ctx *ctx);

/* ---- tags_in_regions (src/tags_in_regions.cpp:131-199) on the GPU ---------
 * A stream is one sample's alignment records in the order the reference's
 * readAlign() returns them (ParseAlignStream / NondirParseAlignStream,
 * misc/format.cpp:503-565, 873-895): key[i] = contig << 32 | firstPos,
 * count[i] (> 0), forward[i].  The reference walks one cursor per stream
 * through the regions (skip to the region's strand at (contig, left), then
 * count every record on the contig at firstPos <= right, any strand: quirk
 * Q12).  up_tir_query answers every (region, stream) pair as if that
 * stream's cursor started at its first record: first = the record the skip
 * loop stops at, end = the record the count loop stops at (n: exhausted),
 * hits = sum of counts in [first, end) (uint32, wrapping like HitCount).
 * That is the reference's answer whenever the real cursor has not passed
 * `first` (nothing in between qualifies); the caller walks the other regions
 * itself (bin/tags_in_regions does).  UP_TIR_HOST in first/end:
 * the query crossed more unsorted runs of the stream than the device walks
 * (an unsorted stream); the caller walks that pair. */
#define UP_TIR_HOST 0xFFFFFFFFu
typedef struct up_tir up_tir;
int up_tir_open(int hip_device, up_tir **out);
void up_tir_close(up_tir *h);
/* upload stream `stream` (0..4095) and build its prefix sums and skip tables
 * on the device (blocking; the host arrays may be freed afterwards) */
int up_tir_set_stream(up_tir *h, uint32_t stream, uint64_t n, const uint64_t *key,
                      const uint32_t *count, const uint8_t *forward);
/* regions r = 0..n_regions-1 against streams 0..n_streams-1; outputs are
 * [n_regions][n_streams] */
int up_tir_query(up_tir *h, uint32_t n_streams, uint64_t n_regions, const uint32_t *contig,
                 const uint32_t *left, const uint32_t *right, const uint8_t *forward,
                 uint32_t *first, uint32_t *end, uint32_t *hits);
/* device time in ms: [0] the last up_tir_set_stream's table build (after the
 * upload), [1] the last up_tir_query's kernel */
int up_tir_timings(up_tir *h, double *ms, int n);

/* ---- convert_align's CountMap (misc/data.cpp:263-314, 321-596) on the GPU --
 * Per (strand, contig) position -> count, as dense uint32 tracks in HBM
 * (2 x the table's total length x 4 B).  up_cm_add = CountMap::add for n
 * alignments (contig < n_contigs, 1 <= pos <= its length, else UP_E_ARG;
 * count NULL = 1 each; per-position counts wrap at 2^32 like HitCount).
 * up_cm_collect = the nonzero entries in the order convert_align writes
 * them: nondir 0 -- CountMap::ConstIterator, forward strand then reverse,
 * contigs in table order, positions ascending; nondir 1 --
 * ConstNondirIterator, both strands merged by position with their counts
 * added (forward[] = 1).  With every output NULL only *n is set; cap is the
 * output arrays' length. */
typedef struct up_cm up_cm;
int up_cm_open(int hip_device, uint32_t n_contigs, const uint32_t *contig_len, up_cm **out);
void up_cm_close(up_cm *h);
int up_cm_add(up_cm *h, uint64_t n, const uint32_t *contig, const uint32_t *pos,
              const uint8_t *forward, const uint32_t *count);
int up_cm_collect(up_cm *h, int nondir, uint64_t *n, uint32_t *contig, uint32_t *pos,
                  uint32_t *count, uint8_t *forward, uint64_t cap);
/* device time in ms: [0] every up_cm_add kernel so far, [1] the last collect */
int up_cm_timings(up_cm *h, double *ms, int n);

/* ---- deflate: a DEFLATE (RFC 1951) encoder on the GPU ----------------------
 * One workgroup encodes one independent block of at most up_dfl_block() input
 * bytes: LZ77 inside the block (distance <= 32,768, length 3..258, every
 * candidate verified), one dynamic-Huffman block, or stored blocks where that
 * is not smaller.  A block's output is a function of its input bytes alone.
 *
 * up_dfl_stream: src is host memory; *out points at pinned host memory of the
 * handle, valid until its next call.  The output is raw DEFLATE, byte-aligned
 * at the end (every block closes with an empty stored block, like a sync
 * flush), no block marked final: put a gzip or zlib header in front,
 * concatenate the outputs of several calls, close with an empty final block
 * (03 00) and the trailer.  *crc32 = CRC-32 of src[0, n).  n = 0 gives zero
 * bytes.  *n_out <= up_dfl_bound(n).
 *
 * up_dfl_segments: segment i = src[seg_off[i], seg_off[i + 1]), at most
 * 65,536 bytes (UP_E_ARG otherwise), becomes one complete zlib stream
 * (RFC 1950: header, last block final, Adler-32) at
 * out[out_off[i], out_off[i + 1]).  Lengths 0 and 1 are valid.
 *
 * up_dfl_code_lengths: the length-limited Huffman code lengths the kernel
 * builds, on the host: len[s] = 0 for freq[s] = 0, else 1..max_len with a
 * Kraft sum of exactly 1 when two or more symbols are used (one used symbol
 * gets length 1).  n <= 288, max_len <= 15, sum of freq < 2^32, and at most
 * 2^max_len used symbols (UP_E_ARG otherwise: no such code exists). */
typedef struct up_dfl up_dfl;
int up_dfl_open(int device, up_dfl **h);
void up_dfl_close(up_dfl *h);
uint32_t up_dfl_block(void);       /* input bytes per independent block */
uint64_t up_dfl_bound(uint64_t n); /* upper bound of up_dfl_stream's output for n input bytes */
int up_dfl_stream(up_dfl *h, const void *src, uint64_t n, const void **out, uint64_t *n_out,
                  uint32_t *crc32);
int up_dfl_segments(up_dfl *h, const void *src, const uint64_t *seg_off /* n_seg + 1 */,
                    uint32_t n_seg, const void **out, uint64_t *out_off /* n_seg + 1 */);
/* totals since open: [0] device ms of the encode and compact kernels,
 * [1] input bytes, [2] output bytes, [3] calls */
int up_dfl_timings(up_dfl *h, double *v, int n);
int up_dfl_code_lengths(const uint32_t *freq, uint32_t n, uint32_t max_len, uint8_t *len);

/* ---- bunzip: a bzip2 decoder, parallel over blocks --------------------------
 * A .bz2 file is a chain of independent blocks.  The device path scans every
 * bit offset for the two 48-bit magics, decodes every candidate block's
 * entropy stage at once, links the candidates into the exact chain on the
 * host (a candidate that no block ends at is a false positive and is dropped;
 * a chain that breaks is a corrupt file), then runs the inverse BWT, the
 * run-length stage and the CRCs per block.  Concatenated streams decode to
 * the concatenation; anything else after a stream's end is an error.
 *
 * up_bz_decode: src is a whole file image in host memory; *out points at
 * pinned host memory of the handle, valid until its next call.  Corrupt data
 * is UP_E_ARG with info->reason (a UP_BZ_* code) and info->fail_bit set, and
 * *n_out = 0: never a partial result.
 *
 * up_bz_scan: stage 1 alone.  Every bit offset at which a block magic
 * (kind 0) or an end-of-stream magic (kind 1) stands, ascending; *n_cand is
 * the full count, also when cap is smaller.
 *
 * up_bz_decode_host: the same block decoder (csrc/bz_block.h) on the host,
 * serial along the chain; needs no device.  Writes at most cap bytes to dst;
 * *n_out is the full decoded size.  A cap that is too small is UP_E_ARG with
 * reason UP_BZ_NOSPACE and *n_out set, so a second call can succeed. */
#define UP_BZ_OK 0
#define UP_BZ_NOT_BZIP2 1   /* no "BZh" where a stream must start */
#define UP_BZ_BAD_LEVEL 2   /* level byte outside '1'..'9' */
#define UP_BZ_TRUNCATED 3   /* the data ends inside a stream */
#define UP_BZ_BAD_MAGIC 4   /* neither a block nor an end magic where one must stand */
#define UP_BZ_RANDOMISED 5  /* the pre-0.9.5 "randomised" bit is set */
#define UP_BZ_ORIGPTR 6     /* origPtr not below the block's length */
#define UP_BZ_SYMMAP 7      /* no symbol in use */
#define UP_BZ_NGROUPS 8     /* coding tables outside 2..6 */
#define UP_BZ_NSELECTORS 9  /* no selector */
#define UP_BZ_SELECTOR 10   /* selector index >= nGroups, or selectors used up */
#define UP_BZ_CODELEN 11    /* code length outside 1..20 */
#define UP_BZ_BAD_CODE 12   /* bit pattern that no symbol owns */
#define UP_BZ_OVERFLOW 13   /* more symbols than the block capacity */
#define UP_BZ_BLOCK_CRC 14
#define UP_BZ_STREAM_CRC 15
#define UP_BZ_TRAILING 16   /* bytes after the last stream */
#define UP_BZ_NOSPACE 17    /* up_bz_decode_host: dst too small (not a data error) */
typedef struct up_bz_info {
    uint32_t streams;  /* complete streams */
    uint32_t blocks;   /* blocks on the chain */
    uint32_t dropped;  /* scan candidates that were not on the chain */
    int32_t reason;    /* UP_BZ_* */
    uint64_t fail_bit; /* bit offset of the stream, block or field that failed */
} up_bz_info_t;
typedef struct up_bz up_bz;
int up_bz_open(int device, up_bz **h);
void up_bz_close(up_bz *h);
int up_bz_decode(up_bz *h, const void *src, uint64_t n, const void **out, uint64_t *n_out,
                 up_bz_info_t *info);
int up_bz_scan(up_bz *h, const void *src, uint64_t n, uint64_t *bit_off, uint8_t *kind, uint64_t cap,
               uint64_t *n_cand);
/* totals since open, device ms: [0] scan, [1] entropy stage, [2] rank (successor vector),
 * [3] inverse-BWT walks, [4] run-length stage and CRC; then [5] input bytes, [6] output
 * bytes, [7] calls */
int up_bz_timings(up_bz *h, double *v, int n);
int up_bz_decode_host(const void *src, uint64_t n, void *dst, uint64_t cap, uint64_t *n_out,
                      up_bz_info_t *info);
const char *up_bz_reason(int reason);

#ifdef __cplusplus
}
#endif
#endif
