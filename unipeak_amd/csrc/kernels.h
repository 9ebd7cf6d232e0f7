// unipeak_amd/csrc/kernels.h -- device data layout shared by the gfx950
// kernels (kernels.hip) and the C-ABI implementation (api.hip).
//
// HBM layout (DESIGN.md "Data layout"): every (unit, strand, sample) track is
// a dense array of kTB-bit tag counts ("fields"), kPerByte positions per
// byte: position p (1-based) is field n = kPadPos + p - 1, i.e. bits
// kTB * (n % kPerByte) .. + kTB - 1 of byte n / kPerByte.  kPadPos zero
// positions (kPadBytes bytes) sit in front and at least as many behind the
// unit's scan domain [1, len + bw], so every halo load is in bounds and reads
// zeros outside the contig.  A count >= kEsc (the all-ones field) is stored
// as kEsc and its value in the unit's overflow table (entries
// (pos << 32 | count), sorted by track then position).  Tracks of one unit
// are contiguous: track(s, k) = base + (s * S + k) * stride bytes.
//
// kTB = 2 (UPK_TRACK_BITS): counts 0, 1, 2 in place, 3 = escape.  The
// streaming scan (K1a) reads a quarter byte per position; ~99.6 % of
// positions hold 0 and counts >= 3 occur at peaks only (a few per peak,
// resolved through the per-block overflow index).  UPK_TRACK_BITS=4 builds
// the 4-bit layout of round 2 (escape 15) for A/B measurements.
#pragma once
#include <stdint.h>

namespace upk {

constexpr int kWave = 64;           // CDNA wavefront
constexpr int kStripWords = 256;    // one strip (wave task) = 256 words of 64 positions
constexpr int kStrip = kStripWords * kWave;  // 16384 positions per wave task
constexpr int kStepWords = 16;      // words per block (= one 1024-position dwordx4 wave load)
constexpr int kBlocks = kStripWords / kStepWords;  // 16 blocks per strip
constexpr int kChunk = 16;          // positions per screening chunk (one chunk sum each)
#ifndef UPK_TRACK_BITS
#define UPK_TRACK_BITS 2
#endif
constexpr int kTB = UPK_TRACK_BITS;               // bits per stored count
static_assert(kTB == 2 || kTB == 4, "2- or 4-bit tracks");
constexpr int kPerByte = 8 / kTB;                 // positions per byte
constexpr int kLogPerByte = kTB == 2 ? 2 : 1;
constexpr uint32_t kTMask = (1u << kTB) - 1u;     // one field
constexpr int kWordBytes = kWave / kPerByte;      // bytes of one 64-position word
constexpr int kChunkBytes = kChunk / kPerByte;    // bytes of one 16-position chunk
constexpr int kPadBytes = 256;      // zero bytes before position 1 and after the domain
constexpr int kPadPos = kPerByte * kPadBytes;  // the same padding in positions
constexpr int kStripBytes = kStrip / kPerByte;  // one strip of one track
constexpr int kMaxBw = 511;         // register-resident halo: NH <= 8 words (wider: K1w or the replay)
// K1w (wide.hip) and the segmented replay: windows of at most 65,535 cells,
// i.e. bw <= 32,767 (wider: the reference's UShort retirement count wraps,
// misc/peakcall.cpp:172-177, and only the whole-buffer replay models it)
constexpr int kMaxWideBw = 32767;
// samples per context: the reference's nExpt_ is a UShort (misc/peakcall.hpp:49);
// K3 keeps up to 256 exptSums in registers and up to kMaxSamples in an LDS
// row per wave, K0 one add's counts per sample in LDS
constexpr int kMaxSamples = 1024;
// K3L (one lane per region): a region with more hits than this sums its
// kurtosis terms with the whole wave instead of its lane (stats1.hip)
constexpr int kK3LHeavy = 512;
// Chunk-sum planes (2-bit tracks): after a unit's tracks, one byte per track
// per 16-position chunk -- byte j = the tag sum of fields 16j .. 16j+15 (the
// track's dword j), escaped fields at their overflow counts, saturated at 255
// (>= 255 tags: unbounded for the screen).  Plane of track t at base +
// ntracks * stride + t * (stride / 4), built by csum_kernel whenever a track
// changes; then the unit's pooled plane (base + ntracks * stride * 5 / 4):
// per chunk the screen's weighted sum over the non-control samples (weights
// ScanParams::wscreen) and both strands of a nondirectional unit, saturated
// at 255 (pool_kernel, rebuilt when a track or the pooling changes).  K1a
// streams the track's plane (one directional pooled track) or the pooled
// plane.
constexpr int kPlanePad = kPadPos / 16;      // chunks (bytes) before position 1
constexpr int kPlaneStrip = kStrip / 16;     // chunks (bytes) of one strip
// K1a screen: chunks of halo on each side -- kScrHalo places the halos in the
// LDS layout and bounds the fine-screen weights; a kernel of window width NH
// loads scr_halo(NH) of them (16 up to bw 255: the halo bytes a narrow
// kernel streams stay 3 % of a strip)
constexpr int kScrHalo = 32;        // kMaxBw / kChunk, rounded up
__host__ __device__ constexpr int scr_halo(int nh) { return nh <= 4 ? 16 : 32; }
constexpr int kCap = 32;            // inline run records per strip (starts, ends each)
constexpr int kOvfHalf = kStrip / 2 + 1;  // max starts (= max ends) of one strip
// record areas (uint32 words): starts [0,H), ends [H,2H), end-peak positions
// [2H,3H), end-peak scores as doubles at word 4H (8-byte aligned); H = kCap
// inline per strip, kOvfHalf per spilled strip's overflow slot
constexpr int kRecStride = 6 * kCap;
constexpr int kOvfStride = 6 * kOvfHalf;
constexpr uint32_t kEsc = kTMask;   // escape field: the count lives in the overflow table
constexpr int kXEntry = 2 + kWave / 2;  // strip, exact-block mask, 64 x 16-bit chunk masks
constexpr int kMaxK1aWaves = 16384;     // K1a grid cap (stash regions)
// K1 variants; kModeScreenF: K1a streaming the 2-bit fields where kModeScreen
// would stream the chunk-sum plane (a pass without the per-dataset index:
// DESIGN.md §3 "Index policy")
constexpr int kModeFused = 0, kModeScreen = 1, kModeExact = 2, kModeScreenF = 3;
constexpr uint32_t kBig = 1u << 22; // screen value of a chunk holding an escape (4-bit: a count >= 8)

// overflow entries are indexed per block of kOvfBlk positions, so a lookup
// searches one block's entries instead of the whole track's
constexpr uint32_t kOvfBlkShift = 10, kOvfBlk = 1u << kOvfBlkShift;
__host__ __device__ inline uint32_t ovf_nblk(uint32_t len) { return (len + kOvfBlk - 1) >> kOvfBlkShift; }
static_assert(kStepWords * kWave == (int)kOvfBlk, "an overflow block is one scan block (escape bitmap per strip)");

struct UnitDesc {
    uint64_t base;      // device address of track (0, 0)
    uint64_t stride;    // bytes per track (multiple of 256)
    uint32_t len;       // contig length
    uint32_t strip0;    // first global strip index
    uint32_t nstrips;   // strips covering [1, len + bw]
    int32_t nstrands;   // 1 or 2
    uint64_t ovf;       // overflow entries (uint64 pos << 32 | count) or 0
    uint64_t ovf_off;   // uint32[ntracks][nblk + 1], nblk = ceil(len / kOvfBlk): index of
                        // the track's first entry at or after block b's first position
                        // (b = nblk: the track's end), or 0
    uint64_t ovf_tidx;  // uint32[ntracks][nblk]: escape tile of block b (kNoTile: none)
    uint64_t ovf_tiles; // uint8[ntiles][kOvfBlk]: min(count, 255) of every escaped position
                        // of the tile's block (255: the entries hold it)
    uint64_t pct;       // pooled count track (several pooled samples, POOL 1) or 0:
                        // uint8[nstrands][kPerByte * stride], byte n = field n of the 2-bit
                        // tracks, min(sum of the pooled samples' counts, 255) -- 255: sum
                        // the samples (pct_kernel, rebuilt with the pooled plane)
};
constexpr uint32_t kNoTile = 0xFFFFFFFFu;

// packed per-strip summary written by the scan kernel (uint64):
//   bits  0-15 interior run starts, 16-31 interior run ends,
//   bit  32 flag(first position), 33 flag(last position),
//   bit  34 first strip of its unit, 35 last strip of its unit,
//   bit  36 records spilled to the overflow area
__host__ __device__ inline uint32_t si_starts(uint64_t v) { return (uint32_t)(v & 0xFFFFu); }
__host__ __device__ inline uint32_t si_ends(uint64_t v) { return (uint32_t)((v >> 16) & 0xFFFFu); }
__host__ __device__ inline uint32_t si_bit(uint64_t v, int b) { return (uint32_t)((v >> b) & 1u); }

struct ScanParams {
    const UnitDesc *units;
    uint32_t nunits;
    uint32_t nstrips;
    int32_t S;          // all samples
    int32_t nnc;        // non-control samples
    const int32_t *nc;  // indices of non-control samples, in sample order
    const double *coef; // per non-control sample (pool mode 2) or null
    const double *kern; // 2*bw+1 weights
    const uint32_t *wscreen;  // per non-control sample: integer weight >= |pooled share|
    uint32_t wskip;     // a window whose weighted tag sum is <= wskip cannot reach thr
    float fw[kScrHalo + 1];  // fine screen: weight bound per chunk distance 0..32 (K1 screen_bits)
    float fthr;         // a chunk whose weighted bound is <= fthr cannot reach thr
    int32_t bw;
    double thr;
    uint64_t *strip_info;
    uint32_t *rec;          // [nstrips][kRecStride]: starts, ends, end peaks (0: unknown)
    uint32_t *ovf_count;
    uint32_t *ovf_rec;      // [ovf_cap][kOvfStride]
    // K1a -> K1b work list.  Every K1a wave stashes the entries of its strips
    // that need exact blocks in its own xcap-entry region of xlist (multi-block
    // strips from the front, single-block ones from the back) and their counts
    // in xwcount -- no atomics on shared counters; xref_kernel then lists the
    // stash indices (front entries first) in xref and the totals in xcount.
    uint32_t *xlist;        // [K1a waves][xcap][kXEntry]
    uint32_t *xwcount;      // [K1a waves][2]: front / back entries stashed
    uint32_t *xref;         // [nstrips]: stash index of every listed entry
    uint32_t *xcount;       // [2] front / back entries in xref
    uint32_t xcap;          // stash entries per K1a wave
    uint64_t *spk;          // [nstrips][4]: peak (f+r bits, position) of the run open at
                            // the strip's first position ([0..1], written when it closes
                            // inside the strip) and of the run open at its last position
                            // ([2..3], from its start or the strip's first position)
    uint32_t ovf_cap;
    // Integer screen of K1b ("K1b keys"): with qmode set, a
    // live word's flags come from Q(x) = sum_h c_h (bw^2 - (x-h)^2), exact in
    // uint32 arithmetic, where Q <= qno proves score < thr and Q >= qyes
    // proves score >= thr; only words with a lane in between run the FP64 walk
    int32_t qmode;
    uint32_t qno, qyes;
    // escape bitmap: bit g of row (strand * S + sample) = global strip g or
    // its halo blocks hold an escaped field of that track (null: unknown, so
    // every strip counts as escaped).  K1a's one-track screen bounds a
    // strip's tags by 2 x popcount of its bytes, valid without escapes only
    const uint32_t *esc;
    uint32_t esc_nw;        // words per row
#if defined(UPK_DEBUG_COUNTS) || defined(UPK_DEBUG_TIMES)
    unsigned long long *dbg;  // counters: exact blocks, live words
#endif
    double *prof_f, *prof_r;  // optional dense profile of one unit's positions
    uint32_t prof_unit, prof_len;  // [prof_first, prof_first + prof_len)
    int64_t prof_first;
};

struct StatParams {
    const UnitDesc *units;
    int32_t S, nnc;
    const int32_t *nc;
    const uint8_t *is_control;
    const double *coef;
    const double *kern;
    int32_t bw;
    int32_t nondir;
    int32_t want_corr;
    double region_thr, kurt_thr, corr_thr, hit_thr;
    const uint32_t *starts, *ends, *reg_unit;
    const uint32_t *peak_pos;  // from K1 (0: the run crossed a strip edge -> spk)
    const uint64_t *spk;       // K1's per-strip partial peaks (ScanParams::spk)
    const double *peak_val;
    const uint64_t *nreg;
    uint64_t cap;         // records the output areas hold
    void *out;            // up_region records (mapped host memory in up_run)
    uint32_t *out_counts; // [n][S]
    double *corr_scratch; // -D -y: per K3 wave corr_cap (f, r) pairs, or null
    uint32_t corr_cap;
    int32_t qmode;        // K1 peaks are Q keys (ScanParams::qmode): K3 scores the peak
    int32_t q11;          // runs of K1q (threshold <= 0): the peak skips the run's first
                          // position (it joined by a leap, peakcall.cpp:76-78)
    int32_t planes;       // the chunk-sum planes are current (range sums may read them)
    int32_t cut;          // measurement aid (UNIPEAK_K3L_CUT): K3L stops after phase `cut` (wrong records)
    int32_t heavy;        // K3L: regions with more hits take the wave's kurtosis path (UNIPEAK_K3L_HEAVY)
    int32_t w2hits;       // K3L second walk: 1 = four hits per step, 0 = 16 fields per dword (UNIPEAK_K3L_W2)
    const double *corr_in; // -D -y behind K1w: strandCorr(0) per region (wide_corr_kernel), or null --
                           // set: K3 keeps K1w's peaks, runs no KDE of its own and takes corr from it
};

// The templated K1 / K3 / K4 kernels of one window width NH: selectors that
// return the address of the instantiation to launch (host side; nh_tu.hip
// defines one set per width, api.hip indexes them by the bandwidth)
struct WidthKernels {
    const void *(*scan)(int pool, bool nd, bool prof, int mode);  // K1a / K1b / the profile kernel
    const void *(*exact1)();                                      // K1b for one directional sample
    const void *(*stats)(int pool, bool nd, int one);             // K3
    const void *(*shift)(int pool);                               // K4
};

}  // namespace upk
