"""ctypes binding of include/unipeak_hip.h (libunipeak_hip.so).

Mirrors the C-ABI one-to-one; every failing call raises UpError carrying
the library's error text (up_strerror), the analogue of the reference's
`error: ...` exits.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# UNIPEAK_LIB overrides the in-tree build (A/B experiments with variant builds)
LIB_PATH = os.environ.get("UNIPEAK_LIB") or os.path.join(_HERE, "lib", "libunipeak_hip.so")

UP_OK = 0
UP_E_ARG, UP_E_NOMEM, UP_E_STATE = -1, -3, -4  # (include/unipeak_hip.h)
MAX_IN_FLIGHT = 5  # UP_MAX_IN_FLIGHT (include/unipeak_hip.h)


class UpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{msg} (code {code})")
        self.code = code


class Params(ctypes.Structure):
    _fields_ = [
        ("bw", ctypes.c_uint16),
        ("n_samples", ctypes.c_uint16),
        ("nondir", ctypes.c_int32),
        ("background", ctypes.c_double),
        ("region_thr", ctypes.c_double),
        ("kurt_thr", ctypes.c_double),
        ("corr_thr", ctypes.c_double),
        ("hit_thr", ctypes.c_double),
        ("is_control", ctypes.POINTER(ctypes.c_uint8)),
        ("coeffs", ctypes.POINTER(ctypes.c_double)),
        ("n_coeffs", ctypes.c_uint32),
        ("want_corr", ctypes.c_int32),
    ]


class Region(ctypes.Structure):
    _fields_ = [
        ("unit", ctypes.c_uint32),
        ("left", ctypes.c_uint32),
        ("right", ctypes.c_uint32),
        ("peak", ctypes.c_uint32),
        ("sum", ctypes.c_uint32),
        ("nonctl_sum", ctypes.c_uint32),
        ("accepted", ctypes.c_int32),
        ("close_pos", ctypes.c_uint32),
        ("peak_score", ctypes.c_double),
        ("kurtosis", ctypes.c_double),
        ("corr", ctypes.c_double),
    ]


REGION_DTYPE = np.dtype([
    ("unit", "<u4"), ("left", "<u4"), ("right", "<u4"), ("peak", "<u4"),
    ("sum", "<u4"), ("nonctl_sum", "<u4"), ("accepted", "<i4"), ("close_pos", "<u4"),
    ("peak_score", "<f8"), ("kurtosis", "<f8"), ("corr", "<f8")])
assert REGION_DTYPE.itemsize == ctypes.sizeof(Region)

_lib = None

EXPORTS = [
    "up_version", "up_track_bits", "up_strerror", "up_device_count", "up_kernel_weights", "up_open",
    "up_close", "up_set_params", "up_add_unit", "up_unit_count", "up_unit_pack",
    "up_unit_scatter", "up_unit_synth", "up_unit_synth_offset", "up_unit_synth_ex", "up_unit_tag_total", "up_unit_set_last_add", "up_unit_last_add",
    "up_reset_units", "up_run", "up_get_regions", "up_regions_view", "up_shift_scan", "up_shift_best",
    "up_timings", "up_scan_density", "up_unit_profile", "up_hbm_copy_gbps", "up_set_record_target",
    "up_host_register", "up_unit_profile_range", "up_unit_profile_text", "up_unit_profile_bigwig", "up_run_async", "up_run_wait", "up_set_timing",
    "up_set_profile_capture", "up_unit_replay_profile", "up_set_wide_nd_full",
    "up_set_index_policy", "up_invalidate_index", "up_index_state", "up_unit_layout", "up_unit_index_read",
    "up_last_stats_kind", "up_last_exact_kind",
    "up_last_scan_kind", "up_set_head_place", "up_last_head_kind",
    "up_tir_open", "up_tir_close", "up_tir_set_stream", "up_tir_query", "up_tir_timings",
    "up_cm_open", "up_cm_close", "up_cm_add", "up_cm_collect", "up_cm_timings",
    "up_dfl_open", "up_dfl_close", "up_dfl_block", "up_dfl_bound", "up_dfl_stream", "up_dfl_segments",
    "up_dfl_timings", "up_dfl_code_lengths",
    "up_bz_open", "up_bz_close", "up_bz_decode", "up_bz_scan", "up_bz_timings", "up_bz_decode_host",
    "up_bz_reason",
]
# (up_set_wide_q11_nd, up_format_g6 and up_g6_to_float are bound in load_library like the rest; they are not listed here because
# tests/test_capi.py compares this list with the header's names as its pattern reads them,
# letters and underscores only)
TIR_HOST = 0xFFFFFFFF  # UP_TIR_HOST
INDEX_AUTO, INDEX_NEVER, INDEX_ALWAYS = 0, 1, 2  # UP_INDEX_*
IDX_TRACKS, IDX_CSUM, IDX_POOLED, IDX_PCT = 0, 1, 2, 3  # UP_IDX_*


class UnitLayout(ctypes.Structure):  # up_unit_layout_t
    _fields_ = [
        ("stride", ctypes.c_uint64),
        ("len", ctypes.c_uint32),
        ("nstrands", ctypes.c_int32),
        ("n_samples", ctypes.c_int32),
        ("pad_pos", ctypes.c_int32),
        ("track_bits", ctypes.c_int32),
        ("index_on", ctypes.c_int32),
        ("has_pooled", ctypes.c_int32),
        ("has_pct", ctypes.c_int32),
    ]


def load_library(path=LIB_PATH):
    """Load libunipeak_hip.so (raises OSError when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise OSError(f"{path} not built: run `python __graft_entry__.py` / tools/build.py")
    L = ctypes.CDLL(path)
    c = ctypes
    vp, u32p = c.c_void_p, c.POINTER(c.c_uint32)
    sig = {
        "up_version": (c.c_int, []),
        "up_track_bits": (c.c_int, []),
        "up_strerror": (c.c_char_p, [c.c_int]),
        "up_device_count": (c.c_int, [c.POINTER(c.c_int)]),
        "up_kernel_weights": (c.c_int, [c.c_uint16, c.c_double, vp]),
        "up_format_g6": (c.c_int, [c.c_double, vp, c.POINTER(c.c_int)]),
        "up_g6_to_float": (c.c_int, [c.c_double, c.POINTER(c.c_float), c.POINTER(c.c_int)]),
        "up_open": (c.c_int, [c.c_int, c.POINTER(vp)]),
        "up_close": (None, [vp]),
        "up_set_params": (c.c_int, [vp, c.POINTER(Params)]),
        "up_add_unit": (c.c_int, [vp, c.c_uint32, c.c_int32, c.c_int32, u32p]),
        "up_unit_count": (c.c_int, [vp, u32p]),
        "up_unit_pack": (c.c_int, [vp, c.c_uint32, c.c_int32, c.c_uint16, vp]),
        "up_unit_scatter": (c.c_int, [vp, c.c_uint32, c.c_int32, c.c_uint16, c.c_size_t, vp, vp]),
        "up_unit_synth": (c.c_int, [vp, c.c_uint32, c.c_int32, c.c_uint16, c.c_uint64,
                                    c.c_uint32, c.c_int32, c.c_int32, c.c_int32]),
        "up_unit_synth_offset": (c.c_int, [vp, c.c_uint32, c.c_int32, c.c_uint16, c.c_uint64,
                                           c.c_uint32, c.c_int32, c.c_int32, c.c_int32, c.c_int32]),
        "up_unit_synth_ex": (c.c_int, [vp, c.c_uint32, c.c_int32, c.c_uint16, c.c_uint64,
                                       c.c_uint32, c.c_int32, c.c_int32, c.c_int32, c.c_int32,
                                       c.c_uint64]),
        "up_unit_tag_total": (c.c_int, [vp, c.c_uint32, c.c_int32, c.c_uint16,
                                        c.POINTER(c.c_uint64)]),
        "up_unit_set_last_add": (c.c_int, [vp, c.c_uint32, c.c_uint32]),
        "up_unit_last_add": (c.c_int, [vp, c.c_uint32, u32p]),
        "up_reset_units": (c.c_int, [vp]),
        "up_run": (c.c_int, [vp, c.POINTER(c.c_uint64)]),
        "up_run_async": (c.c_int, [vp]),
        "up_run_wait": (c.c_int, [vp, c.POINTER(c.c_uint64)]),
        "up_set_timing": (c.c_int, [vp, c.c_int]),
        "up_get_regions": (c.c_int, [vp, vp, vp, c.c_size_t]),
        "up_regions_view": (c.c_int, [vp, c.POINTER(vp), c.POINTER(vp), c.POINTER(c.c_uint64)]),
        "up_shift_scan": (c.c_int, [vp, vp, c.c_size_t, c.c_uint16, vp]),
        "up_shift_best": (c.c_int, [vp, vp, c.c_size_t, c.c_uint16, vp, vp]),
        "up_timings": (c.c_int, [vp, vp, c.c_int]),
        "up_scan_density": (c.c_int, [vp, u32p]),
        "up_set_index_policy": (c.c_int, [vp, c.c_int]),
        "up_invalidate_index": (c.c_int, [vp]),
        "up_index_state": (c.c_int, [vp, c.POINTER(c.c_int), c.POINTER(c.c_uint64)]),
        "up_unit_layout": (c.c_int, [vp, c.c_uint32, c.POINTER(UnitLayout)]),
        "up_unit_index_read": (c.c_int, [vp, c.c_uint32, c.c_int, vp, c.c_uint64, c.POINTER(c.c_uint64)]),
        "up_last_stats_kind": (c.c_int, [vp]),
        "up_last_exact_kind": (c.c_int, [vp]),
        "up_last_scan_kind": (c.c_int, [vp]),
        "up_unit_profile": (c.c_int, [vp, c.c_uint32, vp, vp, c.c_uint32]),
        "up_hbm_copy_gbps": (c.c_int, [vp, c.c_uint64, c.c_int, c.POINTER(c.c_double)]),
        "up_set_record_target": (c.c_int, [vp, vp, c.c_uint64]),
        "up_host_register": (c.c_int, [vp, vp, c.c_uint64]),
        "up_unit_profile_range": (c.c_int, [vp, c.c_uint32, c.c_uint64, c.c_uint32, vp, vp]),
        "up_unit_profile_text": (c.c_int, [vp, c.c_uint32, c.c_uint64, c.c_uint32, c.c_int32, c.c_uint32, vp, vp,
                                           c.POINTER(vp), c.POINTER(c.c_uint64), c.POINTER(c.c_uint64),
                                           c.POINTER(c.c_int32)]),
        "up_unit_profile_bigwig": (c.c_int, [vp, c.c_uint32, c.c_uint64, c.c_uint32, c.c_int32, c.c_uint64,
                                             c.c_uint32, c.c_uint32, c.c_uint32, c.POINTER(vp),
                                             c.POINTER(c.c_uint64), c.POINTER(vp), c.POINTER(c.c_uint64), vp, vp,
                                             c.POINTER(c.c_int32)]),
        "up_set_profile_capture": (c.c_int, [vp, c.c_int]),
        "up_set_wide_nd_full": (c.c_int, [vp, c.c_int]),
        "up_set_wide_q11_nd": (c.c_int, [vp, c.c_int]),
        "up_set_head_place": (c.c_int, [vp, c.c_int]),
        "up_last_head_kind": (c.c_int, [vp]),
        "up_unit_replay_profile": (c.c_int, [vp, c.c_uint32, u32p, c.POINTER(c.c_uint64), vp, vp, vp,
                                             c.c_uint64]),
        "up_tir_open": (c.c_int, [c.c_int, c.POINTER(vp)]),
        "up_tir_close": (None, [vp]),
        "up_tir_set_stream": (c.c_int, [vp, c.c_uint32, c.c_uint64, vp, vp, vp]),
        "up_tir_query": (c.c_int, [vp, c.c_uint32, c.c_uint64, vp, vp, vp, vp, vp, vp, vp]),
        "up_tir_timings": (c.c_int, [vp, vp, c.c_int]),
        "up_cm_open": (c.c_int, [c.c_int, c.c_uint32, vp, c.POINTER(vp)]),
        "up_cm_close": (None, [vp]),
        "up_cm_add": (c.c_int, [vp, c.c_uint64, vp, vp, vp, vp]),
        "up_cm_collect": (c.c_int, [vp, c.c_int, c.POINTER(c.c_uint64), vp, vp, vp, vp, c.c_uint64]),
        "up_cm_timings": (c.c_int, [vp, vp, c.c_int]),
        "up_dfl_open": (c.c_int, [c.c_int, c.POINTER(vp)]),
        "up_dfl_close": (None, [vp]),
        "up_dfl_block": (c.c_uint32, []),
        "up_dfl_bound": (c.c_uint64, [c.c_uint64]),
        "up_dfl_stream": (c.c_int, [vp, vp, c.c_uint64, c.POINTER(vp), c.POINTER(c.c_uint64), u32p]),
        "up_dfl_segments": (c.c_int, [vp, vp, vp, c.c_uint32, c.POINTER(vp), vp]),
        "up_dfl_timings": (c.c_int, [vp, vp, c.c_int]),
        "up_dfl_code_lengths": (c.c_int, [vp, c.c_uint32, c.c_uint32, vp]),
        "up_bz_open": (c.c_int, [c.c_int, c.POINTER(vp)]),
        "up_bz_close": (None, [vp]),
        "up_bz_decode": (c.c_int, [vp, vp, c.c_uint64, c.POINTER(vp), c.POINTER(c.c_uint64), vp]),
        "up_bz_scan": (c.c_int, [vp, vp, c.c_uint64, vp, vp, c.c_uint64, c.POINTER(c.c_uint64)]),
        "up_bz_timings": (c.c_int, [vp, vp, c.c_int]),
        "up_bz_decode_host": (c.c_int, [vp, c.c_uint64, vp, c.c_uint64, c.POINTER(c.c_uint64), vp]),
        "up_bz_reason": (c.c_char_p, [c.c_int]),
    }
    for name, (res, args) in sig.items():
        if os.environ.get("UNIPEAK_LIB") and not hasattr(L, name):
            continue  # an A/B library of an older commit: calling what it lacks still raises
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def _ck(code):
    if code != UP_OK:
        raise UpError(code, _lib.up_strerror(code).decode())


def kernel_weights(bw, total=1.0):
    L = load_library()
    w = np.zeros(2 * bw + 1, np.float64)
    _ck(L.up_kernel_weights(bw, total, w.ctypes.data))
    return w


def format_g6(v):
    """printf("%g", v) as bytes by the routine the device formatter runs, or None when
    v is outside the range it formats itself (up_format_g6)"""
    L = load_library()
    buf = ctypes.create_string_buffer(16)  # UP_G6_MAX
    n = ctypes.c_int(0)
    _ck(L.up_format_g6(float(v), buf, ctypes.byref(n)))
    return buf.raw[:n.value] if n.value else None


def g6_to_float(v):
    """(float)strtod(printf("%g", v)) as a numpy.float32 by the routine the device's bigWig
    kernels run, or None when it refuses v: outside format_g6's range, or a text below
    1e-17 (up_g6_to_float)"""
    L = load_library()
    out, ok = ctypes.c_float(0), ctypes.c_int(0)
    _ck(L.up_g6_to_float(float(v), ctypes.byref(out), ctypes.byref(ok)))
    return np.float32(out.value) if ok.value else None


def g6_to_float_bits(values):
    """up_g6_to_float over an array of doubles: (float32 bits as uint32[], ok as bool[])"""
    L = load_library()
    v = np.ascontiguousarray(values, np.float64)
    bits, oks = np.zeros(v.size, np.uint32), np.zeros(v.size, bool)
    out, ok = ctypes.c_float(0), ctypes.c_int(0)
    po, pk, fn = ctypes.byref(out), ctypes.byref(ok), L.up_g6_to_float
    view = ctypes.cast(ctypes.pointer(out), ctypes.POINTER(ctypes.c_uint32))
    for i, x in enumerate(v.tolist()):
        fn(x, po, pk)
        bits[i] = view[0]
        oks[i] = ok.value != 0
    return bits, oks


BW_ITEM_DTYPE = np.dtype([("start", "<u4"), ("value", "<f4")])  # up_bw_item
BW_SECTION_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("count", "<u4"), ("pad", "<u4"),
                             ("vmin", "<f4"), ("vmax", "<f4"), ("sum", "<f8"), ("sumsq", "<f8")])  # up_bw_section
BW_ZOOM_DTYPE = np.dtype([("chrom", "<u4"), ("start", "<u4"), ("end", "<u4"), ("valid", "<u4"),
                          ("vmin", "<f4"), ("vmax", "<f4"), ("sum", "<f4"), ("sumsq", "<f4")])  # up_bw_zoom
BW_MAX_LEVELS = 10  # UP_BW_MAX_LEVELS


def track_bits():
    """bits per stored count in a device track (up_track_bits)"""
    return load_library().up_track_bits()


def device_count():
    L = load_library()
    n = ctypes.c_int(0)
    _ck(L.up_device_count(ctypes.byref(n)))
    return n.value


# Mixing with torch: torch's bundled HIP runtime must initialise the GPU
# before this library's (system ROCm) runtime does, or torch then reports no
# GPU -- touch torch.cuda first (tools/mix_probe.py shows both orders).
class Lib:
    """One up_ctx (one GPU)."""

    def __init__(self, device=0):
        self.L = load_library()
        self.ctx = ctypes.c_void_p()
        _ck(self.L.up_open(device, ctypes.byref(self.ctx)))
        self.S = None

    def close(self):
        if self.ctx:
            self.L.up_close(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_params(self, bw, n_samples, background, region_thr=25.0, kurt_thr=50.0,
                   corr_thr=-1.0, hit_thr=10.0, nondir=False, control=None, coeffs=None,
                   want_corr=False):
        p = Params()
        p.bw, p.n_samples, p.nondir = bw, n_samples, int(bool(nondir))
        p.background, p.region_thr, p.kurt_thr = background, region_thr, kurt_thr
        p.corr_thr, p.hit_thr, p.want_corr = corr_thr, hit_thr, int(bool(want_corr))
        self._ctl = None
        if control is not None:
            self._ctl = (ctypes.c_uint8 * n_samples)(*[1 if x else 0 for x in control])
            p.is_control = self._ctl
        self._coef = None
        if coeffs is not None and len(coeffs):
            self._coef = (ctypes.c_double * len(coeffs))(*coeffs)
            p.coeffs = self._coef
            p.n_coeffs = len(coeffs)
        _ck(self.L.up_set_params(self.ctx, ctypes.byref(p)))
        self.S = n_samples
        self.nondir = bool(nondir)

    def add_unit(self, length, buffer_id=0):
        u = ctypes.c_uint32()
        _ck(self.L.up_add_unit(self.ctx, length, 2 if self.nondir else 1, buffer_id,
                               ctypes.byref(u)))
        return u.value

    def scatter(self, unit, strand, sample, pos, counts):
        pos = np.ascontiguousarray(pos, np.uint32)
        counts = np.ascontiguousarray(counts, np.uint32)
        assert pos.shape == counts.shape
        _ck(self.L.up_unit_scatter(self.ctx, unit, strand, sample, pos.size,
                                   pos.ctypes.data, counts.ctypes.data))

    def synth(self, unit, strand, sample, seed, contig_index, synth_strand, nondir=False,
              peaks=True, offset=0, peak_seed=0):
        """peak_seed != 0: replicate mode (shared peak centres)"""
        if peak_seed:
            _ck(self.L.up_unit_synth_ex(self.ctx, unit, strand, sample, seed, contig_index,
                                        synth_strand, int(nondir), int(peaks), int(offset),
                                        int(peak_seed)))
        elif offset:
            _ck(self.L.up_unit_synth_offset(self.ctx, unit, strand, sample, seed, contig_index,
                                            synth_strand, int(nondir), int(peaks), int(offset)))
        else:
            _ck(self.L.up_unit_synth(self.ctx, unit, strand, sample, seed, contig_index,
                                     synth_strand, int(nondir), int(peaks)))

    def tag_total(self, unit, strand, sample):
        v = ctypes.c_uint64()
        _ck(self.L.up_unit_tag_total(self.ctx, unit, strand, sample, ctypes.byref(v)))
        return v.value

    def pack(self, unit, strand, sample, dev_ptr):
        """replace a track from a device uint32 array (e.g. a torch tensor's
        data_ptr()) of contig_len counts"""
        _ck(self.L.up_unit_pack(self.ctx, unit, strand, sample, ctypes.c_void_p(dev_ptr)))

    def set_last_add(self, unit, pos):
        _ck(self.L.up_unit_set_last_add(self.ctx, unit, pos))

    def last_add(self, unit):
        v = ctypes.c_uint32()
        _ck(self.L.up_unit_last_add(self.ctx, unit, ctypes.byref(v)))
        return v.value

    def reset_units(self):
        _ck(self.L.up_reset_units(self.ctx))

    def run(self):
        n = ctypes.c_uint64()
        _ck(self.L.up_run(self.ctx, ctypes.byref(n)))
        return n.value

    def run_async(self):
        """enqueue one pass (at most MAX_IN_FLIGHT in flight); see up_run_async"""
        _ck(self.L.up_run_async(self.ctx))

    def run_wait(self):
        """complete the oldest pass in flight -> its region count"""
        n = ctypes.c_uint64()
        _ck(self.L.up_run_wait(self.ctx, ctypes.byref(n)))
        return n.value

    def set_timing(self, level):
        """0: wall only, 1: + K1a events, 2: every phase (default)"""
        _ck(self.L.up_set_timing(self.ctx, int(level)))

    def regions(self, n, with_counts=True):
        out = np.zeros(n, REGION_DTYPE)
        cnt = np.zeros((n, self.S), np.uint32) if with_counts else None
        _ck(self.L.up_get_regions(self.ctx, out.ctypes.data,
                                  cnt.ctypes.data if cnt is not None else None, n))
        return out, cnt

    def regions_view(self):
        """(records, counts) as numpy views of the context's pinned host copy;
        valid until the next run()."""
        r, k, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint64()
        _ck(self.L.up_regions_view(self.ctx, ctypes.byref(r), ctypes.byref(k), ctypes.byref(n)))
        n = n.value
        if n == 0:
            return np.zeros(0, REGION_DTYPE), np.zeros((0, self.S), np.uint32)
        regs = np.frombuffer((ctypes.c_char * (n * REGION_DTYPE.itemsize)).from_address(r.value),
                             REGION_DTYPE)
        cnt = np.frombuffer((ctypes.c_char * (n * self.S * 4)).from_address(k.value),
                            np.uint32).reshape(n, self.S)
        return regs, cnt

    def shift_scan(self, idx, max_shift):
        idx = np.ascontiguousarray(idx, np.uint64)
        out = np.zeros((idx.size, max_shift + 1), np.float64)
        _ck(self.L.up_shift_scan(self.ctx, idx.ctypes.data, idx.size, max_shift,
                                 out.ctypes.data))
        return out

    def shift_best(self, idx, max_shift):
        """-> (best shift uint16[n], best corr f8[n]) per region (up_shift_best)"""
        idx = np.ascontiguousarray(idx, np.uint64)
        best = np.zeros(idx.size, np.uint16)
        corr = np.zeros(idx.size, np.float64)
        _ck(self.L.up_shift_best(self.ctx, idx.ctypes.data, idx.size, max_shift, best.ctypes.data,
                                 corr.ctypes.data))
        return best, corr

    def set_record_target(self, dev_ptr, cap):
        """records of the next runs go to a device buffer (see the header);
        dev_ptr = 0 restores host delivery"""
        _ck(self.L.up_set_record_target(self.ctx, ctypes.c_void_p(dev_ptr or None), cap))

    def host_register(self, ptr, nbytes):
        _ck(self.L.up_host_register(self.ctx, ctypes.c_void_p(ptr), nbytes))

    def hbm_copy_gbps(self, nbytes=1 << 30, reps=5):
        v = ctypes.c_double()
        _ck(self.L.up_hbm_copy_gbps(self.ctx, nbytes, reps, ctypes.byref(v)))
        return v.value

    def set_index_policy(self, policy):
        """INDEX_AUTO / INDEX_NEVER / INDEX_ALWAYS (up_set_index_policy)"""
        _ck(self.L.up_set_index_policy(self.ctx, int(policy)))

    def invalidate_index(self):
        _ck(self.L.up_invalidate_index(self.ctx))

    def index_state(self):
        """(the next pass uses the index, index builds so far)"""
        on, b = ctypes.c_int(0), ctypes.c_uint64(0)
        _ck(self.L.up_index_state(self.ctx, ctypes.byref(on), ctypes.byref(b)))
        return bool(on.value), int(b.value)

    def unit_layout(self, unit):
        """the geometry of a unit's tracks and index arrays as a UnitLayout, after the
        sync a pass would run (up_unit_layout)"""
        lay = UnitLayout()
        _ck(self.L.up_unit_layout(self.ctx, unit, ctypes.byref(lay)))
        return lay

    def index_read(self, unit, what):
        """one of a unit's arrays as it lies on the device, a numpy.uint8 array: IDX_TRACKS,
        IDX_CSUM, IDX_POOLED or IDX_PCT; builds a stale index first, as the next pass would
        (up_unit_index_read)"""
        lay = self.unit_layout(unit)
        ntracks = lay.nstrands * lay.n_samples
        size = {IDX_TRACKS: ntracks * lay.stride, IDX_CSUM: ntracks * (lay.stride // 4),
                IDX_POOLED: lay.stride // 4, IDX_PCT: lay.nstrands * 4 * lay.stride}.get(what, 1)
        out = np.zeros(size, np.uint8)
        n = ctypes.c_uint64(0)
        _ck(self.L.up_unit_index_read(self.ctx, unit, int(what), out.ctypes.data, out.size, ctypes.byref(n)))
        assert n.value == out.size, (n.value, out.size)
        return out

    def last_k3_kind(self):
        """K3 of the pass completed last: 0 general, 1 a wave per region, 2 a lane
        per region, -1 none launched (up_last_stats_kind)"""
        return int(self.L.up_last_stats_kind(self.ctx))

    def last_exact_kind(self):
        """K1b of the pass completed last: 0 the generic scan kernel, 1 the
        pipelined kernel for one directional sample, -1 none launched
        (up_last_exact_kind)"""
        return int(self.L.up_last_exact_kind(self.ctx))

    def last_scan_kind(self):
        """how the pass completed last found its regions: 0 K1, 1 K1w, 2 K1q (above bw
        511 its wide form), 3 the exact replay of every unit, -1 no pass or no units
        (up_last_scan_kind)"""
        return int(self.L.up_last_scan_kind(self.ctx))

    def scan_density(self):
        """bytes K1a streams per 1,024 positions of a unit (up_scan_density)"""
        v = ctypes.c_uint32()
        _ck(self.L.up_scan_density(self.ctx, ctypes.byref(v)))
        return v.value

    def timings(self):
        t = np.zeros(5, np.float64)
        _ck(self.L.up_timings(self.ctx, t.ctypes.data, 5))
        return t

    def profile(self, unit, length):
        f = np.zeros(length, np.float64)
        r = np.zeros(length, np.float64)
        _ck(self.L.up_unit_profile(self.ctx, unit, f.ctypes.data, r.ctypes.data, length))
        return f, r

    def profile_range(self, unit, first, count):
        """(f, r) of positions [first, first + count), first >= 1; the range may run
        past the contig end into the scan domain (up_unit_profile_range)"""
        f = np.zeros(count, np.float64)
        r = np.zeros(count, np.float64)
        _ck(self.L.up_unit_profile_range(self.ctx, unit, first, count, f.ctypes.data, r.ctypes.data))
        return f, r

    def profile_kernel_ms(self):
        """device time of the last profile()/profile_range() kernel (up_timings [5])"""
        t = np.zeros(6, np.float64)
        _ck(self.L.up_timings(self.ctx, t.ctypes.data, 6))
        return float(t[5])

    def profile_text(self, unit, first, count, negate=False, cuts=None):
        """the -w lines of positions [first, first + count) formatted on the device:
        (text bytes or None, cut_off uint64[], n_lines, exact); cuts: non-decreasing
        positions in [first, first + count] whose byte offsets are wanted; exact False:
        the range holds a score the device does not format, text None
        (up_unit_profile_text)"""
        cp = np.ascontiguousarray(cuts if cuts is not None else [], np.uint64)
        co = np.zeros(len(cp), np.uint64)
        text, nb, nl, ex = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int32()
        _ck(self.L.up_unit_profile_text(self.ctx, unit, first, count, int(bool(negate)), len(cp),
                                        cp.ctypes.data if len(cp) else None,
                                        co.ctypes.data if len(cp) else None, ctypes.byref(text),
                                        ctypes.byref(nb), ctypes.byref(nl), ctypes.byref(ex)))
        if not ex.value:
            return None, co, 0, False
        data = ctypes.string_at(text.value, nb.value) if nb.value else b""
        return data, co, nl.value, True

    def profile_text_ms(self):
        """device time of the text kernels of the last profile_text() (up_timings [8])"""
        t = np.zeros(9, np.float64)
        _ck(self.L.up_timings(self.ctx, t.ctypes.data, 9))
        return float(t[8])

    def profile_bigwig(self, unit, first, count, negate=False, clip_end=None, reduction0=10, n_levels=0,
                       chrom_id=0):
        """the -w profile of positions [first, first + count) as bigWig pieces made on the
        device: (items BW_ITEM_DTYPE[], sections BW_SECTION_DTYPE[], [zoom records
        BW_ZOOM_DTYPE[] per level], exact); copies.  clip_end: the contig's size (default:
        no clipping inside the range); exact False: the range holds a score the device does
        not convert, the arrays are None (up_unit_profile_bigwig)"""
        if clip_end is None:
            clip_end = first + count
        it, sec = ctypes.c_void_p(), ctypes.c_void_p()
        ni, ns, ex = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int32()
        nl = max(int(n_levels), 0)
        zp = (ctypes.c_void_p * max(nl, 1))()
        zn = (ctypes.c_uint64 * max(nl, 1))()
        _ck(self.L.up_unit_profile_bigwig(self.ctx, unit, first, count, int(bool(negate)), clip_end, reduction0,
                                          n_levels, chrom_id, ctypes.byref(it), ctypes.byref(ni), ctypes.byref(sec),
                                          ctypes.byref(ns), ctypes.cast(zp, ctypes.c_void_p),
                                          ctypes.cast(zn, ctypes.c_void_p), ctypes.byref(ex)))
        if not ex.value:
            return None, None, None, False

        def arr(ptr, n, dt):
            if not n:
                return np.zeros(0, dt)
            return np.frombuffer(ctypes.string_at(ptr, n * dt.itemsize), dt).copy()
        return (arr(it.value, ni.value, BW_ITEM_DTYPE), arr(sec.value, ns.value, BW_SECTION_DTYPE),
                [arr(zp[z], zn[z], BW_ZOOM_DTYPE) for z in range(nl)], True)

    def profile_bigwig_ms(self):
        """device time of the bigWig kernels of the last profile_bigwig() (up_timings [9])"""
        t = np.zeros(10, np.float64)
        _ck(self.L.up_timings(self.ctx, t.ctypes.data, 10))
        return float(t[9])

    def set_profile_capture(self, on):
        _ck(self.L.up_set_profile_capture(self.ctx, int(bool(on))))

    def set_wide_nd_full(self, on):
        """nondirectional units at bw 512..32767: K1w with the -w capture on, the dense
        profile and run_async() as well (up_set_wide_nd_full; off by default)"""
        _ck(self.L.up_set_wide_nd_full(self.ctx, int(bool(on))))

    def set_wide_q11_nd(self, on):
        """nondirectional units at bw 512..32767 and a threshold <= 0: wide K1q instead of
        the replay, inside the blocking run() (up_set_wide_q11_nd; off by default)"""
        _ck(self.L.up_set_wide_q11_nd(self.ctx, int(bool(on))))

    def set_head_place(self, on):
        """head units (quirk Q1) replayed and merged on the device inside the pass
        (up_set_head_place; off by default, UNIPEAK_HEAD_PLACE=1 at open turns it on)"""
        _ck(self.L.up_set_head_place(self.ctx, int(bool(on))))

    def last_head_kind(self):
        """head units of the pass completed last: 0 merged on the host, 1 replayed and
        placed inside the pass, -1 none / a whole-context path (up_last_head_kind)"""
        return int(self.L.up_last_head_kind(self.ctx))

    def unit_resync(self, unit):
        """the unit's resync position after the last pass: 0 not replayed, X replayed up
        to X, 0xFFFFFFFF to its end (up_unit_replay_profile, with or without the capture)"""
        rs, n = ctypes.c_uint32(), ctypes.c_uint64()
        rc = self.L.up_unit_replay_profile(self.ctx, unit, ctypes.byref(rs), ctypes.byref(n), None, None,
                                           None, 0)
        if rc not in (UP_OK, UP_E_STATE) or (rc == UP_E_STATE and rs.value == 0):
            _ck(rc)
        return rs.value

    def replay_profile(self, unit):
        """(resync, event[], pos[], score[]) of a replayed unit (up_unit_replay_profile)"""
        rs, n = ctypes.c_uint32(), ctypes.c_uint64()
        _ck(self.L.up_unit_replay_profile(self.ctx, unit, ctypes.byref(rs), ctypes.byref(n), None, None,
                                          None, 0))
        ev = np.zeros(n.value, np.uint32)
        pos = np.zeros(n.value, np.uint32)
        sc = np.zeros(n.value, np.float64)
        if n.value:
            _ck(self.L.up_unit_replay_profile(self.ctx, unit, ctypes.byref(rs), ctypes.byref(n),
                                              ev.ctypes.data, pos.ctypes.data, sc.ctypes.data, n.value))
        return rs.value, ev, pos, sc


class Tir:
    """One up_tir handle: tags_in_regions' streams and queries on one GPU."""

    def __init__(self, device=0):
        self.L = load_library()
        self.h = ctypes.c_void_p()
        _ck(self.L.up_tir_open(device, ctypes.byref(self.h)))
        self.n = 0

    def close(self):
        if self.h:
            self.L.up_tir_close(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, idx, contig, first, count, forward):
        key = (np.asarray(contig, np.uint64) << np.uint64(32)) | np.asarray(first, np.uint64)
        cnt = np.ascontiguousarray(count, np.uint32)
        fwd = np.ascontiguousarray(forward, np.uint8)
        _ck(self.L.up_tir_set_stream(self.h, idx, len(key), key.ctypes.data, cnt.ctypes.data,
                                     fwd.ctypes.data))
        self.n = max(self.n, idx + 1)

    def query(self, contig, left, right, forward, n_streams=None):
        """(first, end, hits), each [R][n_streams] uint32"""
        S = n_streams or self.n
        rc = np.ascontiguousarray(contig, np.uint32)
        rl = np.ascontiguousarray(left, np.uint32)
        rr = np.ascontiguousarray(right, np.uint32)
        rf = np.ascontiguousarray(forward, np.uint8)
        R = len(rc)
        out = [np.zeros((R, S), np.uint32) for _ in range(3)]
        _ck(self.L.up_tir_query(self.h, S, R, rc.ctypes.data, rl.ctypes.data, rr.ctypes.data,
                                rf.ctypes.data, *(o.ctypes.data for o in out)))
        return tuple(out)

    def timings(self):
        t = np.zeros(2, np.float64)
        _ck(self.L.up_tir_timings(self.h, t.ctypes.data, 2))
        return t


class CountMap:
    """One up_cm handle: convert_align's CountMap as dense HBM tracks."""

    def __init__(self, contig_lens, device=0):
        self.L = load_library()
        self.h = ctypes.c_void_p()
        lens = np.ascontiguousarray(contig_lens, np.uint32)
        _ck(self.L.up_cm_open(device, len(lens), lens.ctypes.data, ctypes.byref(self.h)))

    def close(self):
        if self.h:
            self.L.up_cm_close(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def add(self, contig, pos, forward, count=None):
        c = np.ascontiguousarray(contig, np.uint32)
        p = np.ascontiguousarray(pos, np.uint32)
        f = np.ascontiguousarray(forward, np.uint8)
        k = None if count is None else np.ascontiguousarray(count, np.uint32)
        _ck(self.L.up_cm_add(self.h, len(p), c.ctypes.data, p.ctypes.data, f.ctypes.data,
                             None if k is None else k.ctypes.data))

    def collect(self, nondir=False):
        """(contig, pos, count, forward) in the iterators' order"""
        n = ctypes.c_uint64()
        _ck(self.L.up_cm_collect(self.h, int(nondir), ctypes.byref(n), None, None, None, None, 0))
        out = [np.zeros(n.value, np.uint32) for _ in range(3)] + [np.zeros(n.value, np.uint8)]
        if n.value:
            _ck(self.L.up_cm_collect(self.h, int(nondir), ctypes.byref(n), *(o.ctypes.data for o in out),
                                     n.value))
        return tuple(out)


def dfl_block():
    """input bytes per independent block of the device's DEFLATE encoder (up_dfl_block)"""
    return int(load_library().up_dfl_block())


def dfl_bound(n):
    """upper bound of Deflate.stream's output for n input bytes (up_dfl_bound)"""
    return int(load_library().up_dfl_bound(int(n)))


def dfl_code_lengths(freq, max_len=15):
    """length-limited Huffman code lengths as the encoder's kernel builds them, on the
    host (up_dfl_code_lengths): a uint8 array, 0 for an unused symbol"""
    L = load_library()
    f = np.ascontiguousarray(freq, np.uint32)
    out = np.zeros(len(f), np.uint8)
    _ck(L.up_dfl_code_lengths(f.ctypes.data, len(f), int(max_len), out.ctypes.data))
    return out


class Deflate:
    """One up_dfl handle: the DEFLATE encoder on the device."""

    def __init__(self, device=0):
        self.L = load_library()
        self.h = ctypes.c_void_p()
        _ck(self.L.up_dfl_open(device, ctypes.byref(self.h)))

    def close(self):
        if self.h:
            self.L.up_dfl_close(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def stream(self, data):
        """(raw DEFLATE bytes without a final block, CRC-32 of data)"""
        buf = np.frombuffer(bytes(data), np.uint8)
        out, n, crc = ctypes.c_void_p(), ctypes.c_uint64(0), ctypes.c_uint32(0)
        _ck(self.L.up_dfl_stream(self.h, buf.ctypes.data if len(buf) else None, len(buf), ctypes.byref(out),
                                 ctypes.byref(n), ctypes.byref(crc)))
        return ctypes.string_at(out.value, n.value) if n.value else b"", crc.value

    def segments(self, data, offsets):
        """one zlib stream per segment data[offsets[i]:offsets[i + 1]], as a list of bytes"""
        buf = np.frombuffer(bytes(data), np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        n_seg = len(off) - 1
        out, oo = ctypes.c_void_p(), np.zeros(n_seg + 1, np.uint64)
        _ck(self.L.up_dfl_segments(self.h, buf.ctypes.data if len(buf) else None, off.ctypes.data, n_seg,
                                   ctypes.byref(out), oo.ctypes.data))
        raw = ctypes.string_at(out.value, int(oo[n_seg])) if oo[n_seg] else b""
        return [raw[int(oo[i]):int(oo[i + 1])] for i in range(n_seg)]

    def timings(self):
        """[device ms of the kernels, input bytes, output bytes, calls] since open"""
        t = np.zeros(4, np.float64)
        _ck(self.L.up_dfl_timings(self.h, t.ctypes.data, 4))
        return t


# UP_BZ_* reasons (include/unipeak_hip.h)
(BZ_OK, BZ_NOT_BZIP2, BZ_BAD_LEVEL, BZ_TRUNCATED, BZ_BAD_MAGIC, BZ_RANDOMISED, BZ_ORIGPTR, BZ_SYMMAP,
 BZ_NGROUPS, BZ_NSELECTORS, BZ_SELECTOR, BZ_CODELEN, BZ_BAD_CODE, BZ_OVERFLOW, BZ_BLOCK_CRC, BZ_STREAM_CRC,
 BZ_TRAILING, BZ_NOSPACE) = range(18)


class BzInfo(ctypes.Structure):  # up_bz_info_t
    _fields_ = [
        ("streams", ctypes.c_uint32),
        ("blocks", ctypes.c_uint32),
        ("dropped", ctypes.c_uint32),
        ("reason", ctypes.c_int32),
        ("fail_bit", ctypes.c_uint64),
    ]


class BzError(ValueError):
    """corrupt bzip2 data: .reason is a BZ_* code, .info the whole up_bz_info_t"""

    def __init__(self, info):
        self.info, self.reason = info, int(info.reason)
        text = load_library().up_bz_reason(self.reason).decode()
        super().__init__(f"{text} (reason {self.reason}, bit {int(info.fail_bit)})")


def _bz_result(rc, info):
    if rc == -1 and info.reason != BZ_OK:  # UP_E_ARG with a reason: the data, not the call
        raise BzError(info)
    _ck(rc)


def bunzip_host(data):
    """(decoded bytes, BzInfo) through the host twin (up_bz_decode_host); BzError on corrupt data"""
    L = load_library()
    buf = np.frombuffer(bytes(data), np.uint8)
    src = buf.ctypes.data if len(buf) else None
    cap = max(4 * len(buf), 1 << 16)
    for _ in range(2):
        dst, n, info = np.zeros(cap, np.uint8), ctypes.c_uint64(0), BzInfo()
        rc = L.up_bz_decode_host(src, len(buf), dst.ctypes.data, cap, ctypes.byref(n), ctypes.byref(info))
        if rc == -1 and info.reason == BZ_NOSPACE:
            cap = int(n.value)  # the full size: the second call fits
            continue
        _bz_result(rc, info)
        return dst[:n.value].tobytes(), info
    raise RuntimeError("up_bz_decode_host: size changed between calls")


class Bunzip:
    """One up_bz handle: the bzip2 decoder on the device."""

    def __init__(self, device=0):
        self.L = load_library()
        self.h = ctypes.c_void_p()
        _ck(self.L.up_bz_open(device, ctypes.byref(self.h)))

    def close(self):
        if self.h:
            self.L.up_bz_close(self.h)
            self.h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def decode(self, data):
        """(decoded bytes, BzInfo) of a whole .bz2 file image; BzError on corrupt data"""
        buf = np.frombuffer(bytes(data), np.uint8)
        out, n, info = ctypes.c_void_p(), ctypes.c_uint64(0), BzInfo()
        rc = self.L.up_bz_decode(self.h, buf.ctypes.data if len(buf) else None, len(buf), ctypes.byref(out),
                                 ctypes.byref(n), ctypes.byref(info))
        _bz_result(rc, info)
        return (ctypes.string_at(out.value, n.value) if n.value else b""), info

    def scan(self, data):
        """(bit offsets, kinds) of every block magic (kind 0) and end magic (kind 1), ascending"""
        buf = np.frombuffer(bytes(data), np.uint8)
        src = buf.ctypes.data if len(buf) else None
        n = ctypes.c_uint64(0)
        _ck(self.L.up_bz_scan(self.h, src, len(buf), None, None, 0, ctypes.byref(n)))
        bits, kinds = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint8)
        if n.value:
            _ck(self.L.up_bz_scan(self.h, src, len(buf), bits.ctypes.data, kinds.ctypes.data, n.value,
                                  ctypes.byref(n)))
        return bits, kinds

    def timings(self):
        """device ms of [scan, entropy, rank, walks, run-length + CRC], then input bytes, output
        bytes and calls, since open"""
        t = np.zeros(8, np.float64)
        _ck(self.L.up_bz_timings(self.h, t.ctypes.data, 8))
        return t
