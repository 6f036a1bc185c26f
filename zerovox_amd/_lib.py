"""ctypes binding of libzvx (include/zvx.h).  No fallback: if the HIP library or a GPU is missing,
every entry point raises -- the product path never routes through a CPU implementation."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libzvx.so")

ZVX_OK = 0
ZVX_E_INVALID, ZVX_E_MANIFEST, ZVX_E_HIP, ZVX_E_STATE, ZVX_E_BUFFER, ZVX_E_UNSUPPORTED = 1, 2, 3, 4, 5, 6
ZVX_DEVICE_OUT, ZVX_NO_SYNC, ZVX_PCM16, ZVX_DEVICE_IN, ZVX_HOST_ASYNC, ZVX_NATIVE_RATE = 1, 2, 4, 8, 16, 32
ZVX_DEVICE_SPK = 64                                  # zvx_synthesize / zvx_synthesize_ex: spk is a device pointer
STAGES = ("encoder", "variance", "lenreg", "decoder", "vocoder", "spkemb")
ZVX_T_RESAMPLE = 6                                   # its own accessor (Context.resample_ms): stage_times() keeps exactly STAGES
ZVX_T_JOIN = 7                                       # likewise (Context.join_ms)
ZVX_T_COUNT = 8

EXPORTS = ("zvx_create", "zvx_destroy", "zvx_last_error", "zvx_get_int", "zvx_set_int", "zvx_spkemb", "zvx_melspec", "zvx_encode",
           "zvx_decode", "zvx_decode_features", "zvx_vocode", "zvx_vocode_mel", "zvx_synthesize", "zvx_fetch",
           "zvx_sync", "zvx_stage_times", "zvx_kernel_stats", "zvx_tag_stats", "zvx_reset_stats",
           "zvx_comm_unique_id", "zvx_comm_init", "zvx_comm_gather", "zvx_comm_barrier", "zvx_comm_max_f64", "zvx_comm_info", "zvx_comm_destroy",
           "zvx_dev_alloc", "zvx_dev_free", "zvx_dev_from_host", "zvx_dev_to_host", "zvx_spkemb_ex", "zvx_wait_host",
           "zvx_encode_ex", "zvx_synthesize_ex", "zvx_resample", "zvx_resample_ex", "zvx_trim_bounds", "zvx_join",
           "zvx_loudness", "zvx_normalize", "zvx_true_peak", "zvx_limit", "zvx_spkemb_wav", "zvx_limit_ex", "zvx_denoise_bias", "zvx_denoise",
           "zvx_denoise_ex", "zvx_stream_open", "zvx_stream_next", "zvx_stream_info", "zvx_stream_close", "zvx_stream_next_many",
           "zvx_denoise_rows", "zvx_limit_rows", "zvx_resample_rows", "zvx_level", "zvx_level_ex", "zvx_level_rows", "zvx_loudness_stats",
           "zvx_pitch", "zvx_watermark", "zvx_watermark_ex", "zvx_watermark_detect", "zvx_watermark_rows", "zvx_watermark_identify",
           "zvx_stream_open_ex", "zvx_spk_score", "zvx_spk_topk", "zvx_dev_copy", "zvx_dtw", "zvx_align_wav", "zvx_fir", "zvx_fir_ex",
           "zvx_fir_rows")
# columns of zvx_align_wav's stats[B][ZVX_AL_COUNT]
ZVX_AL_FRAMES_A, ZVX_AL_FRAMES_B, ZVX_AL_PATH_LEN, ZVX_AL_COST, ZVX_AL_MCD_DB, ZVX_AL_COUNT = range(6)
DTW_MAX_FRAMES, DTW_MAX_DIM = 4096, 32               # zvx_dtw's caps (csrc/zvx_kernels.h; ZVX_E_UNSUPPORTED beyond)
ZVX_SPK_TOP_MAX = 32                                 # the most places zvx_spk_topk returns per query
ZVX_STREAM_MANY_MAX_SESSIONS, ZVX_STREAM_MANY_MAX_ROWS = 64, 256
ZVX_COMM_ID_BYTES = 128
ZVX_LOUD_PER_ROW, ZVX_LOUD_COMMON = 0, 1
# columns of zvx_loudness_stats' stats[B][ZVX_LS_COUNT], and the keys Context.loudness_stats gives them
(ZVX_LS_INTEGRATED, ZVX_LS_MOMENTARY_MAX, ZVX_LS_SHORT_MAX, ZVX_LS_LRA, ZVX_LS_LRA_LOW, ZVX_LS_LRA_HIGH, ZVX_LS_SHORT_GATED, ZVX_LS_PEAK,
 ZVX_LS_COUNT) = range(9)
LOUDNESS_STATS_KEYS = ("integrated", "max_momentary", "max_short_term", "lra", "lra_low", "lra_high", "short_gated", "peak")
LOUDNESS_STATS_MAX_UNITS = 65536                     # the longest row zvx_loudness_stats takes, in 100 ms units
# columns of zvx_pitch's stats[B][ZVX_PS_COUNT], and the keys Context.pitch gives them
ZVX_PS_FRAMES, ZVX_PS_VOICED, ZVX_PS_MEDIAN, ZVX_PS_LOW, ZVX_PS_HIGH, ZVX_PS_MEAN, ZVX_PS_COUNT = range(7)
PITCH_STATS_KEYS = ("frames", "voiced", "median", "low", "high", "mean")
PITCH_MAX_WINDOW, PITCH_MAX_TAU, PITCH_MAX_FRAMES = 4096, 2048, 65536     # zvx_pitch's caps (csrc/zvx_kernels.h; ZVX_E_UNSUPPORTED beyond)
LIMIT_TILE = 1024                                    # samples per workgroup of both limiter kernels (csrc/zvx_kernels.h, LIMIT_TILE)
LIMIT_MAX_W = 4096                                   # the longest window, in samples (LIMIT_MAX_W)
LIMIT_ENV_REACH = 11                                 # samples the oversampled envelope reads to either side (LIMIT_ENV_REACH; limiter.reach)
ZVX_FIR_MAX_TAPS = 4096                              # the longest filter zvx_fir takes (ZVX_E_UNSUPPORTED beyond)


def resampled_len(n, rate_in, rate_out):
    """ceil(n * L / M) with L / M = rate_out / rate_in in lowest terms: the samples zvx_resample makes of n (exact integers)."""
    from math import gcd
    g = gcd(int(rate_in), int(rate_out))
    L, M = int(rate_out) // g, int(rate_in) // g
    return (int(n) * L + M - 1) // M


class ZvxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"zvx error {code}: {msg}")
        self.code = code


class JoinParams(C.Structure):
    """zvx_join_params (include/zvx.h)"""
    _fields_ = [("frame", C.c_int32), ("hop", C.c_int32), ("top_db", C.c_float), ("keep", C.c_int32), ("fade", C.c_int32)]


class RefParams(C.Structure):
    """zvx_ref_params (include/zvx.h)"""
    _fields_ = [("frame", C.c_int32), ("hop", C.c_int32), ("top_db", C.c_float), ("keep", C.c_int32), ("max_samples", C.c_int32)]


class LoudnessParams(C.Structure):
    """zvx_loudness_params (include/zvx.h)"""
    _fields_ = [("target_lufs", C.c_float), ("peak_ceiling", C.c_float), ("max_gain_db", C.c_float), ("mode", C.c_int32)]


class LimitParams(C.Structure):
    """zvx_limit_params (include/zvx.h)"""
    _fields_ = [("ceiling", C.c_float), ("window_ms", C.c_float), ("oversample", C.c_int32)]


class LevelParams(C.Structure):
    """zvx_level_params (include/zvx.h)"""
    _fields_ = [("target_lufs", C.c_float), ("max_gain_db", C.c_float), ("window_ms", C.c_float), ("lookahead_ms", C.c_float)]


class PitchParams(C.Structure):
    """zvx_pitch_params (include/zvx.h)"""
    _fields_ = [("fmin", C.c_float), ("fmax", C.c_float), ("threshold", C.c_float), ("gate_db", C.c_float), ("window", C.c_int32),
                ("hop", C.c_int32)]


class DtwParams(C.Structure):
    """zvx_dtw_params (include/zvx.h)"""
    _fields_ = [("reserved", C.c_int32 * 4)]


class AlignParams(C.Structure):
    """zvx_align_params (include/zvx.h)"""
    _fields_ = [("n_cep", C.c_int32), ("reserved", C.c_int32 * 3)]


class DenoiseParams(C.Structure):
    """zvx_denoise_params (include/zvx.h)"""
    _fields_ = [("strength", C.c_float), ("floor", C.c_float)]


class WatermarkParams(C.Structure):
    """zvx_watermark_params (include/zvx.h)"""
    _fields_ = [("key", C.c_uint64), ("depth_db", C.c_float), ("lo_hz", C.c_float), ("hi_hz", C.c_float), ("block_frames", C.c_int32),
                ("band_bins", C.c_int32), ("period_blocks", C.c_int32), ("reserved", C.c_int32)]


class RowWindow(C.Structure):
    """zvx_row_window (include/zvx.h)"""
    _fields_ = [("in_origin", C.c_int64), ("out_begin", C.c_int64), ("out_count", C.c_int64), ("last", C.c_int32), ("reserved", C.c_int32)]


class StreamParams(C.Structure):
    """zvx_stream_params (include/zvx.h)"""
    _fields_ = [("chunk_frames", C.c_int32), ("chunks_per_call", C.c_int32), ("halo", C.c_int32), ("denoise", C.POINTER(DenoiseParams)),
                ("denoise_bias", C.c_void_p), ("limit", C.POINTER(LimitParams))]


class StreamStages(C.Structure):
    """zvx_stream_stages (include/zvx.h): the stages zvx_stream_open_ex adds to zvx_stream_params"""
    _fields_ = [("level", C.POINTER(LevelParams)), ("watermark", C.POINTER(WatermarkParams)), ("reserved", C.c_int64 * 2)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("launches", C.c_int64), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


_lib = None


def load():
    """dlopen libzvx.so (built in-tree by zerovox_amd.build).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ZvxError(ZVX_E_HIP, f"{LIB_PATH} not found: build it with `python -m zerovox_amd.build` "
                                  f"(there is no CPU fallback)")
    lib = C.CDLL(LIB_PATH)
    vp, i32p, f32p = C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_float)
    lib.zvx_create.argtypes = [C.c_char_p, vp, C.c_size_t, C.c_int, C.POINTER(vp)]
    lib.zvx_destroy.argtypes = [vp]
    lib.zvx_destroy.restype = None
    lib.zvx_last_error.argtypes = [vp]
    lib.zvx_last_error.restype = C.c_char_p
    lib.zvx_get_int.argtypes = [vp, C.c_char_p]
    lib.zvx_get_int.restype = C.c_int64
    lib.zvx_set_int.argtypes = [vp, C.c_char_p, C.c_int64]
    lib.zvx_spkemb.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
    lib.zvx_melspec.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, vp]
    lib.zvx_encode.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp]
    lib.zvx_encode_ex.argtypes = lib.zvx_encode.argtypes + [vp]
    lib.zvx_decode.argtypes = [vp, vp, C.c_int, C.c_int]
    lib.zvx_decode_features.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int]
    lib.zvx_vocode.argtypes = [vp, vp, vp, C.c_int64, C.c_int]
    lib.zvx_vocode_mel.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int64, C.c_int]
    lib.zvx_synthesize.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int, vp, C.c_int64, vp, vp,
                                   C.c_int, vp, C.c_int]
    lib.zvx_synthesize_ex.argtypes = lib.zvx_synthesize.argtypes + [vp]
    lib.zvx_fetch.argtypes = [vp, C.c_char_p, vp, C.c_size_t]
    lib.zvx_sync.argtypes = [vp]
    lib.zvx_stage_times.argtypes = [vp, vp]
    lib.zvx_kernel_stats.argtypes = [vp, C.POINTER(KernelStat), C.c_int]
    lib.zvx_reset_stats.argtypes = [vp]
    lib.zvx_tag_stats.argtypes = [vp, C.POINTER(KernelStat), C.c_int]
    lib.zvx_comm_unique_id.argtypes = [vp]
    lib.zvx_comm_init.argtypes = [vp, vp, C.c_int, C.c_int]
    lib.zvx_comm_gather.argtypes = [vp, vp, C.c_size_t, vp, C.c_int, C.c_int]
    lib.zvx_comm_barrier.argtypes = [vp]
    lib.zvx_comm_max_f64.argtypes = [vp, C.POINTER(C.c_double)]
    lib.zvx_comm_info.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
    lib.zvx_comm_destroy.argtypes = [vp]
    lib.zvx_comm_destroy.restype = None
    lib.zvx_dev_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.zvx_dev_free.argtypes = [vp, vp]
    lib.zvx_dev_to_host.argtypes = [vp, vp, vp, C.c_size_t]
    lib.zvx_dev_copy.argtypes = [vp, vp, vp, C.c_size_t]
    lib.zvx_spk_score.argtypes = [vp, vp, C.c_int, vp, C.c_int64, C.c_int, vp, C.c_int]
    lib.zvx_spk_topk.argtypes = [vp, vp, C.c_int, vp, C.c_int64, C.c_int, C.c_int, vp, vp, C.c_int]
    lib.zvx_dev_from_host.argtypes = [vp, vp, vp, C.c_size_t]
    lib.zvx_spkemb_ex.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int]
    lib.zvx_wait_host.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.zvx_resample.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int64, vp, C.c_int]
    lib.zvx_resample_ex.argtypes = lib.zvx_resample.argtypes + [C.c_int64, C.c_int64, C.c_int64]
    lib.zvx_trim_bounds.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(JoinParams), vp, vp, C.c_int]
    lib.zvx_join.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(JoinParams), vp, C.c_int64, C.POINTER(C.c_int64), vp, vp, vp, C.c_int]
    lib.zvx_loudness.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, C.c_int]
    lib.zvx_normalize.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(LoudnessParams), vp, C.c_int64, vp, vp, vp, C.c_int]
    lib.zvx_loudness_stats.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp, C.c_int64, C.c_int]
    lib.zvx_pitch.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(PitchParams), vp, vp, C.c_int64, vp, vp, C.c_int]
    lib.zvx_dtw.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(DtwParams), vp, vp, vp, C.c_int64, vp, C.c_int]
    lib.zvx_align_wav.argtypes = [vp, vp, vp, C.c_int, vp, vp, C.c_int, C.c_int, C.POINTER(AlignParams), vp, vp, C.c_int64, vp, C.c_int64, vp, vp,
                                  C.c_int64, C.c_int]
    lib.zvx_true_peak.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, C.c_int]
    lib.zvx_limit.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(LimitParams), vp, C.c_int64, vp, vp, C.c_int]
    lib.zvx_limit_ex.argtypes = lib.zvx_limit.argtypes + [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    lib.zvx_spkemb_wav.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(RefParams), vp, vp, vp, vp, C.c_int]
    lib.zvx_denoise_bias.argtypes = [vp, vp]
    lib.zvx_denoise.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.POINTER(DenoiseParams), vp, C.c_int64, C.c_int]
    lib.zvx_denoise_ex.argtypes = lib.zvx_denoise.argtypes + [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    lib.zvx_denoise_rows.argtypes = lib.zvx_denoise.argtypes + [C.POINTER(RowWindow)]
    lib.zvx_watermark.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(WatermarkParams), vp, C.c_int64, C.c_int]
    lib.zvx_watermark_ex.argtypes = lib.zvx_watermark.argtypes + [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    lib.zvx_watermark_detect.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(WatermarkParams), C.c_int, vp, vp, vp, vp, vp, C.c_int, C.c_int]
    lib.zvx_watermark_rows.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(WatermarkParams), vp, vp, C.c_int64, C.c_int, C.POINTER(RowWindow)]
    lib.zvx_watermark_identify.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.POINTER(WatermarkParams), vp, C.c_int, C.c_int, vp, vp, vp, vp, C.c_int]
    lib.zvx_limit_rows.argtypes = lib.zvx_limit.argtypes + [C.POINTER(RowWindow)]
    lib.zvx_resample_rows.argtypes = lib.zvx_resample.argtypes + [C.POINTER(RowWindow)]
    lib.zvx_level.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.POINTER(LevelParams), vp, C.c_int64, vp, vp, C.c_int]
    lib.zvx_level_ex.argtypes = lib.zvx_level.argtypes + [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    lib.zvx_level_rows.argtypes = lib.zvx_level.argtypes + [C.POINTER(RowWindow)]
    lib.zvx_fir.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, vp, C.c_int64, C.c_int]
    lib.zvx_fir_ex.argtypes = lib.zvx_fir.argtypes + [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    lib.zvx_fir_rows.argtypes = lib.zvx_fir.argtypes + [C.POINTER(RowWindow)]
    lib.zvx_stream_open.argtypes = [vp, vp, C.c_int, C.POINTER(StreamParams), C.c_int, C.POINTER(vp)]
    lib.zvx_stream_open_ex.argtypes = [vp, vp, C.c_int, C.POINTER(StreamParams), C.POINTER(StreamStages), C.c_int, C.POINTER(vp)]
    lib.zvx_stream_next.argtypes = [vp, vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int]
    lib.zvx_stream_info.argtypes = [vp, C.POINTER(C.c_int64), C.c_int]
    lib.zvx_stream_close.argtypes = [vp]
    lib.zvx_stream_next_many.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.c_int]
    _lib = lib
    return lib


def _ptr(a):
    """the array's address; the pointer object holds the array, which so lives as long as the arguments of the call it goes into"""
    if a is None:
        return None
    p = a.ctypes.data_as(C.c_void_p)
    p._array = a
    return p


def _i32(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.int32)
    if shape is not None:
        assert a.shape == tuple(shape), (a.shape, shape)
    return a


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class Stream:
    """One stream session (wraps zvx_stream*; Context.stream_open makes it).  Iterating yields the float32 pieces, skipping empty ones;
    the session closes itself when exhausted or collected.  It belongs to its context and must not outlive it."""

    def __init__(self, ctx, handle, keep):
        self._ctx, self._h, self._keep, self.done = ctx, handle, keep, False

    def info(self):
        """-> dict(total, emitted, rate, delay, max_piece): zvx_stream_info's five values"""
        v = (C.c_int64 * 5)()
        self._ctx._chk(self._ctx._lib.zvx_stream_info(self._h, v, 5))
        return dict(zip(("total", "emitted", "rate", "delay", "max_piece"), (int(x) for x in v)))

    def next_piece(self, capacity=None):
        """one zvx_stream_next into host memory -> the piece (np.float32, possibly empty); self.done tells whether it was the last.
        capacity: samples of the buffer handed in (None: max_piece); too small raises ZvxError(ZVX_E_BUFFER) with nothing consumed,
        its ``n_out`` attribute carrying the size the piece needs."""
        cap = self.info()["max_piece"] if capacity is None else int(capacity)
        out = np.empty(max(cap, 1), np.float32)
        n, done = self._next(_ptr(out), cap, 0)
        return out[:n]

    def next_device(self, ptr, capacity, no_sync=False):
        """one zvx_stream_next into device memory at ``ptr`` (ZVX_DEVICE_OUT; with no_sync the call only queues) -> samples written"""
        return self._next(C.c_void_p(int(ptr)), int(capacity), ZVX_DEVICE_OUT | (ZVX_NO_SYNC if no_sync else 0))[0]

    def _next(self, out, capacity, flags):
        n, done = C.c_int64(-1), C.c_int32(0)
        rc = self._ctx._lib.zvx_stream_next(self._h, out, capacity, C.byref(n), C.byref(done), flags)
        if rc != ZVX_OK:
            e = ZvxError(rc, self._ctx._lib.zvx_last_error(self._ctx._h).decode())
            e.n_out = int(n.value)
            raise e
        self.done = bool(done.value)
        return int(n.value), self.done

    def __iter__(self):
        try:
            while self._h and not self.done:
                piece = self.next_piece()
                if len(piece):
                    yield piece
        finally:
            self.close()

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._ctx._lib.zvx_stream_close(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One synthesis context on one HIP device (wraps zvx_ctx*)."""

    def __init__(self, manifest: str, blob: np.ndarray, device: int = 0):
        self._lib = load()
        self._h = C.c_void_p()
        blob = _f32(blob)
        rc = self._lib.zvx_create(manifest.encode(), _ptr(blob), blob.nbytes, device, C.byref(self._h))
        if rc != ZVX_OK:
            raise ZvxError(rc, self._lib.zvx_last_error(None).decode())
        self.hidden = self.get_int("hidden")
        self.n_mels = self.get_int("n_mels")
        self.hop = self.get_int("hop")
        self.device = device
        self.rank, self.world = 0, 1                 # until comm_init: comm_info() then reports the C side's ZVX_E_STATE, not an AttributeError

    def close(self):
        if getattr(self, "_h", None):
            self._lib.zvx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != ZVX_OK:
            raise ZvxError(rc, self._lib.zvx_last_error(self._h).decode())

    def get_int(self, key):
        return int(self._lib.zvx_get_int(self._h, key.encode()))

    def set_int(self, key, value):
        self._chk(self._lib.zvx_set_int(self._h, key.encode(), int(value)))

    # ---- stages -------------------------------------------------------------------------------
    def spkemb(self, ref_mels, lens):
        ref_mels = _f32(ref_mels)
        B, Tmax, F = ref_mels.shape
        assert F == self.n_mels
        lens = _i32(lens, (B,))
        out = np.empty((B, self.hidden), np.float32)
        self._chk(self._lib.zvx_spkemb(self._h, _ptr(ref_mels), _ptr(lens), B, Tmax, _ptr(out)))
        return out

    def spkemb_wav(self, rows, rate=None, *, frame=2048, hop=512, top_db=40.0, keep=0, max_samples=0, lengths=None):
        """zvx_spkemb_wav on host rows: reference clips at `rate` Hz (None: the model's) -> speaker embeddings, every step on the device:
        conversion to the model's rate, the silence trim of mels.trim_silence (frame / hop / top_db / keep as for trim_bounds; top_db <= 0:
        none), a cut to the first max_samples samples of the trimmed clip (0: none), the log-mel front end and the speaker encoder
        -> (emb [B][hidden] float32, begin [B], end [B], frames [B] int32; the bounds are in samples at the model's rate).
        rows: a list of 1-D float waveforms, or a padded 2-D array + lengths."""
        x, n = self._rows(rows, lengths)
        B, Nmax = x.shape
        prm = RefParams(int(frame), int(hop), float(top_db), int(keep), int(max_samples))
        out = np.empty((B, self.hidden), np.float32)
        begin, end, frames = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._chk(self._lib.zvx_spkemb_wav(self._h, _ptr(x), _ptr(n), B, Nmax, self._rate(rate), C.byref(prm), _ptr(out), _ptr(begin), _ptr(end),
                                           _ptr(frames), 0))
        return out, begin, end, frames

    def spkemb_wav_device(self, ptr, lengths, Nmax, out_ptr, rate=None, *, frame=2048, hop=512, top_db=40.0, keep=0, max_samples=0, no_sync=False):
        """zvx_spkemb_wav on device rows [B][Nmax] f32 at `ptr` (ZVX_DEVICE_IN; they may be the output of a synthesize(..., no_sync=True)
        call queued just before: stream order is the fence) into device embeddings [B][hidden] f32 at out_ptr (ZVX_DEVICE_OUT) -- what
        synthesize(..., spk=out_ptr) takes.  The call waits once, for the bounds; with no_sync everything behind that wait is only queued.
        -> (begin, end, frames)."""
        n = _i32(lengths)
        B = len(n)
        prm = RefParams(int(frame), int(hop), float(top_db), int(keep), int(max_samples))
        begin, end, frames = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._chk(self._lib.zvx_spkemb_wav(self._h, C.c_void_p(int(ptr)), _ptr(n), B, int(Nmax), self._rate(rate), C.byref(prm), C.c_void_p(int(out_ptr)),
                                           _ptr(begin), _ptr(end), _ptr(frames), ZVX_DEVICE_IN | ZVX_DEVICE_OUT | (ZVX_NO_SYNC if no_sync else 0)))
        return begin, end, frames

    # ---- voice matching (include/zvx.h: zvx_spk_score, zvx_spk_topk) -----------------------------------------------
    def _spk_queries(self, queries, dim):
        """host queries [B][dim] (or [B][1][dim], or one [dim]) -> (pointer, B, dim, flags 0)"""
        dim = self.hidden if dim is None else int(dim)
        q = _f32(queries)
        if q.ndim == 3 and q.shape[1] == 1:
            q = q[:, 0, :]
        q = np.ascontiguousarray(q.reshape(-1, dim) if q.ndim == 1 else q)
        if q.ndim != 2 or q.shape[1] != dim:
            raise ValueError(f"queries of shape {tuple(np.shape(queries))} are not [B][{dim}]")
        return _ptr(q), q.shape[0], dim, 0

    def spk_score(self, queries, lib_ptr, K, dim=None):
        """zvx_spk_score: cosine scores of host queries [B][dim] against the K device rows at lib_ptr -> score [B][K] float32
        (dim: None = the model's hidden width).  A score that is not finite is -2."""
        qp, B, dim, flags = self._spk_queries(queries, dim)
        out = np.empty((B, int(K)), np.float32)
        self._chk(self._lib.zvx_spk_score(self._h, qp, B, C.c_void_p(int(lib_ptr)), int(K), dim, _ptr(out), flags))
        return out

    def spk_score_device(self, q_ptr, B, lib_ptr, K, out_ptr=None, dim=None, no_sync=False):
        """zvx_spk_score with device queries [B][dim] at q_ptr (ZVX_DEVICE_IN; stream order is the fence behind a queued zvx_spkemb_wav)
        -> score [B][K] float32 on the host, or with out_ptr into device scores there (ZVX_DEVICE_OUT; with no_sync the call only queues)"""
        dim = self.hidden if dim is None else int(dim)
        if out_ptr is None:
            out = np.empty((int(B), int(K)), np.float32)
            self._chk(self._lib.zvx_spk_score(self._h, C.c_void_p(int(q_ptr)), int(B), C.c_void_p(int(lib_ptr)), int(K), dim, _ptr(out), ZVX_DEVICE_IN))
            return out
        self._chk(self._lib.zvx_spk_score(self._h, C.c_void_p(int(q_ptr)), int(B), C.c_void_p(int(lib_ptr)), int(K), dim, C.c_void_p(int(out_ptr)),
                                          ZVX_DEVICE_IN | ZVX_DEVICE_OUT | (ZVX_NO_SYNC if no_sync else 0)))

    def spk_topk(self, queries, lib_ptr, K, top=5, dim=None):
        """zvx_spk_topk: per host query the `top` best cosine scores against the K device rows at lib_ptr, by descending score and
        ascending index among equal scores -> (score [B][top] float32, index [B][top] int32)"""
        qp, B, dim, flags = self._spk_queries(queries, dim)
        score, index = np.empty((B, int(top)), np.float32), np.empty((B, int(top)), np.int32)
        self._chk(self._lib.zvx_spk_topk(self._h, qp, B, C.c_void_p(int(lib_ptr)), int(K), dim, int(top), _ptr(score), _ptr(index), flags))
        return score, index

    def spk_topk_device(self, q_ptr, B, lib_ptr, K, score_ptr=None, index_ptr=None, top=5, dim=None, no_sync=False):
        """zvx_spk_topk with device queries (ZVX_DEVICE_IN) -> (score, index) [B][top] on the host, or with score_ptr / index_ptr into
        device results [B][top] f32 / int32 there (ZVX_DEVICE_OUT [| ZVX_NO_SYNC])"""
        dim = self.hidden if dim is None else int(dim)
        if score_ptr is None:
            score, index = np.empty((int(B), int(top)), np.float32), np.empty((int(B), int(top)), np.int32)
            self._chk(self._lib.zvx_spk_topk(self._h, C.c_void_p(int(q_ptr)), int(B), C.c_void_p(int(lib_ptr)), int(K), dim, int(top), _ptr(score),
                                             _ptr(index), ZVX_DEVICE_IN))
            return score, index
        self._chk(self._lib.zvx_spk_topk(self._h, C.c_void_p(int(q_ptr)), int(B), C.c_void_p(int(lib_ptr)), int(K), dim, int(top),
                                         C.c_void_p(int(score_ptr)), C.c_void_p(int(index_ptr)),
                                         ZVX_DEVICE_IN | ZVX_DEVICE_OUT | (ZVX_NO_SYNC if no_sync else 0)))

    def melspec(self, wavs):
        """list of 1-D float waveforms -> (log-mel [B][Tmax][n_mels], frames [B])   (get_mel_from_wav on the device)"""
        B = len(wavs)
        n = np.array([len(w) for w in wavs], np.int32)
        Nmax = int(n.max())
        wav = np.zeros((B, Nmax), np.float32)
        for b, w in enumerate(wavs):
            wav[b, :n[b]] = np.asarray(w, np.float32)
        pad = (self.get_int("fft_size") - self.hop) // 2
        Tmax = max(1, 1 + (Nmax + 2 * pad - self.get_int("fft_size")) // self.hop)
        mel = np.zeros((B, Tmax, self.n_mels), np.float32)
        frames = np.zeros(B, np.int32)
        self._chk(self._lib.zvx_melspec(self._h, _ptr(wav), _ptr(n), B, Nmax, _ptr(mel), Tmax, _ptr(frames)))
        return mel, frames

    def resample(self, rows, rate_in, rate_out, pcm16=False, lengths=None):
        """zvx_resample: a list of 1-D float waveforms (or a padded 2-D array + lengths) at rate_in -> (out [B][max out_len], out_len [B])
        at rate_out: float32, or int16 PCM (x32760, clamped, truncated) with pcm16; row b holds out_len[b] samples, then zeros."""
        return self.resample_window(rows, rate_in, rate_out, pcm16=pcm16, lengths=lengths)

    def resample_window(self, rows, rate_in, rate_out, in_origin=0, out_begin=0, out_count=-1, pcm16=False, lengths=None):
        """zvx_resample_ex: the rows hold samples [in_origin, in_origin + len) of signals that are zero elsewhere; outputs
        [out_begin, out_begin + out_count) (out_count -1: to the end of each row's signal) -> (out [B][n], out_len [B])."""
        x, n = self._rows(rows, lengths)
        B, Nmax = x.shape
        if out_count >= 0:
            cols = int(out_count)
        else:
            cols = max(0, max(resampled_len(int(in_origin) + int(v), rate_in, rate_out) for v in n) - int(out_begin))
        out = np.empty((B, max(cols, 1)), np.int16 if pcm16 else np.float32)
        if cols == 0:
            out[:] = 0
        out_len = np.zeros(B, np.int32)
        self._chk(self._lib.zvx_resample_ex(self._h, _ptr(x), _ptr(n), B, Nmax, int(rate_in), int(rate_out), _ptr(out), max(cols, 1), _ptr(out_len),
                                            ZVX_PCM16 if pcm16 else 0, int(in_origin), int(out_begin), int(out_count)))
        return out[:, :cols], out_len

    @staticmethod
    def _rows(rows, lengths):
        """a list of 1-D waveforms, or a padded 2-D array + lengths -> (x [B][Nmax] f32, n [B] i32)"""
        if lengths is None:
            B = len(rows)
            n = np.array([len(w) for w in rows], np.int32)
            x = np.zeros((B, max(int(n.max()) if B else 0, 1)), np.float32)
            for b, w in enumerate(rows):
                x[b, :n[b]] = np.asarray(w, np.float32)
            return x, n
        x = _f32(rows)
        return x, _i32(lengths, (x.shape[0],))

    def _rows_arg(self, rows, lengths, device_ptr=None, Nmax=None):
        """the rows of a call: a list of 1-D waveforms or a padded 2-D array + lengths on the host, or, with device_ptr, device rows
        [B][Nmax] f32 there and `lengths` -> (pointer, n [B] i32, B, Nmax, flags: 0 or ZVX_DEVICE_IN); the pointer holds the host array
        (_ptr)"""
        if device_ptr is None:
            x, n = self._rows(rows, lengths)
            return _ptr(x), n, x.shape[0], x.shape[1], 0
        n = _i32(lengths)
        return C.c_void_p(int(device_ptr)), n, len(n), int(Nmax), ZVX_DEVICE_IN

    @staticmethod
    def _window_out(n, Nmax, in_origin, out_begin, out_count, pcm16):
        """the output rows of a zvx_limit_ex / zvx_denoise_ex call -> (out [B][stride] of zeros, cols: the longest emitted row)"""
        cols = int(out_count) if out_count >= 0 else max(0, int(in_origin) + int(n.max() if len(n) else 0) - int(out_begin))
        return np.zeros((len(n), max(cols, Nmax)), np.int16 if pcm16 else np.float32), cols

    @staticmethod
    def _row_windows(windows, n, Nmax, pcm16, count=int):
        """a list of (in_origin, out_begin, out_count, last), one per row -> (RowWindow array, out [B][stride] of zeros, cnt [B]: the
        emitted samples of each row).  count: the outputs a signal of so many samples has (the resampler's is resampled_len)"""
        if len(windows) != len(n):
            raise ValueError(f"{len(windows)} windows for {len(n)} rows")
        win = (RowWindow * max(len(n), 1))()
        cnt = np.zeros(len(n), np.int64)
        for b, (in_origin, out_begin, out_count, last) in enumerate(windows):
            win[b] = RowWindow(int(in_origin), int(out_begin), int(out_count), 1 if last else 0, 0)
            cnt[b] = int(out_count) if out_count >= 0 else max(0, count(int(in_origin) + int(n[b])) - int(out_begin))
        cols = int(cnt.max()) if len(cnt) else 0
        return win, np.zeros((len(n), max(cols, Nmax)), np.int16 if pcm16 else np.float32), cnt

    @staticmethod
    def _flags(pcm16=False, device=False, no_sync=False):
        return (ZVX_PCM16 if pcm16 else 0) | (ZVX_DEVICE_IN | ZVX_DEVICE_OUT if device else 0) | (ZVX_NO_SYNC if no_sync else 0)

    # The effects as (symbol stem, a rate follows Nmax, the dtypes of the [B] result arrays behind out_stride)
    _LIMIT = ("limit", True, (np.float32, np.float32))
    _LEVEL = ("level", True, (np.float32, np.float32))
    _DENOISE = ("denoise", False, ())
    _WATERMARK = ("watermark", False, ())
    _FIR = ("fir", False, ())
    _NORMALIZE = ("normalize", True, (np.float64, np.float32, np.float32))       # (whole rows and in place only)

    def _effect(self, fx, mid, rows, lengths, *, rate=None, pcm16=False, window=None, windows=None, device=None, no_sync=False):
        """One call of the effect `fx` in one of its four forms: the whole rows (zvx_X); window = (in_origin, out_begin, out_count, last),
        one for all rows (zvx_X_ex); windows, one per row (zvx_X_rows); device = (ptr, Nmax), in place on device rows (zvx_X with
        ZVX_DEVICE_IN | ZVX_DEVICE_OUT [| ZVX_NO_SYNC]).  mid: the arguments between Nmax [, rate] and out (bias, params, keys).
        -> (out, *results): out [B][Nmax], out [B][cols], a list of each row's emitted samples, or None in place; no results with no_sync."""
        stem, takes_rate, res_dtypes = fx
        ptr, ptr_Nmax = device if device is not None else (None, None)
        xp, n, B, Nmax, _ = self._rows_arg(rows, lengths, ptr, ptr_Nmax)
        sym, tail, flags = "zvx_" + stem, (), self._flags(pcm16=pcm16, device=device is not None, no_sync=no_sync)
        if device is not None:
            out = None
        elif windows is not None:
            win, out, cnt = self._row_windows(windows, n, Nmax, pcm16)
            sym, tail = sym + "_rows", (win,)
        elif window is not None:
            out, cols = self._window_out(n, Nmax, *window[:3], pcm16)
            sym, tail = sym + "_ex", (int(window[0]), int(window[1]), int(window[2]), 1 if window[3] else 0)
        else:
            out = np.zeros((B, Nmax), np.int16 if pcm16 else np.float32)
        res = [None if no_sync else np.zeros(B, dt) for dt in res_dtypes]
        self._chk(getattr(self._lib, sym)(self._h, xp, _ptr(n), B, Nmax, *([self._rate(rate)] if takes_rate else []), *mid,
                                          xp if out is None else _ptr(out), Nmax if out is None else out.shape[1], *(_ptr(r) for r in res),
                                          flags, *tail))
        if windows is not None:
            out = [out[b, :cnt[b]] for b in range(B)]
        elif window is not None:
            out = out[:, :cols]
        return (out, *(r for r in res if r is not None))

    def _effect_in_place(self, fx, mid, ptr, lengths, Nmax, no_sync, rate=None):
        """_effect in place on device rows -> the effect's results; None where it has none or, with no_sync, has only queued"""
        results = self._effect(fx, mid, None, lengths, rate=rate, device=(ptr, Nmax), no_sync=no_sync)[1:]
        return results if results else None

    def trim_bounds(self, rows, frame=2048, hop=512, top_db=40.0, keep=0, lengths=None):
        """zvx_trim_bounds: per row the samples [begin, end) that join keeps (the decisions of mels.trim_silence, made on the device)
        -> (begin [B], end [B]) int32.  rows: a list of 1-D float waveforms, or a padded 2-D array + lengths."""
        x, n = self._rows(rows, lengths)
        B, Nmax = x.shape
        prm = JoinParams(int(frame), int(hop), float(top_db), int(keep), 0)
        begin, end = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._chk(self._lib.zvx_trim_bounds(self._h, _ptr(x), _ptr(n), B, Nmax, C.byref(prm), _ptr(begin), _ptr(end), 0))
        return begin, end

    def join(self, rows, gaps=None, *, frame=2048, hop=512, top_db=40.0, keep=0, fade=0, pcm16=False, lengths=None):
        """zvx_join on host rows: every row trimmed (top_db <= 0: not), faded over `fade` samples at both cuts and written with gaps[b]
        zeros behind it into ONE row -> (wav 1-D float32 / int16, seg_pos [B] int64, seg_begin [B], seg_len [B])."""
        x, n = self._rows(rows, lengths)
        return self._join(_ptr(x), n, x.shape[1], gaps, frame, hop, top_db, keep, fade, pcm16, 0)

    def join_device(self, ptr, lengths, Nmax, gaps=None, *, frame=2048, hop=512, top_db=40.0, keep=0, fade=0, pcm16=False,
                    out_device_ptr=None, out_capacity=None):
        """zvx_join on device rows [B][Nmax] f32 at `ptr` (ZVX_DEVICE_IN; they may be the output of a synthesize(..., no_sync=True) call
        queued just before: stream order is the fence).  Returns as join(); with out_device_ptr (ZVX_DEVICE_OUT, out_capacity samples)
        the row stays on the device and (out_len, seg_pos, seg_begin, seg_len) comes back."""
        n = _i32(lengths)
        return self._join(C.c_void_p(int(ptr)), n, int(Nmax), gaps, frame, hop, top_db, keep, fade, pcm16, ZVX_DEVICE_IN,
                          out_device_ptr, out_capacity)

    def _join(self, xptr, n, Nmax, gaps, frame, hop, top_db, keep, fade, pcm16, flags, out_device_ptr=None, out_capacity=None):
        B = len(n)
        g = _i32(gaps, (B,)) if gaps is not None else None
        prm = JoinParams(int(frame), int(hop), float(top_db), int(keep), int(fade))
        out_len = C.c_int64(0)
        pos, begin, ln = np.zeros(B, np.int64), np.zeros(B, np.int32), np.zeros(B, np.int32)
        flags |= ZVX_PCM16 if pcm16 else 0
        if out_device_ptr is not None:
            self._chk(self._lib.zvx_join(self._h, xptr, _ptr(n), B, Nmax, _ptr(g), C.byref(prm), C.c_void_p(int(out_device_ptr)), int(out_capacity),
                                         C.byref(out_len), _ptr(pos), _ptr(begin), _ptr(ln), flags | ZVX_DEVICE_OUT))
            return int(out_len.value), pos, begin, ln
        cap = int(n.astype(np.int64).sum()) + (int(g.astype(np.int64).sum()) if g is not None else 0)      # nothing trimmed: the most it can be
        out = np.empty(max(cap, 1), np.int16 if pcm16 else np.float32)
        self._chk(self._lib.zvx_join(self._h, xptr, _ptr(n), B, Nmax, _ptr(g), C.byref(prm), _ptr(out), cap, C.byref(out_len), _ptr(pos), _ptr(begin),
                                     _ptr(ln), flags))
        return out[:int(out_len.value)], pos, begin, ln

    def _rate(self, rate):
        return self.get_int("sampling_rate") if rate is None else int(rate)

    def loudness(self, rows, rate=None, lengths=None):
        """zvx_loudness: integrated loudness (BS.1770 / R128, LUFS; -inf where undefined) and sample peak of every row -> (lufs [B] float64,
        peak [B] float32).  rows: a list of 1-D float waveforms, or a padded 2-D array + lengths; rate None: the model's sampling rate."""
        x, n = self._rows(rows, lengths)
        B, Nmax = x.shape
        lufs, peak = np.zeros(B, np.float64), np.zeros(B, np.float32)
        self._chk(self._lib.zvx_loudness(self._h, _ptr(x), _ptr(n), B, Nmax, self._rate(rate), _ptr(lufs), _ptr(peak), 0))
        return lufs, peak

    def loudness_stats(self, rows, rate=None, lengths=None, curves=False):
        """zvx_loudness_stats: the programme loudness report of every row -> a dict of [B] float64 arrays: integrated (LUFS, bit for bit
        loudness()'s), max_momentary, max_short_term (LUFS; -inf where the row has no 400 ms block / 3 s window), lra (LU, EBU Tech 3342),
        lra_low, lra_high (LUFS: the 10th and 95th percentile of the gated short-term windows), short_gated (their number) and peak (linear
        sample peak).  curves: also momentary and short_term, lists of B float64 arrays: the LUFS curves at a 100 ms step, n / h - 3 and
        n / h - 29 entries.  rows: a list of 1-D float waveforms, or a padded 2-D array + lengths; rate None: the model's sampling rate."""
        return self._loudness_stats(self._rows_arg(rows, lengths), rate, curves)

    def loudness_stats_device(self, ptr, lengths, Nmax, rate=None, curves=False):
        """zvx_loudness_stats on device rows [B][Nmax] f32 at `ptr` (ZVX_DEVICE_IN; they may be the output of a synthesize / normalize_device /
        limit_device call queued just before: stream order is the fence) -> as loudness_stats()."""
        return self._loudness_stats(self._rows_arg(None, lengths, ptr, Nmax), rate, curves)

    def _loudness_stats(self, rows_arg, rate, curves, momentary=None, short_term=None):
        """rows_arg: what _rows_arg gives; momentary / short_term: [B][stride] float64 arrays of the caller's to receive the curves
        instead of fresh ones"""
        (xptr, n, B, Nmax, flags), rate = rows_arg, self._rate(rate)
        h = (rate + 5) // 10
        stats = np.zeros((B, ZVX_LS_COUNT), np.float64)
        if curves and momentary is None:
            momentary = np.full((B, max(1, Nmax // h - 3)), -np.inf, np.float64)
        if curves and short_term is None:
            short_term = np.full((B, max(1, Nmax // h - 3)), -np.inf, np.float64)
        stride = momentary.shape[1] if momentary is not None else short_term.shape[1] if short_term is not None else 0
        self._chk(self._lib.zvx_loudness_stats(self._h, xptr, _ptr(n), B, Nmax, rate, _ptr(stats), _ptr(momentary), _ptr(short_term), stride, flags))
        res = {k: stats[:, i].copy() for i, k in enumerate(LOUDNESS_STATS_KEYS)}
        if curves:
            U = n.astype(np.int64) // h
            res["momentary"] = [momentary[b, :max(U[b] - 3, 0)] for b in range(B)]
            res["short_term"] = [short_term[b, :max(U[b] - 29, 0)] for b in range(B)]
        return res

    def pitch(self, rows, rate=None, fmin=60.0, fmax=500.0, threshold=0.15, gate_db=-60.0, window=None, hop=None, lengths=None, curves=True):
        """zvx_pitch: the F0 track (YIN) of every row on a frame grid and its statistics -> a dict of [B] arrays: frames (int32), voiced
        (float64, like the rest: their counts), median, low, high (Hz: the 50th, 5th and 95th percentile of the voiced frames, nearest rank) and mean (Hz); all four
        are 0 where nothing is voiced.  curves: also f0 (Hz, 0 = unvoiced) and aper (d' at the pick: near 0 for a clean period, towards 1
        for noise), lists of B float32 arrays of each row's own frames.  fmin / fmax: the search range; threshold: YIN's absolute
        threshold on d'; gate_db: frames whose mean power is not above it are unvoiced.  window: samples integrated per lag (None: two
        periods of fmin); hop: samples between frames (None: the model's hop at the model's rate, otherwise 10 ms); frame f is centred on
        sample f * hop.  rows: a list of 1-D float waveforms, or a padded 2-D array + lengths; rate None: the model's sampling rate."""
        return self._pitch(self._rows_arg(rows, lengths), rate, fmin, fmax, threshold, gate_db, window, hop, curves)

    def pitch_device(self, ptr, lengths, Nmax, rate=None, fmin=60.0, fmax=500.0, threshold=0.15, gate_db=-60.0, window=None, hop=None, curves=True):
        """zvx_pitch on device rows [B][Nmax] f32 at `ptr` (ZVX_DEVICE_IN; stream order is the fence) -> as pitch()."""
        return self._pitch(self._rows_arg(None, lengths, ptr, Nmax), rate, fmin, fmax, threshold, gate_db, window, hop, curves)

    def _pitch(self, rows_arg, rate, fmin, fmax, threshold, gate_db, window, hop, curves):
        from . import pitch as _p
        (xptr, n, B, Nmax, flags), rate = rows_arg, self._rate(rate)
        if window is None:
            window = _p.default_window(rate, fmin) if float(fmin) > 0.0 and np.isfinite(fmin) else 2
        if hop is None:
            hop = _p.default_hop(rate, self.get_int("sampling_rate"), self.hop)
        prm = PitchParams(float(fmin), float(fmax), float(threshold), float(gate_db), int(window), int(hop))
        stats = np.zeros((B, ZVX_PS_COUNT), np.float64)
        fr = np.zeros(B, np.int32)
        stride = max(1, Nmax // max(int(hop), 1))
        f0 = np.zeros((B, stride), np.float32) if curves else None
        aper = np.zeros((B, stride), np.float32) if curves else None
        self._chk(self._lib.zvx_pitch(self._h, xptr, _ptr(n), B, Nmax, rate, C.byref(prm), _ptr(f0), _ptr(aper), stride, _ptr(fr), _ptr(stats), flags))
        res = {k: stats[:, i].copy() for i, k in enumerate(PITCH_STATS_KEYS)}
        res["frames"] = fr
        if curves:
            res["f0"] = [f0[b, :fr[b]] for b in range(B)]
            res["aper"] = [aper[b, :fr[b]] for b in range(B)]
        return res

    @staticmethod
    def _feature_rows(rows, lengths):
        """a list of [T][dim] arrays, or a padded [B][Tmax][dim] array + lengths -> (x [B][Tmax][dim] f32, T [B] i32)"""
        if lengths is None:
            rows = [np.asarray(r, np.float32) for r in rows]
            rows = [r.reshape(-1, 1) if r.ndim == 1 else r for r in rows]
            T = np.array([r.shape[0] for r in rows], np.int32)
            dim = rows[0].shape[1] if rows else 0
            if any(r.ndim != 2 or r.shape[1] != dim for r in rows):
                raise ValueError("feature rows must all be [T][dim] with one dim")
            x = np.zeros((len(rows), max(int(T.max()) if len(rows) else 0, 1), dim), np.float32)
            for b, r in enumerate(rows):
                x[b, :T[b]] = r
            return x, T
        x = np.ascontiguousarray(rows, np.float32)
        if x.ndim != 3:
            raise ValueError(f"padded feature rows of shape {x.shape} are not [B][Tmax][dim]")
        return x, _i32(lengths, (x.shape[0],))

    def dtw(self, a, b, lengths_a=None, lengths_b=None, path=True):
        """zvx_dtw: dynamic time warping of B pairs of feature sequences (lists of [T][dim] arrays, or padded [B][Tmax][dim] arrays +
        lengths) under the Euclidean local distance in double -> a dict: cost [B] float64, path_len [B] int32, a2b (a list of B int32
        arrays [Ta][2]: the first and last frame of b matched to each frame of a) and, with path, path (a list of B int32 arrays
        [path_len][2] of cells (i, j) from (0, 0) on)."""
        xa, Ta = self._feature_rows(a, lengths_a)
        xb, Tb = self._feature_rows(b, lengths_b)
        if xa.shape[0] != xb.shape[0] or xa.shape[2] != xb.shape[2]:
            raise ValueError(f"a {xa.shape} and b {xb.shape} do not pair up ([B][T][dim])")
        return self._dtw(_ptr(xa), Ta, xa.shape[1], _ptr(xb), Tb, xb.shape[1], xa.shape[2], path, 0)

    def dtw_device(self, a_ptr, lengths_a, Tamax, b_ptr, lengths_b, Tbmax, dim, path=True):
        """zvx_dtw on device rows [B][Tamax][dim] / [B][Tbmax][dim] f32 (ZVX_DEVICE_IN; stream order is the fence) -> as dtw()."""
        return self._dtw(C.c_void_p(int(a_ptr)), _i32(lengths_a), int(Tamax), C.c_void_p(int(b_ptr)), _i32(lengths_b), int(Tbmax), int(dim), path,
                         ZVX_DEVICE_IN)

    def _dtw(self, ap, Ta, Tamax, bp, Tb, Tbmax, dim, path, flags):
        B = len(Ta)
        if len(Tb) != B:
            raise ValueError(f"{B} lengths of a and {len(Tb)} of b")
        cost, plen = np.zeros(B, np.float64), np.zeros(B, np.int32)
        stride = max(1, int(np.max(Ta.astype(np.int64) + Tb) - 1)) if B else 1
        cells = np.zeros((B, stride, 2), np.int32) if path else None
        a2b = np.zeros((B, max(Tamax, 1), 2), np.int32)
        self._chk(self._lib.zvx_dtw(self._h, ap, _ptr(Ta), Tamax, bp, _ptr(Tb), Tbmax, B, dim, None, _ptr(cost), _ptr(plen), _ptr(cells), stride,
                                    _ptr(a2b), flags))
        res = {"cost": cost, "path_len": plen, "a2b": [a2b[b, :Ta[b]] for b in range(B)]}
        if path:
            res["path"] = [cells[b, :plen[b]] for b in range(B)]
        return res

    def align(self, rows_a, rows_b, n_cep=13, lengths_a=None, lengths_b=None, cepstra=False):
        """zvx_align_wav: two batches of waveforms at the model's rate (lists of 1-D arrays, or padded 2-D arrays + lengths) -> a dict:
        frames_a, frames_b, path_len (int32 [B]), cost, mcd_db (float64 [B]), path and a2b as dtw() gives them and, with cepstra, cep_a /
        cep_b (lists of float32 [frames][n_cep]).  mcd_db is the distortion between DCT cepstra of the model's own log-mel (c0 left out)
        averaged over the cells of the DTW path: not comparable with SPTK / WORLD figures, and no perceptual claim."""
        xa, na = self._rows(rows_a, lengths_a)
        xb, nb = self._rows(rows_b, lengths_b)
        B = xa.shape[0]
        if xb.shape[0] != B:
            raise ValueError(f"{B} rows of a and {xb.shape[0]} of b")
        n_fft, hop = self.get_int("fft_size"), self.hop
        pad = (n_fft - hop) // 2
        fmax = [max(1, 1 + (int(x.shape[1]) + 2 * pad - n_fft) // hop) for x in (xa, xb)]
        stride = fmax[0] + fmax[1]
        stats = np.zeros((B, ZVX_AL_COUNT), np.float64)
        cells, a2b = np.zeros((B, stride, 2), np.int32), np.zeros((B, fmax[0], 2), np.int32)
        cs = max(fmax)
        ca = np.zeros((B, cs, int(n_cep)), np.float32) if cepstra else None
        cb = np.zeros((B, cs, int(n_cep)), np.float32) if cepstra else None
        prm = AlignParams(int(n_cep))
        self._chk(self._lib.zvx_align_wav(self._h, _ptr(xa), _ptr(na), xa.shape[1], _ptr(xb), _ptr(nb), xb.shape[1], B, C.byref(prm), _ptr(stats),
                                          _ptr(cells), stride, _ptr(a2b), fmax[0], _ptr(ca), _ptr(cb), cs, 0))
        fa, fb, plen = (stats[:, k].astype(np.int32) for k in (ZVX_AL_FRAMES_A, ZVX_AL_FRAMES_B, ZVX_AL_PATH_LEN))
        res = {"frames_a": fa, "frames_b": fb, "path_len": plen, "cost": stats[:, ZVX_AL_COST].copy(), "mcd_db": stats[:, ZVX_AL_MCD_DB].copy(),
               "path": [cells[b, :plen[b]] for b in range(B)], "a2b": [a2b[b, :fa[b]] for b in range(B)]}
        if cepstra:
            res["cep_a"] = [ca[b, :fa[b]] for b in range(B)]
            res["cep_b"] = [cb[b, :fb[b]] for b in range(B)]
        return res

    def normalize(self, rows, target, *, peak_ceiling=0.891, max_gain_db=20.0, common=False, pcm16=False, rate=None, lengths=None):
        """zvx_normalize on host rows: every row (common: all rows as one programme, one gain) brought to `target` LUFS, the gain bounded by
        max_gain_db and by the linear sample-peak ceiling (<= 0: none) -> (rows_out [B][Nmax] float32 / int16 -- row b holds its samples
        times gain[b], then zeros --, lufs [B] float64, peak [B], gain [B] float32)."""
        return self._effect(self._NORMALIZE, self._normalize_mid(target, peak_ceiling, max_gain_db, common), rows, lengths, rate=rate, pcm16=pcm16)

    def normalize_device(self, ptr, lengths, Nmax, target, *, peak_ceiling=0.891, max_gain_db=20.0, common=False, rate=None, no_sync=False):
        """zvx_normalize IN PLACE on device rows [B][Nmax] f32 at `ptr` (they may be the output of a synthesize(..., no_sync=True) call queued
        just before: stream order is the fence) -> (lufs, peak, gain); with no_sync the call only queues and returns None."""
        return self._effect_in_place(self._NORMALIZE, self._normalize_mid(target, peak_ceiling, max_gain_db, common), ptr, lengths, Nmax, no_sync, rate)

    @staticmethod
    def _normalize_mid(target, peak_ceiling, max_gain_db, common):
        return (C.byref(LoudnessParams(float(target), float(peak_ceiling), float(max_gain_db), ZVX_LOUD_COMMON if common else ZVX_LOUD_PER_ROW)),)

    def true_peak(self, rows, oversample=4, rate=None, lengths=None):
        """zvx_true_peak: per row max(max |x|, max |y|), y the row oversampled `oversample` (1, 2, 4, 8) times by zvx_resample's filter
        -> [B] float32.  rows: a list of 1-D float waveforms, or a padded 2-D array + lengths; rate None: the model's sampling rate."""
        return self._true_peak(self._rows_arg(rows, lengths), oversample, rate)

    def true_peak_device(self, ptr, lengths, Nmax, oversample=4, rate=None):
        """zvx_true_peak on device rows [B][Nmax] f32 at `ptr` (ZVX_DEVICE_IN; stream order is the fence) -> [B] float32"""
        return self._true_peak(self._rows_arg(None, lengths, ptr, Nmax), oversample, rate)

    def _true_peak(self, rows_arg, oversample, rate):
        xptr, n, B, Nmax, flags = rows_arg
        tp = np.zeros(B, np.float32)
        self._chk(self._lib.zvx_true_peak(self._h, xptr, _ptr(n), B, Nmax, self._rate(rate), int(oversample), _ptr(tp), flags))
        return tp

    def limit(self, rows, ceiling, window_ms=5.0, oversample=4, pcm16=False, rate=None, lengths=None):
        """zvx_limit on host rows: a look-ahead limiter that leaves no sample above the linear `ceiling`, its gain smoothed over
        window_ms on either side and driven by the `oversample`-times oversampled envelope -> (rows_out [B][Nmax] float32 / int16 -- row
        b holds its limited samples, then zeros --, peak_in [B] float32: the envelope's maximum, min_gain [B] float32)."""
        return self._effect(self._LIMIT, self._limit_mid(ceiling, window_ms, oversample), rows, lengths, rate=rate, pcm16=pcm16)

    @staticmethod
    def _limit_mid(ceiling, window_ms, oversample):
        return (C.byref(LimitParams(float(ceiling), float(window_ms), int(oversample))),)

    def limit_window(self, rows, ceiling, window_ms=5.0, oversample=4, in_origin=0, out_begin=0, out_count=-1, last=True, pcm16=False,
                     rate=None, lengths=None):
        """zvx_limit_ex on host rows: the rows hold samples [in_origin, in_origin + len) of signals that start at sample 0 and, with
        `last`, end with the row; the outputs [out_begin, out_begin + out_count) of the whole-signal limiter (out_count -1, which needs
        last: to the end of each row's signal) -> (out [B][n] float32 / int16 -- row b holds its emitted samples, then zeros --,
        peak_in [B], min_gain [B] float32, both over the emitted samples only).  The window must carry limiter.reach(W, oversample)
        samples of support on either side of the outputs, except at the signal's own ends (include/zvx.h)."""
        return self._effect(self._LIMIT, self._limit_mid(ceiling, window_ms, oversample), rows, lengths, rate=rate, pcm16=pcm16,
                            window=(in_origin, out_begin, out_count, last))

    def limit_device(self, ptr, lengths, Nmax, ceiling, *, window_ms=5.0, oversample=4, rate=None, no_sync=False):
        """zvx_limit IN PLACE on device rows [B][Nmax] f32 at `ptr` (they may be the output of a synthesize / normalize_device call queued
        just before: stream order is the fence) -> (peak_in, min_gain); with no_sync the call only queues and returns None."""
        return self._effect_in_place(self._LIMIT, self._limit_mid(ceiling, window_ms, oversample), ptr, lengths, Nmax, no_sync, rate)

    def denoise_bias(self):
        """zvx_denoise_bias: the magnitude spectrum of what the context's vocoder emits for 88 silent mel frames, the mean over the STFT
        frames -> [fft_size / 2 + 1] float32.  Recompute it after a switch that changes the vocoder's arithmetic."""
        bias = np.zeros(self.get_int("fft_size") // 2 + 1, np.float32)
        self._chk(self._lib.zvx_denoise_bias(self._h, _ptr(bias)))
        return bias

    def _denoise_bias_arg(self, bias):
        bias = _f32(bias).reshape(-1)
        nf = self.get_int("fft_size") // 2 + 1
        if bias.shape[0] != nf:
            raise ValueError(f"denoise: bias has {bias.shape[0]} entries, the model's STFT has {nf} bins")
        return bias

    def _denoise_mid(self, bias, strength, floor):
        return _ptr(self._denoise_bias_arg(bias)), C.byref(DenoiseParams(float(strength), float(floor)))

    def denoise(self, rows, bias, strength, floor=0.0, pcm16=False, lengths=None):
        """zvx_denoise on host rows: strength * bias[k] is taken off the magnitude of every STFT bin of every frame (never below floor
        times the magnitude), the phase kept, and the frames are overlap-added back -> rows_out [B][Nmax] float32 / int16 -- row b holds
        its denoised samples, then zeros.  rows: a list of 1-D float waveforms, or a padded 2-D array + lengths, at the model's rate."""
        return self._effect(self._DENOISE, self._denoise_mid(bias, strength, floor), rows, lengths, pcm16=pcm16)[0]

    def denoise_window(self, rows, bias, strength, floor=0.0, in_origin=0, out_begin=0, out_count=-1, last=True, pcm16=False, lengths=None):
        """zvx_denoise_ex on host rows: the rows hold samples [in_origin, in_origin + len) of signals that start at sample 0 and, with
        `last`, end with the row; the outputs [out_begin, out_begin + out_count) of the whole-signal denoiser (out_count -1, which needs
        last: to the end of each row's signal) -> out [B][n] float32 / int16 -- row b holds its emitted samples, then zeros.  The window
        must carry denoiser.reach(fft_size) = fft_size - 1 samples of support on either side of the outputs, except at the signal's own
        ends (include/zvx.h)."""
        return self._effect(self._DENOISE, self._denoise_mid(bias, strength, floor), rows, lengths, pcm16=pcm16,
                            window=(in_origin, out_begin, out_count, last))[0]

    def denoise_rows(self, rows, bias, strength, windows, floor=0.0, pcm16=False, lengths=None):
        """zvx_denoise_rows on host rows: denoise_window with a window per row -- windows[b] = (in_origin, out_begin, out_count, last) says
        which samples of its signal row b holds and which outputs of the whole-signal denoiser it emits -> a list of B arrays, row b's
        emitted samples (float32 / int16), bit for bit those of denoise_window on that row alone."""
        return self._effect(self._DENOISE, self._denoise_mid(bias, strength, floor), rows, lengths, pcm16=pcm16, windows=windows)[0]

    def limit_rows(self, rows, ceiling, windows, window_ms=5.0, oversample=4, pcm16=False, rate=None, lengths=None):
        """zvx_limit_rows on host rows: limit_window with a window per row (windows[b] = (in_origin, out_begin, out_count, last)) -> (a list
        of B arrays, row b's emitted samples, peak_in [B], min_gain [B] float32, both over each row's emitted samples only), bit for bit
        what limit_window gives on each row alone."""
        return self._effect(self._LIMIT, self._limit_mid(ceiling, window_ms, oversample), rows, lengths, rate=rate, pcm16=pcm16, windows=windows)

    @staticmethod
    def _level_mid(target, max_gain_db, window_ms, lookahead_ms):
        return (C.byref(LevelParams(float(target), float(max_gain_db), float(window_ms), float(lookahead_ms))),)

    def level(self, rows, target, max_gain_db=20.0, window_ms=3000.0, lookahead_ms=100.0, pcm16=False, rate=None, lengths=None):
        """zvx_level on host rows: a gain curve that steers the gated short-term loudness of the last window_ms towards `target` LUFS,
        looking lookahead_ms ahead and never above max_gain_db (an AGC, not R128 normalisation; zerovox_amd.leveler) -> (rows_out
        [B][Nmax] float32 / int16 -- row b holds its levelled samples, then zeros --, gain_lo [B], gain_hi [B] float32: the smallest and
        the largest gain applied)."""
        return self._effect(self._LEVEL, self._level_mid(target, max_gain_db, window_ms, lookahead_ms), rows, lengths, rate=rate, pcm16=pcm16)

    def level_window(self, rows, target, max_gain_db=20.0, window_ms=3000.0, lookahead_ms=100.0, in_origin=0, out_begin=0, out_count=-1,
                     last=True, pcm16=False, rate=None, lengths=None):
        """zvx_level_ex on host rows: the rows hold samples [in_origin, in_origin + len) of signals that start at sample 0 and, with
        `last`, end with the row; the outputs [out_begin, out_begin + out_count) of the whole-signal leveler (out_count -1, which needs
        last: to the end of each row's signal) -> (out [B][n] float32 / int16, gain_lo [B], gain_hi [B] float32, both over the emitted
        samples only).  The window must carry leveler.reach(rate, window_ms, lookahead_ms) = (RL, RR) samples of support to the left and
        to the right of the outputs, except at the signal's own ends (include/zvx.h)."""
        return self._effect(self._LEVEL, self._level_mid(target, max_gain_db, window_ms, lookahead_ms), rows, lengths, rate=rate, pcm16=pcm16,
                            window=(in_origin, out_begin, out_count, last))

    def level_rows(self, rows, windows, target, max_gain_db=20.0, window_ms=3000.0, lookahead_ms=100.0, pcm16=False, rate=None, lengths=None):
        """zvx_level_rows on host rows: level_window with a window per row (windows[b] = (in_origin, out_begin, out_count, last)) -> (a list
        of B arrays, row b's emitted samples, gain_lo [B], gain_hi [B] float32, both over each row's emitted samples only), bit for bit
        what level_window gives on each row alone."""
        return self._effect(self._LEVEL, self._level_mid(target, max_gain_db, window_ms, lookahead_ms), rows, lengths, rate=rate, pcm16=pcm16,
                            windows=windows)

    @staticmethod
    def _fir_mid(taps, delay):
        """the arguments between Nmax and out: the taps (a host array, float32), their number and the delay (None: (K - 1) // 2, which
        time-aligns a symmetric filter)"""
        taps = _f32(taps).reshape(-1)
        K = int(taps.shape[0])
        return _ptr(taps), K, (K - 1) // 2 if delay is None else int(delay)

    def fir(self, rows, taps, delay=None, pcm16=False, lengths=None):
        """zvx_fir on host rows: y[i] = sum_k taps[k] x[i + delay - k], zeros outside the row, accumulated in double in ascending k and
        rounded once (include/zvx.h) -> rows_out [B][Nmax] float32 / int16 -- row b holds its filtered samples, then zeros.  rows: a list
        of 1-D float waveforms, or a padded 2-D array + lengths.  delay None: (K - 1) // 2.  zerovox_amd.equaliser designs taps."""
        return self._effect(self._FIR, self._fir_mid(taps, delay), rows, lengths, pcm16=pcm16)[0]

    def fir_window(self, rows, taps, delay=None, in_origin=0, out_begin=0, out_count=-1, last=True, pcm16=False, lengths=None):
        """zvx_fir_ex on host rows: the rows hold samples [in_origin, in_origin + len) of signals that start at sample 0 and, with `last`,
        end with the row; the outputs [out_begin, out_begin + out_count) of the whole-signal filter (out_count -1, which needs last: to
        the end of each row's signal) -> out [B][n] float32 / int16.  The window must carry equaliser.reach(K, delay) = (K - 1 - delay,
        delay) samples of support to the left and to the right of the outputs, except at the signal's own ends (include/zvx.h)."""
        return self._effect(self._FIR, self._fir_mid(taps, delay), rows, lengths, pcm16=pcm16, window=(in_origin, out_begin, out_count, last))[0]

    def fir_rows(self, rows, taps, windows, delay=None, pcm16=False, lengths=None):
        """zvx_fir_rows on host rows: fir_window with a window per row (windows[b] = (in_origin, out_begin, out_count, last)) -> a list of
        B arrays, row b's emitted samples (float32 / int16), bit for bit those of fir_window on that row alone.  One filter per call."""
        return self._effect(self._FIR, self._fir_mid(taps, delay), rows, lengths, pcm16=pcm16, windows=windows)[0]

    def fir_device(self, ptr, lengths, Nmax, taps, delay=None, *, no_sync=False):
        """zvx_fir IN PLACE on device rows [B][Nmax] f32 at `ptr` (the filter writes a work buffer of the context and copies back; the
        bits are the out-of-place call's); with no_sync the call only queues.  taps is a host array and may be reused at once."""
        self._effect_in_place(self._FIR, self._fir_mid(taps, delay), ptr, lengths, Nmax, no_sync)

    def resample_rows(self, rows, rate_in, rate_out, windows, pcm16=False, lengths=None):
        """zvx_resample_rows on host rows: resample_window with a window per row -- windows[b] = (in_origin, out_begin, out_count) or
        (in_origin, out_begin, out_count, last); row b holds samples [in_origin, in_origin + len) of a signal that is zero elsewhere ->
        (a list of B arrays, row b's emitted samples (float32 / int16), bit for bit those of resample_window on that row alone,
        out_len [B])."""
        xp, n, B, Nmax, _ = self._rows_arg(rows, lengths)
        windows = [tuple(w[:3]) + (len(w) > 3 and w[3],) for w in windows]
        win, out, _ = self._row_windows(windows, n, 1, pcm16, lambda end: resampled_len(end, rate_in, rate_out))
        out_len = np.zeros(B, np.int32)
        self._chk(self._lib.zvx_resample_rows(self._h, xp, _ptr(n), B, Nmax, int(rate_in), int(rate_out), _ptr(out), out.shape[1], _ptr(out_len),
                                              ZVX_PCM16 if pcm16 else 0, win))
        return [out[b, :out_len[b]] for b in range(B)], out_len

    def denoise_device(self, ptr, lengths, Nmax, bias, strength, *, floor=0.0, no_sync=False):
        """zvx_denoise IN PLACE on device rows [B][Nmax] f32 at `ptr` (they may be the output of a synthesize / vocode_device call queued
        just before: stream order is the fence); with no_sync the call only queues.  bias is a host array and may be reused at once."""
        self._effect_in_place(self._DENOISE, self._denoise_mid(bias, strength, floor), ptr, lengths, Nmax, no_sync)

    @staticmethod
    def _watermark_params(key, depth_db=1.0, lo_hz=250.0, hi_hz=8000.0, block_frames=8, band_bins=4, period_blocks=64):
        return WatermarkParams(int(key) & 0xFFFFFFFFFFFFFFFF, float(depth_db), float(lo_hz), float(hi_hz), int(block_frames), int(band_bins),
                               int(period_blocks), 0)

    def watermark(self, rows, key, *, pcm16=False, lengths=None, **params):
        """zvx_watermark on host rows: the keyed mark of zerovox_amd.watermark laid on every row (params: depth_db, lo_hz, hi_hz,
        block_frames, band_bins, period_blocks; the defaults are watermark.EMBED_DEFAULTS) -> rows_out [B][Nmax] float32 / int16 -- row b
        holds its marked samples, then zeros.  rows: a list of 1-D float waveforms, or a padded 2-D array + lengths, at the model's rate."""
        return self._effect(self._WATERMARK, (C.byref(self._watermark_params(key, **params)),), rows, lengths, pcm16=pcm16)[0]

    def watermark_window(self, rows, key, *, in_origin=0, out_begin=0, out_count=-1, last=True, pcm16=False, lengths=None, **params):
        """zvx_watermark_ex on host rows: the rows hold samples [in_origin, in_origin + len) of signals that start at sample 0 and, with
        `last`, end with the row; the outputs [out_begin, out_begin + out_count) of the whole-signal call (out_count -1, which needs
        last: to the end of each row's signal) -> out [B][n] float32 / int16.  The window must carry watermark.reach(fft_size) =
        fft_size - 1 samples of support on either side of the outputs, except at the signal's own ends (include/zvx.h)."""
        return self._effect(self._WATERMARK, (C.byref(self._watermark_params(key, **params)),), rows, lengths, pcm16=pcm16,
                            window=(in_origin, out_begin, out_count, last))[0]

    def watermark_device(self, ptr, lengths, Nmax, key, *, no_sync=False, **params):
        """zvx_watermark IN PLACE on device rows [B][Nmax] f32 at `ptr` (they may be the output of a call queued just before: stream
        order is the fence); with no_sync the call only queues."""
        self._effect_in_place(self._WATERMARK, (C.byref(self._watermark_params(key, **params)),), ptr, lengths, Nmax, no_sync)

    def watermark_detect(self, rows, key, *, window_frames=256, threshold=None, lengths=None, device_ptr=None, Nmax=None, **params):
        """zvx_watermark_detect: per row the best score over every window of window_frames frames (0: the row) and every offset, with the
        key's pattern (params: lo_hz, hi_hz, block_frames, band_bins, period_blocks as embedded; hi_hz may be lower) -> a list of B
        watermark.WatermarkResult.  rows: a list of 1-D float waveforms, or a padded 2-D array + lengths, at the model's rate; or, with
        device_ptr, device rows [B][Nmax] f32 there and `lengths`."""
        from . import watermark as wm
        xp, n, B, Nmax, flags = self._rows_arg(rows, lengths, device_ptr, Nmax)
        params.pop("depth_db", None)
        prm = self._watermark_params(key, **params)
        fft, hop, wf = self.get_int("fft_size"), self.hop, int(window_frames)
        pad = (fft - hop) // 2
        F = max(0, 1 + (Nmax + 2 * pad - fft) // hop)
        nw = 1 if wf < 2 or F <= wf else 1 + -(-(F - wf) // (wf // 2))
        score, off, win = np.zeros(B, np.float32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        ws, wo = np.zeros((B, nw), np.float32), np.zeros((B, nw), np.int32)
        self._chk(self._lib.zvx_watermark_detect(self._h, xp, _ptr(n), B, Nmax, C.byref(prm), wf, _ptr(score), _ptr(off), _ptr(win),
                                                 _ptr(ws), _ptr(wo), nw, flags))
        thr = wm.THRESHOLD if threshold is None else float(threshold)
        res = []
        for b in range(B):
            Fb = max(0, 1 + (int(n[b]) + 2 * pad - fft) // hop) if n[b] > 0 else 0
            k = 0 if Fb <= 0 else (1 if wf < 2 or Fb <= wf else 1 + -(-(Fb - wf) // (wf // 2)))
            res.append(wm.WatermarkResult(float(score[b]), int(off[b]), int(win[b]), bool(score[b] >= thr), thr,
                                          [(float(ws[b, w]), int(wo[b, w])) for w in range(k)]))
        return res

    @staticmethod
    def _keys_arg(keys):
        """ints in [0, 2^64) -> a contiguous uint64 array"""
        ks = [int(k) for k in keys]
        if any(k < 0 or k > 0xFFFFFFFFFFFFFFFF for k in ks):
            raise ValueError("watermark: every key must lie in [0, 2^64)")
        return np.array(ks, np.uint64)

    def watermark_rows(self, rows, keys, windows=None, pcm16=False, lengths=None, **params):
        """zvx_watermark_rows on host rows: watermark_window with a window AND a key per row, in one call -- keys[b] is row b's key (None:
        params['key'] for every row), windows[b] = (in_origin, out_begin, out_count, last) says which samples of its signal row b holds
        and which outputs of the whole-signal call it emits (None: every row whole) -> a list of B arrays, row b's emitted samples
        (float32 / int16), bit for bit those of watermark_window on that row alone with its key."""
        B = len(rows)
        if windows is None:
            windows = [(0, 0, -1, True)] * B
        if keys is None:
            kp, key0 = None, params.pop("key")
        else:
            ka = self._keys_arg(keys)
            if len(ka) != B:
                raise ValueError(f"{len(ka)} keys for {B} rows")
            params.pop("key", None)
            kp, key0 = _ptr(ka), 0
        return self._effect(self._WATERMARK, (C.byref(self._watermark_params(key0, **params)), kp), rows, lengths, pcm16=pcm16, windows=windows)[0]

    def watermark_identify(self, rows, keys, *, window_frames=256, threshold=None, lengths=None, device_ptr=None, Nmax=None, **params):
        """zvx_watermark_identify: which of the candidate `keys` marked each row -- one analysis and one search launch for all K keys, each
        key's score bit for bit watermark_detect's (params: lo_hz, hi_hz, block_frames, band_bins, period_blocks as embedded; hi_hz may be
        lower) -> a list of B watermark.IdentifyResult.  rows as watermark_detect's.  The largest score of WRONG keys grows with their
        number: watermark.THRESHOLD was measured over 256 of them, so with many more candidates judge by `margin` as well."""
        from . import watermark as wm
        xp, n, B, Nmax, flags = self._rows_arg(rows, lengths, device_ptr, Nmax)
        ka = self._keys_arg(keys)
        K = len(ka)
        params.pop("depth_db", None)
        params.pop("key", None)
        prm = self._watermark_params(0, **params)
        score, off, win = np.zeros((B, max(K, 1)), np.float32), np.zeros((B, max(K, 1)), np.int32), np.zeros((B, max(K, 1)), np.int32)
        best = np.zeros(B, np.int32)
        self._chk(self._lib.zvx_watermark_identify(self._h, xp, _ptr(n), B, Nmax, C.byref(prm), _ptr(ka), K, int(window_frames), _ptr(score),
                                                   _ptr(off), _ptr(win), _ptr(best), flags))
        return [wm.identify_result(ka, score[b], off[b], win[b], int(best[b]), threshold) for b in range(B)]

    def stream_open(self, mel=None, frames=0, *, chunk_frames, chunks_per_call=1, halo=16, denoise=None, bias=None, limit=None, flags=0,
                    level=None, watermark=None):
        """zvx_stream_open -> Stream.  mel: [frames, n_mels] float32 on the host; an int, a device pointer to ``frames`` rows
        (ZVX_DEVICE_IN); or None: the mel the context holds after decode (frames 0).  denoise: None or dict(strength, floor) with ``bias``
        (denoise_bias()); limit: None or dict(ceiling, window_ms, oversample).  The context's out_rate at this moment is the stream's.
        level: None or level_window's keywords (target, and optionally max_gain_db, window_ms, lookahead_ms); watermark: None or a
        watermark.params(...) dict (``key`` is this session's key).  With either the session is opened by zvx_stream_open_ex and runs
        denoise -> level -> watermark -> limit -> rate conversion; with neither this is zvx_stream_open as before."""
        keep = []
        if mel is None:
            mptr = None
        elif isinstance(mel, (int, np.integer)):
            mptr, flags = C.c_void_p(int(mel)), flags | ZVX_DEVICE_IN
        else:
            mel = _f32(mel)
            if mel.ndim != 2 or mel.shape[1] != self.n_mels:
                raise ValueError(f"stream_open: mel must be [frames, {self.n_mels}], not {mel.shape}")
            frames, mptr = mel.shape[0], _ptr(mel)
        prm = StreamParams(int(chunk_frames), int(chunks_per_call), int(halo), None, None, None)
        if denoise is not None:
            dn = DenoiseParams(float(denoise["strength"]), float(denoise.get("floor", 0.0)))
            keep.append(dn)
            prm.denoise = C.pointer(dn)
        if bias is not None:
            b = self._denoise_bias_arg(bias)
            keep.append(b)
            prm.denoise_bias = b.ctypes.data
        if limit is not None:
            lm = LimitParams(float(limit["ceiling"]), float(limit.get("window_ms", 5.0)), int(limit.get("oversample", 4)))
            keep.append(lm)
            prm.limit = C.pointer(lm)
        h = C.c_void_p()
        if level is None and watermark is None:
            self._chk(self._lib.zvx_stream_open(self._h, mptr, int(frames), C.byref(prm), int(flags), C.byref(h)))
            return Stream(self, h, keep)
        more = StreamStages()
        if level is not None:
            level = dict(level)
            lv = LevelParams(float(level.pop("target")), float(level.pop("max_gain_db", 20.0)), float(level.pop("window_ms", 3000.0)),
                             float(level.pop("lookahead_ms", 100.0)))
            if level:
                raise TypeError(f"stream_open: unknown level keywords {sorted(level)}")
            keep.append(lv)
            more.level = C.pointer(lv)
        if watermark is not None:
            wm = self._watermark_params(**watermark)
            keep.append(wm)
            more.watermark = C.pointer(wm)
        self._chk(self._lib.zvx_stream_open_ex(self._h, mptr, int(frames), C.byref(prm), C.byref(more), int(flags), C.byref(h)))
        return Stream(self, h, keep)

    def stream_next_many(self, streams, capacities=None):
        """one zvx_stream_next_many into host memory: every session of ``streams`` (open sessions of this context) advances by one piece,
        their groups vocoded as one batch -> the pieces in order (np.float32, possibly empty), each what the session's own next_piece()
        would have returned; sets each Stream.done.  capacities: samples per buffer (None: each session's max_piece); one too small raises
        ZvxError(ZVX_E_BUFFER) with nothing consumed in any session.  A ZvxError carries ``n_out`` as a list."""
        streams = list(streams)
        caps = [s.info()["max_piece"] for s in streams] if capacities is None else [int(v) for v in capacities]
        if len(caps) != len(streams):
            raise ValueError(f"stream_next_many: {len(caps)} capacities for {len(streams)} streams")
        bufs = [np.empty(max(v, 1), np.float32) for v in caps]
        n = self._stream_next_many(streams, [b.ctypes.data for b in bufs], caps, 0)
        return [b[:k] for b, k in zip(bufs, n)]

    def stream_next_many_device(self, streams, ptrs, capacities, no_sync=False):
        """one zvx_stream_next_many into device memory at ``ptrs`` (ZVX_DEVICE_OUT; with no_sync the call only queues) -> samples written
        per session"""
        streams, ptrs, caps = list(streams), [int(p) for p in ptrs], [int(v) for v in capacities]
        if not len(streams) == len(ptrs) == len(caps):
            raise ValueError(f"stream_next_many_device: {len(streams)} streams, {len(ptrs)} pointers, {len(caps)} capacities")
        return self._stream_next_many(streams, ptrs, caps, ZVX_DEVICE_OUT | (ZVX_NO_SYNC if no_sync else 0))

    def _stream_next_many(self, streams, ptrs, caps, flags):
        k = len(streams)
        hs = (C.c_void_p * max(k, 1))(*[s._h for s in streams])
        out = (C.c_void_p * max(k, 1))(*ptrs)
        cap = (C.c_int64 * max(k, 1))(*caps)
        n = (C.c_int64 * max(k, 1))(*([-1] * k))
        done = (C.c_int32 * max(k, 1))()
        rc = self._lib.zvx_stream_next_many(hs, k, out, cap, n, done, flags)
        if rc != ZVX_OK:
            e = ZvxError(rc, self._lib.zvx_last_error(self._h).decode())
            e.n_out = [int(v) for v in n[:k]]
            raise e
        for s, d in zip(streams, done):
            s.done = bool(d)
        return [int(v) for v in n[:k]]

    def resample_device(self, ptr, n, rate_in, rate_out, pcm16=False):
        """zvx_resample of ONE device-resident row of n f32 samples (ZVX_DEVICE_IN) -> host row at rate_out"""
        cols = resampled_len(int(n), rate_in, rate_out)
        out = np.empty(max(cols, 1), np.int16 if pcm16 else np.float32)
        nn = np.array([int(n)], np.int32)
        self._chk(self._lib.zvx_resample(self._h, C.c_void_p(int(ptr)), _ptr(nn), 1, max(int(n), 1), int(rate_in), int(rate_out), _ptr(out), max(cols, 1),
                                         None, ZVX_DEVICE_IN | (ZVX_PCM16 if pcm16 else 0)))
        return out[:cols]

    def _prosody(self, prosody, B, Tmax):
        """-> (struct, keep-alive) for the _ex entry points, or (None, None): the plain ones run."""
        from .prosody import resolve
        p = resolve(prosody, B, Tmax)
        return (None, None) if p is None else (p.struct(), p)

    def encode(self, phoneme, puncts, T, spk, duration=None, prosody=None):
        """prosody: None, a prosody.Prosody or a dict of Prosody.create keywords (zvx_encode_ex)."""
        phoneme = _i32(phoneme)
        B, Tmax = phoneme.shape
        puncts = _i32(puncts, (B, Tmax))
        T = _i32(T, (B,))
        spk = _f32(spk).reshape(B, self.hidden)
        dur = _i32(duration, (B, Tmax)) if duration is not None else None
        mel_len = np.zeros(B, np.int32)
        logd = np.zeros((B, Tmax), np.float32)
        pitch = np.zeros((B, Tmax), np.float32)
        energy = np.zeros((B, Tmax), np.float32)
        ps, _keep = self._prosody(prosody, B, Tmax)
        args = (self._h, _ptr(phoneme), _ptr(puncts), _ptr(dur), _ptr(T), B, Tmax, _ptr(spk), _ptr(mel_len), _ptr(logd), _ptr(pitch), _ptr(energy))
        self._chk(self._lib.zvx_encode(*args) if ps is None else self._lib.zvx_encode_ex(*args, C.byref(ps)))
        return mel_len, logd, pitch, energy

    def decode(self, B, Lmax):
        # the library writes rows [0, ctx Lmax) of every utterance; a larger (or degenerate) request keeps zeros in the rest
        mel = np.zeros((B, max(Lmax, 1), self.n_mels), np.float32)
        self._chk(self._lib.zvx_decode(self._h, _ptr(mel), max(Lmax, 1), 0))
        return mel

    def decode_features(self, features, L, spk):
        features = _f32(features)
        B, Lmax, H = features.shape
        assert H == self.hidden
        L = _i32(L, (B,))
        spk = _f32(spk).reshape(B, H)
        mel = np.empty((B, Lmax, self.n_mels), np.float32)
        self._chk(self._lib.zvx_decode_features(self._h, _ptr(features), _ptr(L), B, Lmax, _ptr(spk), _ptr(mel), Lmax))
        return mel

    def out_samples(self, n_native, native_rate=False):
        """samples a waveform call hands back for n_native generator samples: the same at the model's rate (out_rate 0 or native_rate),
        else resampled_len to the context's out_rate"""
        rate = 0 if native_rate else self.get_int("out_rate")
        return int(n_native) if not rate else resampled_len(n_native, self.get_int("sampling_rate"), rate)

    def vocode(self, B, mel_len, pad_to=None, pcm16=False, native_rate=False):
        """wav [B][max(mel_len)*hop]: float32, or int16 PCM (x32760, truncated) with pcm16.  The array is created with
        np.empty on purpose: the library owns every byte it hands back (valid samples, then zeros).  Under an output rate
        (set_int("out_rate", hz)) the rows are out_samples(mel_len*hop) long; native_rate=True (ZVX_NATIVE_RATE) ignores it."""
        n0 = self.out_samples(int(np.max(mel_len)) * self.hop, native_rate)
        n = max(n0, 1)
        wav = (np.empty if n0 > 0 else np.zeros)((B, n), np.int16 if pcm16 else np.float32)    # all lengths 0: nothing is copied back
        pt = _i32(pad_to, (B,)) if pad_to is not None else None
        self._chk(self._lib.zvx_vocode(self._h, _ptr(pt), _ptr(wav), n, (ZVX_PCM16 if pcm16 else 0) | (ZVX_NATIVE_RATE if native_rate else 0)))
        return wav

    def vocode_device(self, mel_len, pad_to, wav_ptr, wav_stride, native_rate=False, no_sync=False):
        """zvx_vocode into device rows [B][wav_stride] f32 at wav_ptr (ZVX_DEVICE_OUT); with no_sync the call only queues"""
        B = len(mel_len)
        pt = _i32(pad_to, (B,)) if pad_to is not None else None
        self._chk(self._lib.zvx_vocode(self._h, _ptr(pt), C.c_void_p(int(wav_ptr)), int(wav_stride),
                                       ZVX_DEVICE_OUT | (ZVX_NO_SYNC if no_sync else 0) | (ZVX_NATIVE_RATE if native_rate else 0)))

    def vocode_mel(self, mel, P, pcm16=False, host_async=False, native_rate=False):
        """host_async: the call only queues work and returns the pinned host slot (wait_host(slot) hands out the rows).
        Rows are in samples of the context's out_rate unless native_rate (ZVX_NATIVE_RATE)."""
        fl = (ZVX_PCM16 if pcm16 else 0) | (ZVX_NATIVE_RATE if native_rate else 0)
        mel = _f32(mel)
        B, Pmax, nm = mel.shape
        assert nm == self.n_mels
        P = _i32(P, (B,))
        if host_async:
            self._chk(self._lib.zvx_vocode_mel(self._h, _ptr(mel), _ptr(P), B, Pmax, None, 0, ZVX_HOST_ASYNC | fl))
            return self.get_int("host_slot")
        n = self.out_samples(int(P.max()) * self.hop, native_rate)
        wav = np.empty((B, n), np.int16 if pcm16 else np.float32)
        self._chk(self._lib.zvx_vocode_mel(self._h, _ptr(mel), _ptr(P), B, Pmax, _ptr(wav), n, fl))
        nfull = self.out_samples(Pmax * self.hop, native_rate)
        if n < nfull:                                                # callers index rows up to Pmax*hop (in output samples)
            wav = np.concatenate([wav, np.zeros((B, nfull - n), wav.dtype)], axis=1)
        return wav

    def synthesize(self, phoneme, puncts, T, spk, duration=None, pad_to=None, want_mel=True, Lmax_cap=0,
                   wav_device_ptr=None, wav_stride=None, no_sync=False, pcm16=False, mel_device_ptr=None, host_async=False, prosody=None,
                   native_rate=False):
        """Batched phoneme -> waveform.  Returns dict(wav [B][N] (None if device output), mel_len, mel, log_duration).
        host_async: the call only queues work and returns dict(..., slot=s); wait_host(s) hands out the waveform rows in the
        context's pinned host memory (ZVX_HOST_ASYNC: forced durations, no mel / log-duration output).
        spk: [B][hidden] floats, or an int: a device pointer to them (ZVX_DEVICE_SPK, e.g. what spkemb_wav_device wrote; the copy is
        ordered behind everything queued so far on the context).
        With a device waveform (wav_device_ptr) the mel, if wanted, is a device buffer too (ZVX_DEVICE_OUT covers both outputs):
        mel_device_ptr -> [B][Lmax][n_mels] f32 with Lmax = the longest utterance's forced-duration sum (or Lmax_cap).
        prosody: None, a prosody.Prosody or a dict of Prosody.create keywords (zvx_synthesize_ex); forced durations are then sized
        by the scaled lengths.  Under an output rate (set_int("out_rate", hz)) the waveform rows, wav_stride and wait_host's rows are
        in samples of that rate: row b carries out_samples(mel_len[b] * hop) of them; native_rate=True (ZVX_NATIVE_RATE) takes this
        call out of it."""
        phoneme = _i32(phoneme)
        B, Tmax = phoneme.shape
        puncts = _i32(puncts, (B, Tmax))
        T = _i32(T, (B,))
        if isinstance(spk, (int, np.integer)):
            sptr, sflag = C.c_void_p(int(spk)), ZVX_DEVICE_SPK
        else:
            spk = _f32(spk).reshape(B, self.hidden)
            sptr, sflag = _ptr(spk), 0
        dur = _i32(duration, (B, Tmax)) if duration is not None else None
        pt = _i32(pad_to, (B,)) if pad_to is not None else None
        ps, keep = self._prosody(prosody, B, Tmax)
        if dur is not None:
            Lmax = int(max(np.maximum(dur[b, :T[b]], 0).sum() for b in range(B))) if ps is None else int(keep.scaled_lengths(dur, T).max())
        else:
            Lmax = int(Lmax_cap)
            if Lmax <= 0:
                raise ZvxError(ZVX_E_INVALID, "predicted durations need Lmax_cap (or use encode/decode/vocode)")
        mel_len = np.zeros(B, np.int32)
        if host_async:
            if want_mel or wav_device_ptr is not None:
                raise ZvxError(ZVX_E_INVALID, "host_async delivers the waveform only (want_mel=False, no device pointer)")
            args = (self._h, _ptr(phoneme), _ptr(puncts), _ptr(dur), _ptr(T), B, Tmax, sptr, _ptr(pt), Lmax, None, 0, _ptr(mel_len),
                    None, max(Lmax, 1), None, ZVX_HOST_ASYNC | (ZVX_PCM16 if pcm16 else 0) | (ZVX_NATIVE_RATE if native_rate else 0) | sflag)
            self._chk(self._lib.zvx_synthesize(*args) if ps is None else self._lib.zvx_synthesize_ex(*args, C.byref(ps)))
            return dict(wav=None, mel_len=mel_len, mel=None, log_duration=None, slot=self.get_int("host_slot"))
        # a queued call (device output, no_sync) must not ask for host outputs: a copy into pageable memory would wait for the stream
        logd = None if (wav_device_ptr is not None and no_sync) else np.zeros((B, Tmax), np.float32)
        mel = np.zeros((B, max(Lmax, 1), self.n_mels), np.float32) if (want_mel and wav_device_ptr is None) else None
        mptr = _ptr(mel)
        flags = (ZVX_PCM16 if pcm16 else 0) | (ZVX_NATIVE_RATE if native_rate else 0) | sflag
        if wav_device_ptr is not None:
            wav, wptr, stride = None, C.c_void_p(int(wav_device_ptr)), int(wav_stride)
            flags |= ZVX_DEVICE_OUT | (ZVX_NO_SYNC if no_sync else 0)
            if want_mel:
                if mel_device_ptr is None:
                    raise ZvxError(ZVX_E_INVALID, "a device waveform output takes a device mel output (mel_device_ptr) or want_mel=False")
                mptr = C.c_void_p(int(mel_device_ptr))
        else:
            stride = max(self.out_samples(Lmax * self.hop, native_rate), 1)
            wav = np.zeros((B, stride), np.int16 if pcm16 else np.float32)
            wptr = _ptr(wav)
        args = (self._h, _ptr(phoneme), _ptr(puncts), _ptr(dur), _ptr(T), B, Tmax, sptr, _ptr(pt), Lmax, wptr, stride, _ptr(mel_len),
                mptr, max(Lmax, 1), _ptr(logd), flags)
        self._chk(self._lib.zvx_synthesize(*args) if ps is None else self._lib.zvx_synthesize_ex(*args, C.byref(ps)))
        return dict(wav=wav, mel_len=mel_len, mel=mel, log_duration=logd)

    def wait_host(self, slot: int, pcm16=False):
        """Waveform rows of the ZVX_HOST_ASYNC call that used `slot`: an ndarray VIEW [B][valid samples] of the context's pinned host
        memory (no copy; valid until the second next host_async call -- copy it to keep it)."""
        rows, stride, nrows, valid = C.c_void_p(), C.c_int64(), C.c_int32(), C.c_int64()
        self._chk(self._lib.zvx_wait_host(self._h, int(slot), C.byref(rows), C.byref(stride), C.byref(nrows), C.byref(valid)))
        ct = C.c_int16 if pcm16 else C.c_float
        n = int(nrows.value) * int(stride.value)
        flat = np.ctypeslib.as_array(C.cast(rows, C.POINTER(ct)), shape=(n,))
        return flat.reshape(int(nrows.value), int(stride.value))[:, :max(int(valid.value), 1)]

    # ---- introspection ------------------------------------------------------------------------
    def fetch(self, what, shape):
        out = np.zeros(shape, np.float32)
        self._chk(self._lib.zvx_fetch(self._h, what.encode(), _ptr(out), out.size))
        return out

    def sync(self):
        self._chk(self._lib.zvx_sync(self._h))

    def _stage_ms(self):
        """zvx_stage_times: every stage slot's hipEvent time, [ZVX_T_COUNT] float32"""
        ms = np.zeros(ZVX_T_COUNT, np.float32)
        self._chk(self._lib.zvx_stage_times(self._h, _ptr(ms)))
        return ms

    def stage_times(self):
        ms = self._stage_ms()
        return {n: float(ms[i]) for i, n in enumerate(STAGES)}

    def resample_ms(self):
        """hipEvent time of the resample stage of the last waveform call or resample() (profile >= 1; 0.0: that call ran none)"""
        return float(self._stage_ms()[ZVX_T_RESAMPLE])

    def join_ms(self):
        """hipEvent time of the launches of the last join() / join_device() / trim_bounds() (profile >= 1)"""
        return float(self._stage_ms()[ZVX_T_JOIN])

    def kernel_stats(self):
        arr = (KernelStat * 32)()
        n = self._lib.zvx_kernel_stats(self._h, arr, 32)
        return [dict(name=arr[i].name.decode(), launches=int(arr[i].launches), ms=float(arr[i].ms),
                     flops=float(arr[i].flops), bytes=float(arr[i].bytes)) for i in range(n)]

    def tag_stats(self):
        """per pipeline stage: launches, ms, algorithmic FLOPs and bytes (profile 2, profile_only -1)"""
        arr = (KernelStat * 64)()
        n = self._lib.zvx_tag_stats(self._h, arr, 64)
        return [dict(name=arr[i].name.decode(), launches=int(arr[i].launches), ms=float(arr[i].ms),
                     flops=float(arr[i].flops), bytes=float(arr[i].bytes)) for i in range(n)]

    def reset_stats(self):
        self._chk(self._lib.zvx_reset_stats(self._h))

    # ---- device buffers + the multi-GPU waveform gather (RCCL inside libzvx; no torch) ----------------------------
    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        self._chk(self._lib.zvx_dev_alloc(self._h, int(nbytes), C.byref(p)))
        return int(p.value)

    def dev_free(self, ptr: int):
        self._chk(self._lib.zvx_dev_free(self._h, C.c_void_p(int(ptr))))

    def dev_from_host(self, ptr: int, arr):
        arr = np.ascontiguousarray(arr)
        self._chk(self._lib.zvx_dev_from_host(self._h, C.c_void_p(int(ptr)), _ptr(arr), arr.nbytes))

    def spkemb_device(self, mels_ptr: int, lens, B: int, Tmax: int, out_ptr: int, no_sync=False):
        """speaker encoder on device-resident mels [B][Tmax][n_mels] -> device embeddings [B][hidden]"""
        lens = _i32(lens, (B,))
        self._chk(self._lib.zvx_spkemb_ex(self._h, C.c_void_p(int(mels_ptr)), _ptr(lens), B, Tmax, C.c_void_p(int(out_ptr)),
                                          ZVX_DEVICE_IN | ZVX_DEVICE_OUT | (ZVX_NO_SYNC if no_sync else 0)))

    def vocode_mel_device(self, mel_ptr: int, P, Pmax: int, wav_ptr: int, wav_stride: int, no_sync=False, pcm16=False):
        """stand-alone vocoder on a device-resident mel [B][Pmax][n_mels] -> device waveform rows"""
        P = _i32(P)
        self._chk(self._lib.zvx_vocode_mel(self._h, C.c_void_p(int(mel_ptr)), _ptr(P), len(P), int(Pmax), C.c_void_p(int(wav_ptr)), int(wav_stride),
                                           ZVX_DEVICE_IN | ZVX_DEVICE_OUT | (ZVX_NO_SYNC if no_sync else 0) | (ZVX_PCM16 if pcm16 else 0)))

    def dev_copy(self, dst: int, src: int, nbytes: int):
        """device to device (zvx_dev_copy), behind everything queued on the context's stream; the ranges must not overlap"""
        self._chk(self._lib.zvx_dev_copy(self._h, C.c_void_p(int(dst)), C.c_void_p(int(src)), int(nbytes)))

    def dev_to_host(self, ptr: int, shape, dtype):
        out = np.empty(shape, dtype)
        self._chk(self._lib.zvx_dev_to_host(self._h, _ptr(out), C.c_void_p(int(ptr)), out.nbytes))
        return out

    @staticmethod
    def comm_unique_id() -> bytes:
        """rank 0: a fresh RCCL communicator id (128 bytes) to hand to every rank's comm_init."""
        lib = load()
        buf = C.create_string_buffer(ZVX_COMM_ID_BYTES)
        rc = lib.zvx_comm_unique_id(buf)
        if rc != ZVX_OK:
            raise ZvxError(rc, lib.zvx_last_error(None).decode())
        return buf.raw

    def comm_init(self, comm_id, rank: int, world: int):
        buf = C.create_string_buffer(bytes(comm_id), ZVX_COMM_ID_BYTES) if comm_id is not None else None
        self._chk(self._lib.zvx_comm_init(self._h, buf, int(rank), int(world)))
        self.rank, self.world = int(rank), int(world)

    def comm_gather(self, local_ptr: int, nbytes: int, recv_ptr, root: int = 0, no_sync: bool = False):
        self._chk(self._lib.zvx_comm_gather(self._h, C.c_void_p(int(local_ptr)), int(nbytes),
                                            C.c_void_p(int(recv_ptr)) if recv_ptr else None, int(root),
                                            ZVX_NO_SYNC if no_sync else 0))

    def comm_barrier(self):
        self._chk(self._lib.zvx_comm_barrier(self._h))

    def comm_info(self) -> dict:
        """Collective: what the communicator itself reports (ranks, RCCL version) and every rank's device PCI address."""
        n = 4 + self.world
        out = (C.c_int64 * n)()
        self._chk(self._lib.zvx_comm_info(self._h, out, n))
        ver = int(out[2])
        pci = [int(out[4 + r]) for r in range(self.world)]
        return {"world": int(out[0]), "comm_count": int(out[1]), "version_code": ver,
                "version": (f"{ver // 10000}.{(ver // 100) % 100}.{ver % 100}" if ver > 0 else None),
                "ranks_seen": int(out[3]),
                "device_pci": [(f"{p >> 16:04x}:{(p >> 8) & 0xff:02x}:{(p >> 3) & 0x1f:02x}.{p & 7}" if p >= 0 else None) for p in pci]}

    def comm_max(self, value: float) -> float:
        v = C.c_double(float(value))
        self._chk(self._lib.zvx_comm_max_f64(self._h, C.byref(v)))
        return float(v.value)
