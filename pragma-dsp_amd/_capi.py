"""ctypes binding of include/pdsp_hip.h (pragma-dsp_amd/csrc/libpdsp_hip.so).

This is the only door to compute: there is no Python/NumPy fallback.  If the
library has not been built, importing fails loudly; if there is no GPU, every
compute entry point raises PdspError(PDSP_ERR_DEVICE).
"""
from __future__ import annotations

import ctypes as C
import os

# ONE HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so (SONAME
# libamdhip64.so.7) and pulls it in by file name; libpdsp_hip.so needs "libamdhip64.so.7".
# Loaded after torch, ours resolves onto torch's already-mapped copy by SONAME.  Loaded
# BEFORE torch, the system copy is mapped first and torch then maps a second runtime: device
# pointers would still work, but streams/events would not be shared, and whichever runtime
# initialises second can fail ("no HIP device").  So torch, when present, is imported first.
try:
    import torch  # noqa: F401
except ImportError:  # pure drop-in use without torch: the system runtime is the only one
    pass

_HERE = os.path.dirname(os.path.abspath(__file__))
# PDSP_LIB_PATH: another build of the same library (development A/B runs of compile-time kernel options)
LIB_PATH = os.environ.get("PDSP_LIB_PATH") or os.path.join(_HERE, "csrc", "libpdsp_hip.so")

# pdsp_status
OK = 0
ERR_SIZE_NOT_POW2 = 1
ERR_INPUT_LENGTH = 2
ERR_WINDOW_SIZE = 3
ERR_WINDOW_LENGTH = 4
ERR_WINDOW_TYPE = 5
ERR_FFT_SIZE = 6
ERR_SAMPLE_RATE = 7
ERR_UNSUPPORTED_SIZE = 8
ERR_BAD_ARG = 9
ERR_DEVICE = 10

WINDOW_TYPES = {"rect": 0, "hann": 1, "hamming": 2, "blackman": 3}
SIDES = {"one": 0, "two": 1}
FIR_MODES = {"full": 0, "same": 1, "valid": 2, "filter": 3}
DCT_NORMS = {"backward": 0, "ortho": 1, "forward": 2}
HILBERT_OUT = {"analytic": 0, "imag": 1, "envelope": 2, "phase": 3}
COMPLEX_OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3, "conj": 4, "scale": 5, "mulScalar": 6}


class PdspError(Exception):
    """Raised with the reference's message text (the JS API throws `Error(message)`)."""

    def __init__(self, code: int, message: str):
        super().__init__(message)
        self.code = code


class Peak(C.Structure):
    _fields_ = [("index", C.c_int32), ("frequency", C.c_double),
                ("amplitude", C.c_double), ("phase", C.c_double)]


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C pragma-dsp_amd/csrc`).  pragma-dsp_amd has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    ll, i32, dbl, vp = C.c_longlong, C.c_int, C.c_double, C.c_void_p
    dp = C.POINTER(C.c_double)
    u64 = C.c_uint64
    sigs = {
        "pdsp_version": ([], i32),
        "pdsp_last_error": ([], C.c_char_p),
        "pdsp_device_count": ([], i32),
        "pdsp_max_size": ([i32], i32),
        "pdsp_set_host_precision": ([i32], i32),
        "pdsp_set_split16k": ([i32], i32),
        "pdsp_set_staged_small": ([i32], i32),
        "pdsp_set_fused_window": ([i32], i32),
        "pdsp_set_twopass": ([i32], i32),
        "pdsp_set_real_packed": ([i32], i32),
        "pdsp_plan_window_f32": ([vp, i32, C.POINTER(vp)], i32),
        "pdsp_plan_window_f64": ([vp, i32, C.POINTER(vp)], i32),
        "pdsp_is_pow2": ([ll], i32),
        "pdsp_next_pow2": ([ll], ll),
        "pdsp_window_make": ([i32, ll, dp], i32),
        "pdsp_bin_frequencies": ([ll, dbl, i32, dp, C.POINTER(ll)], i32),
        "pdsp_fft_shift_f64": ([dp, ll, dp], i32),
        "pdsp_find_peak_f64": ([dp, ll], ll),
        "pdsp_plan_create": ([ll, i32, C.POINTER(vp)], i32),
        "pdsp_plan_destroy": ([vp], i32),
        "pdsp_plan_size": ([vp], ll),
        "pdsp_plan_cache_clear": ([], i32),
        "pdsp_plan_device": ([vp], i32),
        "pdsp_planes_alloc": ([vp, ll, i32, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                               C.POINTER(C.c_ulonglong)], i32),
        "pdsp_planes_free": ([vp], i32),
        "pdsp_fft_forward_real_f32": ([vp, ll, vp, vp, vp, vp], i32),
        "pdsp_fft_forward_complex_f32": ([vp, ll, vp, vp, vp, vp, vp], i32),
        "pdsp_fft_inverse_f32": ([vp, ll, vp, vp, vp, vp, vp], i32),
        "pdsp_fft_forward_interleaved_f32": ([vp, ll, vp, vp, vp], i32),
        "pdsp_fft_inverse_interleaved_f32": ([vp, ll, vp, vp, vp], i32),
        "pdsp_apply_window_f32": ([ll, ll, vp, vp, vp, vp], i32),
        "pdsp_magnitude_f32": ([ll, vp, vp, vp, vp], i32),
        "pdsp_phase_f32": ([ll, vp, vp, vp, vp], i32),
        "pdsp_complex_op_f32": ([i32, ll, vp, vp, vp, vp, ll, dbl, dbl, vp, vp, vp], i32),
        "pdsp_spectrum_f32": ([vp, ll, vp, ll, ll, vp, i32, vp, vp, vp, vp], i32),
        "pdsp_fft_forward_real_f64": ([vp, ll, vp, vp, vp, vp], i32),
        "pdsp_fft_forward_complex_f64": ([vp, ll, vp, vp, vp, vp, vp], i32),
        "pdsp_fft_inverse_f64": ([vp, ll, vp, vp, vp, vp, vp], i32),
        "pdsp_fft_forward_interleaved_f64": ([vp, ll, vp, vp, vp], i32),
        "pdsp_fft_inverse_interleaved_f64": ([vp, ll, vp, vp, vp], i32),
        "pdsp_apply_window_f64": ([ll, ll, vp, vp, vp, vp], i32),
        "pdsp_magnitude_f64": ([ll, vp, vp, vp, vp], i32),
        "pdsp_phase_f64": ([ll, vp, vp, vp, vp], i32),
        "pdsp_spectrum_f64": ([vp, ll, vp, ll, ll, vp, i32, vp, vp, vp, vp], i32),
        "pdsp_spectrum_peaks_f32": ([vp, ll, vp, ll, ll, vp, i32, dbl, vp, vp, vp, vp], i32),
        "pdsp_fft_transform_host_f64": ([vp, ll, ll, dp, dp, dp, dp, i32], i32),
        "pdsp_fft_transform_rows_host_f64": ([vp, ll, ll, C.POINTER(dp), C.POINTER(dp), dp, dp, i32], i32),
        "pdsp_apply_window_host_f64": ([dp, ll, dp, ll, dp], i32),
        "pdsp_magnitude_host_f64": ([dp, dp, ll, dp], i32),
        "pdsp_phase_host_f64": ([dp, dp, ll, dp], i32),
        "pdsp_spectrum_host_f64": ([dp, ll, dbl, ll, i32, i32, dp, dp, dp, C.POINTER(Peak), C.POINTER(ll)], i32),
        "pdsp_spectrum_batch_host_f64": ([dp, ll, ll, dbl, ll, i32, i32, dp, dp, dp, C.POINTER(Peak), C.POINTER(ll)], i32),
        "pdsp_spectrum_rows_host_f64": ([C.POINTER(dp), ll, ll, dbl, ll, i32, i32, dp, dp, dp, C.POINTER(Peak), C.POINTER(ll)], i32),
        "pdsp_spectrum_rows_host_f32in": ([C.POINTER(C.POINTER(C.c_float)), ll, ll, dbl, ll, i32, i32, dp, dp, dp, C.POINTER(Peak), C.POINTER(ll)], i32),
        "pdsp_fir_spectrum_f32": ([vp, vp, ll, vp, vp, vp], i32),
        "pdsp_fir_spectrum_f64": ([vp, vp, ll, vp, vp, vp], i32),
        "pdsp_fir_filter_f32": ([vp, ll, vp, ll, ll, vp, vp, ll, ll, ll, vp, ll, vp], i32),
        "pdsp_fir_filter_f64": ([vp, ll, vp, ll, ll, vp, vp, ll, ll, ll, vp, ll, vp], i32),
        "pdsp_fir_output_range": ([ll, ll, i32, C.POINTER(ll), C.POINTER(ll)], i32),
        "pdsp_fir_block_size": ([ll], ll),
        "pdsp_fir_filter_host_f64": ([dp, ll, ll, dp, ll, i32, dp], i32),
        "pdsp_stft_complex_f32": ([vp, ll, vp, ll, ll, vp, vp, vp, vp], i32),
        "pdsp_stft_complex_f64": ([vp, ll, vp, ll, ll, vp, vp, vp, vp], i32),
        "pdsp_istft_f32": ([vp, ll, vp, vp, ll, vp, vp, vp], i32),
        "pdsp_istft_f64": ([vp, ll, vp, vp, ll, vp, vp, vp], i32),
        "pdsp_stft_host_f64": ([dp, ll, ll, ll, i32, dp, dp], i32),
        "pdsp_istft_host_f64": ([dp, dp, ll, ll, ll, i32, dp], i32),
        "pdsp_set_istft_chunk_frames": ([i32], i32),
        "pdsp_dct_f32": ([vp, ll, vp, ll, i32, i32, vp, ll, vp], i32),
        "pdsp_dct_f64": ([vp, ll, vp, ll, i32, i32, vp, ll, vp], i32),
        "pdsp_dct_host_f64": ([dp, ll, ll, i32, i32, dp], i32),
        "pdsp_hilbert_f32": ([vp, ll, vp, ll, ll, i32, vp, ll, vp], i32),
        "pdsp_hilbert_f64": ([vp, ll, vp, ll, ll, i32, vp, ll, vp], i32),
        "pdsp_hilbert_host_f64": ([dp, ll, ll, ll, i32, dp], i32),
        "pdsp_resampler_create": ([i32, ll, ll, dp, ll, ll, C.POINTER(vp)], i32),
        "pdsp_resampler_create_poly": ([i32, ll, ll, dp, ll, C.POINTER(vp)], i32),
        "pdsp_resampler_destroy": ([vp], i32),
        "pdsp_resampler_up": ([vp], ll),
        "pdsp_resampler_down": ([vp], ll),
        "pdsp_resampler_ntaps": ([vp], ll),
        "pdsp_resampler_t0": ([vp], ll),
        "pdsp_resampler_taps": ([vp, dp], i32),
        "pdsp_resample_output_len": ([vp, ll, i32, C.POINTER(ll)], i32),
        "pdsp_upfirdn_f32": ([vp, ll, vp, ll, ll, vp, ll, ll, vp], i32),
        "pdsp_upfirdn_f64": ([vp, ll, vp, ll, ll, vp, ll, ll, vp], i32),
        "pdsp_resample_design_f64": ([ll, ll, dp, C.POINTER(ll)], i32),
        "pdsp_resample_poly_host_f64": ([dp, ll, ll, ll, ll, dp, ll, dp], i32),
        "pdsp_upfirdn_host_f64": ([dp, ll, dp, ll, ll, ll, ll, dp], i32),
        "pdsp_dft_create": ([ll, i32, C.POINTER(vp)], i32),
        "pdsp_dft_destroy": ([vp], i32),
        "pdsp_dft_length": ([vp], ll),
        "pdsp_dft_conv_size": ([vp], ll),
        "pdsp_dft_c2c_f32": ([vp, ll, vp, vp, ll, vp, vp, ll, i32, vp], i32),
        "pdsp_dft_c2c_f64": ([vp, ll, vp, vp, ll, vp, vp, ll, i32, vp], i32),
        "pdsp_dft_host_f64": ([dp, dp, ll, ll, i32, dp, dp], i32),
        "pdsp_czt_create": ([ll, ll, dbl, dbl, dbl, i32, C.POINTER(vp)], i32),
        "pdsp_czt_destroy": ([vp], i32),
        "pdsp_czt_length": ([vp], ll),
        "pdsp_czt_bins": ([vp], ll),
        "pdsp_czt_conv_size": ([vp], ll),
        "pdsp_czt_f32": ([vp, ll, vp, vp, ll, vp, vp, ll, vp], i32),
        "pdsp_czt_f64": ([vp, ll, vp, vp, ll, vp, vp, ll, vp], i32),
        "pdsp_czt_host_f64": ([dp, dp, ll, ll, ll, dbl, dbl, dbl, dp, dp], i32),
        "pdsp_dwt_create": ([i32, C.c_char_p, dp, ll, i32, C.POINTER(vp)], i32),
        "pdsp_dwt_destroy": ([vp], i32),
        "pdsp_dwt_ntaps": ([vp], ll),
        "pdsp_dwt_levels": ([vp], i32),
        "pdsp_dwt_taps": ([vp, dp], i32),
        "pdsp_wavelet_taps": ([C.c_char_p, dp, C.POINTER(ll)], i32),
        "pdsp_dwt_max_levels": ([ll, ll, i32], i32),
        "pdsp_dwt_forward_f32": ([vp, ll, vp, ll, ll, vp, ll, vp], i32),
        "pdsp_dwt_forward_f64": ([vp, ll, vp, ll, ll, vp, ll, vp], i32),
        "pdsp_dwt_inverse_f32": ([vp, ll, vp, ll, ll, vp, ll, vp], i32),
        "pdsp_dwt_inverse_f64": ([vp, ll, vp, ll, ll, vp, ll, vp], i32),
        "pdsp_dwt_forward_host_f64": ([dp, ll, ll, C.c_char_p, dp, ll, i32, dp], i32),
        "pdsp_dwt_inverse_host_f64": ([dp, ll, ll, C.c_char_p, dp, ll, i32, dp], i32),
        "pdsp_ntt_create": ([ll, i32, C.POINTER(vp)], i32),
        "pdsp_ntt_destroy": ([vp], i32),
        "pdsp_ntt_size": ([vp], ll),
        "pdsp_ntt_forward_u64": ([vp, ll, vp, ll, vp, ll, vp], i32),
        "pdsp_ntt_inverse_u64": ([vp, ll, vp, ll, vp, ll, vp], i32),
        "pdsp_ntt_conv_u64": ([vp, ll, vp, ll, ll, vp, ll, ll, vp, ll, ll, vp], i32),
        "pdsp_ntt_mul_u64": ([ll, vp, vp, vp, vp], i32),
        "pdsp_ntt_host_u64": ([vp, ll, ll, i32, vp], i32),
        "pdsp_ntt_conv_host_u64": ([vp, ll, vp, ll, i32, ll, ll, vp, ll], i32),
        "pdsp_ntt_modulus": ([], u64),
        "pdsp_ntt_root": ([ll], u64),
        "pdsp_ntt_mulmod": ([u64, u64], u64),
        "pdsp_ntt_powmod": ([u64, u64], u64),
        "pdsp_ntt_invmod": ([u64], u64),
        "pdsp_sdft_create": ([ll, ll, dp, ll, i32, i32, C.POINTER(vp)], i32),
        "pdsp_sdft_destroy": ([vp], i32),
        "pdsp_sdft_length": ([vp], ll),
        "pdsp_sdft_bins": ([vp], ll),
        "pdsp_sdft_bin": ([vp, ll], dbl),
        "pdsp_sdft_hop": ([vp], ll),
        "pdsp_sdft_components": ([vp], ll),
        "pdsp_sdft_frames": ([vp, ll], ll),
        "pdsp_sdft_f32": ([vp, ll, vp, ll, ll, vp, vp, ll, vp], i32),
        "pdsp_sdft_f64": ([vp, ll, vp, ll, ll, vp, vp, ll, vp], i32),
        "pdsp_sdft_host_f64": ([dp, ll, ll, ll, ll, dp, ll, i32, dp, dp], i32),
        "pdsp_sdft_window_weights": ([i32, dp], i32),
        "pdsp_sdft_phase_table": ([ll, dbl, i32, dp, dp], i32),
        "pdsp_set_upfirdn_tile": ([i32], i32),
        "pdsp_set_dwt_tile": ([i32], i32),
        "pdsp_dev_dwt_tile": ([ll, i32, ll, i32, i32, C.POINTER(ll)], i32),
        "pdsp_dev_upfirdn_tile": ([ll, ll, ll, ll, i32, C.POINTER(ll)], i32),
        "pdsp_dev_complex_op_vec4": ([i32, ll, vp, vp, vp, vp, ll, vp, vp, C.POINTER(i32)], i32),
        "pdsp_dev_transform_path_f32": ([vp, ll, vp, vp, vp, vp, i32, C.POINTER(i32)], i32),
        "pdsp_dev_transform_path_f64": ([vp, ll, vp, vp, vp, vp, i32, C.POINTER(i32)], i32),
        "pdsp_dev_spectrum_path_f32": ([vp, ll, vp, ll, ll, vp, i32, vp, vp, vp, vp, C.c_double, C.POINTER(i32)], i32),
        "pdsp_dev_spectrum_path_f64": ([vp, ll, vp, ll, ll, vp, i32, vp, vp, vp, vp, C.c_double, C.POINTER(i32)], i32),
        "pdsp_dev_host_transform_chunks": ([vp, ll, i32, C.POINTER(ll)], i32),
        "pdsp_dev_host_spectrum_chunks": ([vp, ll, i32, i32, C.POINTER(ll)], i32),
        "pdsp_dev_live_resources": ([C.POINTER(ll)], i32),
    }
    for name, (args, res) in sigs.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.argtypes = args
        fn.restype = res
    lib._pdsp_symbols = tuple(sigs)
    # include/pdsp_hip_fft2d.h: a header of its own, bound from a table of its own onto the same library
    fft2d_sigs = {
        "pdsp_fft2d_create": ([ll, ll, i32, C.POINTER(vp)], i32),
        "pdsp_fft2d_destroy": ([vp], i32),
        "pdsp_fft2d_height": ([vp], ll),
        "pdsp_fft2d_width": ([vp], ll),
        "pdsp_fft2d_c2c_f32": ([vp, ll, vp, vp, vp, vp, i32, i32, vp], i32),
        "pdsp_fft2d_c2c_f64": ([vp, ll, vp, vp, vp, vp, i32, i32, vp], i32),
        "pdsp_fft2d_host_f64": ([dp, dp, ll, ll, ll, i32, i32, dp, dp], i32),
        "pdsp_fft2d_query": ([ll, ll, i32, C.POINTER(i32)], i32),
    }
    for name, (args, res) in fft2d_sigs.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = res
    lib._pdsp_fft2d_symbols = tuple(fft2d_sigs)
    return lib


lib = _load()


def check(rc: int) -> None:
    if rc != OK:
        raise PdspError(rc, lib.pdsp_last_error().decode("utf-8", "replace"))


LIVE_FIELDS = ("cached_plans", "pinned", "evictions", "tables", "table_bytes", "host_stage", "dev_stage", "streams")


def live_resources() -> dict:
    """pdsp_dev_live_resources (include/pdsp_hip_dev.h) by field name: exact counters, for the tests."""
    info = (C.c_longlong * len(LIVE_FIELDS))()
    check(lib.pdsp_dev_live_resources(info))
    return dict(zip(LIVE_FIELDS, info))


def dptr(a):
    """numpy float64 array -> double* (None passes NULL)."""
    return a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None
