"""FIR filtering on the device: linear convolution of real rows with one real filter, run as one fused
overlap-save launch per call (include/pdsp_hip.h, "FIR filtering").  The reference names the module it would
live in -- pragma-dsp/filters, "FIR helpers, convolution ... frequency response analysis via FFT utilities"
(ROADMAP.md, "Filters and utilities") -- but has no such function yet.

    FirFilter(taps, device=None, dtype=torch.float32, block=None)   plan + the filter's device spectrum
    fir_filter(x, taps, mode="full")                                 one-shot device form
    firFilter(signal, taps, mode="full")                             host f64 form, numpy in / numpy out

Modes count in the full convolution (length len + ntaps - 1), m = min(len, ntaps): "full", "same" and
"valid" follow numpy.convolve; "filter" is the first len outputs, scipy.signal.lfilter(taps, 1, x).

torch is used for device memory and streams only; the arithmetic is the HIP kernels behind the C ABI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import PdspError, check, lib

MAX_TAPS = 8192  # N/2 of the largest block (16384); longer filters need partitioned convolution


def block_size(ntaps: int) -> int:
    """The default block N for a filter of `ntaps` taps: the smallest power of two >= 8 * ntaps, at least 4096 and
    at most 16384 -- so hop = N - ntaps + 1 >= 7/8 N up to ntaps = 2048 ("FIR filtering")."""
    n = int(lib.pdsp_fir_block_size(int(ntaps)))
    if n == 0:
        if ntaps < 1:
            raise PdspError(_capi.ERR_BAD_ARG, f"filter must have at least one tap, got {ntaps}")
        raise PdspError(_capi.ERR_UNSUPPORTED_SIZE,
                        f"filter of {ntaps} taps exceeds N/2 = {MAX_TAPS} of the largest block (no partitioned convolution)")
    return n


def output_range(length: int, ntaps: int, mode: str) -> tuple[int, int]:
    """(offset, length) of a mode's outputs in the full convolution."""
    if mode not in _capi.FIR_MODES:
        raise PdspError(_capi.ERR_BAD_ARG, f"unknown FIR mode {mode!r}")
    off, n = C.c_longlong(), C.c_longlong()
    check(lib.pdsp_fir_output_range(int(length), int(ntaps), _capi.FIR_MODES[mode], C.byref(off), C.byref(n)))
    return off.value, n.value


def _rows(t: torch.Tensor, name: str):
    """(rows, row stride) of a tensor of rows [..., len]: contiguous, or 2-D with unit stride along the row."""
    if t.dim() == 0:
        raise PdspError(_capi.ERR_BAD_ARG, f"{name} must have at least one axis")
    if t.is_contiguous():
        return int(np.prod(t.shape[:-1], dtype=np.int64)), t.shape[-1]
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1]:
        return t.shape[0], t.stride(0)
    raise PdspError(_capi.ERR_BAD_ARG, f"{name}: rows at a stride are taken in 2-D tensors only")


class FirFilter:
    """One real FIR filter on one GPU: the plan of block size N and the filter's spectrum H (N/2 + 1 bins) on the
    device.  `block` = N (a power of two, 2 * ntaps <= N <= 16384); None picks block_size(ntaps)."""

    def __init__(self, taps, device=None, dtype=torch.float32, block=None):
        if dtype not in (torch.float32, torch.float64):
            raise PdspError(_capi.ERR_BAD_ARG, f"unsupported dtype {dtype}")
        from .batch import BatchedFft  # the plan object (and its device checks)

        self.dtype = dtype
        self._sfx = "f32" if dtype == torch.float32 else "f64"
        if isinstance(taps, torch.Tensor):
            taps = taps.detach().cpu().numpy()
        taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1))
        self.ntaps = int(taps.size)
        n = block_size(self.ntaps) if block is None else int(block)
        self.plan = BatchedFft(n, device, dtype)
        self.device = self.plan.device
        self.size = n
        self.taps = torch.from_numpy(taps).to(dtype).to(self.device)
        bins = n // 2 + 1
        self.h_re = torch.empty(bins, dtype=dtype, device=self.device)
        self.h_im = torch.empty(bins, dtype=dtype, device=self.device)
        with torch.cuda.device(self.device):
            fn = getattr(lib, f"pdsp_fir_spectrum_{self._sfx}")
            stream = torch.cuda.current_stream(self.device)
            check(fn(self.plan._h, C.c_void_p(self.taps.data_ptr()), self.ntaps, C.c_void_p(self.h_re.data_ptr()),
                     C.c_void_p(self.h_im.data_ptr()), C.c_void_p(stream.cuda_stream)))
            # H is written on the stream current at construction; apply() may run on another one
            self._ready = torch.cuda.Event()
            self._ready.record(stream)

    def _wait_ready(self):
        torch.cuda.current_stream(self.device).wait_event(self._ready)

    def frequency_response(self):
        """H[k] = sum_j taps[j] e^{-2 pi i j k / N}, k = 0 ... N/2, as two device tensors (re, im), ordered on the
        current stream."""
        self._wait_ready()
        return self.h_re, self.h_im

    def apply(self, x: torch.Tensor, mode: str = "full", out: torch.Tensor | None = None) -> torch.Tensor:
        """y = x * taps over the last axis of x ([..., len], rows contiguous or a 2-D view with a row stride),
        restricted to the mode's range: shape [..., y_len]."""
        if x.dtype != self.dtype or not x.is_cuda or x.device != self.device:
            raise PdspError(_capi.ERR_BAD_ARG, f"input must be a {self.dtype} tensor on {self.device}")
        length = x.shape[-1] if x.dim() else 0
        y_off, y_len = output_range(length, self.ntaps, mode)
        rows, x_stride = _rows(x, "input")
        if out is None:
            out = torch.empty(*x.shape[:-1], y_len, dtype=self.dtype, device=self.device)
        elif out.dtype != self.dtype or out.device != self.device or tuple(out.shape) != (*x.shape[:-1], y_len):
            raise PdspError(_capi.ERR_BAD_ARG, f"out must be a {self.dtype} tensor of shape {(*x.shape[:-1], y_len)}")
        _, y_stride = _rows(out, "out")
        with torch.cuda.device(self.device):
            self._wait_ready()
            fn = getattr(lib, f"pdsp_fir_filter_{self._sfx}")
            check(fn(self.plan._h, rows, C.c_void_p(x.data_ptr()), length, x_stride, C.c_void_p(self.h_re.data_ptr()),
                     C.c_void_p(self.h_im.data_ptr()), self.ntaps, y_off, y_len, C.c_void_p(out.data_ptr()), y_stride,
                     C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

    __call__ = apply


def fir_filter(x: torch.Tensor, taps, mode: str = "full", block=None) -> torch.Tensor:
    """One-shot device form: FirFilter(taps, x.device, x.dtype, block).apply(x, mode)."""
    return FirFilter(taps, x.device, x.dtype, block).apply(x, mode)


def firFilter(signal, taps, mode: str = "full") -> np.ndarray:
    """Host f64 form (numpy in, numpy out) through pdsp_fir_filter_host_f64: signal [len] or [batch, len]."""
    if mode not in _capi.FIR_MODES:
        raise PdspError(_capi.ERR_BAD_ARG, f"unknown FIR mode {mode!r}")
    x = np.ascontiguousarray(np.asarray(signal, dtype=np.float64))
    h = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1))
    one = x.ndim == 1
    x2 = x.reshape(1, -1) if one else x.reshape(-1, x.shape[-1])
    y_off, y_len = output_range(x2.shape[1], h.size, mode)
    y = np.empty((x2.shape[0], y_len), dtype=np.float64)
    check(lib.pdsp_fir_filter_host_f64(_capi.dptr(x2), x2.shape[0], x2.shape[1], _capi.dptr(h), h.size,
                                       _capi.FIR_MODES[mode], _capi.dptr(y)))
    return y[0] if one else y.reshape(*x.shape[:-1], y_len)
