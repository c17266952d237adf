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

from . import _capi, _device
from ._capi import PdspError, check, lib
from ._device import ptr, stream_ptr

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


class FirFilter:
    """One real FIR filter on one GPU: the plan of block size N and the filter's spectrum H (N/2 + 1 bins) on the
    device.  `block` = N (a power of two, 2 * ntaps <= N <= 16384); None picks block_size(ntaps)."""

    def __init__(self, taps, device=None, dtype=torch.float32, block=None):
        from .batch import BatchedFft  # the plan object (and its device checks)

        self._sfx = _device.suffix(dtype)
        if isinstance(taps, torch.Tensor):
            taps = taps.detach().cpu().numpy()
        taps = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1))
        self.ntaps = int(taps.size)
        n = block_size(self.ntaps) if block is None else int(block)
        self.plan = BatchedFft(n, device, dtype)
        self.dtype, self.device = dtype, self.plan.device
        self.size = n
        self.taps = torch.from_numpy(taps).to(dtype).to(self.device)
        bins = n // 2 + 1
        self.h_re = torch.empty(bins, dtype=dtype, device=self.device)
        self.h_im = torch.empty(bins, dtype=dtype, device=self.device)
        with torch.cuda.device(self.device):
            fn = getattr(lib, f"pdsp_fir_spectrum_{self._sfx}")
            check(fn(self.plan._h, ptr(self.taps), self.ntaps, ptr(self.h_re), ptr(self.h_im), stream_ptr(self.device)))
            # H is written on the stream current at construction; apply() may run on another one
            self._ready = torch.cuda.Event()
            self._ready.record(torch.cuda.current_stream(self.device))

    def _wait_ready(self):
        """Orders the current stream behind the launch that wrote H, until that launch is known to have completed:
        from then on a call enqueues its kernel and nothing else ("Streams and graphs").  The event is
        never queried on a capturing stream."""
        ready = self._ready  # read once: another thread may drop it meanwhile
        if ready is None:
            return
        with torch.cuda.device(self.device):
            if not torch.cuda.is_current_stream_capturing() and ready.query():
                self._ready = None
                return
        torch.cuda.current_stream(self.device).wait_event(ready)

    def frequency_response(self):
        """H[k] = sum_j taps[j] e^{-2 pi i j k / N}, k = 0 ... N/2, as two device tensors (re, im), ordered on the
        current stream."""
        self._wait_ready()
        return self.h_re, self.h_im

    def apply(self, x: torch.Tensor, mode: str = "full", out: torch.Tensor | None = None) -> torch.Tensor:
        """y = x * taps over the last axis of x ([..., len], rows contiguous or a 2-D view with a row stride),
        restricted to the mode's range: shape [..., y_len]."""
        _device.operand(x, "input", self.device, self.dtype, layout="rows")
        y_off, y_len = output_range(x.shape[-1] if x.dim() else 0, self.ntaps, mode)
        self._wait_ready()
        return _device.launch_rows(getattr(lib, f"pdsp_fir_filter_{self._sfx}"), self.plan._h, self, x, out, y_len,
                                   (ptr(self.h_re), ptr(self.h_im), self.ntaps, y_off, y_len))

    __call__ = apply


def fir_filter(x: torch.Tensor, taps, mode: str = "full", block=None) -> torch.Tensor:
    """One-shot device form: FirFilter(taps, x.device, x.dtype, block).apply(x, mode)."""
    return FirFilter(taps, x.device, x.dtype, block).apply(x, mode)


def firFilter(signal, taps, mode: str = "full") -> np.ndarray:
    """Host f64 form (numpy in, numpy out) through pdsp_fir_filter_host_f64: signal [len] or [batch, len]."""
    if mode not in _capi.FIR_MODES:
        raise PdspError(_capi.ERR_BAD_ARG, f"unknown FIR mode {mode!r}")
    x, x2 = _device.host_rows(signal)
    h = np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1))
    y_off, y_len = output_range(x2.shape[1], h.size, mode)
    y = np.empty((x2.shape[0], y_len), dtype=np.float64)
    check(lib.pdsp_fir_filter_host_f64(_capi.dptr(x2), x2.shape[0], x2.shape[1], _capi.dptr(h), h.size,
                                       _capi.FIR_MODES[mode], _capi.dptr(y)))
    return y.reshape(*x.shape[:-1], y_len)
