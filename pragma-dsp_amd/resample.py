"""Polyphase rate change on the device: upsample by `up`, filter, keep every `down`-th sample, as one time-domain
launch per call (include/pdsp_hip.h, "polyphase rate change").  The reference's roadmap asks for it under "Filters and
utilities" ("resampling to a uniform grid", "windowed-sinc filter design helpers") and has no such function yet; the
conventions are scipy.signal.resample_poly's (padtype "constant") and scipy.signal.upfirdn's.

    Resampler(up, down, taps=None, device=None, dtype=torch.float32)   resample_poly: gcd reduction, default design
    Upfirdn(h, up=1, down=1, device=None, dtype=torch.float32)          upfirdn: taps and ratio as given, full output
    resample_poly(x, up, down, taps=None) / upfirdn(h, x, up=1, down=1)  one-shot device forms
    resamplePoly(signal, up, down, taps=None) / upfirdnHost(h, x, up=1, down=1)   host f64 forms, numpy in / numpy out
    design_taps(up, down)                                               the default filter (times up), numpy f64

torch is used for device memory and streams only; the arithmetic is the HIP kernel behind the C ABI.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi
from ._capi import PdspError, check, lib
from .filters import _rows

MAX_RATIO = 8192  # up and down
MAX_TAPS = 8192   # the FIR module's limit; the default design needs 20 * max(up, down) + 1


def _ratio(up, down) -> tuple[int, int]:
    for name, v in (("up", up), ("down", down)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -2 ** 63 <= int(v) < 2 ** 63:
            raise PdspError(_capi.ERR_BAD_ARG, f"{name} must be an integer, got {v!r}")
    return int(up), int(down)


def _taps(taps):
    if taps is None:
        return None
    if isinstance(taps, torch.Tensor):
        taps = taps.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(taps, dtype=np.float64).reshape(-1))


def design_taps(up, down) -> np.ndarray:
    """The filter resample_poly(x, up, down) convolves with: scipy.signal.firwin(20 m + 1, 1 / m, window=("kaiser",
    5.0)) * up, m = max(up, down), after up and down are divided by their gcd.  Computed on the host."""
    up, down = _ratio(up, down)
    n = C.c_longlong()
    check(lib.pdsp_resample_design_f64(up, down, None, C.byref(n)))
    h = np.empty(n.value, dtype=np.float64)
    check(lib.pdsp_resample_design_f64(up, down, _capi.dptr(h), C.byref(n)))
    return h


class _Handle:
    """A pdsp_resampler on one GPU and what both classes do with it."""

    _full = 0

    def _init(self, device, dtype, create):
        if dtype not in (torch.float32, torch.float64):
            raise PdspError(_capi.ERR_BAD_ARG, f"unsupported dtype {dtype}")
        self.dtype = dtype
        self._sfx = "f32" if dtype == torch.float32 else "f64"
        self._h = C.c_void_p()
        if not torch.cuda.is_available():
            # argument errors come first, as everywhere: the library checks them without a device
            probe = C.c_void_p()
            check(create(-1, C.byref(probe)))
            lib.pdsp_resampler_destroy(probe)
            raise PdspError(_capi.ERR_DEVICE, "no HIP device available (the pdsp engine has no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        check(create(self.device.index, C.byref(self._h)))
        self.up = int(lib.pdsp_resampler_up(self._h))
        self.down = int(lib.pdsp_resampler_down(self._h))
        self.ntaps = int(lib.pdsp_resampler_ntaps(self._h))
        self.t0 = int(lib.pdsp_resampler_t0(self._h))
        self.taps = np.empty(self.ntaps, dtype=np.float64)
        check(lib.pdsp_resampler_taps(self._h, _capi.dptr(self.taps)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib.pdsp_resampler_destroy(h)
            self._h = None

    def output_len(self, length: int) -> int:
        """Outputs per row of `length` samples."""
        n = C.c_longlong()
        check(lib.pdsp_resample_output_len(self._h, int(length), self._full, C.byref(n)))
        return n.value

    def apply(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """Rows along the last axis of x ([..., len], contiguous or a 2-D view with a row stride) -> [..., y_len]."""
        if not isinstance(x, torch.Tensor) or x.dtype != self.dtype or not x.is_cuda or x.device != self.device:
            raise PdspError(_capi.ERR_BAD_ARG, f"input must be a {self.dtype} tensor on {self.device}")
        length = x.shape[-1] if x.dim() else 0
        y_len = self.output_len(length)
        rows, x_stride = _rows(x, "input")
        shape = (*x.shape[:-1], y_len)
        if out is None:
            out = torch.empty(shape, dtype=self.dtype, device=self.device)
        elif (not isinstance(out, torch.Tensor) or out.dtype != self.dtype or out.device != self.device
              or tuple(out.shape) != shape):
            raise PdspError(_capi.ERR_BAD_ARG, f"out must be a {self.dtype} tensor of shape {shape} on {self.device}")
        _, y_stride = _rows(out, "out")
        with torch.cuda.device(self.device):
            fn = getattr(lib, f"pdsp_upfirdn_{self._sfx}")
            check(fn(self._h, rows, C.c_void_p(x.data_ptr()), length, x_stride, C.c_void_p(out.data_ptr()), y_len,
                     y_stride, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))
        return out

    __call__ = apply


class Resampler(_Handle):
    """scipy.signal.resample_poly(x, up, down, window=taps, axis=-1) on one GPU: up / down reduced by their gcd
    (.up, .down), the taps -- the default design, or the array given -- times up (.taps), ceil(len up / down) outputs
    per row.  up == down is the identity."""

    def __init__(self, up, down, taps=None, device=None, dtype=torch.float32):
        up, down = _ratio(up, down)
        h = _taps(taps)
        self._init(device, dtype, lambda dev, out: lib.pdsp_resampler_create_poly(
            dev, up, down, _capi.dptr(h), 0 if h is None else h.size, out))


class Upfirdn(_Handle):
    """scipy.signal.upfirdn(h, x, up, down, axis=-1) on one GPU: the taps and the ratio as given, the full output of
    ((len - 1) up + ntaps - 1) // down + 1 samples per row."""

    _full = 1

    def __init__(self, h, up=1, down=1, device=None, dtype=torch.float32):
        up, down = _ratio(up, down)
        h = _taps(h)
        self._init(device, dtype, lambda dev, out: lib.pdsp_resampler_create(dev, up, down, _capi.dptr(h), h.size, 0, out))


def resample_poly(x: torch.Tensor, up, down, taps=None) -> torch.Tensor:
    """One-shot device form: Resampler(up, down, taps, x.device, x.dtype).apply(x)."""
    return Resampler(up, down, taps, x.device, x.dtype).apply(x)


def upfirdn(h, x: torch.Tensor, up=1, down=1) -> torch.Tensor:
    """One-shot device form: Upfirdn(h, up, down, x.device, x.dtype).apply(x)."""
    return Upfirdn(h, up, down, x.device, x.dtype).apply(x)


def _host_rows(signal):
    x = np.ascontiguousarray(np.asarray(signal, dtype=np.float64))
    if x.ndim == 0:
        raise PdspError(_capi.ERR_BAD_ARG, "signal must have at least one axis")
    rows = int(np.prod(x.shape[:-1], dtype=np.int64))
    return x, x.reshape(rows, x.shape[-1])


def _host_out(x, x2, y_len_of):
    """The output buffer, or none for arguments the library will refuse before it writes."""
    try:
        y_len = y_len_of(x2.shape[1])
    except (ZeroDivisionError, OverflowError):
        y_len = 0
    return np.empty((x2.shape[0], max(y_len, 0)), dtype=np.float64)


def resamplePoly(signal, up, down, taps=None) -> np.ndarray:
    """Host f64 form (numpy in, numpy out) through pdsp_resample_poly_host_f64: signal [len] or [..., len]."""
    up, down = _ratio(up, down)
    h = _taps(taps)
    x, x2 = _host_rows(signal)
    y = _host_out(x, x2, lambda n: -(-n * up // down))
    check(lib.pdsp_resample_poly_host_f64(_capi.dptr(x2), x2.shape[0], x2.shape[1], up, down, _capi.dptr(h),
                                          0 if h is None else h.size, _capi.dptr(y)))
    return y.reshape(*x.shape[:-1], y.shape[1])


def upfirdnHost(h, x, up=1, down=1) -> np.ndarray:
    """Host f64 form (numpy in, numpy out) through pdsp_upfirdn_host_f64: x [len] or [..., len]."""
    up, down = _ratio(up, down)
    h = _taps(h)
    x, x2 = _host_rows(x)
    y = _host_out(x, x2, lambda n: ((n - 1) * up + h.size - 1) // down + 1)
    check(lib.pdsp_upfirdn_host_f64(_capi.dptr(h), h.size, _capi.dptr(x2), x2.shape[0], x2.shape[1], up, down,
                                    _capi.dptr(y)))
    return y.reshape(*x.shape[:-1], y.shape[1])
