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

from . import _capi, _device
from ._capi import check, lib
from ._device import host_rows, integer

MAX_RATIO = 8192  # up and down
MAX_TAPS = 8192   # the FIR module's limit; the default design needs 20 * max(up, down) + 1


def _ratio(up, down) -> tuple[int, int]:
    return integer(up, "up"), integer(down, "down")


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


class _Handle(_device.Handle):
    """A pdsp_resampler on one GPU and what both classes do with it."""

    _destroy = lib.pdsp_resampler_destroy
    _full = 0

    def _init(self, device, dtype, create):
        self._open(create, device, dtype)
        self.up = int(lib.pdsp_resampler_up(self._h))
        self.down = int(lib.pdsp_resampler_down(self._h))
        self.ntaps = int(lib.pdsp_resampler_ntaps(self._h))
        self.t0 = int(lib.pdsp_resampler_t0(self._h))
        self.taps = np.empty(self.ntaps, dtype=np.float64)
        check(lib.pdsp_resampler_taps(self._h, _capi.dptr(self.taps)))

    def output_len(self, length: int) -> int:
        """Outputs per row of `length` samples."""
        n = C.c_longlong()
        check(lib.pdsp_resample_output_len(self._h, int(length), self._full, C.byref(n)))
        return n.value

    def apply(self, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """Rows along the last axis of x ([..., len], contiguous or a 2-D view with a row stride) -> [..., y_len]."""
        _device.operand(x, "input", self.device, self.dtype, layout="rows")
        y_len = self.output_len(x.shape[-1] if x.dim() else 0)
        return _device.launch_rows(getattr(lib, f"pdsp_upfirdn_{self._sfx}"), self._h, self, x, out, y_len, (), (y_len,))

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
    x, x2 = host_rows(signal)
    y = _host_out(x, x2, lambda n: -(-n * up // down))
    check(lib.pdsp_resample_poly_host_f64(_capi.dptr(x2), x2.shape[0], x2.shape[1], up, down, _capi.dptr(h),
                                          0 if h is None else h.size, _capi.dptr(y)))
    return y.reshape(*x.shape[:-1], y.shape[1])


def upfirdnHost(h, x, up=1, down=1) -> np.ndarray:
    """Host f64 form (numpy in, numpy out) through pdsp_upfirdn_host_f64: x [len] or [..., len]."""
    up, down = _ratio(up, down)
    h = _taps(h)
    x, x2 = host_rows(x)
    y = _host_out(x, x2, lambda n: ((n - 1) * up + h.size - 1) // down + 1)
    check(lib.pdsp_upfirdn_host_f64(_capi.dptr(h), h.size, _capi.dptr(x2), x2.shape[0], x2.shape[1], up, down,
                                    _capi.dptr(y)))
    return y.reshape(*x.shape[:-1], y.shape[1])
