"""The sliding DFT of rows -- K chosen bins of a window of N samples at every hop-th start -- one launch per call
(include/pdsp_hip.h, "sliding DFT"):

    Y[j][m] = sum_{n < N} w[n] x[m h + n] exp(-2 pi i b_j n / N),   m < F = 1 + (T - N) // h

with 2 <= N <= 16384 (any integer), bins b_j in CYCLES PER WINDOW (f64: fractional, negative and >= N allowed) and one
of the library's four windows.  Parallel in time, O(K) per sample and free of drift: a frame's bits depend on its own N
samples and on (m h) mod N alone.

    SlidingDft(length, bins, hop=1, window="rect", device=None)   the tables of one transform on one GPU (f32 and f64)
      .frames(samples)                                            F for rows of `samples` values
      .forward(x, out=None)                                       torch rows [..., T] -> (re, im) of [..., K, F]
    sliding_dft(x, length, bins, hop=1, window="rect")            host f64 form: numpy in, complex128 [..., K, F] out
    goertzel(x, bins)                                             one frame, N = len(x): complex128 [..., K]

torch is used for device memory and streams only; the arithmetic is the HIP kernel behind the C ABI.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi, _device
from ._capi import PdspError, check, lib
from ._device import integer, operand, ptr, rows

MAX_LENGTH, MAX_BINS = 16384, 256


def _bins(bins) -> np.ndarray:
    """The bins as a contiguous f64 vector; a scalar is one bin."""
    b = np.atleast_1d(np.asarray(bins))
    if b.ndim != 1 or b.dtype == bool or not (np.issubdtype(b.dtype, np.integer) or np.issubdtype(b.dtype, np.floating)):
        raise PdspError(_capi.ERR_BAD_ARG, "bins must be a real number or a vector of real numbers")
    return np.ascontiguousarray(b, dtype=np.float64)


def _window(window) -> int:
    if window not in _capi.WINDOW_TYPES:
        raise PdspError(_capi.ERR_BAD_ARG, f"Unsupported window type: {window}")
    return _capi.WINDOW_TYPES[window]


class SlidingDft(_device.Handle):
    """A pdsp_sdft on one GPU: the phase tables of K bins of a window of `length` samples, both precisions.

    When to use it: its time is proportional to K x components (1 rect, 3 Hann / Hamming, 5 Blackman) and almost
    independent of the hop, where BatchedFft.stft_complex costs 1 / hop per sample and nothing per bin.  Measured on an
    MI355X in f32 (profiles/sdft_rate.jsonl): the two take equal time at K hop = 450 ... 870
    (rectangular; Hann 270 ... 490) for N = 1024 and at 1300 ... 2000 (1100 ... 1550) for N = 4096; f64 is within 1.5x
    of that.  Below the crossover this class wins (32x at K = 1, hop 16, N = 1024; at hop 1 stft_complex's output does
    not fit at all), above it stft_complex plus a gather of the K bins is the better tool."""

    _destroy = lib.pdsp_sdft_destroy

    def __init__(self, length, bins, hop=1, window="rect", device=None):
        length, hop = integer(length, "length"), integer(hop, "hop")
        b, win = _bins(bins), _window(window)
        self._open(lambda dev, out: lib.pdsp_sdft_create(length, b.size, _capi.dptr(b), hop, win, dev, out), device)
        self.length = int(lib.pdsp_sdft_length(self._h))
        self.hop = int(lib.pdsp_sdft_hop(self._h))
        self.bins = np.array([lib.pdsp_sdft_bin(self._h, j) for j in range(int(lib.pdsp_sdft_bins(self._h)))])
        self.components = int(lib.pdsp_sdft_components(self._h))  # rectangular sliding sums per bin: 1, 3 or 5
        self.window = window

    def frames(self, samples) -> int:
        """F = 1 + (samples - N) // hop, the values of a series for rows of `samples` values (0: shorter than N)."""
        return int(lib.pdsp_sdft_frames(self._h, integer(samples, "samples")))

    def forward(self, x: torch.Tensor, out=None):
        """Rows along the last axis ([..., T] contiguous, or a 2-D view with a row stride >= T), float32 or float64 ->
        (re, im) of [..., K, F].  One launch on the current stream.  out: a pair of contiguous planes [..., K, F]."""
        operand(x, "input", self.device, layout="rows")
        sfx = _device.suffix(x.dtype, "input")
        n, stride = rows(x, "input")
        samples = x.shape[-1]
        frames = self.frames(samples)
        oshape = x.shape[:-1] + (self.bins.size, frames)
        if out is None:
            out = (torch.empty(oshape, dtype=x.dtype, device=self.device),
                   torch.empty(oshape, dtype=x.dtype, device=self.device))
        elif not isinstance(out, (tuple, list)) or len(out) != 2:
            raise PdspError(_capi.ERR_BAD_ARG, "out must be a pair of tensors (re, im)")
        if frames:  # rows shorter than the window: the library refuses them below, before it looks at a buffer
            for o in out:
                operand(o, "out", self.device, x.dtype, shape=oshape)
        with torch.cuda.device(self.device):
            check(getattr(lib, "pdsp_sdft_" + sfx)(self._h, n, ptr(x), stride, samples, ptr(out[0]), ptr(out[1]),
                                                   frames, _device.stream_ptr(self.device)))
        return out[0], out[1]


def sliding_dft(x, length, bins, hop=1, window="rect") -> np.ndarray:
    """The sliding DFT along the last axis, computed on the device in f64: complex128 [..., K, F]."""
    length, hop = integer(length, "length"), integer(hop, "hop")
    b, win = _bins(bins), _window(window)
    a, r = _device.host_rows(x, "x")
    samples = r.shape[1]
    # sizes the library refuses get no buffers: the library fails before it writes
    ok = 2 <= length <= MAX_LENGTH and hop >= 1 and 1 <= b.size <= MAX_BINS and samples >= length and r.shape[0] >= 1
    frames = 1 + (samples - length) // hop if ok else 0
    ore, oim = (np.empty((r.shape[0], b.size, frames), dtype=np.float64) for _ in range(2))
    check(lib.pdsp_sdft_host_f64(_capi.dptr(r), r.shape[0], samples, length, b.size, _capi.dptr(b), hop, win,
                                 _capi.dptr(ore), _capi.dptr(oim)))
    return (ore + 1j * oim).reshape(a.shape[:-1] + (b.size, frames))


def goertzel(x, bins) -> np.ndarray:
    """K bins (cycles per len(x), fractional allowed) of whole rows -- one frame with N = len(x), the Goertzel
    algorithm's use -- computed on the device in f64: complex128 [..., K]."""
    a = np.asarray(x)
    return sliding_dft(a, a.shape[-1] if a.ndim else 0, bins)[..., 0]
