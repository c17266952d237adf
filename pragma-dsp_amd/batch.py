"""Device-resident batched API (an extension: the reference has no batch shape,
only the caller loop of bench/reallife/signals.ts:264-270).  Row b of every call
means exactly `Radix2Fft.forward / forwardComplex / inverse` or the body of
`spectrum()` applied to row b.

torch is used for device memory and streams only; the arithmetic is the HIP
kernels behind include/pdsp_hip.h, reached with raw device pointers.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi, _device
from ._capi import PdspError, check, lib
from ._device import COMPLEX, operand
from ._device import ptr as _ptr, stream_ptr as _stream_ptr  # noqa: F401  (stream.py and tests take them from here)
from .core import isPowerOfTwo, js_num
from .fourier import createWindow


class PlanWindow:
    """The plan's own device copy of createWindow(kind, N) (pdsp_plan_window_*): a borrowed device
    pointer, valid while the plan lives.  Passing it as `window` tells the engine which window it is,
    so the kernels that can fuse createWindow do (include/pdsp_hip.h); `.tensor()` gives a torch copy."""

    def __init__(self, plan: "BatchedFft", kind: str, ptr: int):
        self._plan = plan  # keeps the owner alive (the plan caches pointers, not these objects: no cycle)
        self._p = ptr
        self.kind = kind
        self.shape = (plan.size,)
        self.dtype = plan.dtype
        self.device = plan.device

    def data_ptr(self) -> int:
        return self._p

    def tensor(self) -> torch.Tensor:
        return torch.from_numpy(createWindow(self.kind, self.shape[0])).to(self.dtype).to(self.device)


class BatchedFft(_device.Handle):
    """One plan, many rows.  Tensors are contiguous, shape [..., N], on the plan's GPU, of the
    plan's dtype: torch.float32 (default; sizes up to 2^28) or torch.float64 (up to 2^26; single-pass
    transforms up to N = 8192, spectrum up to N = 16384, four-step beyond)."""

    _destroy = lib.pdsp_plan_destroy

    def __init__(self, size, device=None, dtype=torch.float32):
        _device.suffix(dtype)
        if not isPowerOfTwo(size):
            raise PdspError(_capi.ERR_SIZE_NOT_POW2, f"FFT size must be power of two, got {js_num(size)}")
        self.size = int(size)
        self._windows = {}
        self.arena = None  # the allocation behind the planes of the last alloc_planes() call, if any
        self._open(lambda dev, out: lib.pdsp_plan_create(self.size, dev, out), device, dtype)

    def close(self):
        """Destroys the native plan now (also done when the object is collected).  For a size beyond the single-pass
        limit this also hands the engine's scratch planes -- as large as the largest such transform run -- back to
        the device, where the caller's allocator can use them again."""
        super().close()
        self._windows = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    # -- helpers -------------------------------------------------------------
    def _plane(self, t, name, count):
        operand(t, name, self.device, self.dtype, last=self.size)
        if t.numel() != count:
            raise PdspError(_capi.ERR_BAD_ARG, f"{name} has {t.numel()} elements, input.real has {count}")
        return t

    def _planes(self, re, im, out):
        """The operands of forward / inverse: (batch, out.real, out.imag).  Every plane is [..., N] with the element
        count of re -- the count, not the shape: callers pass reshaped views."""
        operand(re, "input.real", self.device, self.dtype, last=self.size)
        count = re.numel()
        if im is not None:
            self._plane(im, "input.imag", count)
        if out is None:
            return count // self.size, torch.empty_like(re), torch.empty_like(re)
        return count // self.size, self._plane(out[0], "out.real", count), self._plane(out[1], "out.imag", count)

    def window(self, kind: str) -> PlanWindow:
        """The plan's device copy of createWindow(kind, N), cached per kind like FourierLive's window
        cache (src/effect/index.ts:39-48).  A window named by kind is known to the engine (fused
        createWindow where a kernel supports it); a caller's own tensor is read as a table."""
        p = self._windows.get(kind)
        if p is None:
            if kind not in _capi.WINDOW_TYPES:
                raise PdspError(_capi.ERR_WINDOW_TYPE, f"Unsupported window type: {kind}")
            # the first use uploads the table (a synchronous allocation and copy), which no capture allows; the
            # library call has no stream to ask, so the refusal of pdsp_upfirdn_* and the others is made here
            if torch.cuda.is_current_stream_capturing():
                raise PdspError(_capi.ERR_BAD_ARG, f"stream is capturing: the {kind} window table is uploaded on its "
                                                   "first use, which no capture allows; call plan.window"
                                                   f"({kind!r}) once outside the capture first")
            out = C.c_void_p()
            check(getattr(lib, "pdsp_plan_window_" + self._sfx)(self._h, _capi.WINDOW_TYPES[kind], C.byref(out)))
            p = self._windows[kind] = out.value
        return PlanWindow(self, kind, p)

    # -- plane layout ----------------------------------------------------------
    # Where the four planes of a transform lie in HBM decides 8-14 % of the N = 4096 kernel's rate (DESIGN section 5,
    # "What the spread of configs[2] is made of"): inside one large allocation the card's address space behaves as
    # regions of 32 GiB, and the launch runs at its upper plateau (83-85 % of the HBM roofline against 76 % for four
    # planes back to back, 71-73 % for unlucky ones) when the two INPUT planes share a region and each OUTPUT plane
    # has a region of its own.  Offsets of 0 | plane | 40 GiB | 80 GiB put the outputs one and two regions beyond the
    # inputs whatever the phase of the allocation against the region grid (40 - plane > 32 > 40 - 32; 80 likewise).
    ARENA_OUT_GIB = (40, 80)

    def alloc_planes(self, batch: int, real_input: bool = False):
        """(re_in, im_in | None, re_out, im_out) for `batch` rows, carved out of ONE allocation of 80 GiB + one plane
        with the layout above -- the card has 288 GB; the gaps stay usable through `.arena` (a uint8 tensor) -- or,
        when that much memory is not free or a plane is below 256 MiB or above 8 GiB, four plain allocations (`.arena` is None).
        The tensors keep the allocation alive."""
        rows, n = int(batch), self.size
        esize = 4 if self.dtype == torch.float32 else 8
        plane = rows * n * esize
        gib = 1 << 30
        arena = None
        if (256 << 20) <= plane <= 8 * gib:  # planes below 256 MiB: nothing to gain, plain allocations
            try:
                free, _total = torch.cuda.mem_get_info(self.device)
                need = self.ARENA_OUT_GIB[1] * gib + plane
                if free >= need + 4 * gib:
                    arena = torch.empty(need, dtype=torch.uint8, device=self.device)
            except RuntimeError:
                arena = None
        self.arena = arena
        if arena is None:
            mk = lambda: torch.empty((rows, n), dtype=self.dtype, device=self.device)  # noqa: E731
            return mk(), (None if real_input else mk()), mk(), mk()
        pad = (plane + 255) & ~255  # the second input plane starts on a 256-byte boundary

        def view(off):
            return arena[off:off + plane].view(self.dtype).view(rows, n)

        return (view(0), (None if real_input else view(pad)), view(self.ARENA_OUT_GIB[0] * gib),
                view(self.ARENA_OUT_GIB[1] * gib))

    # -- transforms ------------------------------------------------------------
    def forward(self, re: torch.Tensor, im: torch.Tensor | None = None, out=None):
        """Rows of Radix2Fft.forward (im None) or .forwardComplex.  out = (out_re, out_im), or None for fresh planes.
        Aliasing (include/pdsp_hip.h): up to the single-pass size (N <= 16384 in f32, 8192 in f64; f64 real rows also
        16384) an output plane may share bytes with an input plane only where the two begin at the same address --
        out=(re, im) runs in place, out=(im, re) and one plane of either are fine too, for real rows out_re or
        out_im may be re -- and any other overlap raises PdspError(ERR_BAD_ARG, "output overlaps input ...") before
        anything is launched; larger sizes take any overlap.  out_re and out_im never overlap each other."""
        batch, ore, oim = self._planes(re, im, out)
        s = _stream_ptr(self.device)
        if im is None:
            check(getattr(lib, "pdsp_fft_forward_real_" + self._sfx)(self._h, batch, _ptr(re), _ptr(ore), _ptr(oim), s))
        else:
            check(getattr(lib, "pdsp_fft_forward_complex_" + self._sfx)(self._h, batch, _ptr(re), _ptr(im), _ptr(ore),
                                                                      _ptr(oim), s))
        return ore, oim

    def inverse(self, re: torch.Tensor, im: torch.Tensor, out=None):
        """Rows of Radix2Fft.inverse; `out` and its aliasing rule as forward()."""
        if im is None:
            raise PdspError(_capi.ERR_BAD_ARG, "the inverse needs both planes")
        batch, ore, oim = self._planes(re, im, out)
        check(getattr(lib, "pdsp_fft_inverse_" + self._sfx)(self._h, batch, _ptr(re), _ptr(im), _ptr(ore), _ptr(oim),
                                                          _stream_ptr(self.device)))
        return ore, oim

    def forward_interleaved(self, z: torch.Tensor, out: torch.Tensor | None = None, inverse: bool = False):
        """forwardComplex (or inverse) on rows of a complex64 / complex128 tensor [..., N] -- the
        interleaved (re, im) layout of I/Q streams.  Single-pass sizes only.  out=z runs in place; an `out` that
        overlaps z in any other way raises PdspError(ERR_BAD_ARG, "output overlaps input ...")."""
        operand(z, "input", self.device, COMPLEX[self.dtype], last=self.size)
        if out is None:
            out = torch.empty_like(z)
        else:
            operand(out, "out", self.device, z.dtype, shape=z.shape)
        fn = getattr(lib, ("pdsp_fft_inverse_interleaved_" if inverse else "pdsp_fft_forward_interleaved_") + self._sfx)
        check(fn(self._h, z.numel() // self.size, _ptr(z), _ptr(out), _stream_ptr(self.device)))
        return out

    def inverse_interleaved(self, z: torch.Tensor, out: torch.Tensor | None = None):
        return self.forward_interleaved(z, out, inverse=True)

    # -- what the spectrum and short-time methods share ---------------------------
    def _table_window(self, window, name="window", spectral=False):
        """A window argument: a type name (the plan's table; "rect" = none), a PlanWindow of this plan, or a contiguous
        device tensor of N values in the plan's dtype.  The spectrum family (`spectral`) also takes None, and at
        N = 1, where the reference never builds a window, any name."""
        if spectral and (window is None or (self.size == 1 and isinstance(window, str))):
            return None
        if isinstance(window, str):
            if window not in _capi.WINDOW_TYPES:
                raise PdspError(_capi.ERR_WINDOW_TYPE, f"Unsupported window type: {window}")
            return None if window == "rect" else self.window(window)
        if isinstance(window, PlanWindow):
            if window._plan is not self:
                raise PdspError(_capi.ERR_BAD_ARG, f"{name} belongs to another plan")
            return window
        if not isinstance(window, torch.Tensor):
            raise PdspError(_capi.ERR_BAD_ARG, f"{name} must be a window type name or a device tensor")
        if window.dim() != 1 or window.shape[0] != self.size:
            raise PdspError(_capi.ERR_WINDOW_LENGTH, "Window length must match input length.")
        operand(window, name, self.device, self.dtype)
        return window

    def _frames(self, frames):
        """frames [..., L], contiguous -> (batch, L, the shape of one output value per frame)."""
        operand(frames, "frames", self.device, self.dtype)
        length = frames.shape[-1]
        return (frames.numel() // length if length else 0), length, tuple(frames.shape[:-1])

    def _signal(self, signal, hop):
        """One contiguous 1-D signal of at least one frame -> (hop, frames)."""
        operand(signal, "signal", self.device, self.dtype, ndim=1)
        if int(hop) < 1:
            raise PdspError(_capi.ERR_BAD_ARG, f"hop must be >= 1, got {hop}")
        if signal.numel() < self.size:
            raise PdspError(_capi.ERR_INPUT_LENGTH,
                            f"signal length {signal.numel()} is shorter than one frame ({self.size})")
        return int(hop), 1 + (signal.numel() - self.size) // int(hop)

    def _bins(self, sides):
        return self.size // 2 + 1 if sides == "one" else self.size

    def _outputs(self, shape, bins, amp, phase, peak):
        """Fresh outputs of the spectrum family: amplitude and phase [..., bins] in the plan's dtype and the int32 peak
        output [..., *peak], each only where asked for (else None)."""
        def new(tail, dtype=self.dtype):
            return torch.empty(shape + tail, dtype=dtype, device=self.device)
        return (new((bins,)) if amp else None, new((bins,)) if phase else None,
                new(peak, torch.int32) if peak is not None else None)

    def spectrum(self, frames: torch.Tensor, window="rect", sides: str = "one", want_phase: bool = False,
                 want_peak: bool = False, out=None):
        """Rows of spectrum()'s body: frames [..., L] (L <= N zero-padded, L > N
        truncated: spectrum.ts:36-43) -> amplitude [..., bins] (+ phase, + peak bin).  There is no in-place form:
        an `out` that shares a byte with `frames` or with a window tensor raises PdspError(ERR_BAD_ARG, "output
        overlaps input (the spectrum has no in-place form)") before anything is launched."""
        batch, length, shape = self._frames(frames)
        bins = self._bins(sides)
        # the amplitude rows are written through a raw pointer: exactly [..., bins], contiguous, on the plan's device
        if out is not None:
            operand(out, "out", self.device, self.dtype, shape=shape + (bins,))
        win = self._table_window(window, spectral=True)
        amp, ph, pk = self._outputs(shape, bins, out is None, want_phase, () if want_peak else None)
        amp = out if out is not None else amp
        check(getattr(lib, "pdsp_spectrum_" + self._sfx)(self._h, batch, _ptr(frames), min(length, self.size), length, _ptr(win),
                                    int(sides != "one"), _ptr(amp), _ptr(ph), _ptr(pk), _stream_ptr(self.device)))
        return amp, ph, pk

    def stft(self, signal: torch.Tensor, hop: int, window="hann", sides: str = "one", want_phase: bool = False,
             want_peak: bool = False):
        """Short-time transform of one contiguous 1-D signal: frame b = signal[b*hop : b*hop + N], the
        body of spectrum() on every frame.  The frames are never materialised -- the kernels read the
        signal with row stride `hop`, so overlapping frames cost no extra HBM footprint.  Returns
        (amplitude [frames, bins], phase or None, peak bin or None)."""
        hop, frames = self._signal(signal, hop)
        win = self._table_window(window, spectral=True)
        amp, ph, pk = self._outputs((frames,), self._bins(sides), True, want_phase, () if want_peak else None)
        check(getattr(lib, "pdsp_spectrum_" + self._sfx)(self._h, frames, _ptr(signal), self.size, hop, _ptr(win),
                                                         int(sides != "one"), _ptr(amp), _ptr(ph), _ptr(pk),
                                                         _stream_ptr(self.device)))
        return amp, ph, pk

    def stft_complex(self, signal: torch.Tensor, hop: int, window="hann"):
        """Complex short-time transform of one contiguous 1-D signal: frame b = signal[b*hop : b*hop + N], the tail
        shorter than a hop ignored (as stft()).  Returns (re, im), each [frames, N/2 + 1]: the one-sided DFT of
        w * frame, unscaled.  One launch; the frames are read in place at row stride `hop`.  64 <= N <= 16384."""
        hop, frames = self._signal(signal, hop)
        win = self._table_window(window)
        re, im, _ = self._outputs((frames,), self.size // 2 + 1, True, True, None)  # two planes [frames, bins]
        check(getattr(lib, "pdsp_stft_complex_" + self._sfx)(self._h, frames, _ptr(signal), self.size, hop, _ptr(win),
                                                             _ptr(re), _ptr(im), _stream_ptr(self.device)))
        return re, im

    def istft(self, re: torch.Tensor, im: torch.Tensor, hop: int, window="hann", out: torch.Tensor | None = None):
        """Weighted overlap-add inverse of complex bins re / im [frames, N/2 + 1] (include/pdsp_hip.h,
        pdsp_istft_*): [(frames - 1) * hop + N] samples, sum_b w y_b / sum_b w^2 over the frames covering each
        sample, 0 where that denominator is <= 1e-11.  Bit-identical from call to call."""
        n = self.size
        for t, name in ((re, "re"), (im, "im")):
            operand(t, name, self.device, self.dtype, ndim=2, last=n // 2 + 1)
        if re.shape != im.shape:
            raise PdspError(_capi.ERR_BAD_ARG, f"re {tuple(re.shape)} and im {tuple(im.shape)} differ in shape")
        frames = re.shape[0]
        if frames < 1:
            raise PdspError(_capi.ERR_BAD_ARG, "frames must be >= 1, got 0")
        if int(hop) < 1:
            raise PdspError(_capi.ERR_BAD_ARG, f"hop must be >= 1, got {hop}")
        win = self._table_window(window)
        total = (frames - 1) * int(hop) + n
        if out is None:
            out = torch.empty((total,), dtype=self.dtype, device=self.device)
        else:
            operand(out, "out", self.device, self.dtype, ndim=1, last=total)
        check(getattr(lib, "pdsp_istft_" + self._sfx)(self._h, frames, _ptr(re), _ptr(im), int(hop), _ptr(win), _ptr(out),
                                                      _stream_ptr(self.device)))
        return out

    def _dct_call(self, x, type, norm, out, name):
        """Validation shared by dct / idct: x [rows, N] with contiguous rows at any row stride >= N (x.stride(0));
        out None, x itself (exact in place) or a tensor of the same shape with its own row stride."""
        n = self.size
        operand(x, f"{name}: x", self.device, self.dtype, ndim=2, last=n, layout="strided")
        if out is not None:
            operand(out, f"{name}: out", self.device, self.dtype, ndim=2, last=n, layout="strided")
        if out is not None and out.shape != x.shape:
            raise PdspError(_capi.ERR_BAD_ARG, f"{name}: out {tuple(out.shape)} and x {tuple(x.shape)} differ in shape")
        if type not in (2, 3):
            raise PdspError(_capi.ERR_BAD_ARG, f"DCT type must be 2 or 3, got {type}")
        if norm is None:
            norm = "backward"
        if norm not in _capi.DCT_NORMS:
            raise PdspError(_capi.ERR_BAD_ARG, f"DCT norm must be 'backward', 'ortho' or 'forward', got {norm!r}")
        rows = x.shape[0]
        if rows < 1:
            raise PdspError(_capi.ERR_BAD_ARG, "batch must be >= 1, got 0")
        if out is None:
            out = torch.empty((rows, n), dtype=self.dtype, device=self.device)
        xs = x.stride(0) if rows > 1 else n
        ys = out.stride(0) if rows > 1 else n
        if out.data_ptr() == x.data_ptr() and rows > 1 and ys != xs:
            raise PdspError(_capi.ERR_BAD_ARG, "output overlaps input (only y == x with y_stride == x_stride may share bytes)")
        if out.data_ptr() == x.data_ptr():
            ys = xs
        check(getattr(lib, "pdsp_dct_" + self._sfx)(self._h, rows, _ptr(x), xs, int(type), _capi.DCT_NORMS[norm],
                                                    _ptr(out), ys, _stream_ptr(self.device)))
        return out

    def dct(self, x: torch.Tensor, type: int = 2, norm: str = "backward", out: torch.Tensor | None = None):
        """scipy dct(x, type, norm=norm, axis=-1) of the rows of x [rows, N] (types 2 and 3; norm "backward",
        "ortho" or "forward"), one launch.  Rows may sit at any stride >= N (x.stride(0)); out=x runs in place.
        64 <= N <= 16384."""
        return self._dct_call(x, type, norm, out, "dct")

    def idct(self, x: torch.Tensor, type: int = 2, norm: str = "backward", out: torch.Tensor | None = None):
        """scipy idct(x, type, norm=norm, axis=-1): the DCT of type 5 - type with backward and forward norms
        exchanged (ortho kept), as dct()."""
        if type not in (2, 3):
            raise PdspError(_capi.ERR_BAD_ARG, f"DCT type must be 2 or 3, got {type}")
        swap = {"backward": "forward", "forward": "backward", None: "forward"}
        return self._dct_call(x, 5 - type, swap.get(norm, norm), out, "idct")

    def _hilbert_call(self, x, mode, out, name):
        """Validation shared by hilbert / hilbert_imag / envelope / instantaneous_phase: x [rows, len <= N] with
        contiguous rows at any row stride (x.stride(0)); out None, a tensor [rows, N] with its own row stride (hilbert:
        complex), or, in the N-out modes, the rows x lies in (exact in place: out begins where x does and has x's row
        stride; x is out itself, or out[:, :len] when len < N)."""
        n = self.size
        analytic = mode == "analytic"
        operand(x, f"{name}: x", self.device, self.dtype, ndim=2, layout="strided")
        rows, ln = x.shape
        if rows < 1:
            raise PdspError(_capi.ERR_BAD_ARG, "batch must be >= 1, got 0")
        if ln < 1 or ln > n:
            raise PdspError(_capi.ERR_BAD_ARG, f"len must be 1 ... N = {n}, got {ln}")
        odt = COMPLEX[self.dtype] if analytic else self.dtype
        k = 2 if analytic else 1  # plan-dtype values per output element
        if out is None:
            out = torch.empty((rows, n), dtype=odt, device=self.device)
        else:
            operand(out, f"{name}: out", self.device, odt, ndim=2, shape=(rows, n), layout="strided")
        xs = x.stride(0) if rows > 1 else max(ln, n)
        ys = k * out.stride(0) if rows > 1 else k * n
        if out.data_ptr() == x.data_ptr() and not analytic:
            if rows > 1 and ys != xs:
                raise PdspError(_capi.ERR_BAD_ARG,
                                "output overlaps input (only y == x with y_stride == x_stride may share bytes)")
            ys = xs
        check(getattr(lib, "pdsp_hilbert_" + self._sfx)(self._h, rows, _ptr(x), xs, ln, _capi.HILBERT_OUT[mode],
                                                        _ptr(out), ys, _stream_ptr(self.device)))
        return out

    def hilbert(self, x: torch.Tensor, out: torch.Tensor | None = None):
        """scipy.signal.hilbert(x, N=self.size, axis=-1): the analytic signal x + i Hx of the rows of x
        [rows, len <= N] (zero-padded to N), a complex tensor [rows, N], one launch.  torch.view_as_real(result) is
        the interleaved buffer the kernel wrote; its real parts are x bit for bit.  Never in place.
        64 <= N <= 16384."""
        return self._hilbert_call(x, "analytic", out, "hilbert")

    def hilbert_imag(self, x: torch.Tensor, out: torch.Tensor | None = None):
        """The Hilbert transform Hx = imag(scipy.signal.hilbert(x, N)) of the rows of x, [rows, N], one launch;
        out=x runs in place (len < N: x = out[:, :len])."""
        return self._hilbert_call(x, "imag", out, "hilbert_imag")

    def envelope(self, x: torch.Tensor, out: torch.Tensor | None = None):
        """abs(scipy.signal.hilbert(x, N)) of the rows of x, [rows, N], one launch; out=x runs in place.  f64 holds
        over its whole range; f32 squares in f32: samples with 1.1e-19 <= |a| <= 1.8e19 (include/pdsp_hip.h)."""
        return self._hilbert_call(x, "envelope", out, "envelope")

    def instantaneous_phase(self, x: torch.Tensor, out: torch.Tensor | None = None):
        """angle(scipy.signal.hilbert(x, N)) of the rows of x in (-pi, pi], not unwrapped, [rows, N], one launch;
        out=x runs in place."""
        return self._hilbert_call(x, "phase", out, "instantaneous_phase")

    def spectrum_peaks(self, frames: torch.Tensor, window="rect", sides: str = "one", sample_rate: float = 1.0,
                       want_amp: bool = False, want_phase: bool = False):
        """Rows of the whole spectrum() tail on the device: one SpectrumPeak per frame
        (findPeak fused into the kernel).  Returns (index int32 [...], frequency, amplitude,
        phase float32 [...], amp-or-None, phase-or-None); with want_amp=False only 16 bytes
        per frame leave the kernel."""
        if self.dtype != torch.float32:
            raise PdspError(_capi.ERR_BAD_ARG, "spectrum_peaks is f32 only (16-byte f32 records)")
        batch, length, shape = self._frames(frames)
        if sample_rate <= 0:
            raise PdspError(_capi.ERR_SAMPLE_RATE, f"Sample rate must be positive, got {js_num(sample_rate)}")
        win = self._table_window(window, spectral=True)
        # rec: pdsp_peak32 records
        amp, ph, rec = self._outputs(shape, self._bins(sides), want_amp or want_phase, want_phase, (4,))
        check(lib.pdsp_spectrum_peaks_f32(self._h, batch, _ptr(frames), min(length, self.size), length, _ptr(win),
                                          int(sides != "one"), float(sample_rate), _ptr(amp), _ptr(ph), _ptr(rec),
                                          _stream_ptr(self.device)))
        f = rec.view(torch.float32)
        return rec[..., 0], f[..., 1], f[..., 2], f[..., 3], amp, ph


# -- stand-alone element-wise device helpers ----------------------------------
# The library reads and writes these operands through raw pointers with no shape of their own, so every operand is
# checked here, before any library call: a CUDA tensor, contiguous, on the device and of the dtype of the first
# operand, with the element count the call reads or writes.

def _check_operand(t, name, like=None, numel=None):
    operand(t, name, like.device if like is not None else None, like.dtype if like is not None else None, numel=numel)


def apply_window(frames: torch.Tensor, window: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    _check_operand(frames, "frames")
    sfx = _device.suffix(frames.dtype, "apply_window")
    _check_operand(window, "window", frames)
    n = frames.shape[-1] if frames.dim() else 1
    if window.numel() != n or window.shape[-1:] != (n,):
        raise PdspError(_capi.ERR_WINDOW_LENGTH, "Window length must match input length.")
    if out is not None:
        _check_operand(out, "out", frames, frames.numel())
    out = torch.empty_like(frames) if out is None else out
    check(getattr(lib, "pdsp_apply_window_" + sfx)(frames.numel() // n if n else 0, n, _ptr(frames), _ptr(window),
                                                   _ptr(out), _stream_ptr(frames.device)))
    return out


def _polar(name, re, im, out):
    _check_operand(re, "re")
    sfx = _device.suffix(re.dtype, name)
    _check_operand(im, "im", re, re.numel())
    if out is not None:
        _check_operand(out, "out", re, re.numel())
    out = torch.empty_like(re) if out is None else out
    check(getattr(lib, f"pdsp_{name}_{sfx}")(re.numel(), _ptr(re), _ptr(im), _ptr(out), _stream_ptr(re.device)))
    return out


def magnitude(re: torch.Tensor, im: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """|re + i im| element-wise (f64: hypot, no overflow or underflow of the squares)."""
    return _polar("magnitude", re, im, out)


def phase(re: torch.Tensor, im: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    return _polar("phase", re, im, out)


# -- element-wise complex vector arithmetic (src/math/complex.ts) on device rows ------
# `out` may be `a`, or a `b` as long as `a` (plane on plane: each element is read before it is written); any other
# overlap, and a broadcast row taken from `out` (X.div((X.re[0], X.im[0])): clone the row first), raises
# PdspError "output overlaps input" (include/pdsp_hip.h).

def _complex_op(name, a, b=None, s_re=0.0, s_im=0.0, out=None):
    are, aim = a
    _check_operand(are, "a.real")
    if are.dtype != torch.float32:
        raise PdspError(_capi.ERR_BAD_ARG, f"complex_{name} is float32 only, got {are.dtype}")
    count = are.numel()
    _check_operand(aim, "a.imag", are, count)
    bre = bim = None
    b_len = 0
    if b is not None:
        bre, bim = b
        _check_operand(bre, "b.real", are)
        b_len = bre.numel()
        _check_operand(bim, "b.imag", are, b_len)
        if (b_len == 0 and count != 0) or (b_len and count % b_len != 0):
            raise PdspError(_capi.ERR_BAD_ARG, f"second operand length {b_len} must divide {count}")
    if out is not None:
        _check_operand(out[0], "out.real", are, count)
        _check_operand(out[1], "out.imag", are, count)
    ore, oim = (torch.empty_like(are), torch.empty_like(aim)) if out is None else out
    check(lib.pdsp_complex_op_f32(_capi.COMPLEX_OPS[name], count, _ptr(are), _ptr(aim), _ptr(bre), _ptr(bim),
                                  b_len, float(s_re), float(s_im), _ptr(ore), _ptr(oim), _stream_ptr(are.device)))
    return ore, oim


def complex_add(a, b, out=None):
    return _complex_op("add", a, b, out=out)


def complex_sub(a, b, out=None):
    return _complex_op("sub", a, b, out=out)


def complex_mul(a, b, out=None):
    """Hadamard product; `b` may be one row broadcast over the rows of `a`."""
    return _complex_op("mul", a, b, out=out)


def complex_div(a, b, out=None):
    return _complex_op("div", a, b, out=out)


def complex_conj(a, out=None):
    return _complex_op("conj", a, out=out)


def complex_scale(a, s, out=None):
    return _complex_op("scale", a, s_re=s, out=out)


def complex_mul_scalar(a, re, im, out=None):
    return _complex_op("mulScalar", a, s_re=re, s_im=im, out=out)


def complex_div_scalar(a, re, im, out=None):
    """complex.ts:176-186: multiply by the reciprocal computed on the host."""
    denom = re * re + im * im
    return _complex_op("mulScalar", a, s_re=re / denom, s_im=-im / denom, out=out)
