"""pragma-dsp_amd -- MI355X (gfx950) engine behind pragma-dsp's spectrum(),
FFT.forward() and Radix2Fft surface.

Host mirror of the reference's three export surfaces that sit on the hot path
(`pragma-dsp/core`, `pragma-dsp/xform/fourier`, `pragma-dsp`), all computing on
the GPU through the C ABI of include/pdsp_hip.h.  Import as `pragma_dsp_amd`
(the repo-root shim maps the hyphenated directory name to a module name).
"""
from ._capi import LIB_PATH, PdspError, lib  # noqa: F401  (fails loudly if the .so is missing)
from .core import ComplexArray, Radix2Fft, createComplexArray, isPowerOfTwo, nextPowerOfTwo  # noqa: F401
from .fourier import (  # noqa: F401
    FFT,
    applyWindow,
    binFrequencies,
    createWindow,
    fftShift,
    fftShiftComplex,
    magnitude,
    phase,
)
from .filters import FirFilter, fir_filter, firFilter  # noqa: F401
from .spectrum import SpectrumPeak, SpectrumResult, spectrum, spectrumBatch  # noqa: F401
from .stft import istft, stft  # noqa: F401
from .dct import dct, idct  # noqa: F401
from .hilbert import envelope, hilbert, instantaneous_phase  # noqa: F401
from .dft import Dft, dft, idft  # noqa: F401
from .czt import Czt, czt, czt_points, zoom_fft  # noqa: F401
from .resample import (  # noqa: F401
    Resampler,
    Upfirdn,
    design_taps,
    resample_poly,
    resamplePoly,
    upfirdn,
    upfirdnHost,
)
from .wavelet import Dwt, wavedec, wavedecHost, wavelet_taps, waverec, waverecHost  # noqa: F401
from .ntt import NTT_MODULUS, Ntt, convolve_exact, intt, ntt, ntt_mul, ntt_root, polymul  # noqa: F401
from .sdft import SlidingDft, goertzel, sliding_dft  # noqa: F401
from .fft2d import Fft2d, fft2, ifft2  # noqa: F401

__all__ = [
    "ComplexArray", "Radix2Fft", "createComplexArray", "isPowerOfTwo", "nextPowerOfTwo",
    "FFT", "applyWindow", "binFrequencies", "createWindow", "fftShift", "fftShiftComplex",
    "magnitude", "phase", "spectrum", "spectrumBatch", "SpectrumPeak", "SpectrumResult", "PdspError",
    "FirFilter", "fir_filter", "firFilter", "stft", "istft", "dct", "idct",
    "hilbert", "envelope", "instantaneous_phase", "Dft", "dft", "idft",
    "Czt", "czt", "zoom_fft", "czt_points",
    "Resampler", "Upfirdn", "resample_poly", "upfirdn", "resamplePoly", "upfirdnHost", "design_taps",
    "Dwt", "wavedec", "waverec", "wavedecHost", "waverecHost", "wavelet_taps",
    "Ntt", "ntt_mul", "ntt", "intt", "polymul", "convolve_exact", "NTT_MODULUS", "ntt_root",
    "SlidingDft", "sliding_dft", "goertzel",
    "Fft2d", "fft2", "ifft2",
]
