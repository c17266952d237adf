'use strict';
// Export map mirroring the three reference surfaces that sit on the hot path:
//   require('.../js')            -> { spectrum }            (pragma-dsp)
//   require('.../js').core       -> pragma-dsp/core
//   require('.../js').fourier    -> pragma-dsp/xform/fourier
//   require('.../js').filters    -> pragma-dsp/filters (ROADMAP.md, "Filters and utilities")
//   require('.../js').stft       -> pragma-dsp/xform/stft (ROADMAP.md, "A) STFT")
//   require('.../js').dct        -> pragma-dsp/xform/dct (ROADMAP.md, v0.3)
//   require('.../js').hilbert    -> the Hilbert / analytic signal helpers (ROADMAP.md, v0.3)
//   require('.../js').dft        -> the DFT of any length 2 ... 4096 (an extension: the reference has powers of two only)
//   require('.../js').wavelet    -> the multi-level wavelet transform (ROADMAP.md, "E) Wavelets")
//   require('.../js').czt        -> the chirp-z transform and zoom FFT (an extension: scipy.signal.czt / zoom_fft)
//   require('.../js').ntt        -> the number-theoretic transform and exact products (ROADMAP.md, "F) NTT")
//   require('.../js').sdft       -> the sliding DFT: chosen bins at every hop (ROADMAP.md, "B) Sliding DFT")
const core = require('./core');
const fourier = require('./fourier');
const s = require('./spectrum');
const filters = require('./filters');
const stft = require('./stft');
const dct = require('./dct');
const hilbert = require('./hilbert');
const resample = require('./resample');
const dft = require('./dft');
const wavelet = require('./wavelet');
const czt = require('./czt');
const ntt = require('./ntt');
const sdft = require('./sdft');

module.exports = {
  spectrum: s.spectrum,
  spectrumBatch: s.spectrumBatch,  // extension: spectrumStream's map as one device batch
  spectrumStream: s.spectrumStream,  // extension: the same, frame at a time over any iterable (batched inside)
  core: {
    createComplexArray: core.createComplexArray,
    isPowerOfTwo: core.isPowerOfTwo,
    nextPowerOfTwo: core.nextPowerOfTwo,
    Radix2Fft: core.Radix2Fft,
  },
  fourier: {
    createWindow: fourier.createWindow,
    applyWindow: fourier.applyWindow,
    FFT: fourier.FFT,
    magnitude: fourier.magnitude,
    phase: fourier.phase,
    fftShift: fourier.fftShift,
    fftShiftComplex: fourier.fftShiftComplex,
    binFrequencies: fourier.binFrequencies,
  },
};
// pragma-dsp/filters: a module the reference only plans (ROADMAP.md, "Filters and utilities").  Reachable as
// `.filters` but not enumerated, so that the key list of the reference's three surfaces stays exactly theirs.
Object.defineProperty(module.exports, 'filters', {
  value: {
    firFilter: filters.firFilter,
    resamplePoly: resample.resamplePoly,
    upfirdn: resample.upfirdn,
    designResampleTaps: resample.designResampleTaps,
  },
  enumerable: false,
});
// pragma-dsp/xform/stft: planned by the reference (ROADMAP.md, "A) STFT"), not enumerated for the same reason.
Object.defineProperty(module.exports, 'stft', {
  value: { stft: stft.stft, istft: stft.istft },
  enumerable: false,
});
// pragma-dsp/xform/dct: planned by the reference (ROADMAP.md, v0.3), not enumerated for the same reason.
Object.defineProperty(module.exports, 'dct', {
  value: { dct: dct.dct, idct: dct.idct },
  enumerable: false,
});
// Hilbert / analytic signal helpers: planned by the reference (ROADMAP.md, v0.3), not enumerated for the same reason.
Object.defineProperty(module.exports, 'hilbert', {
  value: { hilbert: hilbert.hilbert, envelope: hilbert.envelope, instantaneousPhase: hilbert.instantaneousPhase },
  enumerable: false,
});
// Any-length DFT: an extension beside the reference's power-of-two Radix2Fft, not enumerated for the same reason.
Object.defineProperty(module.exports, 'dft', {
  value: { dft: dft.dft, idft: dft.idft },
  enumerable: false,
});
// Wavelets: planned by the reference (ROADMAP.md, item E), not enumerated for the same reason.
Object.defineProperty(module.exports, 'wavelet', {
  value: { wavedec: wavelet.wavedec, waverec: wavelet.waverec, waveletTaps: wavelet.waveletTaps },
  enumerable: false,
});
// Chirp-z transform and zoom FFT: an extension beside the any-length DFT, not enumerated for the same reason.
Object.defineProperty(module.exports, 'czt', {
  value: { czt: czt.czt, zoomFft: czt.zoomFft },
  enumerable: false,
});
// Number-theoretic transform: planned by the reference (ROADMAP.md, item F), not enumerated for the same reason.
Object.defineProperty(module.exports, 'ntt', {
  value: { ntt: ntt.ntt, intt: ntt.intt, polymul: ntt.polymul, MODULUS: ntt.MODULUS },
  enumerable: false,
});
// Sliding DFT: planned by the reference (ROADMAP.md, item B), not enumerated for the same reason.
Object.defineProperty(module.exports, 'sdft', {
  value: { slidingDft: sdft.slidingDft, goertzel: sdft.goertzel },
  enumerable: false,
});
