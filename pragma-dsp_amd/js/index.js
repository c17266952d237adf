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
// The modules below are ones the reference only plans (ROADMAP.md) or extensions beside it.  Each is reachable under
// its name but not enumerated, so that the key list of the reference's three surfaces stays exactly theirs.
const hidden = [
  // pragma-dsp/filters (ROADMAP.md, "Filters and utilities")
  ['filters', {
    firFilter: filters.firFilter,
    resamplePoly: resample.resamplePoly,
    upfirdn: resample.upfirdn,
    designResampleTaps: resample.designResampleTaps,
  }],
  // pragma-dsp/xform/stft (ROADMAP.md, "A) STFT")
  ['stft', { stft: stft.stft, istft: stft.istft }],
  // pragma-dsp/xform/dct (ROADMAP.md, v0.3)
  ['dct', { dct: dct.dct, idct: dct.idct }],
  // Hilbert / analytic signal helpers (ROADMAP.md, v0.3)
  ['hilbert', { hilbert: hilbert.hilbert, envelope: hilbert.envelope, instantaneousPhase: hilbert.instantaneousPhase }],
  // any-length DFT: an extension beside the reference's power-of-two Radix2Fft
  ['dft', { dft: dft.dft, idft: dft.idft }],
  // wavelets (ROADMAP.md, item E)
  ['wavelet', { wavedec: wavelet.wavedec, waverec: wavelet.waverec, waveletTaps: wavelet.waveletTaps }],
  // chirp-z transform and zoom FFT: an extension beside the any-length DFT
  ['czt', { czt: czt.czt, zoomFft: czt.zoomFft }],
  // number-theoretic transform (ROADMAP.md, item F)
  ['ntt', { ntt: ntt.ntt, intt: ntt.intt, polymul: ntt.polymul, MODULUS: ntt.MODULUS }],
  // sliding DFT (ROADMAP.md, item B)
  ['sdft', { slidingDft: sdft.slidingDft, goertzel: sdft.goertzel }],
];
for (const [name, value] of hidden) Object.defineProperty(module.exports, name, { value, enumerable: false });
