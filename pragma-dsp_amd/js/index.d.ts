// Export map of the host module: the three reference surfaces that sit on the hot path.
import * as coreNs from './core';
import * as fourierNs from './fourier';
import * as filtersNs from './filters';
import * as resampleNs from './resample';
import * as stftNs from './stft';
import * as dctNs from './dct';
import * as hilbertNs from './hilbert';
import * as dftNs from './dft';
import * as waveletNs from './wavelet';
import * as cztNs from './czt';
import * as nttNs from './ntt';
import * as sdftNs from './sdft';

export { spectrum, spectrumBatch, spectrumStream, SpectrumOptions, SpectrumPeak, SpectrumResult } from './spectrum';
export { ComplexArray } from './core';
export { WindowType } from './fourier';
export { FirMode, FirFilterOptions } from './filters';
export { StftWindow, StftOptions, StftResult } from './stft';
export { DctType, DctNorm, DctOptions } from './dct';
export { HilbertOptions, AnalyticSignal } from './hilbert';
export { DftResult } from './dft';
export { CztInput, CztOptions, ZoomFftOptions, CztResult } from './czt';
export { Words } from './ntt';
export { SdftWindow, SlidingDftResult, GoertzelResult } from './sdft';

export const core: {
  createComplexArray: typeof coreNs.createComplexArray;
  isPowerOfTwo: typeof coreNs.isPowerOfTwo;
  nextPowerOfTwo: typeof coreNs.nextPowerOfTwo;
  Radix2Fft: typeof coreNs.Radix2Fft;
};
export const fourier: {
  createWindow: typeof fourierNs.createWindow;
  applyWindow: typeof fourierNs.applyWindow;
  FFT: typeof fourierNs.FFT;
  magnitude: typeof fourierNs.magnitude;
  phase: typeof fourierNs.phase;
  fftShift: typeof fourierNs.fftShift;
  fftShiftComplex: typeof fourierNs.fftShiftComplex;
  binFrequencies: typeof fourierNs.binFrequencies;
};
export const filters: {
  firFilter: typeof filtersNs.firFilter;
  resamplePoly: typeof resampleNs.resamplePoly;
  upfirdn: typeof resampleNs.upfirdn;
  designResampleTaps: typeof resampleNs.designResampleTaps;
};
export const stft: {
  stft: typeof stftNs.stft;
  istft: typeof stftNs.istft;
};
export const dct: {
  dct: typeof dctNs.dct;
  idct: typeof dctNs.idct;
};
export const hilbert: {
  hilbert: typeof hilbertNs.hilbert;
  envelope: typeof hilbertNs.envelope;
  instantaneousPhase: typeof hilbertNs.instantaneousPhase;
};
export const dft: {
  dft: typeof dftNs.dft;
  idft: typeof dftNs.idft;
};
export const wavelet: {
  wavedec: typeof waveletNs.wavedec;
  waverec: typeof waveletNs.waverec;
  waveletTaps: typeof waveletNs.waveletTaps;
};
export const czt: {
  czt: typeof cztNs.czt;
  zoomFft: typeof cztNs.zoomFft;
};
export const ntt: {
  ntt: typeof nttNs.ntt;
  intt: typeof nttNs.intt;
  polymul: typeof nttNs.polymul;
  MODULUS: typeof nttNs.MODULUS;
};
export const sdft: {
  slidingDft: typeof sdftNs.slidingDft;
  goertzel: typeof sdftNs.goertzel;
};
