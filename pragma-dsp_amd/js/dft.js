'use strict';
// The discrete Fourier transform of a signal of ANY length, 2 ... 4096 (not only the powers of two of core.Radix2Fft),
// computed on the device in f64 by Bluestein's chirp-z algorithm (include/pdsp_hip.h, "any-length DFT").  Conventions
// are numpy's fft / ifft: X[k] = sum_n x[n] exp(-2 pi i n k / L), no scaling forward, 1 / L on the inverse.
const native = require('./native');
const { toF64 } = require('./_util');

function run(inverse, real, imag) {
  const re = toF64(real, 'real');
  const im = imag === undefined || imag === null ? null : toF64(imag, 'imag');
  if (im && im.length !== re.length) throw new Error('real and imag must have the same length, got ' + re.length + ' and ' + im.length);
  // a length the library refuses gets no buffers: the library fails before it writes
  const n = re.length >= 2 && re.length <= 4096 ? re.length : 0;
  const out = { real: new Float64Array(n), imag: new Float64Array(n) };
  native.dft(inverse, re, im, out.real, out.imag);
  return out;
}

// dft(real, imag?) -> { real, imag }: the forward transform; imag left out means a real signal
function dft(real, imag) {
  return run(0, real, imag);
}

// idft(real, imag) -> { real, imag }: the inverse transform, scaled by 1 / L
function idft(real, imag) {
  if (imag === undefined || imag === null) throw new TypeError('imag must be an array or a typed array');
  return run(1, real, imag);
}

module.exports = { dft, idft };
