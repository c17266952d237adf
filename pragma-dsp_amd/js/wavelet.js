'use strict';
// The multi-level discrete wavelet transform of one signal, computed on the device in f64 (include/pdsp_hip.h,
// "multi-level discrete wavelet transform"): orthogonal wavelets, periodic extension, so n samples give n coefficients
// in the Mallat layout [cA_J | cD_J | ... | cD_1].  With h the scaling filter of even length F and
// g[j] = (-1)^j h[F - 1 - j], one level on a row a of even length m is
//   cA[k] = sum_j h[j] a[(2k + j) mod m],   cD[k] = sum_j g[j] a[(2k + j) mod m],   0 <= k < m / 2,
// and the inverse is its transpose.  `wavelet` is 'haar', 'db1' ... 'db10', or an array of taps (even length 2 ... 32,
// orthonormal to 1e-10); the signal's length must be a multiple of 2^levels.
const native = require('./native');
const { toF64 } = require('./_util');

function run(mode, signal, wavelet, levels) {
  const x = toF64(signal, 'signal');
  if (typeof levels !== 'number' || !Number.isInteger(levels)) throw new TypeError('levels must be an integer');
  const named = typeof wavelet === 'string';
  const taps = named ? null : toF64(wavelet, 'wavelet');
  const y = new Float64Array(x.length);
  native.dwt(mode, named ? wavelet : null, taps, levels, x, y);
  return y;
}

// wavedec(signal, wavelet, levels) -> Float64Array of signal.length coefficients
function wavedec(signal, wavelet, levels) {
  return run(0, signal, wavelet, levels);
}

// waverec(coeffs, wavelet, levels) -> Float64Array of coeffs.length samples
function waverec(coeffs, wavelet, levels) {
  return run(1, coeffs, wavelet, levels);
}

// waveletTaps(name) -> the scaling filter of a built-in wavelet (sum sqrt 2)
function waveletTaps(name) {
  if (typeof name !== 'string') throw new TypeError('wavelet name must be a string');
  const none = new Float64Array(0);
  const n = native.dwt(2, name, null, 1, none, none);
  const h = new Float64Array(n);
  native.dwt(2, name, null, 1, none, h);
  return h;
}

module.exports = { wavedec, waverec, waveletTaps };
