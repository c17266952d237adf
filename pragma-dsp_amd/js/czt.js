'use strict';
// The chirp-z transform and the zoom FFT of a signal (scipy.signal.czt / zoom_fft), computed on the device in f64
// (include/pdsp_hip.h, "chirp-z transform"): m points of the z-transform of L samples on an arc of a circle,
//   X[k] = sum_n x[n] a^-n w^(n k),  w = exp(-2 pi i step),  a = radius exp(2 pi i start),  L + m - 1 <= 8192,
// with step and start in TURNS (the tables' phases are formed exactly from these doubles).  There is no inverse.
const native = require('./native');
const { toF64 } = require('./_util');

function num(v, name, dflt) {
  if (v === undefined || v === null) return dflt;
  if (typeof v !== 'number') throw new TypeError(name + ' must be a number');
  return v;
}

// x: a real signal (array / typed array) or a complex one, { real, imag }
function planes(x) {
  if (x !== null && typeof x === 'object' && !Array.isArray(x) && !ArrayBuffer.isView(x) && 'real' in x) {
    const re = toF64(x.real, 'real');
    const im = x.imag === undefined || x.imag === null ? null : toF64(x.imag, 'imag');
    if (im && im.length !== re.length) throw new Error('real and imag must have the same length, got ' + re.length + ' and ' + im.length);
    return [re, im];
  }
  return [toF64(x, 'x'), null];
}

function run(re, im, m, step, start, radius) {
  if (!Number.isInteger(m)) throw new TypeError('m must be an integer');
  // sizes the library refuses get no buffers: the library fails before it writes
  const n = re.length >= 1 && m >= 1 && re.length + m - 1 <= 8192 ? m : 0;
  const out = { real: new Float64Array(n), imag: new Float64Array(n) };
  native.czt(m, step, start, radius, re, im, out.real, out.imag);
  return out;
}

// czt(x, { m, step, start, radius }?) -> { real, imag } of m points (default: x's length) from a = radius
// exp(2 pi i start) (default 1) in steps of w = exp(-2 pi i step) (default step 1 / m: the DFT)
function czt(x, options) {
  const o = options || {};
  const [re, im] = planes(x);
  const m = num(o.m, 'm', re.length);
  return run(re, im, m, num(o.step, 'step', m >= 1 ? 1 / m : 0), num(o.start, 'start', 0), num(o.radius, 'radius', 1));
}

// zoomFft(x, fn, { m, fs, endpoint }?) -> { real, imag } of m points (default: x's length) of the band fn = [f1, f2]
// (a number: [0, fn]) of a signal sampled at fs (default 2)
function zoomFft(x, fn, options) {
  const o = options || {};
  const [re, im] = planes(x);
  const m = num(o.m, 'm', re.length);
  const fs = num(o.fs, 'fs', 2);
  let f1 = 0;
  let f2 = fn;
  if (Array.isArray(fn) || ArrayBuffer.isView(fn)) {
    if (fn.length !== 2) throw new Error('fn must be a number or a pair [f1, f2]');
    [f1, f2] = fn;
  }
  if (typeof f1 !== 'number' || typeof f2 !== 'number') throw new TypeError('fn must be a number or a pair [f1, f2]');
  const div = fs * (o.endpoint ? m - 1 : m);
  if (!Number.isFinite(fs) || fs === 0 || (div === 0 && f2 !== f1 && m >= 1)) throw new Error('fs must be finite and non-zero (and m > 1 with endpoint)');
  return run(re, im, m, div ? (f2 - f1) / div : 0, f1 / fs, 1);
}

module.exports = { czt, zoomFft };
