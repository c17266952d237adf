'use strict';
// The rate-change half of pragma-dsp/filters (the reference's ROADMAP.md, "Filters and utilities": "resampling to a
// uniform grid", "windowed-sinc filter design helpers"; no implementation there yet).  The root export lists these
// under `.filters`, beside firFilter (index.js).
const native = require('./native');
const { looseF64 } = require('./_util');

// Polyphase rate change in f64 (include/pdsp_hip.h, "polyphase rate change"): scipy.signal.resample_poly's and
// scipy.signal.upfirdn's definitions, one time-domain launch on the device per call.
function ratio(up, down) {
  for (const [name, v] of [['up', up], ['down', down]]) {
    if (!Number.isSafeInteger(v)) throw new Error(name + ' must be an integer, got ' + v);
  }
}

// designResampleTaps(up, down): the filter resamplePoly convolves with by default -- a Kaiser (beta = 5) windowed
// sinc of 20 max(up, down) + 1 taps, times up, after up and down are divided by their gcd.
function designResampleTaps(up, down) {
  ratio(up, down);
  const out = new Float64Array(native.resampleDesign(up, down, new Float64Array(0)));
  native.resampleDesign(up, down, out);
  return out;
}

// resamplePoly(signal, up, down, taps?): scipy.signal.resample_poly(signal, up, down, window=taps), padtype
// "constant": ceil(len up / down) outputs.
function resamplePoly(signal, up, down, taps) {
  ratio(up, down);
  const given = taps !== undefined && taps !== null;
  const h = given ? looseF64(taps) : new Float64Array(0);
  if (given && h.length < 1) {
    throw new Error('filter must have at least one tap, got 0');
  }
  const n = up >= 1 && down >= 1 && up <= 8192 && down <= 8192 ? Math.ceil((signal.length * up) / down) : 0;
  const out = new Float64Array(n);
  native.resamplePoly(looseF64(signal), up, down, h, out);
  return out;
}

// upfirdn(h, signal, up = 1, down = 1): scipy.signal.upfirdn(h, signal, up, down), the full output of
// floor(((len - 1) up + ntaps - 1) / down) + 1 samples.
function upfirdn(h, signal, up, down) {
  up = up === undefined ? 1 : up;
  down = down === undefined ? 1 : down;
  ratio(up, down);
  const ok = up >= 1 && down >= 1 && up <= 8192 && down <= 8192 && signal.length >= 1 && h.length >= 1 && h.length <= 8192;
  const out = new Float64Array(ok ? Math.floor(((signal.length - 1) * up + h.length - 1) / down) + 1 : 0);
  native.upfirdn(looseF64(h), looseF64(signal), up, down, out);
  return out;
}

module.exports = { resamplePoly, upfirdn, designResampleTaps };
