'use strict';
// pragma-dsp/filters (the module the reference's ROADMAP.md names under "Filters and utilities"; the reference has
// no implementation yet): FIR filtering as linear convolution, computed on the device by one fused overlap-save
// launch (include/pdsp_hip.h, "FIR filtering") in f64.
const native = require('./native');
const { dflt, lookup, looseF64 } = require('./_util');

const MODES = { full: 0, same: 1, valid: 2, filter: 3 };

// firFilter(signal, taps, { mode }): "full" | "same" | "valid" as numpy.convolve, "filter" = the first
// signal.length outputs (scipy.signal.lfilter(taps, 1, signal)). 
function firFilter(signal, taps, options) {
  const opts = options || {};
  const mode = dflt(opts.mode, 'full');
  const id = lookup(MODES, mode, 'Unsupported FIR mode: ' + mode);
  const len = signal.length, p = taps.length;
  if (len < 1 || p < 1) {
    throw new Error('signal and filter must not be empty (len ' + len + ', ntaps ' + p + ')');
  }
  const n = mode === 'full' ? len + p - 1 : mode === 'same' ? Math.max(len, p)
    : mode === 'valid' ? Math.abs(len - p) + 1 : len;
  const out = new Float64Array(n);
  native.firFilter(looseF64(signal), looseF64(taps), id, out);
  return out;
}

module.exports = { firFilter };
