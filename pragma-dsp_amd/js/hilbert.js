'use strict';
// The Hilbert / analytic signal helpers (the reference's ROADMAP.md, v0.3; not implemented there yet): the analytic
// signal of a real signal, its envelope and its instantaneous phase, computed on the device in f64
// (include/pdsp_hip.h, "Hilbert transform").  Conventions are scipy.signal.hilbert(signal, N = n)'s: the signal is
// zero-padded to n, a power of two, 64 ... 16384 (default: the signal's own length), and every result has n values.
const native = require('./native');
const { dflt, toF64 } = require('./_util');

const MODES = { analytic: 0, imag: 1, envelope: 2, phase: 3 };

function size(x, opts) {
  const o = opts || {};
  const n = dflt(o.n, x.length);
  if (typeof n !== 'number' || !Number.isInteger(n)) throw new Error('n must be an integer, got ' + n);
  return n;
}

function run(signal, opts, mode) {
  const x = toF64(signal, 'signal');
  const n = size(x, opts);
  // a size the library refuses gets no buffer: the library fails before it writes
  const ok = n >= 64 && n <= 16384;
  const y = new Float64Array(ok ? (mode === 'analytic' ? 2 * n : n) : 0);
  native.hilbert(MODES[mode], n, x, y);
  return y;
}

// hilbert(signal, { n }) -> { real, imag }: scipy.signal.hilbert(signal, N = n); real is the zero-padded signal
function hilbert(signal, opts) {
  const y = run(signal, opts, 'analytic');
  const n = y.length / 2;
  const real = new Float64Array(n);
  const imag = new Float64Array(n);
  for (let i = 0; i < n; i++) {
    real[i] = y[2 * i];
    imag[i] = y[2 * i + 1];
  }
  return { real, imag };
}

// envelope(signal, { n }) -> Float64Array: abs(scipy.signal.hilbert(signal, N = n))
function envelope(signal, opts) {
  return run(signal, opts, 'envelope');
}

// instantaneousPhase(signal, { n }) -> Float64Array: angle(scipy.signal.hilbert(signal, N = n)), not unwrapped
function instantaneousPhase(signal, opts) {
  return run(signal, opts, 'phase');
}

module.exports = { hilbert, envelope, instantaneousPhase };
