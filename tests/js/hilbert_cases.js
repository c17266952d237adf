'use strict';
// node hilbert_cases.js cases.json out.json: hilbert / envelope / instantaneousPhase of the JS host
// (pragma-dsp_amd/js, `.hilbert`) on each case {op, signal, n, typed}; typed = 'f32' hands the signal in as
// Float32Array, 'f64' as Float64Array, else a plain array; n null is left out of the options.  Writes the values
// ({real, imag} for hilbert) or {error} in order, then the root's Object.keys as the last entry.
const { p, conv, runCases } = require('./_cases');

runCases((c) => {
  const opts = {};
  if (c.n !== null) opts.n = c.n;
  const y = p.hilbert[c.op](conv(c.signal, c.typed), opts);
  if (c.op === 'hilbert') {
    if (!(y.real instanceof Float64Array) || !(y.imag instanceof Float64Array)) return { error: 'not Float64Arrays' };
    return { real: Array.from(y.real), imag: Array.from(y.imag) };
  }
  if (!(y instanceof Float64Array)) return { error: 'not a Float64Array' };
  return Array.from(y);
}, [Object.keys(p)]);
