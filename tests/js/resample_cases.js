'use strict';
// node resample_cases.js cases.json out.json: resamplePoly / upfirdn / designResampleTaps of the JS host
// (pragma-dsp_amd/js, `.filters`) on each case {op, signal, up, down, taps, typed}; typed = 'f32' hands the signal
// in as Float32Array, 'f64' as Float64Array, else a plain array; taps null is left out; up / down null are left out
// of upfirdn (its defaults).  Writes the values or {error} in order, then the root's Object.keys as the last entry.
const { p, conv, runCases } = require('./_cases');

runCases((c) => {
  let y;
  if (c.op === 'designResampleTaps') y = p.filters.designResampleTaps(c.up, c.down);
  else if (c.op === 'resamplePoly') {
    y = c.taps === null ? p.filters.resamplePoly(conv(c.signal, c.typed), c.up, c.down)
      : p.filters.resamplePoly(conv(c.signal, c.typed), c.up, c.down, c.taps);
  } else {
    y = c.up === null ? p.filters.upfirdn(c.taps, conv(c.signal, c.typed))
      : p.filters.upfirdn(c.taps, conv(c.signal, c.typed), c.up, c.down);
  }
  if (!(y instanceof Float64Array)) return { error: 'not a Float64Array' };
  return Array.from(y);
}, [Object.keys(p)]);
