'use strict';
// node filters_cases.js cases.json out.json: firFilter of the JS host (pragma-dsp_amd/js, `.filters`) on each case
// {signal, taps, mode, typed}; typed = 'f32' hands both arrays in as Float32Array, 'f64' as Float64Array, else plain
// arrays.  Writes the outputs (or {error}) in order.
const { p, conv, runCases } = require('./_cases');

runCases((c) => {
  const opts = c.mode === null ? undefined : { mode: c.mode };
  return Array.from(p.filters.firFilter(conv(c.signal, c.typed), conv(c.taps, c.typed), opts));
});
