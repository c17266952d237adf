'use strict';
// node filters_cases.js cases.json out.json: firFilter of the JS host (pragma-dsp_amd/js, `.filters`) on each case
// {signal, taps, mode, typed}; typed = 'f32' hands both arrays in as Float32Array, 'f64' as Float64Array, else plain
// arrays.  Writes the outputs (or {error}) in order.
const fs = require('fs');
const path = require('path');
const p = require(path.join(__dirname, '..', '..', 'pragma-dsp_amd', 'js'));

const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = cases.map((c) => {
  try {
    const conv = c.typed === 'f32' ? Float32Array.from : c.typed === 'f64' ? Float64Array.from : (a) => a;
    const opts = c.mode === null ? undefined : { mode: c.mode };
    return Array.from(p.filters.firFilter(conv.call(c.typed === 'f32' ? Float32Array : Float64Array, c.signal),
      conv.call(c.typed === 'f32' ? Float32Array : Float64Array, c.taps), opts));
  } catch (e) {
    return { error: e.message };
  }
});
fs.writeFileSync(process.argv[3], JSON.stringify(out));
