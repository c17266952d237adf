'use strict';
// node dct_cases.js cases.json out.json: dct / idct of the JS host (pragma-dsp_amd/js, `.dct`) on each case
// {op, signal, type, norm, typed}; typed = 'f32' hands the signal in as Float32Array, 'f64' as Float64Array, else a
// plain array; type / norm null are left out of the options.  Writes the values (or {error}) in order, then the
// root's Object.keys as the last entry.
const { p, conv, runCases } = require('./_cases');

runCases((c) => {
  const opts = {};
  if (c.type !== null) opts.type = c.type;
  if (c.norm !== null) opts.norm = c.norm;
  const y = p.dct[c.op](conv(c.signal, c.typed), opts);
  if (!(y instanceof Float64Array)) return { error: 'not a Float64Array' };
  return Array.from(y);
}, [Object.keys(p)]);
