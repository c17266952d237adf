'use strict';
// node dft_cases.js cases.json out.json: dft / idft of the JS host (pragma-dsp_amd/js, `.dft`) on each case
// {op, real, imag, typed}; typed = 'f32' hands the planes in as Float32Array, 'f64' as Float64Array, else plain
// arrays; imag null is left out of the call.  Writes {real, imag} or {error} in order, then the root's Object.keys as
// the last entry.
const { p, conv, runCases } = require('./_cases');

runCases((c) => {
  const args = [conv(c.real, c.typed)];
  if (c.imag !== null) args.push(conv(c.imag, c.typed));
  const y = p.dft[c.op](...args);
  if (!(y.real instanceof Float64Array) || !(y.imag instanceof Float64Array)) return { error: 'not Float64Arrays' };
  return { real: Array.from(y.real), imag: Array.from(y.imag) };
}, [Object.keys(p)]);
