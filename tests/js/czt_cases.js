'use strict';
// node czt_cases.js cases.json out.json: czt / zoomFft of the JS host (pragma-dsp_amd/js, `.czt`) on each case
// {op, real, imag, typed, fn, options}; typed = 'f32' hands the planes in as Float32Array, 'f64' as Float64Array, else
// plain arrays; imag null means a real signal handed in bare, else { real, imag }.  Writes {real, imag} or {error} in
// order, then the root's Object.keys as the last entry.
const { p, conv, runCases } = require('./_cases');

runCases((c) => {
  const x = c.imag === null ? conv(c.real, c.typed) : { real: conv(c.real, c.typed), imag: conv(c.imag, c.typed) };
  const y = c.op === 'zoomFft' ? p.czt.zoomFft(x, c.fn, c.options) : p.czt.czt(x, c.options);
  if (!(y.real instanceof Float64Array) || !(y.imag instanceof Float64Array)) return { error: 'not Float64Arrays' };
  return { real: Array.from(y.real), imag: Array.from(y.imag) };
}, [Object.keys(p)]);
