'use strict';
// node czt_cases.js cases.json out.json: czt / zoomFft of the JS host (pragma-dsp_amd/js, `.czt`) on each case
// {op, real, imag, typed, fn, options}; typed = 'f32' hands the planes in as Float32Array, 'f64' as Float64Array, else
// plain arrays; imag null means a real signal handed in bare, else { real, imag }.  Writes {real, imag} or {error} in
// order, then the root's Object.keys as the last entry.
const fs = require('fs');
const path = require('path');
const p = require(path.join(__dirname, '..', '..', 'pragma-dsp_amd', 'js'));

const conv = (a, typed) => (typed === 'f32' ? Float32Array.from(a) : typed === 'f64' ? Float64Array.from(a) : a);
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = cases.map((c) => {
  try {
    const x = c.imag === null ? conv(c.real, c.typed) : { real: conv(c.real, c.typed), imag: conv(c.imag, c.typed) };
    const y = c.op === 'zoomFft' ? p.czt.zoomFft(x, c.fn, c.options) : p.czt.czt(x, c.options);
    if (!(y.real instanceof Float64Array) || !(y.imag instanceof Float64Array)) return { error: 'not Float64Arrays' };
    return { real: Array.from(y.real), imag: Array.from(y.imag) };
  } catch (e) {
    return { error: e.message };
  }
});
out.push(Object.keys(p));
fs.writeFileSync(process.argv[3], JSON.stringify(out));
