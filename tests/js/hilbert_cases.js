'use strict';
// node hilbert_cases.js cases.json out.json: hilbert / envelope / instantaneousPhase of the JS host
// (pragma-dsp_amd/js, `.hilbert`) on each case {op, signal, n, typed}; typed = 'f32' hands the signal in as
// Float32Array, 'f64' as Float64Array, else a plain array; n null is left out of the options.  Writes the values
// ({real, imag} for hilbert) or {error} in order, then the root's Object.keys as the last entry.
const fs = require('fs');
const path = require('path');
const p = require(path.join(__dirname, '..', '..', 'pragma-dsp_amd', 'js'));

const conv = (a, typed) => (typed === 'f32' ? Float32Array.from(a) : typed === 'f64' ? Float64Array.from(a) : a);
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = cases.map((c) => {
  try {
    const opts = {};
    if (c.n !== null) opts.n = c.n;
    const y = p.hilbert[c.op](conv(c.signal, c.typed), opts);
    if (c.op === 'hilbert') {
      if (!(y.real instanceof Float64Array) || !(y.imag instanceof Float64Array)) return { error: 'not Float64Arrays' };
      return { real: Array.from(y.real), imag: Array.from(y.imag) };
    }
    if (!(y instanceof Float64Array)) return { error: 'not a Float64Array' };
    return Array.from(y);
  } catch (e) {
    return { error: e.message };
  }
});
out.push(Object.keys(p));
fs.writeFileSync(process.argv[3], JSON.stringify(out));
