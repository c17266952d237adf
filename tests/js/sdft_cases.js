'use strict';
// node sdft_cases.js cases.json out.json: slidingDft / goertzel of the JS host (pragma-dsp_amd/js, `.sdft`) on each case
// {op, signal, size, bins, hop, window, typed}; typed = 'f32' hands the signal in as Float32Array, 'f64' as
// Float64Array, else a plain array; hop / window null leave the defaults.  Writes {frames, bins, real, imag} /
// {real, imag} (or {error}) in order, then the root's Object.keys as the last entry.
const fs = require('fs');
const path = require('path');
const p = require(path.join(__dirname, '..', '..', 'pragma-dsp_amd', 'js'));

const conv = (a, typed) => (typed === 'f32' ? Float32Array.from(a) : typed === 'f64' ? Float64Array.from(a) : a);
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = cases.map((c) => {
  try {
    const x = conv(c.signal, c.typed);
    if (c.op === 'goertzel') {
      const g = p.sdft.goertzel(x, c.bins);
      if (!(g.real instanceof Float64Array) || !(g.imag instanceof Float64Array)) return { error: 'not Float64Arrays' };
      return { real: Array.from(g.real), imag: Array.from(g.imag) };
    }
    const r = p.sdft.slidingDft(x, c.size, c.bins, c.hop === null ? undefined : c.hop, c.window === null ? undefined : c.window);
    if (!(r.real instanceof Float64Array) || !(r.imag instanceof Float64Array)) return { error: 'not Float64Arrays' };
    return { frames: r.frames, bins: r.bins, real: Array.from(r.real), imag: Array.from(r.imag) };
  } catch (e) {
    return { error: e.message };
  }
});
out.push(Object.keys(p));
fs.writeFileSync(process.argv[3], JSON.stringify(out));
