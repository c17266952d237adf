'use strict';
// node stft_cases.js cases.json out.json: stft / istft of the JS host (pragma-dsp_amd/js, `.stft`) on each case
// {op, signal | frames/real/imag, fftSize, hopSize, window, typed}; typed = 'f32' hands the arrays in as Float32Array,
// 'f64' as Float64Array, else plain arrays.  Writes {frames, bins, real, imag} / the samples (or {error}) in order.
const fs = require('fs');
const path = require('path');
const p = require(path.join(__dirname, '..', '..', 'pragma-dsp_amd', 'js'));

const conv = (a, typed) => (typed === 'f32' ? Float32Array.from(a) : typed === 'f64' ? Float64Array.from(a) : a);
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = cases.map((c) => {
  try {
    const opts = { fftSize: c.fftSize, hopSize: c.hopSize };
    if (c.window !== null) opts.window = c.window;
    if (c.op === 'stft') {
      const r = p.stft.stft(conv(c.signal, c.typed), opts);
      return { frames: r.frames, bins: r.bins, real: Array.from(r.real), imag: Array.from(r.imag) };
    }
    return Array.from(p.stft.istft({ frames: c.frames, real: conv(c.real, c.typed), imag: conv(c.imag, c.typed) }, opts));
  } catch (e) {
    return { error: e.message };
  }
});
fs.writeFileSync(process.argv[3], JSON.stringify(out));
