'use strict';
// node stft_cases.js cases.json out.json: stft / istft of the JS host (pragma-dsp_amd/js, `.stft`) on each case
// {op, signal | frames/real/imag, fftSize, hopSize, window, typed}; typed = 'f32' hands the arrays in as Float32Array,
// 'f64' as Float64Array, else plain arrays.  Writes {frames, bins, real, imag} / the samples (or {error}) in order.
const { p, conv, runCases } = require('./_cases');

runCases((c) => {
  const opts = { fftSize: c.fftSize, hopSize: c.hopSize };
  if (c.window !== null) opts.window = c.window;
  if (c.op === 'stft') {
    const r = p.stft.stft(conv(c.signal, c.typed), opts);
    return { frames: r.frames, bins: r.bins, real: Array.from(r.real), imag: Array.from(r.imag) };
  }
  return Array.from(p.stft.istft({ frames: c.frames, real: conv(c.real, c.typed), imag: conv(c.imag, c.typed) }, opts));
});
