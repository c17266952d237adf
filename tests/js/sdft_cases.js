'use strict';
// node sdft_cases.js cases.json out.json: slidingDft / goertzel of the JS host (pragma-dsp_amd/js, `.sdft`) on each case
// {op, signal, size, bins, hop, window, typed}; typed = 'f32' hands the signal in as Float32Array, 'f64' as
// Float64Array, else a plain array; hop / window null leave the defaults.  Writes {frames, bins, real, imag} /
// {real, imag} (or {error}) in order, then the root's Object.keys as the last entry.
const { p, conv, runCases } = require('./_cases');

runCases((c) => {
  const x = conv(c.signal, c.typed);
  if (c.op === 'goertzel') {
    const g = p.sdft.goertzel(x, c.bins);
    if (!(g.real instanceof Float64Array) || !(g.imag instanceof Float64Array)) return { error: 'not Float64Arrays' };
    return { real: Array.from(g.real), imag: Array.from(g.imag) };
  }
  const r = p.sdft.slidingDft(x, c.size, c.bins, c.hop === null ? undefined : c.hop, c.window === null ? undefined : c.window);
  if (!(r.real instanceof Float64Array) || !(r.imag instanceof Float64Array)) return { error: 'not Float64Arrays' };
  return { frames: r.frames, bins: r.bins, real: Array.from(r.real), imag: Array.from(r.imag) };
}, [Object.keys(p)]);
