'use strict';
// node dwt_cases.js cases.json out.json: wavedec / waverec / waveletTaps of the JS host (pragma-dsp_amd/js, `.wavelet`)
// on each case {op, signal, wavelet, levels, typed}; typed = 'f32' hands the arrays in as Float32Array, 'f64' as
// Float64Array, else plain arrays; a wavelet given as an array of taps is converted the same way.  Writes {values} or
// {error} in order, then the root's Object.keys as the last entry.
const { p, conv, runCases } = require('./_cases');

runCases((c) => {
  const wv = Array.isArray(c.wavelet) ? conv(c.wavelet, c.typed === 'f32' ? 'f64' : c.typed) : c.wavelet;
  const y = c.op === 'waveletTaps' ? p.wavelet.waveletTaps(c.wavelet) : p.wavelet[c.op](conv(c.signal, c.typed), wv, c.levels);
  if (!(y instanceof Float64Array)) return { error: 'not a Float64Array' };
  return { values: Array.from(y) };
}, [Object.keys(p)]);
