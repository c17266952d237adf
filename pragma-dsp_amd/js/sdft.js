'use strict';
// pragma-dsp/xform/sdft (the reference's ROADMAP.md, "B) Sliding DFT"; not implemented there yet): chosen bins of a
// window of `size` samples at every hop-th start, computed on the device in f64 (include/pdsp_hip.h, "sliding DFT").
// Frame m is signal[m*hop, m*hop + size); bin b of it is Y = sum_n w[n] x[n] e^{-2 pi i b n / size}, unscaled, with b
// in cycles per window: fractional, negative and >= size all allowed.  2 <= size <= 16384 (any integer), 1 ... 256 bins.
const native = require('./native');
const { dflt, toF64, windowId } = require('./_util');

// slidingDft(signal, size, bins, hop = 1, window = 'rect') -> { frames, bins, real, imag }, real / imag row-major
// [bins][frames] Float64Arrays (time fastest), frames = 1 + floor((signal.length - size) / hop).
function slidingDft(signal, size, bins, hop, window) {
  const h = dflt(hop, 1);
  const w = windowId(dflt(window, 'rect'));
  if (!Number.isInteger(size)) throw new Error('size must be an integer, got ' + size);
  if (!Number.isInteger(h)) throw new Error('hop must be an integer, got ' + h);
  const x = toF64(signal, 'signal');
  const b = toF64(typeof bins === 'number' ? [bins] : bins, 'bins');
  // sizes the library refuses go to it with empty outputs: it fails before touching them, with its own message
  const ok = size >= 2 && size <= 16384 && h >= 1 && x.length >= size && b.length >= 1 && b.length <= 256;
  const frames = ok ? 1 + Math.floor((x.length - size) / h) : 0;
  const real = new Float64Array(frames * b.length), imag = new Float64Array(frames * b.length);
  native.sdft(x, size, b, h, w, real, imag);
  return { frames, bins: b.length, real, imag };
}

// goertzel(signal, bins) -> { real, imag } of bins.length values: the bins of the one frame that is the whole signal
// (size = signal.length, rectangular), Goertzel's use case.
function goertzel(signal, bins) {
  const x = toF64(signal, 'signal');
  const y = slidingDft(x, x.length, bins, 1, 'rect');
  return { real: y.real, imag: y.imag };
}

module.exports = { slidingDft, goertzel };
