'use strict';
// pragma-dsp/xform/stft (the reference's ROADMAP.md, "A) STFT"; not implemented there yet): the short-time transform
// with complex output and its weighted overlap-add inverse, computed on the device in f64 (include/pdsp_hip.h,
// "short-time transform").  Frame b is signal[b*hopSize, b*hopSize + fftSize); its bins are unscaled,
// X[k] = sum_n w[n] x[n] e^{-2 pi i k n / N}, k = 0 ... N/2.  64 <= fftSize <= 16384.
const native = require('./native');
const { dflt, toF64, windowId } = require('./_util');

function options(opts) {
  const o = opts || {};
  const window = windowId(dflt(o.window, 'hann'));
  const fftSize = o.fftSize, hopSize = o.hopSize;
  if (!Number.isInteger(fftSize)) throw new Error('fftSize must be an integer, got ' + fftSize);
  if (!Number.isInteger(hopSize)) throw new Error('hopSize must be an integer, got ' + hopSize);
  // sizes the library refuses go to it with empty outputs: it fails before touching them, with its own message
  const ok = fftSize >= 64 && fftSize <= 16384 && hopSize >= 1;
  return { fftSize, hopSize, window, ok };
}

// stft(signal, { fftSize, hopSize, window = 'hann' }) -> { frames, bins, real, imag }, real / imag row-major
// [frames][bins] Float64Arrays, frames = 1 + floor((signal.length - fftSize) / hopSize) (the tail is ignored).
function stft(signal, opts) {
  const o = options(opts);
  const x = toF64(signal, 'signal');
  const ok = o.ok && x.length >= o.fftSize;
  const frames = ok ? 1 + Math.floor((x.length - o.fftSize) / o.hopSize) : 0;
  const bins = o.fftSize / 2 + 1;
  const real = new Float64Array(ok ? frames * bins : 0), imag = new Float64Array(ok ? frames * bins : 0);
  native.stft(x, o.fftSize, o.hopSize, o.window, real, imag);
  return { frames, bins, real, imag };
}

// istft({ frames, real, imag }, { fftSize, hopSize, window = 'hann' }) -> Float64Array of
// (frames - 1) * hopSize + fftSize samples: sum_b w y_b / sum_b w^2 over the frames covering each sample, y_b the
// inverse real transform of frame b's bins, and 0 where the denominator is <= 1e-11.
function istft(spec, opts) {
  const o = options(opts);
  const s = spec || {};
  const frames = s.frames;
  if (!Number.isInteger(frames) || frames < 1) throw new Error('frames must be an integer >= 1, got ' + frames);
  const re = toF64(s.real, 'real'), im = toF64(s.imag, 'imag');
  if (o.ok) {
    const want = frames * (o.fftSize / 2 + 1);
    if (re.length !== want || im.length !== want) {
      throw new Error('real and imag must hold frames * (fftSize/2 + 1) = ' + want + ' values, got ' + re.length +
        ' and ' + im.length);
    }
  }
  const total = (frames - 1) * o.hopSize + o.fftSize;
  const out = new Float64Array(o.ok && total <= 2 ** 32 ? total : 0);
  native.istft(re, im, frames, o.fftSize, o.hopSize, o.window, out);
  return out;
}

module.exports = { stft, istft };
