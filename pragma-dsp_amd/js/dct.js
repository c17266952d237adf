'use strict';
// pragma-dsp/xform/dct (the reference's ROADMAP.md, v0.3: "dct(signal, { type }), idct(...)"; not implemented there
// yet): the discrete cosine transform of types 2 and 3 and its inverses, computed on the device in f64
// (include/pdsp_hip.h, "discrete cosine transform").  Conventions are scipy dct / idct's; norm 'backward'
// (default), 'ortho' or 'forward'.  The signal length is a power of two, 64 ... 16384.
const native = require('./native');
const { dflt, lookup, toF64 } = require('./_util');

const NORMS = { backward: 0, ortho: 1, forward: 2 };
const SWAP = { backward: 'forward', ortho: 'ortho', forward: 'backward' };

function options(opts) {
  const o = opts || {};
  const type = dflt(o.type, 2);
  const norm = dflt(o.norm, 'backward');
  if (type !== 2 && type !== 3) throw new Error('DCT type must be 2 or 3, got ' + type);
  lookup(NORMS, norm, "DCT norm must be 'backward', 'ortho' or 'forward', got " + norm);
  return { type, norm };
}

function run(signal, type, norm) {
  const x = toF64(signal, 'signal');
  const y = new Float64Array(x.length);
  native.dct(type, NORMS[norm], x, y);
  return y;
}

// dct(signal, { type = 2, norm = 'backward' }) -> Float64Array: scipy dct(signal, type, norm=norm)
function dct(signal, opts) {
  const o = options(opts);
  return run(signal, o.type, o.norm);
}

// idct(signal, { type = 2, norm = 'backward' }) -> Float64Array: scipy idct(signal, type, norm=norm), the dct of
// type 5 - type with 'backward' and 'forward' exchanged
function idct(signal, opts) {
  const o = options(opts);
  return run(signal, 5 - o.type, SWAP[o.norm]);
}

module.exports = { dct, idct };
