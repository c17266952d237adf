'use strict';
// What the modules of this directory share: private (not exported from index.js, no .d.ts).  Node-12 compatible, so
// the first two stand in for `??` and for a checked table lookup.

// v ?? d
function dflt(v, d) {
  return v === undefined || v === null ? d : v;
}

// table[key] for an own key of the table; anything else throws new Error(text)
function lookup(table, key, text) {
  if (!Object.prototype.hasOwnProperty.call(table, key)) throw new Error(text);
  return table[key];
}

// the pdsp_window ids of include/pdsp_hip.h by the reference's window names (fourier.ts:14-52)
const WINDOW_IDS = { rect: 0, hann: 1, hamming: 2, blackman: 3 };
function windowId(type) {
  return lookup(WINDOW_IDS, type, 'Unsupported window type: ' + type);
}

// plain arrays or typed arrays only: nothing else reaches the addon
function toF64(a, name) {
  if (a instanceof Float64Array) return a;
  if (Array.isArray(a) || (ArrayBuffer.isView(a) && !(a instanceof DataView))) return Float64Array.from(a);
  throw new TypeError(name + ' must be an array or a typed array');
}

// the loose form of filters / resample: any iterable or array-like that Float64Array.from takes
function looseF64(a) {
  return a instanceof Float64Array ? a : Float64Array.from(a);
}

module.exports = { dflt, lookup, WINDOW_IDS, windowId, toF64, looseF64 };
