'use strict';
// The number-theoretic transform over GF(p), p = 2^64 - 2^32 + 1, computed on the device (include/pdsp_hip.h,
// "number-theoretic transform"): X[k] = sum_n x[n] w^(n k) mod p with w = 7^((p - 1) / N), natural order in and out,
// N = 2^k, 64 <= N <= 16384.  An element is a 64-bit word: any pattern goes in (taken mod p), a canonical value in
// [0, p) comes out, and nothing is rounded.  Arrays are BigUint64Array, or arrays of BigInt.
const native = require('./native');

const MODULUS = 0xffffffff00000001n;
const MIN_SIZE = 64;
const MAX_SIZE = 16384;

// BigUint64Array, BigInt64Array (the same bits) or an array of BigInt: nothing else reaches the addon
function toU64(a, name) {
  if (a instanceof BigUint64Array) return a;
  if (a instanceof BigInt64Array) return new BigUint64Array(a.buffer, a.byteOffset, a.length);
  if (Array.isArray(a) && a.every((v) => typeof v === 'bigint')) return BigUint64Array.from(a, (v) => BigInt.asUintN(64, v));
  throw new TypeError(name + ' must be a BigUint64Array, a BigInt64Array or an array of BigInt');
}

function run(inverse, values) {
  const x = toU64(values, 'values');
  const y = new BigUint64Array(x.length);
  native.ntt(inverse, x, null, x.length, y);
  return y;
}

// ntt(values) -> BigUint64Array, the transform of values.length points
function ntt(values) {
  return run(0, values);
}

// intt(values) -> BigUint64Array: intt(ntt(x)) is x mod p
function intt(values) {
  return run(1, values);
}

// polymul(a, b) -> the a.length + b.length - 1 coefficients of the product mod p, on the transform of the next power
// of two >= that length, at least 64
function polymul(a, b) {
  const x = toU64(a, 'a');
  const h = toU64(b, 'b');
  const len = x.length + h.length - 1;
  if (x.length < 1 || h.length < 1 || len > MAX_SIZE) {
    throw new RangeError(`the product of ${x.length} and ${h.length} coefficients needs a transform of 1 ... ${MAX_SIZE} points`);
  }
  let n = MIN_SIZE;
  while (n < len) n *= 2;
  const y = new BigUint64Array(len);
  native.ntt(2, x, h, n, y);
  return y;
}

module.exports = { ntt, intt, polymul, MODULUS };
