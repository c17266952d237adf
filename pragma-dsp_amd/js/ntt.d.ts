// Number-theoretic transform over GF(p), p = 2^64 - 2^32 + 1, on the device: natural order in and out, 64 ... 16384
// points (a power of two); any 64-bit pattern in, canonical values in [0, p) out.
export type Words = BigUint64Array | BigInt64Array | bigint[];
export function ntt(values: Words): BigUint64Array;
export function intt(values: Words): BigUint64Array;
// the linear product mod p of two rows of coefficients: a.length + b.length - 1 <= 16384 values
export function polymul(a: Words, b: Words): BigUint64Array;
export const MODULUS: bigint;
