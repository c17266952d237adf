'use strict';
// node ntt_cases.js cases.json out.json: ntt / intt / polymul of the JS host (pragma-dsp_amd/js, `.ntt`) on each case
// {op, a, b, typed}; the 64-bit values travel as decimal strings.  typed = 'u64' hands the rows in as BigUint64Array,
// 'i64' as BigInt64Array (the same bits), else arrays of BigInt; `raw` cases hand `a` over as it stands (error paths).
// Writes {values} (decimal strings) or {error} in order, then the root's Object.keys and the modulus as the last entries.
const { p, runCases } = require('./_cases');

const conv = (a, typed) => {
  const v = a.map((s) => BigInt(s));
  if (typed === 'u64') return BigUint64Array.from(v);
  if (typed === 'i64') return BigInt64Array.from(v, (x) => BigInt.asIntN(64, x));
  return v;
};

runCases((c) => {
  const a = c.raw ? c.a : conv(c.a, c.typed);
  const y = c.op === 'polymul' ? p.ntt.polymul(a, conv(c.b, c.typed)) : p.ntt[c.op](a);
  if (!(y instanceof BigUint64Array)) return { error: 'not a BigUint64Array' };
  return { values: Array.from(y, (v) => v.toString()) };
}, [Object.keys(p), p.ntt.MODULUS.toString()]);
