'use strict';
// node native_cases.js <addon>: the argument handling of every export of the N-API addon, driven directly (no JS host)
// and printed as one JSON log of [list, export, name, kind, value, wantKind, wantValue] rows, kind 'ok' | 'throws'.
// tests/test_js_native_cpu.py compares the two halves of each row.  Lists:
//   'pinned'   outcomes that do not depend on a device: a throw the addon raises itself or one a library check raises
//              ahead of its device check, or a value a host-only call returns;
//   'planned'  the same for the exports whose first argument is a plan: creating one needs a device, so these rows
//              run only where planCreate succeeds (the log's last entry says whether it did);
//   'changed'  the rows whose outcome the shared argument reader changed on purpose, (a) to (e) below.
const native = require(process.argv[2]);
const { MessageChannel } = require('worker_threads');

const log = [];
let list = 'pinned';
const show = (r) => (r === undefined ? null : typeof r === 'bigint' ? String(r) : r);
function run(exp, name, fn, wantKind, want) {
  let kind = 'ok', value;
  try { value = show(fn()); } catch (e) { kind = 'throws'; value = (e instanceof TypeError ? 'TypeError: ' : '') + e.message; }
  log.push([list, exp, name, kind, value, wantKind, want]);
}
const throws = (exp, name, fn, text) => run(exp, name, fn, 'throws', text);
const gives = (exp, name, fn, value) => run(exp, name, fn, 'ok', value);

const f = (n) => new Float64Array(n);
const u = (n) => new BigUint64Array(n);
const ARITY = 'TypeError: pdsp_napi: wrong number of arguments';
const NUMBER = 'TypeError: pdsp_napi: expected a number';
const F64 = 'TypeError: pdsp_napi: expected a Float64Array';
const U64 = 'TypeError: pdsp_napi: expected a BigUint64Array';
const F64_OR_F32 = 'TypeError: pdsp_napi: expected a Float64Array or a Float32Array';

// ---- every export's parameters: n = number, a = Float64Array, u = BigUint64Array, s = optional string; the sample
// arguments are well-formed values of each kind, so a row that replaces one of them fails on that one alone ---------
const SIGNATURES = {
  planCreate: ['n', () => [64]],
  windowMake: ['nna', () => [1, 8, f(8)]],
  applyWindow: ['aaa', () => [f(4), f(4), f(4)]],
  magnitude: ['aaa', () => [f(4), f(4), f(4)]],
  phase: ['aaa', () => [f(4), f(4), f(4)]],
  spectrum: ['annnnaaa', () => [f(8), 48000, -1, 0, 0, f(5), f(5), f(5)]],
  spectrumBatch: ['annnnnnaaaa', () => [f(16), 2, 8, 48000, -1, 0, 0, f(5), f(10), f(10), f(8)]],
  spectrumRows: ['-nnnnnnnaaaa', () => [[f(8), f(8)], 0, 2, 8, 48000, -1, 0, 0, f(5), f(10), f(10), f(8)]],
  binFrequencies: ['nnna', () => [8, 48000, 0, f(5)]],
  fftShift: ['aa', () => [f(5), f(5)]],
  nextPow2: ['n', () => [5]],
  firFilter: ['aana', () => [f(8), f(3), 0, f(10)]],
  resamplePoly: ['annaa', () => [f(8), 2, 1, f(0), f(16)]],
  upfirdn: ['aanna', () => [f(3), f(8), 2, 1, f(17)]],
  resampleDesign: ['nna', () => [2, 1, f(0)]],
  stft: ['annnaa', () => [f(128), 64, 32, 1, f(99), f(99)]],
  istft: ['aannnna', () => [f(99), f(99), 3, 64, 32, 1, f(128)]],
  dct: ['nnaa', () => [2, 0, f(64), f(64)]],
  hilbert: ['nnaa', () => [1, 64, f(64), f(64)]],
  dft: ['naaaa', () => [0, f(12), f(12), f(12), f(12)]],
  czt: ['nnnnaaaa', () => [8, 0.125, 0, 1, f(4), f(4), f(8), f(8)]],
  dwt: ['nsanaa', () => [0, 'haar', null, 1, f(8), f(8)]],
  ntt: ['nuunu', () => [0, u(64), null, 64, u(64)]],
  sdft: ['anannaa', () => [f(16), 8, f(2), 1, 0, f(18), f(18)]],
};
const WRONG = { n: ['a string', 'x', NUMBER], a: ['a plain array', [1, 2, 3], F64], u: ['a plain array', [1n, 2n], U64],
                s: ['a number', 7, 'TypeError: pdsp_napi: expected a string'] };
function signatureRows(exp, kinds, sample, from) {
  throws(exp, 'too few arguments', () => native[exp](...sample().slice(0, kinds.length - 1)), ARITY);
  for (let i = from; i < kinds.length; i++) {
    if (!WRONG[kinds[i]]) continue;
    const [what, bad, text] = WRONG[kinds[i]];
    throws(exp, 'argument ' + i + ' ' + what, () => { const v = sample(); v[i] = bad; return native[exp](...v); }, text);
  }
}
for (const exp of Object.keys(SIGNATURES)) signatureRows(exp, SIGNATURES[exp][0], SIGNATURES[exp][1], 0);
gives('deviceCount', 'a number', () => typeof native.deviceCount(), 'number');

// ---- the addon's own refusals, letter for letter ---------------------------------------------------------------------
const outs = (bins, batch) => [f(bins), f(batch * bins), f(batch * bins), f(4 * batch)];
const rowsArgs = (frames, start, batch, o) => [frames, start, batch, 8, 48000, -1, 0, 0, ...(o || outs(5, batch))];
throws('windowMake', 'short out', () => native.windowMake(1, 64, f(8)), 'pdsp_napi: window output too small');
throws('windowMake', 'null out', () => native.windowMake(1, 64, null), 'pdsp_napi: window output too small');
throws('applyWindow', 'short out', () => native.applyWindow(f(4), f(4), f(3)), 'pdsp_napi: applyWindow output too small');
throws('magnitude', 'short imag', () => native.magnitude(f(8), f(4), f(8)), 'pdsp_napi: magnitude/phase planes too small');
throws('phase', 'short out', () => native.phase(f(8), f(8), f(4)), 'pdsp_napi: magnitude/phase planes too small');
throws('spectrum', 'short freq', () => native.spectrum(f(8), 48000, -1, 0, 0, f(2), f(5), f(5)), 'pdsp_napi: spectrum outputs too small');
throws('spectrum', 'two-sided short phase', () => native.spectrum(f(8), 48000, 8, 0, 1, f(8), f(8), f(5)), 'pdsp_napi: spectrum outputs too small');
throws('spectrumBatch', 'short frames', () => native.spectrumBatch(f(15), 2, 8, 48000, -1, 0, 0, ...outs(5, 2)), 'pdsp_napi: spectrumBatch frames buffer too small');
throws('spectrumBatch', 'negative batch', () => native.spectrumBatch(f(16), -1, 8, 48000, -1, 0, 0, ...outs(5, 2)), 'pdsp_napi: spectrumBatch frames buffer too small');
throws('spectrumBatch', 'short amplitude', () => native.spectrumBatch(f(16), 2, 8, 48000, -1, 0, 0, f(5), f(5), f(10), f(8)), 'pdsp_napi: spectrumBatch outputs too small');
throws('spectrumBatch', 'short peaks', () => native.spectrumBatch(f(16), 2, 8, 48000, -1, 0, 0, f(5), f(10), f(10), f(7)), 'pdsp_napi: spectrumBatch outputs too small');
throws('spectrumRows', 'not an array', () => native.spectrumRows(...rowsArgs(f(8), 0, 1)), 'TypeError: pdsp_napi: spectrumRows expects an array of Float64Arrays');
throws('spectrumRows', 'range past the end', () => native.spectrumRows(...rowsArgs([f(8), f(8)], 1, 2)), 'pdsp_napi: spectrumRows frame range out of bounds');
throws('spectrumRows', 'negative start', () => native.spectrumRows(...rowsArgs([f(8), f(8)], -1, 2)), 'pdsp_napi: spectrumRows frame range out of bounds');
throws('spectrumRows', 'short peaks', () => native.spectrumRows(...rowsArgs([f(8), f(8)], 0, 2, [f(5), f(10), f(10), f(7)])), 'pdsp_napi: spectrumRows outputs too small');
throws('spectrumRows', 'ragged frame', () => native.spectrumRows(...rowsArgs([f(8), f(4)], 0, 2)), 'pdsp_napi: spectrumRows frames must all have frameLen samples');
throws('spectrumRows', 'mixed kinds', () => native.spectrumRows(...rowsArgs([f(8), new Float32Array(8)], 0, 2)), 'TypeError: pdsp_napi: spectrumRows frames must all be of one typed-array kind');
throws('spectrumRows', 'plain-array frame', () => native.spectrumRows(...rowsArgs([f(8), [0, 1, 0, -1, 0, 1, 0, -1]], 0, 2)), F64_OR_F32);
throws('spectrumRows', 'Int32Array frame', () => native.spectrumRows(...rowsArgs([new Int32Array(8)], 0, 1)), F64_OR_F32);
throws('spectrumRows', 'hole', () => native.spectrumRows(...rowsArgs([f(8), , f(8)], 0, 3)), F64_OR_F32);
throws('spectrumRows', 'getter that throws', () => { const fr = [f(8), f(8)]; Object.defineProperty(fr, 1, { get() { throw new RangeError('from the getter'); } }); return native.spectrumRows(...rowsArgs(fr, 0, 2)); }, 'from the getter');
throws('binFrequencies', 'short out', () => native.binFrequencies(8, 48000, 0, f(4)), 'pdsp_napi: binFrequencies output too small');
throws('binFrequencies', 'two-sided short out', () => native.binFrequencies(8, 48000, 1, f(5)), 'pdsp_napi: binFrequencies output too small');
throws('fftShift', 'short out', () => native.fftShift(f(5), f(2)), 'pdsp_napi: fftShift output too small');
throws('firFilter', 'short out', () => native.firFilter(f(8), f(3), 0, f(9)), 'pdsp_napi: firFilter output too small');
throws('resamplePoly', 'short out', () => native.resamplePoly(f(8), 3, 2, f(0), f(11)), 'pdsp_napi: resamplePoly output too small');
throws('upfirdn', 'short out', () => native.upfirdn(f(3), f(8), 2, 1, f(16)), 'pdsp_napi: upfirdn output too small');
throws('resampleDesign', 'short out', () => native.resampleDesign(2, 1, f(40)), 'pdsp_napi: resampleDesign output too small');
throws('stft', 'short real', () => native.stft(f(128), 64, 32, 1, f(98), f(99)), 'pdsp_napi: stft output too small');
throws('istft', 'short imag', () => native.istft(f(99), f(98), 3, 64, 32, 1, f(128)), 'pdsp_napi: istft buffers too small');
throws('istft', 'short out', () => native.istft(f(99), f(99), 3, 64, 32, 1, f(127)), 'pdsp_napi: istft buffers too small');
throws('sdft', 'short imag', () => native.sdft(f(16), 8, f(2), 1, 0, f(18), f(17)), 'pdsp_napi: sdft output too small');
throws('dct', 'short out', () => native.dct(2, 0, f(64), f(63)), 'pdsp_napi: dct output too small');
throws('hilbert', 'short out', () => native.hilbert(1, 64, f(64), f(63)), 'pdsp_napi: hilbert output too small');
throws('hilbert', 'analytic needs 2 n', () => native.hilbert(0, 64, f(64), f(127)), 'pdsp_napi: hilbert output too small');
throws('dft', 'lengths differ', () => native.dft(0, f(12), f(11), f(12), f(12)), 'pdsp_napi: dft real and imag lengths differ');
throws('dft', 'short out', () => native.dft(0, f(12), null, f(12), f(11)), 'pdsp_napi: dft output too small');
throws('czt', 'lengths differ', () => native.czt(8, 0.125, 0, 1, f(4), f(3), f(8), f(8)), 'pdsp_napi: czt real and imag lengths differ');
throws('czt', 'short out', () => native.czt(8, 0.125, 0, 1, f(4), null, f(8), f(7)), 'pdsp_napi: czt output too small');
throws('dwt', 'short out', () => native.dwt(0, 'haar', null, 1, f(8), f(7)), 'pdsp_napi: dwt output too small');
throws('dwt', 'short taps out', () => native.dwt(2, 'db2', null, 1, f(0), f(3)), 'pdsp_napi: dwt output too small');
throws('ntt', 'length differs', () => native.ntt(0, u(64), null, 128, u(128)), 'pdsp_napi: ntt input length differs from the size');
throws('ntt', 'short out', () => native.ntt(1, u(64), null, 64, u(63)), 'pdsp_napi: ntt output too small');

// ---- library refusals: raised by a check the host entry point makes before it asks for a device, and handed on unchanged
throws('planCreate', 'size 12', () => native.planCreate(12), 'FFT size must be power of two, got 12');
throws('planCreate', 'size 0', () => native.planCreate(0), 'FFT size must be power of two, got 0');
throws('windowMake', 'size 0', () => native.windowMake(1, 0, f(8)), 'Window size must be positive, got 0');
throws('windowMake', 'type 9', () => native.windowMake(9, 8, f(8)), 'Unsupported window type: 9');
throws('applyWindow', 'length mismatch', () => native.applyWindow(f(3), f(2), f(3)), 'Window length must match input length.');
throws('spectrum', 'size 12', () => native.spectrum(f(8), 48000, 12, 0, 0, f(7), f(7), f(7)), 'FFT size must be power of two, got 12');
throws('spectrum', 'window 7', () => native.spectrum(f(8), 48000, -1, 7, 0, f(5), f(5), f(5)), 'Unsupported window type: 7');
throws('spectrum', 'sides 2', () => native.spectrum(f(8), 48000, -1, 0, 2, f(8), f(8), f(8)), 'bad sides 2');
throws('spectrumBatch', 'rate 0', () => native.spectrumBatch(f(16), 2, 8, 0, -1, 0, 0, ...outs(5, 2)), 'Sample rate must be positive, got 0');
throws('spectrumRows', 'size 12', () => native.spectrumRows([f(8), f(8)], 0, 2, 8, 48000, 12, 0, 0, ...outs(7, 2)), 'FFT size must be power of two, got 12');
throws('spectrumRows', 'rate 0', () => native.spectrumRows([f(8), f(8)], 0, 2, 8, 0, -1, 0, 0, ...outs(5, 2)), 'Sample rate must be positive, got 0');
throws('binFrequencies', 'size 0', () => native.binFrequencies(0, 48000, 0, f(5)), 'FFT size must be positive, got 0');
throws('binFrequencies', 'rate -1', () => native.binFrequencies(8, -1, 0, f(5)), 'Sample rate must be positive, got -1');
throws('firFilter', 'empty taps', () => native.firFilter(f(8), f(0), 0, f(8)), 'signal and filter must not be empty (len 8, ntaps 0)');
throws('firFilter', 'mode 9', () => native.firFilter(f(8), f(3), 9, f(10)), 'unknown FIR mode 9');
throws('resamplePoly', 'up 0', () => native.resamplePoly(f(8), 0, 1, f(0), f(8)), 'up and down must be >= 1, got up 0, down 1');
throws('upfirdn', 'down 9000', () => native.upfirdn(f(3), f(8), 1, 9000, f(8)), 'up and down must be <= 8192, got up 1, down 9000');
throws('resampleDesign', 'down 0', () => native.resampleDesign(2, 0, f(0)), 'up and down must be >= 1, got up 2, down 0');
throws('stft', 'size 12', () => native.stft(f(128), 12, 32, 1, f(0), f(0)), 'FFT size must be power of two, got 12');
throws('stft', 'hop 0', () => native.stft(f(128), 64, 0, 1, f(0), f(0)), 'hop must be >= 1, got 0');
throws('stft', 'short signal', () => native.stft(f(32), 64, 32, 1, f(0), f(0)), 'signal length 32 is shorter than one frame (64)');
throws('istft', 'size 32', () => native.istft(f(0), f(0), 3, 32, 32, 1, f(0)), 'STFT needs a plan of 64 <= N <= 16384, got 32');
throws('istft', 'frames 0', () => native.istft(f(0), f(0), 0, 64, 32, 1, f(0)), 'frames must be >= 1, got 0');
throws('istft', 'an extent past 2^40', () => native.istft(f(0), f(0), 2 ** 30, 16384, 16384, 1, f(0)), 'frames 1073741824 x hop 16384 overflows');
throws('sdft', 'window 5', () => native.sdft(f(16), 8, f(2), 1, 5, f(18), f(18)), 'Unsupported window type: 5');
throws('dct', '12 values', () => native.dct(2, 0, f(12), f(12)), 'FFT size must be power of two, got 12');
throws('dct', 'type 4', () => native.dct(4, 0, f(64), f(64)), 'DCT type must be 2 or 3, got 4');
throws('dct', 'type past int', () => native.dct(2 ** 32 + 2, 0, f(64), f(64)), 'DCT type must be 2 or 3, got 0');
throws('dct', 'norm past int', () => native.dct(2, 2 ** 32, f(64), f(64)), 'DCT norm must be 0 (backward), 1 (ortho) or 2 (forward), got -1');
throws('hilbert', 'n 32', () => native.hilbert(1, 32, f(32), f(32)), 'the Hilbert transform needs a plan of 64 <= N <= 16384, got 32');
throws('hilbert', 'mode past int', () => native.hilbert(2 ** 32 + 1, 64, f(64), f(64)), 'Hilbert output must be 0 (analytic), 1 (imag), 2 (envelope) or 3 (phase), got -1');
throws('hilbert', 'signal longer than n', () => native.hilbert(1, 64, f(65), f(64)), 'len must be 1 ... N = 64, got 65');
throws('dft', 'one value', () => native.dft(0, f(1), null, f(1), f(1)), 'DFT length must be 2 ... 4096, got 1');
throws('czt', 'bins 0', () => native.czt(0, 0.125, 0, 1, f(4), null, f(0), f(0)), 'CZT bins must be >= 1, got 0');
throws('czt', 'radius 0', () => native.czt(8, 0.125, 0, 0, f(4), null, f(8), f(8)), 'CZT radius must be finite and > 0, got 0');
throws('dwt', 'unknown wavelet', () => native.dwt(2, 'sym4', null, 1, f(0), f(0)), 'unknown wavelet "sym4" (haar, db1 ... db10)');
throws('dwt', 'levels past int', () => native.dwt(0, 'haar', null, 2 ** 32 + 1, f(8), f(8)), 'levels must be >= 1, got 0');
throws('dwt', 'length no multiple of 2^levels', () => native.dwt(0, 'haar', null, 2, f(6), f(6)), 'len must be a positive multiple of 2^levels (levels = 2), got 6');
throws('ntt', '100 values', () => native.ntt(0, u(100), null, 100, u(100)), 'NTT size must be power of two, got 100');
throws('ntt', 'product size 100', () => native.ntt(2, u(8), u(8), 100, u(15)), 'NTT size must be power of two, got 100');
throws('sdft', 'size 1', () => native.sdft(f(16), 1, f(2), 1, 0, f(0), f(0)), 'sliding DFT window length must be 2 ... 16384, got 1');
throws('sdft', '257 bins', () => native.sdft(f(16), 8, f(257), 1, 0, f(0), f(0)), 'sliding DFT bins must be 1 ... 256, got 257');

// ---- host-only values ---------------------------------------------------------------------------------------------
gives('windowMake', 'blackman 64, sample 1', () => { const w = f(64); native.windowMake(3, 64, w); return w[1]; }, 0.0008984113451827869);
gives('windowMake', 'size 1 ignores the type', () => { const w = f(1); native.windowMake(9, 1, w); return w[0]; }, 1);
gives('nextPow2', 'values', () => [0, 1, 5, 1025, 2 ** 31 + 5].map(native.nextPow2).join(','), '1,1,8,2048,4294967296');
gives('binFrequencies', 'one-sided', () => { const o = f(5); native.binFrequencies(8, 48000, 0, o); return o.join(','); }, '0,6000,12000,18000,24000');
gives('binFrequencies', 'two-sided', () => { const o = f(8); native.binFrequencies(8, 48000, 1, o); return o.join(','); }, '0,6000,12000,18000,24000,30000,36000,42000');
gives('fftShift', 'odd length', () => { const o = f(5); native.fftShift(Float64Array.from([0, 1, 2, 3, 4]), o); return o.join(','); }, '2,3,4,0,1');
gives('applyWindow', 'empty', () => native.applyWindow(f(0), f(0), f(0)), null);
gives('magnitude', 'empty', () => native.magnitude(f(0), f(0), f(0)), null);
gives('resampleDesign', 'tap count 3 / 2', () => native.resampleDesign(3, 2, f(0)), 61);
gives('resampleDesign', 'taps 3 / 2: count, centre', () => { const h = f(61); return [native.resampleDesign(3, 2, h), h[30] > 0.9 && h[30] === Math.max(...h), h[0] === h[60]].join(','); }, '61,true,true');
gives('dwt', 'mode 2: db2 tap count', () => native.dwt(2, 'db2', null, 1, f(0), f(0)), 4);
gives('dwt', 'mode 2: db2 taps sum to sqrt 2', () => { const h = f(4); const n = native.dwt(2, 'db2', null, 1, f(0), h); return [n, Math.abs(h[0] + h[1] + h[2] + h[3] - Math.SQRT2) < 1e-15].join(','); }, '4,true');
gives('dwt', 'mode 2: haar', () => { const h = f(2); native.dwt(2, 'haar', null, 1, f(0), h); return h.join(','); }, [Math.SQRT1_2, Math.SQRT1_2].join(','));

// ---- exports that take a plan: only where one can be made ------------------------------------------------------------
list = 'planned';
let plan = null;
try { plan = native.planCreate(8); } catch (e) { plan = null; }
if (plan !== null) {
  const PLANNED = {
    transform: ['-aaaa-', () => [plan, f(8), f(8), f(8), f(8), false]],
    transformBatch: ['-naaaa-', () => [plan, 2, f(16), f(16), f(16), f(16), false]],
    transformRows: ['---aa-', () => [plan, [f(8), f(8)], false, f(16), f(16), false]],
  };
  for (const exp of Object.keys(PLANNED)) signatureRows(exp, PLANNED[exp][0], PLANNED[exp][1], 1);
  const rows = (inputs, complex, inverse, n) => [plan, inputs, complex, f(n), f(n), inverse];
  throws('transform', 'short real', () => native.transform(plan, f(3), null, f(8), f(8), false), 'FFT input length 3 != size 8');
  throws('transform', 'short imag', () => native.transform(plan, f(8), f(5), f(8), f(8), false), 'FFT input length 5 != size 8');
  throws('transform', 'short out', () => native.transform(plan, f(8), null, f(8), f(7), false), "pdsp_napi: output planes must have the plan's size");
  throws('transformBatch', 'negative batch', () => native.transformBatch(plan, -1, f(16), null, f(16), f(16), false), 'pdsp_napi: transformBatch bad batch');
  throws('transformBatch', 'batch 2^60', () => native.transformBatch(plan, 2 ** 60, f(16), null, f(16), f(16), false), 'pdsp_napi: transformBatch bad batch');
  throws('transformBatch', 'short plane', () => native.transformBatch(plan, 2, f(16), null, f(16), f(15), false), 'pdsp_napi: transformBatch planes must hold batch * size values');
  throws('transformBatch', 'inverse of real rows', () => native.transformBatch(plan, 2, f(16), null, f(16), f(16), true), 'pdsp_napi: transformBatch inverse needs an imaginary plane');
  throws('transformRows', 'not an array', () => native.transformRows(...rows(f(8), false, false, 8)), 'TypeError: pdsp_napi: transformRows expects an array of rows');
  throws('transformRows', 'short out', () => native.transformRows(...rows([f(8), f(8)], false, false, 15)), 'pdsp_napi: transformRows output planes must hold rows * size values');
  throws('transformRows', 'inverse of real rows', () => native.transformRows(...rows([f(8)], false, true, 8)), 'pdsp_napi: transformRows inverse needs complex rows');
  throws('transformRows', 'a number for a pair', () => native.transformRows(...rows([7], true, false, 8)), 'TypeError: pdsp_napi: transformRows expects { real, imag } rows');
  throws('transformRows', 'short row', () => native.transformRows(...rows([f(8), f(4)], false, false, 16)), "pdsp_napi: transformRows rows must be Float64Arrays of the plan's size");
  throws('transformRows', 'null row', () => native.transformRows(...rows([f(8), null], false, false, 16)), "pdsp_napi: transformRows rows must be Float64Arrays of the plan's size");
  throws('transformRows', 'short imag', () => native.transformRows(...rows([{ real: f(8), imag: f(7) }], true, false, 8)), "pdsp_napi: transformRows rows must be Float64Arrays of the plan's size");
  throws('transformRows', 'plain-array row', () => native.transformRows(...rows([f(8), [1, 2]], false, false, 16)), F64);
  gives('transformRows', 'no rows', () => native.transformRows(...rows([], false, false, 0)), null);
}

// ---- intended changes: each row's expected outcome is the new one --------------------------------------------------
list = 'changed';
// (a) an int64 outside int's range is refused by the library, never truncated into range
throws('windowMake', '(a) type 2^32 + 3', () => native.windowMake(2 ** 32 + 3, 64, f(64)), 'Unsupported window type: -1');
throws('spectrum', '(a) window 2^32 + 1', () => native.spectrum(f(8), 48000, -1, 2 ** 32 + 1, 0, f(5), f(5), f(5)), 'Unsupported window type: -1');
throws('spectrumBatch', '(a) sides 2^32', () => native.spectrumBatch(f(16), 2, 8, 48000, -1, 0, 2 ** 32, ...outs(8, 2)), 'bad sides -1');
throws('spectrumRows', '(a) window 2^33', () => native.spectrumRows(...[[f(8), f(8)], 0, 2, 8, 48000, -1, 2 ** 33, 0, ...outs(5, 2)]), 'Unsupported window type: -1');
throws('firFilter', '(a) mode 2^32', () => native.firFilter(f(8), f(3), 2 ** 32, f(10)), 'unknown FIR mode -1');
throws('stft', '(a) window 2^32 + 1', () => native.stft(f(128), 64, 32, 2 ** 32 + 1, f(99), f(99)), 'Unsupported window type: -1');
throws('istft', '(a) window 2^32 + 1', () => native.istft(f(99), f(99), 3, 64, 32, 2 ** 32 + 1, f(128)), 'Unsupported window type: -1');
throws('sdft', '(a) window 2^32', () => native.sdft(f(16), 8, f(2), 1, 2 ** 32, f(18), f(18)), 'Unsupported window type: -1');
// (the library's binFrequencies refuses no `sides`: any value but 0 is two-sided, and 2^32 no longer truncates to 0)
gives('binFrequencies', '(a) sides 2^32 is two-sided', () => { const o = f(8); native.binFrequencies(8, 48000, 2 ** 32, o); return o.join(','); }, '0,6000,12000,18000,24000,30000,36000,42000');
// (b) a first argument that is no plan
for (const exp of ['transform', 'transformBatch', 'transformRows']) {
  throws(exp, '(b) no plan', () => native[exp]({}, 2, f(16), null, f(16), f(16), false), 'TypeError: pdsp_napi: expected a plan');
}
// (c) batch * len beyond int64
throws('spectrumBatch', '(c) batch * len overflows', () => native.spectrumBatch(f(16), 2 ** 40, 2 ** 40, 48000, 8, 0, 0, ...outs(5, 2)), 'pdsp_napi: spectrumBatch frames buffer too small');
// (d) a scalar and an array both of the wrong type: the scalar's TypeError
throws('spectrum', '(d) samples and rate both wrong', () => native.spectrum([1, 2], 'x', -1, 0, 0, f(5), f(5), f(5)), NUMBER);
throws('firFilter', '(d) signal and mode both wrong', () => native.firFilter([1, 2], f(3), 'x', f(10)), NUMBER);
throws('istft', '(d) real and frames both wrong', () => native.istft([1, 2], f(99), 'x', 64, 32, 1, f(128)), NUMBER);
throws('resamplePoly', '(d) signal and up both wrong', () => native.resamplePoly([1, 2], 'x', 1, f(0), f(16)), NUMBER);
// (e) a getter that detaches a buffer read earlier in the row walk: refused by the length check, nothing reaches the
// library (the transfer through a MessageChannel port detaches synchronously)
function detach(buf) { const { port1, port2 } = new MessageChannel(); port1.postMessage(buf, [buf]); port1.close(); port2.close(); }
throws('spectrumRows', '(e) getter at index 1 detaches frame 0', () => {
  const f0 = f(8), f1 = f(8), frames = [f0, f1];
  Object.defineProperty(frames, 1, { get() { detach(f0.buffer); return f1; } });
  try { return native.spectrumRows(...rowsArgs(frames, 0, 2)); } finally { if (f0.length !== 0) throw new Error('frame 0 was not detached'); }
}, 'pdsp_napi: spectrumRows frames must all have frameLen samples');
if (plan !== null) {
  list = 'changed-planned';
  throws('transformRows', '(e) real getter of row 1 detaches row 0', () => {
    const r0 = { real: f(8), imag: f(8) }, r1 = { imag: f(8) }, re1 = f(8);
    Object.defineProperty(r1, 'real', { get() { detach(r0.real.buffer); return re1; } });
    try { return native.transformRows(plan, [r0, r1], true, f(16), f(16), false); } finally { if (r0.real.length !== 0) throw new Error('row 0 was not detached'); }
  }, "pdsp_napi: transformRows rows must be Float64Arrays of the plan's size");
  throws('transformRows', '(b) complex flag no boolean', () => native.transformRows(plan, [f(8)], 1, f(8), f(8), false), 'TypeError: pdsp_napi: expected a boolean');
}
log.push(['meta', 'exports', Object.keys(native).sort().join(','), plan !== null]);
console.log(JSON.stringify(log));
