// pragma-dsp/filters, rate change: polyphase resampling on the device, f64 (listed under `.filters` of the root).
// scipy.signal.resample_poly(signal, up, down, window=taps), padtype "constant": ceil(len * up / down) outputs
export function resamplePoly(
  signal: number[] | Float64Array | Float32Array,
  up: number,
  down: number,
  taps?: number[] | Float64Array | Float32Array | null,
): Float64Array;
// scipy.signal.upfirdn(h, signal, up, down): the full output
export function upfirdn(
  h: number[] | Float64Array | Float32Array,
  signal: number[] | Float64Array | Float32Array,
  up?: number,
  down?: number,
): Float64Array;
// the default filter of resamplePoly (times up)
export function designResampleTaps(up: number, down: number): Float64Array;
