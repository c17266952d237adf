// pragma-dsp/filters: FIR filtering (linear convolution) on the device, f64.
export type FirMode = 'full' | 'same' | 'valid' | 'filter';
export interface FirFilterOptions {
  mode?: FirMode;
}
export function firFilter(
  signal: number[] | Float64Array | Float32Array,
  taps: number[] | Float64Array | Float32Array,
  options?: FirFilterOptions,
): Float64Array;
