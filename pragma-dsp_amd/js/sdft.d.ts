// Sliding DFT on the device, f64: chosen bins (cycles per window, fractional allowed) of a window of `size` samples,
// 2 <= size <= 16384, at every hop-th start; 1 ... 256 bins.
export type SdftWindow = 'rect' | 'hann' | 'hamming' | 'blackman';
export interface SlidingDftResult {
  frames: number;
  bins: number;
  real: Float64Array; // [bins][frames], time fastest
  imag: Float64Array;
}
export interface GoertzelResult {
  real: Float64Array; // one value per bin
  imag: Float64Array;
}
export function slidingDft(
  signal: ArrayLike<number>,
  size: number,
  bins: ArrayLike<number> | number,
  hop?: number,
  window?: SdftWindow
): SlidingDftResult;
export function goertzel(signal: ArrayLike<number>, bins: ArrayLike<number> | number): GoertzelResult;
