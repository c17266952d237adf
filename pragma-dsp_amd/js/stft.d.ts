// pragma-dsp/xform/stft: complex short-time transform and its overlap-add inverse on the device, f64.
export type StftWindow = 'rect' | 'hann' | 'hamming' | 'blackman';
export interface StftOptions {
  fftSize: number;
  hopSize: number;
  window?: StftWindow;
}
export interface StftResult {
  frames: number;
  bins: number;
  real: Float64Array;
  imag: Float64Array;
}
export function stft(
  signal: number[] | Float64Array | Float32Array,
  options: StftOptions,
): StftResult;
export function istft(
  spec: { frames: number; real: number[] | Float64Array | Float32Array; imag: number[] | Float64Array | Float32Array },
  options: StftOptions,
): Float64Array;
