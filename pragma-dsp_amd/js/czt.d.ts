// Chirp-z transform and zoom FFT on the device, f64 (scipy.signal.czt / zoom_fft conventions), L + m - 1 <= 8192.
export interface CztResult {
  real: Float64Array;
  imag: Float64Array;
}
export type CztInput = ArrayLike<number> | { real: ArrayLike<number>; imag?: ArrayLike<number> | null };
export interface CztOptions {
  m?: number; // points out (default: the signal's length)
  step?: number; // w = exp(-2 pi i step), in turns (default 1 / m)
  start?: number; // a = radius exp(2 pi i start), in turns (default 0)
  radius?: number; // default 1
}
export interface ZoomFftOptions {
  m?: number;
  fs?: number; // default 2
  endpoint?: boolean;
}
export function czt(x: CztInput, options?: CztOptions): CztResult;
export function zoomFft(x: CztInput, fn: number | [number, number], options?: ZoomFftOptions): CztResult;
