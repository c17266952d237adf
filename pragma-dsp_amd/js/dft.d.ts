// Any-length DFT on the device, f64 (numpy fft / ifft conventions), 2 <= length <= 4096.
export interface DftResult {
  real: Float64Array;
  imag: Float64Array;
}
export function dft(real: ArrayLike<number>, imag?: ArrayLike<number> | null): DftResult;
export function idft(real: ArrayLike<number>, imag: ArrayLike<number>): DftResult;
