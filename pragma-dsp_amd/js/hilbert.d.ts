// Hilbert / analytic signal helpers on the device, f64 (scipy.signal.hilbert conventions, even N).
export interface HilbertOptions {
  /** length the signal is zero-padded to and of every result: a power of two, 64 ... 16384; default signal.length */
  n?: number;
}
export interface AnalyticSignal {
  real: Float64Array;
  imag: Float64Array;
}
export function hilbert(signal: number[] | Float64Array | Float32Array, options?: HilbertOptions): AnalyticSignal;
export function envelope(signal: number[] | Float64Array | Float32Array, options?: HilbertOptions): Float64Array;
export function instantaneousPhase(signal: number[] | Float64Array | Float32Array, options?: HilbertOptions): Float64Array;
