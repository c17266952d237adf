// pragma-dsp/xform/dct: DCT-II / DCT-III and their inverses on the device, f64 (scipy dct conventions).
export type DctType = 2 | 3;
export type DctNorm = 'backward' | 'ortho' | 'forward';
export interface DctOptions {
  type?: DctType;
  norm?: DctNorm;
}
export function dct(signal: number[] | Float64Array | Float32Array, options?: DctOptions): Float64Array;
export function idct(signal: number[] | Float64Array | Float32Array, options?: DctOptions): Float64Array;
