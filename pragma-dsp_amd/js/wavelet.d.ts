// Multi-level discrete wavelet transform on the device, f64: orthogonal wavelets, periodic extension, the Mallat
// layout [cA_J | cD_J | ... | cD_1].  wavelet: 'haar', 'db1' ... 'db10', or an orthonormal scaling filter of even
// length 2 ... 32; the length of the signal must be a multiple of 2^levels.
export type Wavelet = string | ArrayLike<number>;
export function wavedec(signal: ArrayLike<number>, wavelet: Wavelet, levels: number): Float64Array;
export function waverec(coeffs: ArrayLike<number>, wavelet: Wavelet, levels: number): Float64Array;
export function waveletTaps(name: string): Float64Array;
