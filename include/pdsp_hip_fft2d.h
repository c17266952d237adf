/* pdsp_hip_fft2d.h -- the transform over two axes: fft2 / ifft2 of batched images, f32 / f64.
 *
 * A header of its own: include/pdsp_hip.h is closed to new stream entry points (each of its 48 has a row in the graph
 * capture table) and claims the prefix pdsp_fft_ for the 1-D calls.  This one includes pdsp_hip.h for PDSP_API,
 * pdsp_stream and the error codes; pdsp_hip.h does not include it.  The symbols live in the same library.
 *
 * Definition: numpy's fft2 / ifft2 over the last two axes of [batch][H][W],
 *   X[k][l] = sum_{h < H} sum_{w < W} x[h][w] exp(-/+ 2 pi i (h k / H + w l / W)),   0 <= k < H, 0 <= l < W,
 * minus for the forward transform, plus for the inverse.  Data are planar complex (re, im), f32 or f64; a null im_in
 * means real images (the same bits as a zero plane) and gives the full complex output.  norm is one of PDSP_NORM_*, as
 * in pdsp_dct_*: the forward transform is scaled by 1 (backward), 1/sqrt(H W) (ortho) or 1/(H W) (forward), the inverse
 * by 1/(H W), 1/sqrt(H W) or 1 -- once, in the last store.  The inverse runs the forward kernels on swapped planes.
 *
 * Domain: H and W powers of two, 16 <= H <= 512, 16 <= W <= 16384 in f32 and 16 <= W <= 8192 in f64 (the single-pass
 * row limits); anything else is PDSP_ERR_UNSUPPORTED_SIZE.  Images are contiguous: row stride W, image stride H W; each
 * of the two input planes and the two output planes holds `batch` images and begins on a 16-byte boundary.
 *
 * Paths (pdsp_fft2d_query reports the one a shape takes; the launch code asks the same function):
 *   resident, H W <= 4096: ONE launch and one pass over HBM.  A 256-thread workgroup holds 4096 / (H W) whole images in
 *     LDS, transforms their rows and then their columns there, and moves them with 16-byte accesses.
 *   two passes, every other shape: the W-point row kernels of the 1-D transform on batch * H rows, from the input into
 *     the output planes, then ONE column launch that transforms the output planes in place and applies the scale.
 * Neither path allocates scratch, and every table (the radix tables of the two lengths) is uploaded by
 * pdsp_fft2d_create: both entry points can be captured into a graph from their first call on.
 *
 * Aliasing: an output plane may share bytes with an input plane only in the exact in-place call, re_out == re_in and
 * im_out == im_in (or im_in null), which gives the bits of the out-of-place call: on the resident path a workgroup
 * loads all of its images before its first barrier and stores only into them; on the two-pass path the row kernels
 * load a row before they store it, and the column pass reads all of a workgroup's tile before it stores any of it, the
 * tiles being disjoint.  Any other overlap of an output with an input, or of the two outputs, is refused with
 * PDSP_ERR_BAD_ARG before any launch.
 *
 * Accuracy: max|err| / max|X| <= 8e-8 log2(H W) in f32 and 2.5e-16 log2(H W) in f64 (the 1-D forward bound at
 * N = H W: a 2-D pass set is that transform's pass set minus its inter-pass twiddles).
 *
 * Every argument is checked before any device work, ahead of the device check: a null handle ("fft2d is null"), batch < 1,
 * a null buffer (im_in excepted; the inverse needs it), a norm outside PDSP_NORM_*, extents that overflow, planes off a
 * 16-byte boundary and the overlaps above give PDSP_ERR_BAD_ARG. */
#ifndef PDSP_HIP_FFT2D_H
#define PDSP_HIP_FFT2D_H

#include "pdsp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PDSP_NORM_BACKWARD = 0, PDSP_NORM_ORTHO = 1, PDSP_NORM_FORWARD = 2 };

typedef struct pdsp_fft2d pdsp_fft2d;

/* The object of one image shape on `device` (< 0: the current one).  It borrows the library's cached plans of W and H
 * points on that device (pinned while the object lives) and owns nothing else; both plans' tables are on the device
 * when this returns. */
PDSP_API int pdsp_fft2d_create(long long height, long long width, int device, pdsp_fft2d **out);
PDSP_API int pdsp_fft2d_destroy(pdsp_fft2d *f);
PDSP_API long long pdsp_fft2d_height(const pdsp_fft2d *f);
PDSP_API long long pdsp_fft2d_width(const pdsp_fft2d *f);

/* `batch` images [H][W] in (device pointers; im_in NULL: real images, forward only) -> `batch` images out.
 * inverse != 0: ifft2.  Formula, scale and aliasing rule: the head of this file. */
PDSP_API int pdsp_fft2d_c2c_f32(const pdsp_fft2d *f, long long batch, const float *re_in, const float *im_in,
                                float *re_out, float *im_out, int inverse, int norm, pdsp_stream stream);
PDSP_API int pdsp_fft2d_c2c_f64(const pdsp_fft2d *f, long long batch, const double *re_in, const double *im_in,
                                double *re_out, double *im_out, int inverse, int norm, pdsp_stream stream);

/* Synchronous f64 host form, one shot (stage, copy, the f64 kernels, copy back): `batch` contiguous images of
 * height x width points in host memory (im_in NULL: real, forward only), contiguous images out.  The outputs may be
 * the inputs. */
PDSP_API int pdsp_fft2d_host_f64(const double *re_in, const double *im_in, long long batch, long long height,
                                 long long width, int inverse, int norm, double *re_out, double *im_out);

/* What a shape takes, host only (no HIP call): scalar_bytes 4 or 8.  info[0] the path, info[1] images per workgroup
 * (resident: 4096 / (H W); else 0), info[2] the column tile width of the second launch (two passes: adjacent columns
 * of one image per workgroup, never more than W; else 0), info[3] launches per call (1 or 2).  Outside the domain:
 * PDSP_ERR_UNSUPPORTED_SIZE with the domain in the message, info unwritten. */
enum { PDSP_FFT2D_RESIDENT = 0, PDSP_FFT2D_TWO_PASS = 1 };
#define PDSP_FFT2D_INFO 4
PDSP_API int pdsp_fft2d_query(long long height, long long width, int scalar_bytes, int info[PDSP_FFT2D_INFO]);

#ifdef __cplusplus
}
#endif
#endif
