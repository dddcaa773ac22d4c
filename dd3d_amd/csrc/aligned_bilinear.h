// One output pixel of the aligned bilinear upsampling by an integer factor f (tridet/utils/tensor2d.py:28-47: replicate-pad by one,
// bilinear with align_corners=True to (f*h+1, f*w+1), crop; offset "half" shifts the result by f/2 with edge replication) of channel 0
// of an NHWC map, fused with the focal-length scaling of DD3DDenseDepth (dense_depth.py:146-151): v /= |(invK00, invK11)| * factor.
//
// The geometry is stated ONCE, in aligned_bilinear_source / aligned_bilinear_taps: the rounded source coordinate, the four tap indices
// with their edge replication, and the row and column weights.  The value direction (aligned_bilinear_at: a gather through the taps)
// and the gradient direction (dense_depth_loss_grads.hip: the transpose, the same weights carried back to the same taps) both read it
// there, so they cannot drift apart.
//
// aligned_bilinear_at is shared by aligned_bilinear_scale_kernel (aux_kernels.hip), which writes the up-sampled map, and
// dense_depth_loss_kernel (dense_depth_loss.hip), which evaluates it in place.  The source coordinate carries its own contract(off); the
// blend is left to the including translation unit's default (every includer contracts), so the kernels make the same arithmetic of it:
// tests/test_dense_depth_loss_gpu.py compares them bit for bit, pixel by pixel.
#pragma once
#include <hip/hip_runtime.h>

namespace dd3d {

// Source coordinate along one axis of output index `s` (after the "half" shift and clamp) for a level of n cells and factor f.
// The coordinate is ROUNDED to f32 before its fraction is taken, as in the reference (upsample_bilinear2d computes the index in the
// map's scalar type).  Left to itself the compiler fuses the product into `r - i0` (one fma, the product unrounded): a fraction that
// differs from the reference's by up to an ulp of the coordinate, i.e. by 6e-5 at column 800 for a factor that is no power of two.
// (The pragma is honoured under hipcc's default -ffp-contract=fast-honor-pragmas; a build with plain -ffp-contract=fast would ignore it,
// and tests/test_glue_kernels_gpu.py section D would say so.)  Host-callable: the gradient's entry point checks on the host that the
// pixels of one cell are a contiguous run (dense_depth_loss_grads.hip).
__host__ __device__ __forceinline__ float aligned_bilinear_source(int s, int n, int f) {
#pragma clang fp contract(off)
  const float scale = (float)n / (float)(f * n);  // (in - 1) / (out - 1) of the padded (n+1) -> (f*n+1) resize, = 1/f
  return scale * (float)s;
}

// The four taps of output pixel (y, x) and their weights: value = sum over (a, c) in {0,1}^2 of wy[a] * wx[c] * src[yi[a]][xi[c]].
struct BilinearTaps {
  int y0, y1, x0, x1;
  float ly, lx;  // the fractions: row weights (1 - ly, ly), column weights (1 - lx, lx)
};

// (y, x): the output pixel; the caller keeps y < f*h and x < f*w below 2^23 (f32 source coordinates).
__device__ __forceinline__ BilinearTaps aligned_bilinear_taps(int y, int x, int h, int w, int f, int half) {
  const int ys = half ? max(y - f / 2, 0) : y, xs = half ? max(x - f / 2, 0) : x;
  const float ry = aligned_bilinear_source(ys, h, f), rx = aligned_bilinear_source(xs, w, f);
  BilinearTaps t;
  t.y0 = (int)ry, t.x0 = (int)rx;  // < h, w: ys <= f*h - 1
  t.ly = ry - (float)t.y0, t.lx = rx - (float)t.x0;
  t.y1 = min(t.y0 + 1, h - 1), t.x1 = min(t.x0 + 1, w - 1);  // row / column h, w of the padded map replicate h-1, w-1
  return t;
}

// The blend of the four tap values, in the one operation order every kernel uses.
__device__ __forceinline__ float aligned_bilinear_blend(const BilinearTaps& t, float v00, float v01, float v10, float v11) {
  const float ly = t.ly, lx = t.lx;
  return (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
}

// dense_depth.py:146-151: the pixel size the value is divided by (and the gradient with it); factor <= 0: no focal scaling, 1.
__device__ __forceinline__ float aligned_bilinear_pixel_size(const float* __restrict__ inv_K, int b, float factor) {
  if (!(factor > 0.f)) return 1.f;
  const float k0 = inv_K[9 * b], k4 = inv_K[9 * b + 4];
  return sqrtf(k0 * k0 + k4 * k4) * factor;
}

__device__ __forceinline__ float aligned_bilinear_at(const float* __restrict__ src, const float* __restrict__ inv_K, int b, int y, int x, int h,
                                                     int w, int pitch, int f, int half, float factor) {
  const BilinearTaps t = aligned_bilinear_taps(y, x, h, w, f, half);
  const float* p = src + (long)b * h * w * pitch;
  const float v00 = p[((long)t.y0 * w + t.x0) * pitch], v01 = p[((long)t.y0 * w + t.x1) * pitch];
  const float v10 = p[((long)t.y1 * w + t.x0) * pitch], v11 = p[((long)t.y1 * w + t.x1) * pitch];
  float v = aligned_bilinear_blend(t, v00, v01, v10, v11);
  if (factor > 0.f) v = v / aligned_bilinear_pixel_size(inv_K, b, factor);
  return v;
}

}  // namespace dd3d
