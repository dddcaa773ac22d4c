// One output pixel of the aligned bilinear upsampling by an integer factor f (tridet/utils/tensor2d.py:28-47: replicate-pad by one,
// bilinear with align_corners=True to (f*h+1, f*w+1), crop; offset "half" shifts the result by f/2 with edge replication) of channel 0
// of an NHWC map, fused with the focal-length scaling of DD3DDenseDepth (dense_depth.py:146-151): v /= |(invK00, invK11)| * factor.
// Shared by aligned_bilinear_scale_kernel (aux_kernels.hip), which writes the up-sampled map, and dense_depth_loss_kernel
// (dense_depth_loss.hip), which evaluates it in place.  The source coordinate carries its own contract(off); the blend is left to the
// including translation unit's default (both includers contract), so the two kernels make the same arithmetic of it:
// tests/test_dense_depth_loss_gpu.py compares them bit for bit, pixel by pixel.
#pragma once
#include <hip/hip_runtime.h>

namespace dd3d {

// (b, y, x): the output pixel; the caller keeps y < f*h and x < f*w below 2^23 (f32 source coordinates).
__device__ __forceinline__ float aligned_bilinear_at(const float* __restrict__ src, const float* __restrict__ inv_K, int b, int y, int x, int h,
                                                     int w, int pitch, int f, int half, float factor) {
  const float scale = (float)h / (float)(f * h);  // (in - 1) / (out - 1) of the padded (h+1) -> (f*h+1) resize, = 1/f
  const float scale_w = (float)w / (float)(f * w);
  const int ys = half ? max(y - f / 2, 0) : y, xs = half ? max(x - f / 2, 0) : x;
  float ry, rx;
  {
    // The source coordinate is ROUNDED to f32 before its fraction is taken, as in the reference (upsample_bilinear2d computes the index in
    // the map's scalar type).  Left to itself the compiler fuses the product into `ry - y0` (one fma, the product unrounded): a fraction
    // that differs from the reference's by up to an ulp of the coordinate, i.e. by 6e-5 at column 800 for a factor that is no power of two.
    // (The pragma is honoured under hipcc's default -ffp-contract=fast-honor-pragmas; a build with plain -ffp-contract=fast would ignore it,
    // and tests/test_glue_kernels_gpu.py section D would say so.)
#pragma clang fp contract(off)
    ry = scale * (float)ys;
    rx = scale_w * (float)xs;
  }
  const int y0 = (int)ry, x0 = (int)rx;  // < h, w: ys <= f*h - 1
  const float ly = ry - (float)y0, lx = rx - (float)x0;
  const int y1 = min(y0 + 1, h - 1), x1 = min(x0 + 1, w - 1);  // row / column h, w of the padded map replicate h-1, w-1
  const float* p = src + (long)b * h * w * pitch;
  const float v00 = p[((long)y0 * w + x0) * pitch], v01 = p[((long)y0 * w + x1) * pitch];
  const float v10 = p[((long)y1 * w + x0) * pitch], v11 = p[((long)y1 * w + x1) * pitch];
  float v = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
  if (factor > 0.f) {
    const float k0 = inv_K[9 * b], k4 = inv_K[9 * b + 4];
    v = v / (sqrtf(k0 * k0 + k4 * k4) * factor);
  }
  return v;
}

}  // namespace dd3d
