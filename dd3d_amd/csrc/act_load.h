// Activation loaders shared by the backward kernels (predictor_grads.hip, tower_grads.hip): the float32 value of one channel of one
// pixel, decoded from whichever storage the forward plan left the tensor in (DD3D_PG_ACT_* of include/dd3d_hip.h).
#pragma once
#include "common.h"

namespace dd3d {

// ---- activation loaders: the value of channel c at pixel `pix` of a level with `npix` pixels, from the storage the plan keeps
template <int MODE>
__device__ __forceinline__ float load_act(const void* base, long npix, long pix, int c, int pitch, float inv_scale);
template <>
__device__ __forceinline__ float load_act<DD3D_PG_ACT_F32>(const void* base, long, long pix, int c, int pitch, float) {
  return reinterpret_cast<const float*>(base)[pix * pitch + c];
}
template <>
__device__ __forceinline__ float load_act<DD3D_PG_ACT_F16X2>(const void* base, long npix, long pix, int c, int, float inv_scale) {
  // [c / 32][pixel][hi, lo][32] halves of value * plane_scale: (hi + lo) / plane_scale, as conv_common.h::unpack_terms decodes them
  const _Float16* p = reinterpret_cast<const _Float16*>(base) + ((long)(c >> 5) * npix + pix) * 64 + (c & 31);
  return ((float)p[0] + (float)p[32]) * inv_scale;
}
template <>
__device__ __forceinline__ float load_act<DD3D_PG_ACT_BF16X3>(const void* base, long npix, long pix, int c, int, float) {
  // [c / 32][pixel][hi, mid, lo][32] bf16 terms, largest first: (hi + mid) + lo
  const unsigned short* p = reinterpret_cast<const unsigned short*>(base) + ((long)(c >> 5) * npix + pix) * 96 + (c & 31);
  const float hi = __uint_as_float((unsigned)p[0] << 16), mid = __uint_as_float((unsigned)p[32] << 16), lo = __uint_as_float((unsigned)p[64] << 16);
  return (hi + mid) + lo;
}

// the same with the storage chosen at run time (a block-uniform switch: staging code, not the matrix loop)
__device__ __forceinline__ float load_act_any(int mode, const void* base, long npix, long pix, int c, int pitch, float inv_scale) {
  switch (mode) {
    case DD3D_PG_ACT_F32: return load_act<DD3D_PG_ACT_F32>(base, npix, pix, c, pitch, inv_scale);
    case DD3D_PG_ACT_F16X2: return load_act<DD3D_PG_ACT_F16X2>(base, npix, pix, c, pitch, inv_scale);
    default: return load_act<DD3D_PG_ACT_BF16X3>(base, npix, pix, c, pitch, inv_scale);
  }
}

}  // namespace dd3d
