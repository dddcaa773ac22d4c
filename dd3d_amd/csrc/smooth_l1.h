// tridet's smooth-L1 (tridet/layers/smooth_l1_loss.py:57-74) and its derivative, shared by the corner losses (loss_common.h,
// loss_grads.hip) and the dense-depth loss (dense_depth_loss.hip, dense_depth_loss_grads.hip).  Contraction is turned off inside both
// functions, so every operation is rounded on its own, like the reference's tensor ops, whatever the including translation unit's default.
#pragma once
#include <math.h>

namespace dd3d {

// 0.5 n^2 below beta (NOT / beta), n - 0.5 beta above; plain L1 for beta < 1e-5
__device__ __forceinline__ float smooth_l1(float x, float y, float beta) {
#pragma clang fp contract(off)
  const float n = fabsf(x - y);
  if (beta < 1e-5f) return n;
  return n < beta ? 0.5f * (n * n) : n - 0.5f * beta;
}

// d smooth_l1 / dx, on the branch the value takes: x - y below beta, sign(x - y) otherwise (|x - y| == beta included) and everywhere
// for beta < 1e-5; sign(0) = 0, as torch's abs gives it, and a NaN difference compares false both ways: 0.
__device__ __forceinline__ float smooth_l1_grad(float x, float y, float beta) {
#pragma clang fp contract(off)
  const float d = x - y;
  const float s = (float)(d > 0.f) - (float)(d < 0.f);
  if (beta < 1e-5f) return s;
  return fabsf(d) < beta ? d : s;
}

}  // namespace dd3d
