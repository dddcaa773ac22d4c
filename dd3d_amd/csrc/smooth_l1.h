// tridet's smooth-L1 (tridet/layers/smooth_l1_loss.py:57-74), shared by the corner losses (loss_common.h) and the dense-depth loss
// (dense_depth_loss.hip).  Contraction is turned off inside the function, so every operation is rounded on its own, like the
// reference's tensor ops, whatever the including translation unit's default.
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

}  // namespace dd3d
