// Shared by the loss kernels (losses.hip) and their backward (loss_grads.hip): block size, the columns of a partial row, the small
// per-element loss functions, the corner builder and the argument check.  The including translation unit turns floating-point
// contraction off before this header.
#pragma once
#include <math.h>

#include "common.h"
#include "box3d_decode.h"

namespace dd3d {

constexpr int LT = 256;              // threads per block of the per-location kernels
constexpr float LOSS_INF = 100000000.f;  // prepare_targets.py:8 INF

// terms of a partial row
enum {
  T_FOCAL = 0, T_NPOS, T_CTR, T_GIOU, T_CTRBCE, T_QUAT, T_PROJ, T_DEPTH, T_SIZE, T_CONF,
  T_ATTR_CE, T_ATTR_N, T_ATTR_W, T_SPEED, T_SPEED_W, T_SPEED_N
};
static_assert(T_SPEED_N + 1 == DD3D_LOSS_TERMS, "term count");

struct LossK {
  dd3d_loss_args a;
};

__device__ __forceinline__ int level_of(const dd3d_loss_args& a, int i) {  // image-local location -> level
  int l = 0;
  while (l + 1 < a.num_levels && i >= a.loc_off[l + 1]) ++l;
  return l;
}

// BCE with logits, stable form: max(x, 0) - x t + log1p(exp(-|x|))
__device__ __forceinline__ float bce_logits(float x, float t) { return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))); }

// tridet/layers/smooth_l1_loss.py:57-74: 0.5 n^2 below beta (NOT / beta), n - 0.5 beta above; plain L1 for beta < 1e-5
__device__ __forceinline__ float smooth_l1(float x, float y, float beta) {
  const float n = fabsf(x - y);
  if (beta < 1e-5f) return n;
  return n < beta ? 0.5f * (n * n) : n - 0.5f * beta;
}

// [ext] fvcore.nn.smooth_l1_loss, which NuscenesLoss imports for the speed term (nuscenes_dd3d.py:4, :261): 0.5 n^2 / beta below beta
__device__ __forceinline__ float smooth_l1_fvcore(float x, float y, float beta) {
  const float n = fabsf(x - y);
  if (beta < 1e-5f) return n;
  return n < beta ? 0.5f * (n * n) / beta : n - 0.5f * beta;
}

// GenericBoxes3D.corners (boxes3d.py:47-64): corner k = R(q) (0.5 lwh * sign_k) + tvec, lwh = size[1], size[0], size[2];
// Boxes3D.tvec = K^-1 [u, v, 1] * depth (boxes3d.py:169-173)
__device__ __forceinline__ void box_corners(const float* q, const float* ctr, float depth, const float* size, const float* K, float* out) {
  const float r = q[0], i = q[1], j = q[2], k = q[3];
  const float two_s = 2.0f / (r * r + i * i + j * j + k * k);
  const float R[9] = {1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                      two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                      two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)};
  const float u = ctr[0], v = ctr[1];
  const float t0 = (K[0] * u + K[1] * v + K[2]) * depth, t1 = (K[3] * u + K[4] * v + K[5]) * depth, t2 = (K[6] * u + K[7] * v + K[8]) * depth;
  const float hl = 0.5f * size[1], hw = 0.5f * size[0], hh = 0.5f * size[2];
  // BOX3D_CORNER_MAPPING (boxes3d.py:12-16), columns = corners
  const float sx[8] = {1, 1, 1, 1, -1, -1, -1, -1}, sy[8] = {1, -1, -1, 1, 1, -1, -1, 1}, sz[8] = {1, 1, -1, -1, 1, 1, -1, -1};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float px = hl * sx[c], py = hw * sy[c], pz = hh * sz[c];
    out[3 * c + 0] = px * R[0] + py * R[1] + pz * R[2] + t0;
    out[3 * c + 1] = px * R[3] + py * R[4] + pz * R[5] + t1;
    out[3 * c + 2] = px * R[6] + py * R[7] + pz * R[8] + t2;
  }
}

__device__ __forceinline__ float corner_group_loss(const float* tc, const float* q, const float* ctr, float depth, const float* size, const float* K,
                                                   float beta) {
  float pc[24];
  box_corners(q, ctr, depth, size, K, pc);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 24; ++e) s += smooth_l1(pc[e], tc[e], beta);
  return s / 24.f;
}

static inline int check_args(const dd3d_loss_args* a, const char* what) {
  DD3D_REQUIRE(a != nullptr, "%s: null args", what);
  DD3D_REQUIRE(a->num_levels >= 1 && a->num_levels <= DD3D_MAX_LEVELS, "%s: num_levels = %d", what, a->num_levels);
  DD3D_REQUIRE(a->B >= 1 && a->B <= 65535 && a->num_classes >= 1, "%s: B = %d, num_classes = %d", what, a->B, a->num_classes);
  DD3D_REQUIRE(a->max_gt >= 0 && a->max_gt <= DD3D_LOSS_MAX_GT, "%s: max_gt = %d outside [0, %d]", what, a->max_gt, DD3D_LOSS_MAX_GT);
  DD3D_REQUIRE(a->locations && a->gt_off && a->gt && a->labels && a->target_inds && a->box2d_reg && a->ctr_target && a->flags,
               "%s: null buffer", what);
  DD3D_REQUIRE(a->loc_off[0] == 0, "%s: loc_off[0] != 0", what);
  for (int l = 0; l < a->num_levels; ++l) {
    DD3D_REQUIRE(a->H[l] > 0 && a->W[l] > 0 && a->loc_off[l + 1] - a->loc_off[l] == a->H[l] * a->W[l], "%s: level %d geometry", what, l);
  }
  DD3D_REQUIRE((long)a->B * a->loc_off[a->num_levels] < (1L << 31), "%s: too many targets", what);
  DD3D_REQUIRE(!a->attributes || (a->speeds && a->num_attr >= 1), "%s: attributes without speeds / num_attr", what);
  return DD3D_OK;
}

}  // namespace dd3d
