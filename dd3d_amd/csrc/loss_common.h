// Shared by the loss kernels (losses.hip) and their backward (loss_grads.hip): block size, the columns of a partial row, the target
// indexing, the small per-element loss functions, the slab's column sum and the argument check; and, as templates over the scalar type
// (float in the losses, the dual number Du of dual.h in the backward; the operations op_* of box3d_decode.h), the corner builder, GIoU,
// the quaternion renormalisation and the entangled corner error.  The including translation unit turns floating-point contraction off
// before this header.
#pragma once
#include <math.h>

#include "common.h"
#include "box3d_decode.h"
#include "smooth_l1.h"

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

// Target n (level-first, then image, then H*W: the order loss_assign_kernel writes) -> level l, image b, pixel p of the level's H*W,
// and pix = b * HW + p, the row of the level's NHWC maps.  The argument block comes by value, as the kernels take it: the copy folds
// away, whereas behind a reference hipcc no longer proves the kernel's loads unclobbered and loss_terms_kernel's code changes throughout.
struct TargetIndex {
  int l, b, p, HW;
  long pix;
};
__device__ __forceinline__ TargetIndex target_index(const dd3d_loss_args a, long n) {
  int l = 0;
  while (l + 1 < a.num_levels && n >= (long)a.B * a.loc_off[l + 1]) ++l;
  const int HW = a.H[l] * a.W[l];
  const long rr = n - (long)a.B * a.loc_off[l];
  const int b = (int)(rr / HW), p = (int)(rr - (long)b * HW);
  return {l, b, p, HW, (long)b * HW + p};
}

// BCE with logits, stable form: max(x, 0) - x t + log1p(exp(-|x|))
__device__ __forceinline__ float bce_logits(float x, float t) { return fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x))); }

// The pieces of [ext] fvcore.nn.sigmoid_focal_loss for logit x and target t in {0, 1}: the loss is ce * mod (times the alpha weight);
// the backward adds its derivative from pr, ce, m and mod
struct FocalPieces {
  float pr, ce, m, mod;
};
__device__ __forceinline__ void focal_pieces(float x, float t, float gamma, FocalPieces& f) {
  f.pr = 1.0f / (1.0f + expf(-x));
  f.ce = bce_logits(x, t);
  const float p_t = f.pr * t + (1.f - f.pr) * (1.f - t);
  f.m = 1.f - p_t;
  f.mod = gamma == 2.0f ? f.m * f.m : powf(f.m, gamma);
}

// [ext] fvcore.nn.smooth_l1_loss, which NuscenesLoss imports for the speed term (nuscenes_dd3d.py:4, :261): 0.5 n^2 / beta below beta
__device__ __forceinline__ float smooth_l1_fvcore(float x, float y, float beta) {
  const float n = fabsf(x - y);
  if (beta < 1e-5f) return n;
  return n < beta ? 0.5f * (n * n) / beta : n - 0.5f * beta;
}

// GenericBoxes3D.corners (boxes3d.py:47-64): corner k = R(q) (0.5 lwh * sign_k) + tvec, lwh = size[1], size[0], size[2];
// Boxes3D.tvec = K^-1 [u, v, 1] * depth (boxes3d.py:169-173).  Element e of the 24 goes to sink(e, value), in order.
template <class T, class F>
__device__ __forceinline__ void box_corners_to(const T* q, const T* ctr, T depth, const T* size, const float* K, F sink) {
  const T r = q[0], i = q[1], j = q[2], k = q[3];
  const T two_s = 2.0f / (r * r + i * i + j * j + k * k);
  const T R[9] = {1.f - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                  two_s * (i * j + k * r), 1.f - two_s * (i * i + k * k), two_s * (j * k - i * r),
                  two_s * (i * k - j * r), two_s * (j * k + i * r), 1.f - two_s * (i * i + j * j)};
  const T u = ctr[0], v = ctr[1];
  const T t0 = (K[0] * u + K[1] * v + K[2]) * depth, t1 = (K[3] * u + K[4] * v + K[5]) * depth, t2 = (K[6] * u + K[7] * v + K[8]) * depth;
  const T hl = 0.5f * size[1], hw = 0.5f * size[0], hh = 0.5f * size[2];
  // BOX3D_CORNER_MAPPING (boxes3d.py:12-16), columns = corners
  const float sx[8] = {1, 1, 1, 1, -1, -1, -1, -1}, sy[8] = {1, -1, -1, 1, 1, -1, -1, 1}, sz[8] = {1, 1, -1, -1, 1, 1, -1, -1};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const T px = hl * sx[c], py = hw * sy[c], pz = hh * sz[c];
    sink(3 * c + 0, px * R[0] + py * R[1] + pz * R[2] + t0);
    sink(3 * c + 1, px * R[3] + py * R[4] + pz * R[5] + t1);
    sink(3 * c + 2, px * R[6] + py * R[7] + pz * R[8] + t2);
  }
}
__device__ __forceinline__ void box_corners(const float* q, const float* ctr, float depth, const float* size, const float* K, float* out) {
  box_corners_to(q, ctr, depth, size, K, [&](int e, float v) { out[e] = v; });
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

// IOULoss "giou" (iou_loss.py:20-71) of the four predicted distances p against the target's: the gious, before 1 - x and the weight
template <class T>
__device__ __forceinline__ T giou(const T* p, const float* tg) {
  const T pl = p[0], pt = p[1], pr_ = p[2], pbm = p[3];
  const float tl = tg[0], tt = tg[1], tr = tg[2], tb = tg[3];
  const float target_area = (tl + tr) * (tt + tb);
  const T pred_area = (pl + pr_) * (pt + pbm);
  const T w_int = op_min(pl, tl) + op_min(pr_, tr);
  const T h_int = op_min(pbm, tb) + op_min(pt, tt);
  const T gw = op_max(pl, tl) + op_max(pr_, tr);
  const T gh = op_max(pbm, tb) + op_max(pt, tt);
  const T ac_union = gw * gh;
  const T area_int = w_int * h_int;
  const T area_union = target_area + pred_area - area_int;
  const T ious = (area_int + 1.0f) / (area_union + 1.0f);
  return ious - (ac_union - area_union) / ac_union;
}

// The decoded box's quaternion, divided by its clamped norm when the batch-wide renormalisation of the positives' allocentric decode
// is on (geometry.py:48-53): flags is the word loss_assign_kernel sets
template <class T>
__device__ __forceinline__ void decoded_quat(const Box3dDecoded<T>& d, int allocentric, const int32_t* flags, T* q) {
  q[0] = d.q0, q[1] = d.q1, q[2] = d.q2, q[3] = d.q3;
  if (allocentric && *flags) {
    const T dn = op_clamp_min(d.qn, DECODE_QEPS);
    q[0] = q[0] / dn, q[1] = q[1] / dn, q[2] = q[2] / dn, q[3] = q[3] / dn;
  }
}

// Entangled L1 of the whole prediction against the target corners tc (fcos3d.py:289-295), a value only: the reference detaches it
template <class T>
__device__ __forceinline__ float entangled_error(const float* tc, const T* q, const T* ctr, T depth, const T* size, const float* K) {
  T ec[24];
  box_corners_to(q, ctr, depth, size, K, [&](int e, T v) { ec[e] = v; });
  float es = 0.f;
#pragma unroll
  for (int e = 0; e < 24; ++e) es += fabsf(tc[e] - op_value(ec[e]));
  return es / 24.f;
}

// Column `col` of the partial slab summed by one block of LT threads in a fixed order (a strided sum per thread, then a halving tree
// over red[LT] in LDS); thread 0 writes *dst, and the block is synchronised on return.
__device__ __forceinline__ void column_sum(const float* partials, int nblocks, int col, float* red, float* dst) {
  float s = 0.f;
  for (int r = threadIdx.x; r < nblocks; r += LT) s += partials[(long)r * DD3D_LOSS_TERMS + col];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int h = LT / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) *dst = red[0];
  __syncthreads();
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
