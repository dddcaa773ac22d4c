// Training losses of DD3D / NuscenesDD3D for gfx950 (their gradients with respect to the head maps: loss_grads.hip): target assignment and the loss dict of the reference's
// training branch (core.py:95-112, nuscenes_dd3d.py:376-397), single process (reduce_sum = identity, world size 1).
//
//   loss_assign_kernel   DD3DTargetPreparer.compute_targets_for_locations + get_sample_region (prepare_targets.py:93-212): one
//                        thread per (image, location), the image's boxes and areas in LDS.  f32 in the reference's operation order,
//                        contraction off, so every target is the reference's bit for bit.
//   loss_terms_kernel    FCOS2DLoss / FCOS3DLoss / DisentangledBox3DLoss / NuscenesLoss per target: focal loss over all classes; for a
//                        positive the GIoU, the centerness BCE, the predicted-box decode (box3d_decode.h, the inference decode), the
//                        target corners and the four disentangled corner sets, entangled L1 -> exp(-err / T) -> conf BCE, the
//                        attribute cross entropy and the speed loss (fvcore's smooth-L1, the corners use tridet's).  Per-block partial sums of DD3D_LOSS_TERMS terms in a fixed tree
//                        order go to a slab.
//   loss_finalize_kernel one block: the slab summed in a fixed order, then the denominators and the loss values.
// The pieces the backward needs as well (target indexing, focal pieces, GIoU, corners, renormalisation, entangled error, the slab's column
// sum) are in loss_common.h, GIoU and the 3D chain as templates over the scalar type: loss_grads.hip instantiates them on dual numbers.
// No float atomics anywhere: the result is the same bit for bit on every run.
#pragma clang fp contract(off)
#include <math.h>

#include "loss_common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

// ------------------------------------------------------------------------------------------------ assignment
__global__ void loss_clear_flags_kernel(int32_t* flags) { flags[0] = 0; }

__global__ __launch_bounds__(LT) void loss_assign_kernel(const LossK P) {
  const dd3d_loss_args& a = P.a;
  const int b = blockIdx.y;
  const int i = blockIdx.x * LT + threadIdx.x;  // image-local location
  const int nloc = a.loc_off[a.num_levels];
  const int g0 = a.gt_off[b];
  const int ng = min(a.gt_off[b + 1] - g0, a.max_gt);  // the LDS holds max_gt <= DD3D_LOSS_MAX_GT boxes (dd3d_hip.h: the caller's bound)
  __shared__ float sbox[DD3D_LOSS_MAX_GT][5];  // x1, y1, x2, y2, area
  for (int g = threadIdx.x; g < ng; g += LT) {
    const float* r = a.gt + (long)(g0 + g) * DD3D_LOSS_GT_FIELDS;
    sbox[g][0] = r[0], sbox[g][1] = r[1], sbox[g][2] = r[2], sbox[g][3] = r[3];
    sbox[g][4] = (r[2] - r[0]) * (r[3] - r[1]);  // Boxes.area
  }
  __syncthreads();
  if (i >= nloc) return;
  const int l = level_of(a, i);
  const int HW = a.H[l] * a.W[l];
  const long n = (long)a.B * a.loc_off[l] + (long)b * HW + (i - a.loc_off[l]);  // level-first, then image, then H*W
  const float x = a.locations[2 * i], y = a.locations[2 * i + 1];
  int label = a.num_classes, tind = -1, best = 0;
  float reg[4] = {0.f, 0.f, 0.f, 0.f};
  float ctr = 0.f;
  if (ng > 0) {
    // get_sample_region (:179-212): all-false for the image when its FIRST GT has x1 + x2 == 0 (the `center_x[..., 0].sum() == 0` test)
    const bool quirk = a.center_sample && (sbox[0][0] + sbox[0][2]) * 0.5f == 0.f;
    const float rad = a.radius[l], lo = a.soi_lo[l], hi = a.soi_hi[l];
    float best_a = INFINITY;
    for (int g = 0; g < ng; ++g) {
      const float x1 = sbox[g][0], y1 = sbox[g][1], x2 = sbox[g][2], y2 = sbox[g][3];
      const float L_ = x - x1, T_ = y - y1, R_ = x2 - x, B_ = y2 - y;
      bool inside;
      if (a.center_sample) {
        if (quirk) {
          inside = false;
        } else {
          const float cx = (x1 + x2) * 0.5f, cy = (y1 + y2) * 0.5f;
          const float xmin = cx - rad, ymin = cy - rad, xmax = cx + rad, ymax = cy + rad;
          const float c0 = xmin > x1 ? xmin : x1, c1 = ymin > y1 ? ymin : y1;
          const float c2 = xmax > x2 ? x2 : xmax, c3 = ymax > y2 ? y2 : ymax;
          inside = fminf(fminf(x - c0, y - c1), fminf(c2 - x, c3 - y)) > 0.f;
        }
      } else {
        inside = fminf(fminf(L_, T_), fminf(R_, B_)) > 0.f;
      }
      const float mx = fmaxf(fmaxf(L_, T_), fmaxf(R_, B_));
      const bool cared = mx >= lo && mx <= hi;
      const float ar = (inside && cared) ? sbox[g][4] : LOSS_INF;
      if (ar < best_a) best_a = ar, best = g;  // strict: the lowest index among equal areas (torch.min)
    }
    const float* r = a.gt + (long)(g0 + best) * DD3D_LOSS_GT_FIELDS;
    reg[0] = x - sbox[best][0], reg[1] = y - sbox[best][1], reg[2] = sbox[best][2] - x, reg[3] = sbox[best][3] - y;
    tind = g0 + best;
    label = best_a == LOSS_INF ? a.num_classes : __float_as_int(r[4]);
    if (label != a.num_classes) {  // compute_ctrness_targets (fcos2d.py:20-27)
      // each quotient and the root rounded once to f32 from the f64 operation, which is the correctly rounded f32 result (53 >= 2 * 24 + 2
      // bits): the reference's IEEE f32 division and torch.sqrt bit for bit, whatever the f32 lowering of / and sqrtf
      const float lr = (float)((double)fminf(reg[0], reg[2]) / (double)fmaxf(reg[0], reg[2]));
      const float tb = (float)((double)fminf(reg[1], reg[3]) / (double)fmaxf(reg[1], reg[3]));
      ctr = (float)sqrt((double)(lr * tb));
    }
  }
  a.labels[n] = label;
  a.target_inds[n] = tind;
  a.box2d_reg[4 * n + 0] = reg[0], a.box2d_reg[4 * n + 1] = reg[1], a.box2d_reg[4 * n + 2] = reg[2], a.box2d_reg[4 * n + 3] = reg[3];
  a.ctr_target[n] = ctr;
  const float* r = ng > 0 ? a.gt + (long)(g0 + best) * DD3D_LOSS_GT_FIELDS : nullptr;
  if (a.box3d_t) {
    float* o = a.box3d_t + n * DD3D_LOSS_BOX3D_FIELDS;
#pragma unroll
    for (int f = 0; f < DD3D_LOSS_BOX3D_FIELDS; ++f) o[f] = r ? r[7 + f] : 0.f;  // images without GT: all-zero Boxes3D (:111-127)
  }
  if (a.attributes) {
    a.attributes[n] = r ? __float_as_int(r[5]) : a.num_attr;
    a.speeds[n] = r ? r[6] : NAN;
  }
  // the batch-wide renormalisation trigger of the positives' allocentric decode (geometry.py:48-53)
  if (label != a.num_classes && a.box3d[l] != nullptr && a.allocentric) {
    const int C3 = a.class_agnostic_3d ? 1 : a.num_classes, c3 = a.class_agnostic_3d ? 0 : label;
    const float* p = a.box3d[l] + ((long)b * HW + (i - a.loc_off[l])) * a.b3d_pitch;
    const Box3dDecodeParams dp{a.scale_depth_by_focal, a.depth_is_distance, a.allocentric, a.focal_factor, a.min_depth, a.max_depth};
    const Box3dDecoded d = decode_box3d(p, C3, c3, x, y, a.inv_K + 9 * b, a.canon_sizes + 3 * label, dp);
    if (d.bad) atomicOr(a.flags, 1);
  }
}

// ------------------------------------------------------------------------------------------------ per-target terms
__global__ __launch_bounds__(LT) void loss_terms_kernel(const LossK P) {
  const dd3d_loss_args& a = P.a;
  const int nloc = a.loc_off[a.num_levels];
  const long N = (long)a.B * nloc;
  const long n = (long)blockIdx.x * LT + threadIdx.x;
  float t[DD3D_LOSS_TERMS];
#pragma unroll
  for (int k = 0; k < DD3D_LOSS_TERMS; ++k) t[k] = 0.f;
  if (n < N) {
    const TargetIndex ti = target_index(a, n);
    const int l = ti.l, b = ti.b, p = ti.p;
    const long pix = ti.pix;
    const int C = a.num_classes;
    const int label = a.labels[n];
    const bool pos = label != C;
    // sigmoid focal loss over every class ([ext] fvcore.nn.sigmoid_focal_loss, reduction "sum")
    const float* cl = a.cls[l] + pix * a.cls_pitch;
    float fs = 0.f;
    for (int c = 0; c < C; ++c) {
      const float xv = cl[c];
      const float tv = (pos && c == label) ? 1.f : 0.f;
      FocalPieces f;
      focal_pieces(xv, tv, a.focal_gamma, f);
      float lv = f.ce * f.mod;
      if (a.focal_alpha >= 0.f) lv = (a.focal_alpha * tv + (1.f - a.focal_alpha) * (1.f - tv)) * lv;
      fs += lv;
    }
    t[T_FOCAL] = fs;
    if (pos) {
      const float ct = a.ctr_target[n];
      t[T_NPOS] = 1.f;
      t[T_CTR] = ct;
      const float* pb = a.box2d[l] + pix * a.b2d_pitch;
      const float* tg = a.box2d_reg + 4 * n;
      t[T_GIOU] = (1.f - giou(pb, tg)) * ct;  // IOULoss "giou", weighted by the centerness target
      t[T_CTRBCE] = bce_logits(pb[4], ct);
      if (a.box3d[l] != nullptr) {
        const int C3 = a.class_agnostic_3d ? 1 : C, c3 = a.class_agnostic_3d ? 0 : label;
        const float* pm = a.box3d[l] + pix * a.b3d_pitch;
        const int i = a.loc_off[l] + p;
        const float lx = a.locations[2 * i], ly = a.locations[2 * i + 1];
        const float* Kp = a.inv_K + 9 * b;
        const Box3dDecodeParams dp{a.scale_depth_by_focal, a.depth_is_distance, a.allocentric, a.focal_factor, a.min_depth, a.max_depth};
        const Box3dDecoded d = decode_box3d(pm, C3, c3, lx, ly, Kp, a.canon_sizes + 3 * label, dp);
        float q[4];
        decoded_quat(d, a.allocentric, a.flags, q);
        const float pc[2] = {d.cx, d.cy}, ps[3] = {d.s0, d.s1, d.s2};
        const float* tb3 = a.box3d_t + n * DD3D_LOSS_BOX3D_FIELDS;  // quat 0-3, proj_ctr 4-5, depth 6, size 7-9, K^-1 10-18
        const float* tK = tb3 + 10;
        float tc[24];
        box_corners(tb3, tb3 + 4, tb3[6], tb3 + 7, tK, tc);
        const float beta = a.smooth_l1_beta;
        // DisentangledBox3DLoss (disentangled_box3d_loss.py:27-54): the target with ONE component replaced by the prediction; the
        // clamp of :42 discards its result, so no clamp
        t[T_QUAT] = corner_group_loss(tc, q, tb3 + 4, tb3[6], tb3 + 7, tK, beta) * ct;
        t[T_PROJ] = corner_group_loss(tc, tb3, pc, tb3[6], tb3 + 7, tK, beta) * ct;
        t[T_DEPTH] = corner_group_loss(tc, tb3, tb3 + 4, d.depth, tb3 + 7, tK, beta) * ct;
        t[T_SIZE] = corner_group_loss(tc, tb3, tb3 + 4, tb3[6], ps, tK, beta) * ct;
        // entangled L1 of the whole prediction (its own K^-1: the image's) -> conf target -> BCE (fcos3d.py:289-295)
        const float err = entangled_error(tc, q, pc, d.depth, ps, Kp);
        const float conf_t = expf(-1.f / a.conf3d_temperature * err);
        t[T_CONF] = bce_logits(pm[10 * C3 + c3], conf_t) * ct;
      }
      if (a.attributes) {  // NuscenesLoss (nuscenes_dd3d.py:219-263)
        const int at = a.attributes[n];
        if (at != a.num_attr) {
          const float* lg = cl + a.attr_off;
          float m = lg[0];
          for (int k = 1; k < a.num_attr; ++k) m = fmaxf(m, lg[k]);
          float se = 0.f;
          for (int k = 0; k < a.num_attr; ++k) se += expf(lg[k] - m);
          t[T_ATTR_CE] = m + logf(se) - lg[at];
          t[T_ATTR_N] = 1.f;
          t[T_ATTR_W] = ct;
        }
        const float sp = a.speeds[n];
        if (!isnan(sp)) {
          t[T_SPEED] = smooth_l1_fvcore(cl[a.speed_off], sp, 0.05f) * ct;
          t[T_SPEED_W] = ct;
          t[T_SPEED_N] = 1.f;
        }
      }
    }
  }
  // fixed-order block reduction: wave butterfly, then the four wave sums in order
  __shared__ float ws[LT / 64][DD3D_LOSS_TERMS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < DD3D_LOSS_TERMS; ++k) {
    float v = t[k];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) ws[wave][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < DD3D_LOSS_TERMS) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < LT / 64; ++w) s += ws[w][threadIdx.x];
    a.partials[(long)blockIdx.x * DD3D_LOSS_TERMS + threadIdx.x] = s;
  }
}

// ------------------------------------------------------------------------------------------------ finalize
__global__ __launch_bounds__(LT) void loss_finalize_kernel(const LossK P, int nblocks) {
  const dd3d_loss_args& a = P.a;
  __shared__ float red[LT];
  __shared__ float S[DD3D_LOSS_TERMS];
  for (int k = 0; k < DD3D_LOSS_TERMS; ++k) column_sum(a.partials, nblocks, k, red, &S[k]);
  if (threadIdx.x != 0) return;
  float* o = a.out;
  const float npos = S[T_NPOS];
  const float num_pos_avg = fmaxf(npos, 1.0f);                     // fcos2d.py:189
  const float loss_denom = fmaxf(S[T_CTR], 1e-6f);                 // fcos2d.py:222
  o[0] = S[T_FOCAL] / num_pos_avg;
  const bool any = npos > 0.f;                                     // empty-positive branches: x.sum() * 0.
  o[1] = any ? S[T_GIOU] / loss_denom : 0.f;
  o[2] = any ? S[T_CTRBCE] / num_pos_avg : 0.f;
  o[3] = any ? a.weight_box3d * S[T_QUAT] / loss_denom : 0.f;      // fcos3d.py:291
  o[4] = any ? a.weight_box3d * S[T_PROJ] / loss_denom : 0.f;
  o[5] = any ? a.weight_box3d * S[T_DEPTH] / loss_denom : 0.f;
  o[6] = any ? a.weight_box3d * S[T_SIZE] / loss_denom : 0.f;
  o[7] = any ? a.weight_conf3d * S[T_CONF] / loss_denom : 0.f;     // fcos3d.py:295
  // attribute: mean CE over the valid attributes times the summed weights over its own denominator (nuscenes_dd3d.py:228-240)
  const float attr_denom = fmaxf(S[T_ATTR_W], 1e-6f);
  o[8] = (any && S[T_ATTR_N] > 0.f) ? a.weight_attr * ((S[T_ATTR_CE] / S[T_ATTR_N]) * S[T_ATTR_W] / attr_denom) : 0.f;
  const float speed_denom = fmaxf(S[T_SPEED_W], 1e-6f);
  o[9] = (any && S[T_SPEED_N] > 0.f) ? a.weight_speed * (S[T_SPEED] / speed_denom) : 0.f;
  o[10] = npos;
  o[11] = loss_denom;
  o[12] = o[13] = o[14] = o[15] = 0.f;
  a.num_pos[0] = (int)npos;
}


}  // namespace dd3d

extern "C" int dd3d_loss_assign(const dd3d_loss_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_args(args, "dd3d_loss_assign");
  if (rc != DD3D_OK) return rc;
  bool any3d = false;
  for (int l = 0; l < args->num_levels; ++l) any3d |= args->box3d[l] != nullptr;
  DD3D_REQUIRE(!any3d || (args->inv_K && args->canon_sizes), "dd3d_loss_assign: box3d maps need inv_K and canon_sizes");
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // The trigger word is cleared by a kernel, not by hipMemsetAsync: captured into a plan's hipGraph, the memset node of the larger
  // training graphs was replayed with other fill bytes than 0 after a dozen replays (0x20202020, 0xF0F0F0F0 read back on the MI355X),
  // which switched every positive of those steps to the renormalised decode (tests/test_loss_plan_history_gpu.py).
  hipLaunchKernelGGL(loss_clear_flags_kernel, dim3(1), dim3(1), 0, s, args->flags);
  int e = check_launch("loss_clear_flags_kernel");
  if (e != DD3D_OK) return e;
  const int nloc = args->loc_off[args->num_levels];
  hipLaunchKernelGGL(loss_assign_kernel, dim3((unsigned)ceil_div(nloc, LT), (unsigned)args->B), dim3(LT), 0, s, LossK{*args});
  return check_launch("loss_assign_kernel");
}

extern "C" int dd3d_loss_terms(const dd3d_loss_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_args(args, "dd3d_loss_terms");
  if (rc != DD3D_OK) return rc;
  const long N = (long)args->B * args->loc_off[args->num_levels];
  const int nblocks = (int)((N + LT - 1) / LT);
  DD3D_REQUIRE(args->partials && args->out && args->num_pos && args->n_partials >= nblocks, "dd3d_loss_terms: partials (%d rows for %d blocks) / out",
               args->n_partials, nblocks);
  bool any3d = false;
  for (int l = 0; l < args->num_levels; ++l) {
    DD3D_REQUIRE(args->cls[l] && args->box2d[l], "dd3d_loss_terms: level %d has no cls / box2d map", l);
    any3d |= args->box3d[l] != nullptr;
  }
  DD3D_REQUIRE(!any3d || (args->box3d_t && args->inv_K && args->canon_sizes), "dd3d_loss_terms: box3d maps need box3d targets, inv_K, canon_sizes");
  DD3D_REQUIRE(!args->attributes || (args->speed_off >= 0 && args->attr_off >= 0), "dd3d_loss_terms: nuScenes channels");
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(loss_terms_kernel, dim3((unsigned)nblocks), dim3(LT), 0, s, LossK{*args});
  int e = check_launch("loss_terms_kernel");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(LT), 0, s, LossK{*args}, nblocks);
  return check_launch("loss_finalize_kernel");
}

extern "C" int dd3d_loss_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 64, "dd3d_loss_layout: need 64 slots");
#define OFF(f) (int64_t) offsetof(dd3d_loss_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_loss_args), OFF(cls), OFF(box2d), OFF(box3d), OFF(locations), OFF(gt_off), OFF(gt), OFF(inv_K),
                       OFF(canon_sizes), OFF(labels), OFF(target_inds), OFF(box2d_reg), OFF(ctr_target), OFF(box3d_t), OFF(attributes),
                       OFF(speeds), OFF(flags), OFF(partials), OFF(out), OFF(num_pos), OFF(H), OFF(W), OFF(loc_off), OFF(soi_lo),
                       OFF(soi_hi), OFF(radius), OFF(num_levels), OFF(B), OFF(num_classes), OFF(max_gt), OFF(n_partials), OFF(cls_pitch),
                       OFF(b2d_pitch), OFF(b3d_pitch), OFF(attr_off), OFF(num_attr), OFF(speed_off), OFF(center_sample),
                       OFF(class_agnostic_3d), OFF(scale_depth_by_focal), OFF(allocentric), OFF(depth_is_distance), OFF(min_depth),
                       OFF(max_depth), OFF(focal_factor), OFF(focal_alpha), OFF(focal_gamma), OFF(smooth_l1_beta),
                       OFF(conf3d_temperature), OFF(weight_box3d), OFF(weight_conf3d), OFF(weight_attr), OFF(weight_speed)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
