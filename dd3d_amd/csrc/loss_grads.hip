// Backward of the training losses of losses.hip with respect to the head maps as loss_terms_kernel reads them: the gradient of
// sum_k upstream[k] * out[k] that torch autograd gives the reference's FCOS2DLoss / FCOS3DLoss / DisentangledBox3DLoss / NuscenesLoss.
//
//   loss_grad_denoms_kernel  one block: the attribute and speed denominators, which out[] does not carry, from the partial slab with the
//                            finalize kernel's column_sum (loss_common.h); clears the primal-mismatch word.
//   loss_backward_kernel     one thread per target, the indexing of loss_terms_kernel.  A thread writes the complete rows of its location
//                            in the three gradient maps (channels [0, nch); the pad words up to the pitch stay untouched): zeros for a
//                            background row and for the 3D channels of classes other than the label.  No word has two writers, so there
//                            is no memset, no atomic on a float, and two runs agree bit for bit.
// The focal loss, the centerness BCE, the conf BCE, the attribute cross entropy and the speed term have closed forms.  GIoU and the 3D
// decode chain (two normalisations, quaternion_to_matrix, the viewing-ray frame, matrix_to_quaternion's selected candidate, the optional
// batch-wide renormalisation, the depth clamp, tanh sizes, the corners) are differentiated in forward mode on a dual number {value,
// tangent}, one input channel at a time: ten directions per positive, each through the decode and the one or two disentangled groups that
// channel reaches.  Decode, corners and GIoU are the templates of box3d_decode.h and loss_common.h that the float kernels instantiate,
// here on Du (dual.h).  The kernel still compares the entangled corner error of its Du instantiation with the float instantiation's,
// bit for bit, and reports a difference in denoms[3]: that guards the value parts of Du's operators and the compiler.
// Conventions at the non-smooth points are torch's (dual.h); |x|' = sign(x) with sign(0) = 0.
#pragma clang fp contract(off)
#include <math.h>

#include "loss_common.h"
#include "dual.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

struct LossGradK {
  dd3d_loss_grad_args g;
};

// The decode on duals: channel `dir` of the ten decode inputs (quat 0-3, ctr 4-5, depth 6, size 7-9) carries the tangent 1, the others 0;
// dir < 0 seeds nothing.
__device__ __forceinline__ Box3dDecoded<Du> decode_box3d_seeded(const float* p, int C3, int c3, int dir, float lx, float ly, const float* K,
                                                                const float* cs, const Box3dDecodeParams& a) {
  Du in[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) in[k] = Du{p[k * C3 + c3], dir == k ? 1.f : 0.f};
  return decode_box3d(in, lx, ly, K, cs, a);
}

// ------------------------------------------------------------------------------------------------ denominators
__global__ __launch_bounds__(LT) void loss_grad_denoms_kernel(const LossK P, float* denoms, int nblocks) {
  const dd3d_loss_args& a = P.a;
  __shared__ float red[LT];
  __shared__ float S[3];
  const int cols[3] = {T_ATTR_N, T_ATTR_W, T_SPEED_W};
  if (a.attributes) {
    for (int k = 0; k < 3; ++k) column_sum(a.partials, nblocks, cols[k], red, &S[k]);  // as loss_finalize_kernel sums them
  }
  if (threadIdx.x != 0) return;
  denoms[0] = a.attributes ? S[0] : 0.f;                       // number of valid attributes
  denoms[1] = a.attributes ? S[1] / fmaxf(S[1], 1e-6f) : 0.f;  // their summed weights over attr_denom
  denoms[2] = a.attributes ? fmaxf(S[2], 1e-6f) : 1.f;         // speed_denom
  reinterpret_cast<int*>(denoms)[3] = 0;                        // primal-mismatch word
}

// ------------------------------------------------------------------------------------------------ per-target gradient rows
__global__ __launch_bounds__(LT) void loss_backward_kernel(const LossK P, const LossGradK G) {
  const dd3d_loss_args& a = P.a;
  const dd3d_loss_grad_args& g = G.g;
  const int nloc = a.loc_off[a.num_levels];
  const long N = (long)a.B * nloc;
  const long n = (long)blockIdx.x * LT + threadIdx.x;
  if (n >= N) return;
  const TargetIndex ti = target_index(a, n);
  const int l = ti.l, b = ti.b, p = ti.p;
  const long pix = ti.pix;
  const int C = a.num_classes;
  const int label = a.labels[n];
  const bool pos = label != C;
  const float* up = g.upstream;
  const float npos = a.out[10], loss_denom = a.out[11];
  const float num_pos_avg = fmaxf(npos, 1.0f);
  const float ct = pos ? a.ctr_target[n] : 0.f;
  const float wden = ct / loss_denom;  // the centerness target over loss_denom: the weight of the box terms

  // ---- cls map: focal loss over every class; attribute and speed channels on nuScenes
  const float* cl = a.cls[l] + pix * a.cls_pitch;
  float* dcl = g.d_cls[l] + pix * a.cls_pitch;
  const float kf = up[0] / num_pos_avg;
  for (int c = 0; c < C; ++c) {
    const float xv = cl[c];
    const float tv = (pos && c == label) ? 1.f : 0.f;
    FocalPieces f;
    focal_pieces(xv, tv, a.focal_gamma, f);
    // d(ce m^gamma)/dx with dce/dx = p - t and dm/dx = (1 - 2t) p (1 - p).  m is exactly 0 in float32 for a confidently classified
    // logit (beyond about +-17): d(m^0)/dm is 0 there as everywhere (torch's pow backward; not 0 * 0^-1 = NaN), gamma >= 1 gives a
    // finite power, and 0 < gamma < 1 gives gamma * 0^(gamma - 1) = inf and a non-finite row, in torch as well: the host refuses
    // that range (engine/losses.py check_loss_config)
    const float dmod = a.focal_gamma == 2.0f ? 2.0f * f.m : a.focal_gamma == 0.0f ? 0.0f : a.focal_gamma * powf(f.m, a.focal_gamma - 1.0f);
    float dv = (f.pr - tv) * f.mod + f.ce * (dmod * ((1.f - 2.f * tv) * (f.pr * (1.f - f.pr))));
    if (a.focal_alpha >= 0.f) dv = (a.focal_alpha * tv + (1.f - a.focal_alpha) * (1.f - tv)) * dv;
    dcl[c] = kf * dv;
  }
  if (a.attributes) {
    const int at = pos ? a.attributes[n] : a.num_attr;
    const float sp = pos ? a.speeds[n] : NAN;
    const float* lg = cl + a.attr_off;
    float m = 0.f, se = 1.f, ka = 0.f;
    if (at != a.num_attr) {
      m = lg[0];
      for (int k = 1; k < a.num_attr; ++k) m = fmaxf(m, lg[k]);
      se = 0.f;
      for (int k = 0; k < a.num_attr; ++k) se += expf(lg[k] - m);
      ka = up[8] * a.weight_attr * (g.denoms[1] / g.denoms[0]);  // mean over the valid attributes, times sum(w) / attr_denom
    }
    const int nch = max(a.attr_off + a.num_attr, a.speed_off + 1);
    for (int ch = C; ch < nch; ++ch) {
      float v = 0.f;
      const int k = ch - a.attr_off;
      if (at != a.num_attr && k >= 0 && k < a.num_attr) v = ka * (expf(lg[k] - m) / se - (k == at ? 1.f : 0.f));
      if (ch == a.speed_off && !isnan(sp)) {  // fvcore's smooth-L1, beta 0.05: (x - y) / beta below beta, sign above
        const float r = cl[ch] - sp;
        const float sg = (float)((r > 0.f) - (r < 0.f));
        v = up[9] * a.weight_speed * (ct / g.denoms[2]) * (fabsf(r) < 0.05f ? r / 0.05f : sg);
      }
      dcl[ch] = v;
    }
  }

  // ---- box2d map: GIoU on the four post-ReLU distances, centerness BCE
  const float* pb = a.box2d[l] + pix * a.b2d_pitch;
  float* db2 = g.d_box2d[l] + pix * a.b2d_pitch;
  if (pos) {
    const float* tg = a.box2d_reg + 4 * n;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const Du pd[4] = {{pb[0], k == 0 ? 1.f : 0.f}, {pb[1], k == 1 ? 1.f : 0.f}, {pb[2], k == 2 ? 1.f : 0.f}, {pb[3], k == 3 ? 1.f : 0.f}};
      db2[k] = up[1] * (wden * (0.f - giou(pd, tg).d));  // (1 - gious) * ct / loss_denom
    }
    db2[4] = up[2] * ((1.0f / (1.0f + expf(-pb[4])) - ct) / num_pos_avg);
  } else {
#pragma unroll
    for (int k = 0; k < 5; ++k) db2[k] = 0.f;
  }

  // ---- box3d map
  if (a.box3d[l] == nullptr) return;
  const int C3 = a.class_agnostic_3d ? 1 : C, c3 = a.class_agnostic_3d ? 0 : label;
  float* db3 = g.d_box3d[l] + pix * a.b3d_pitch;
  for (int ch = 0; ch < 11 * C3; ++ch) {
    if (!pos || ch % C3 != c3) db3[ch] = 0.f;
  }
  if (!pos) return;
  const float* pm = a.box3d[l] + pix * a.b3d_pitch;
  const int i = a.loc_off[l] + p;
  const float lx = a.locations[2 * i], ly = a.locations[2 * i + 1];
  const float* Kp = a.inv_K + 9 * b;
  const float* cs = a.canon_sizes + 3 * label;
  const Box3dDecodeParams dp{a.scale_depth_by_focal, a.depth_is_distance, a.allocentric, a.focal_factor, a.min_depth, a.max_depth};
  const float* tb3 = a.box3d_t + n * DD3D_LOSS_BOX3D_FIELDS;
  const float* tK = tb3 + 10;
  float tc[24];
  box_corners(tb3, tb3 + 4, tb3[6], tb3 + 7, tK, tc);
  const float beta = a.smooth_l1_beta;
  {  // loss_conf3d: the entangled error is detached (disentangled_box3d_loss.py:52), so only the BCE's own derivative
    const Box3dDecoded<Du> D = decode_box3d_seeded(pm, C3, c3, -1, lx, ly, Kp, cs, dp);
    Du Dq[4];
    decoded_quat(D, a.allocentric, a.flags, Dq);
    const Du Dc[2] = {D.cx, D.cy}, Ds[3] = {D.s0, D.s1, D.s2};
    const float err = entangled_error(tc, Dq, Dc, D.depth, Ds, Kp);
    // the float instantiation, what loss_terms_kernel computes: the Du instantiation's value part must be the same number, bit for bit
    const Box3dDecoded d = decode_box3d(pm, C3, c3, lx, ly, Kp, cs, dp);
    float q[4];
    decoded_quat(d, a.allocentric, a.flags, q);
    const float pc[2] = {d.cx, d.cy}, ps[3] = {d.s0, d.s1, d.s2};
    const float errf = entangled_error(tc, q, pc, d.depth, ps, Kp);
    if (__float_as_int(errf) != __float_as_int(err) && !(isnan(errf) && isnan(err))) atomicOr(reinterpret_cast<int*>(g.denoms) + 3, 1);
    const float conf_t = expf(-1.f / a.conf3d_temperature * err);
    db3[10 * C3 + c3] = up[7] * ((a.weight_conf3d * wden) * (1.0f / (1.0f + expf(-pm[10 * C3 + c3])) - conf_t));
  }
  const Du tq[4] = {{tb3[0], 0.f}, {tb3[1], 0.f}, {tb3[2], 0.f}, {tb3[3], 0.f}};
  const Du tctr[2] = {{tb3[4], 0.f}, {tb3[5], 0.f}};
  const Du tdep = {tb3[6], 0.f};
  const Du tsz[3] = {{tb3[7], 0.f}, {tb3[8], 0.f}, {tb3[9], 0.f}};
#pragma unroll 1
  for (int dir = 0; dir < 10; ++dir) {
    const Box3dDecoded<Du> D = decode_box3d_seeded(pm, C3, c3, dir, lx, ly, Kp, cs, dp);
    Du Dq[4];
    decoded_quat(D, a.allocentric, a.flags, Dq);
    const Du Dc[2] = {D.cx, D.cy}, Ds[3] = {D.s0, D.s1, D.s2};
    float acc = 0.f;
#pragma unroll 1
    for (int grp = 0; grp < 4; ++grp) {  // quat, proj_ctr, depth, size: the target with that one component replaced by the prediction
      const bool live = grp == 0 ? (dir < 4 || (dir < 6 && a.allocentric)) : grp == 1 ? (dir == 4 || dir == 5) : grp == 2 ? dir == 6 : dir >= 7;
      if (!live) continue;
      Du q[4], c[2], s[3];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = grp == 0 ? Dq[k] : tq[k];
      c[0] = grp == 1 ? Dc[0] : tctr[0], c[1] = grp == 1 ? Dc[1] : tctr[1];
      const Du dep = grp == 2 ? D.depth : tdep;
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] = grp == 3 ? Ds[k] : tsz[k];
      float sum = 0.f;
      box_corners_to(q, c, dep, s, tK, [&](int e, Du v) { sum += smooth_l1_grad(v.v, tc[e], beta) * v.d; });
      acc += up[3 + grp] * (a.weight_box3d * ((sum / 24.f) * wden));
    }
    db3[dir * C3 + c3] = acc;
  }
}

}  // namespace dd3d

extern "C" int dd3d_loss_backward(const dd3d_loss_args* args, const dd3d_loss_grad_args* grads, void* stream) {
  using namespace dd3d;
  const int rc = check_args(args, "dd3d_loss_backward");
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(grads != nullptr && grads->upstream && grads->denoms, "dd3d_loss_backward: null grads / upstream / denoms");
  const long N = (long)args->B * args->loc_off[args->num_levels];
  const int nblocks = (int)((N + LT - 1) / LT);
  DD3D_REQUIRE(args->partials && args->out && args->n_partials >= nblocks, "dd3d_loss_backward: partials (%d rows for %d blocks) / out",
               args->n_partials, nblocks);
  const int C3 = args->class_agnostic_3d ? 1 : args->num_classes;
  int ncls = args->num_classes;
  if (args->attributes) {
    DD3D_REQUIRE(args->speed_off >= args->num_classes && args->attr_off >= args->num_classes, "dd3d_loss_backward: nuScenes channels");
    ncls = args->attr_off + args->num_attr > args->speed_off + 1 ? args->attr_off + args->num_attr : args->speed_off + 1;
  }
  DD3D_REQUIRE(ncls <= args->cls_pitch && 5 <= args->b2d_pitch, "dd3d_loss_backward: cls_pitch = %d (%d channels), b2d_pitch = %d", args->cls_pitch,
               ncls, args->b2d_pitch);
  bool any3d = false;
  for (int l = 0; l < args->num_levels; ++l) {
    DD3D_REQUIRE(args->cls[l] && args->box2d[l] && grads->d_cls[l] && grads->d_box2d[l], "dd3d_loss_backward: level %d has no cls / box2d map or gradient", l);
    DD3D_REQUIRE(!args->box3d[l] || grads->d_box3d[l], "dd3d_loss_backward: level %d has a box3d map and no gradient buffer", l);
    any3d |= args->box3d[l] != nullptr;
  }
  DD3D_REQUIRE(!any3d || (args->box3d_t && args->inv_K && args->canon_sizes && 11 * C3 <= args->b3d_pitch),
               "dd3d_loss_backward: box3d maps need box3d targets, inv_K, canon_sizes and b3d_pitch >= %d", 11 * C3);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(loss_grad_denoms_kernel, dim3(1), dim3(LT), 0, s, LossK{*args}, grads->denoms, nblocks);
  int e = check_launch("loss_grad_denoms_kernel");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(loss_backward_kernel, dim3((unsigned)nblocks), dim3(LT), 0, s, LossK{*args}, LossGradK{*grads});
  return check_launch("loss_backward_kernel");
}

extern "C" int dd3d_loss_grad_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 8, "dd3d_loss_grad_layout: need 8 slots");
#define OFF(f) (int64_t) offsetof(dd3d_loss_grad_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_loss_grad_args), OFF(d_cls), OFF(d_box2d), OFF(d_box3d), OFF(upstream), OFF(denoms)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
