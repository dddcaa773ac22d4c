// Backward of the training losses of losses.hip with respect to the head maps as loss_terms_kernel reads them: the gradient of
// sum_k upstream[k] * out[k] that torch autograd gives the reference's FCOS2DLoss / FCOS3DLoss / DisentangledBox3DLoss / NuscenesLoss.
//
//   loss_grad_denoms_kernel  one block: the attribute and speed denominators, which out[] does not carry, from the partial slab in the
//                            finalize kernel's summation order; clears the primal-mismatch word.
//   loss_backward_kernel     one thread per target, the indexing of loss_terms_kernel.  A thread writes the complete rows of its location
//                            in the three gradient maps (channels [0, nch); the pad words up to the pitch stay untouched): zeros for a
//                            background row and for the 3D channels of classes other than the label.  No word has two writers, so there
//                            is no memset, no atomic on a float, and two runs agree bit for bit.
// The focal loss, the centerness BCE, the conf BCE, the attribute cross entropy and the speed term have closed forms.  GIoU and the 3D
// decode chain (two normalisations, quaternion_to_matrix, the viewing-ray frame, matrix_to_quaternion's selected candidate, the optional
// batch-wide renormalisation, the depth clamp, tanh sizes, the corners) are differentiated in forward mode on a dual number {value,
// tangent}, one input channel at a time: ten directions per positive, each through the decode and the one or two disentangled groups that
// channel reaches.  The value part of the dual decode restates box3d_decode.h and box_corners operation for operation; the kernel
// compares its entangled corner error with the float path's, bit for bit, and reports a difference in denoms[3].
// Conventions at the non-smooth points are torch's: min / max pass the gradient to the smaller / larger operand and split a tie in
// halves, clamp passes 1 on its closed interval, |x|' = sign(x) with sign(0) = 0, sqrt and the norms have derivative 0 at 0.
#pragma clang fp contract(off)
#include <math.h>

#include "loss_common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

struct LossGradK {
  dd3d_loss_grad_args g;
};

// ------------------------------------------------------------------------------------------------ dual numbers
struct Du {
  float v, d;
};
__device__ __forceinline__ Du operator+(Du a, Du b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Du operator+(Du a, float b) { return {a.v + b, a.d}; }
__device__ __forceinline__ Du operator+(float a, Du b) { return {a + b.v, b.d}; }
__device__ __forceinline__ Du operator-(Du a, Du b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Du operator-(Du a, float b) { return {a.v - b, a.d}; }
__device__ __forceinline__ Du operator-(float a, Du b) { return {a - b.v, 0.f - b.d}; }
__device__ __forceinline__ Du operator*(Du a, Du b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Du operator*(Du a, float b) { return {a.v * b, a.d * b}; }
__device__ __forceinline__ Du operator*(float a, Du b) { return {a * b.v, a * b.d}; }
__device__ __forceinline__ Du operator/(Du a, Du b) {
  const float q = a.v / b.v;
  return {q, (a.d - q * b.d) / b.v};
}
__device__ __forceinline__ Du operator/(Du a, float b) { return {a.v / b, a.d / b}; }
__device__ __forceinline__ Du operator/(float a, Du b) {
  const float q = a / b.v;
  return {q, (0.f - q * b.d) / b.v};
}
__device__ __forceinline__ Du du_sqrt(Du a) {  // derivative 0 at 0: torch's norm backward, and _sqrt_positive_part never sees x <= 0
  const float s = sqrtf(a.v);
  return {s, a.v > 0.f ? a.d / (2.0f * s) : 0.f};
}
__device__ __forceinline__ Du du_sqrt_positive(Du a) { return a.v > 0.f ? du_sqrt(a) : Du{0.f, 0.f}; }
__device__ __forceinline__ Du du_clamp_min(Du a, float m) { return {fmaxf(a.v, m), a.v >= m ? a.d : 0.f}; }  // x.clamp(min=m)
__device__ __forceinline__ Du du_max(Du a, float b) {  // torch.max(a, b): a tie splits in halves
  return {fmaxf(a.v, b), a.v > b ? a.d : (a.v == b ? 0.5f * a.d : 0.f)};
}
__device__ __forceinline__ Du du_min(Du a, float b) { return {fminf(a.v, b), a.v < b ? a.d : (a.v == b ? 0.5f * a.d : 0.f)}; }
__device__ __forceinline__ Du du_tanh(Du a) {
  const float t = tanhf(a.v);
  return {t, (1.0f - t * t) * a.d};
}

// ------------------------------------------------------------------------------------------------ the decode on duals
struct Box3dDual {
  Du q[4], qn, c[2], depth, s[3];
};

// decode_box3d (box3d_decode.h) restated on duals: the value parts are its operations in its order.  Channel `dir` of the ten decode
// inputs (quat 0-3, ctr 4-5, depth 6, size 7-9) carries the tangent 1, the others 0; dir < 0 seeds nothing.
__device__ __forceinline__ Box3dDual decode_box3d_dual(const float* p, int C3, int c3, int dir, float lx, float ly, const float* K, const float* cs,
                                                       const Box3dDecodeParams& a) {
  Box3dDual o;
#define SEED(k) Du{p[(k) * C3 + c3], dir == (k) ? 1.f : 0.f}
  Du qa = SEED(0), qb = SEED(1), qc = SEED(2), qd = SEED(3);
  Du cx = SEED(4), cy = SEED(5);
  Du depth = SEED(6);
  const Du s0 = SEED(7), s1 = SEED(8), s2 = SEED(9);
#undef SEED
  Du q0 = {0.f, 0.f}, q1 = q0, q2 = q0, q3 = q0, qn = {1.f, 0.f};
  Du nrm = du_clamp_min(du_sqrt(qa * qa + qb * qb + qc * qc + qd * qd), DECODE_QEPS);
  qa = qa / nrm, qb = qb / nrm, qc = qc / nrm, qd = qd / nrm;
  nrm = du_sqrt(qa * qa + qb * qb + qc * qc + qd * qd);
  qa = qa / nrm, qb = qb / nrm, qc = qc / nrm, qd = qd / nrm;
  if (a.scale_depth_by_focal) {
    const float pixel_size = sqrtf(K[0] * K[0] + K[4] * K[4]);
    depth = depth / (pixel_size * a.focal_factor);
  }
  if (a.depth_is_distance) {
    const float rx = K[0] * lx + K[1] * ly + K[2], ry = K[3] * lx + K[4] * ly + K[5], rz = K[6] * lx + K[7] * ly + K[8];
    depth = depth / fmaxf(sqrtf(rx * rx + ry * ry + rz * rz), DECODE_QEPS);
  }
  depth = Du{fminf(fmaxf(depth.v, a.min_depth), a.max_depth), (depth.v >= a.min_depth && depth.v <= a.max_depth) ? depth.d : 0.f};
  cx = cx + lx, cy = cy + ly;
  if (a.allocentric) {
    const Du two_s = 2.0f / (qa * qa + qb * qb + qc * qc + qd * qd);
    const Du o00 = 1.f - two_s * (qc * qc + qd * qd), o01 = two_s * (qb * qc - qd * qa), o02 = two_s * (qb * qd + qc * qa);
    const Du o10 = two_s * (qb * qc + qd * qa), o11 = 1.f - two_s * (qb * qb + qd * qd), o12 = two_s * (qc * qd - qb * qa);
    const Du o20 = two_s * (qb * qd - qc * qa), o21 = two_s * (qc * qd + qb * qa), o22 = 1.f - two_s * (qb * qb + qc * qc);
    Du zx = K[0] * cx + K[1] * cy + K[2], zy = K[3] * cx + K[4] * cy + K[5], zz = K[6] * cx + K[7] * cy + K[8];
    const Du zn = du_sqrt(zx * zx + zy * zy + zz * zz);
    zx = zx / zn, zy = zy / zn, zz = zz / zn;
    Du yx = 0.f - zy * zx, yy = 1.f - zy * zy, yz = 0.f - zy * zz;
    const Du yn = du_sqrt(yx * yx + yy * yy + yz * yz);
    yx = yx / yn, yy = yy / yn, yz = yz / yn;
    const Du xx = yy * zz - yz * zy, xy = yz * zx - yx * zz, xz = yx * zy - yy * zx;
    const Du m00 = xx * o00 + yx * o10 + zx * o20, m01 = xx * o01 + yx * o11 + zx * o21, m02 = xx * o02 + yx * o12 + zx * o22;
    const Du m10 = xy * o00 + yy * o10 + zy * o20, m11 = xy * o01 + yy * o11 + zy * o21, m12 = xy * o02 + yy * o12 + zy * o22;
    const Du m20 = xz * o00 + yz * o10 + zz * o20, m21 = xz * o01 + yz * o11 + zz * o21, m22 = xz * o02 + yz * o12 + zz * o22;
    const Du t0 = 1.f + m00 + m11 + m22, t1 = 1.f + m00 - m11 - m22, t2 = 1.f - m00 + m11 - m22, t3 = 1.f - m00 - m11 + m22;
    const Du a0 = du_sqrt_positive(t0), a1 = du_sqrt_positive(t1), a2 = du_sqrt_positive(t2), a3 = du_sqrt_positive(t3);
    int best = 0;
    Du am = a0;
    if (a1.v > am.v) best = 1, am = a1;
    if (a2.v > am.v) best = 2, am = a2;
    if (a3.v > am.v) best = 3, am = a3;
    const Du den = 2.0f * du_max(am, 0.1f);
    if (best == 0) q0 = a0 * a0, q1 = m21 - m12, q2 = m02 - m20, q3 = m10 - m01;
    else if (best == 1) q0 = m21 - m12, q1 = a1 * a1, q2 = m10 + m01, q3 = m02 + m20;
    else if (best == 2) q0 = m02 - m20, q1 = m10 + m01, q2 = a2 * a2, q3 = m12 + m21;
    else q0 = m10 - m01, q1 = m20 + m02, q2 = m21 + m12, q3 = a3 * a3;
    q0 = q0 / den, q1 = q1 / den, q2 = q2 / den, q3 = q3 / den;
    qn = du_sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
  } else {
    q0 = qa, q1 = qb, q2 = qc, q3 = qd;
  }
  o.q[0] = q0, o.q[1] = q1, o.q[2] = q2, o.q[3] = q3, o.qn = qn;
  o.c[0] = cx, o.c[1] = cy, o.depth = depth;
  o.s[0] = (du_tanh(s0) + 1.0f) * cs[0];
  o.s[1] = (du_tanh(s1) + 1.0f) * cs[1];
  o.s[2] = (du_tanh(s2) + 1.0f) * cs[2];
  return o;
}

// box_corners (loss_common.h) restated on duals; element e of the 24 goes to f(e, value) in order
template <class F>
__device__ __forceinline__ void box_corners_dual(const Du* q, const Du* ctr, Du depth, const Du* size, const float* K, F f) {
  const Du r = q[0], i = q[1], j = q[2], k = q[3];
  const Du two_s = 2.0f / (r * r + i * i + j * j + k * k);
  const Du R[9] = {1.f - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                   two_s * (i * j + k * r), 1.f - two_s * (i * i + k * k), two_s * (j * k - i * r),
                   two_s * (i * k - j * r), two_s * (j * k + i * r), 1.f - two_s * (i * i + j * j)};
  const Du u = ctr[0], v = ctr[1];
  const Du t0 = (K[0] * u + K[1] * v + K[2]) * depth, t1 = (K[3] * u + K[4] * v + K[5]) * depth, t2 = (K[6] * u + K[7] * v + K[8]) * depth;
  const Du hl = 0.5f * size[1], hw = 0.5f * size[0], hh = 0.5f * size[2];
  const float sx[8] = {1, 1, 1, 1, -1, -1, -1, -1}, sy[8] = {1, -1, -1, 1, 1, -1, -1, 1}, sz[8] = {1, 1, -1, -1, 1, 1, -1, -1};
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const Du px = hl * sx[c], py = hw * sy[c], pz = hh * sz[c];
    f(3 * c + 0, px * R[0] + py * R[1] + pz * R[2] + t0);
    f(3 * c + 1, px * R[3] + py * R[4] + pz * R[5] + t1);
    f(3 * c + 2, px * R[6] + py * R[7] + pz * R[8] + t2);
  }
}

// d smooth_l1(x, y, beta) / dx (tridet's, loss_common.h): x - y below beta, sign above it, sign everywhere for beta < 1e-5
__device__ __forceinline__ float smooth_l1_grad(float x, float y, float beta) {
  const float r = x - y;
  const float sg = (float)((r > 0.f) - (r < 0.f));
  if (beta < 1e-5f) return sg;
  return fabsf(r) < beta ? r : sg;
}

// IOULoss "giou" (the statement of loss_terms_kernel) on duals
__device__ __forceinline__ Du giou_dual(const Du* p, const float* tg) {
  const Du pl = p[0], pt = p[1], pr_ = p[2], pbm = p[3];
  const float tl = tg[0], tt = tg[1], tr = tg[2], tb = tg[3];
  const float target_area = (tl + tr) * (tt + tb);
  const Du pred_area = (pl + pr_) * (pt + pbm);
  const Du w_int = du_min(pl, tl) + du_min(pr_, tr);
  const Du h_int = du_min(pbm, tb) + du_min(pt, tt);
  const Du gw = du_max(pl, tl) + du_max(pr_, tr);
  const Du gh = du_max(pbm, tb) + du_max(pt, tt);
  const Du ac_union = gw * gh;
  const Du area_int = w_int * h_int;
  const Du area_union = target_area + pred_area - area_int;
  const Du ious = (area_int + 1.0f) / (area_union + 1.0f);
  return ious - (ac_union - area_union) / ac_union;
}

// ------------------------------------------------------------------------------------------------ denominators
__global__ __launch_bounds__(LT) void loss_grad_denoms_kernel(const LossK P, float* denoms, int nblocks) {
  const dd3d_loss_args& a = P.a;
  __shared__ float red[LT];
  __shared__ float S[3];
  const int cols[3] = {T_ATTR_N, T_ATTR_W, T_SPEED_W};
  if (a.attributes) {
    for (int k = 0; k < 3; ++k) {  // the summation of loss_finalize_kernel
      float s = 0.f;
      for (int r = threadIdx.x; r < nblocks; r += LT) s += a.partials[(long)r * DD3D_LOSS_TERMS + cols[k]];
      red[threadIdx.x] = s;
      __syncthreads();
      for (int h = LT / 2; h > 0; h >>= 1) {
        if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
        __syncthreads();
      }
      if (threadIdx.x == 0) S[k] = red[0];
      __syncthreads();
    }
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
  int l = 0;
  while (l + 1 < a.num_levels && n >= (long)a.B * a.loc_off[l + 1]) ++l;
  const int HW = a.H[l] * a.W[l];
  const long rr = n - (long)a.B * a.loc_off[l];
  const int b = (int)(rr / HW), p = (int)(rr - (long)b * HW);
  const long pix = (long)b * HW + p;
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
    const float pr = 1.0f / (1.0f + expf(-xv));
    const float ce = bce_logits(xv, tv);
    const float p_t = pr * tv + (1.f - pr) * (1.f - tv);
    const float m = 1.f - p_t;
    // d(ce m^gamma)/dx with dce/dx = p - t and dm/dx = (1 - 2t) p (1 - p)
    const float mod = a.focal_gamma == 2.0f ? m * m : powf(m, a.focal_gamma);
    const float dmod = a.focal_gamma == 2.0f ? 2.0f * m : a.focal_gamma * powf(m, a.focal_gamma - 1.0f);
    float dv = (pr - tv) * mod + ce * (dmod * ((1.f - 2.f * tv) * (pr * (1.f - pr))));
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
      db2[k] = up[1] * (wden * (0.f - giou_dual(pd, tg).d));  // (1 - gious) * ct / loss_denom
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
  const bool renorm = a.allocentric && *a.flags;
  const float* tb3 = a.box3d_t + n * DD3D_LOSS_BOX3D_FIELDS;
  const float* tK = tb3 + 10;
  float tc[24];
  box_corners(tb3, tb3 + 4, tb3[6], tb3 + 7, tK, tc);
  const float beta = a.smooth_l1_beta;
  {  // loss_conf3d: the entangled error is detached (disentangled_box3d_loss.py:52), so only the BCE's own derivative
    Box3dDual D = decode_box3d_dual(pm, C3, c3, -1, lx, ly, Kp, cs, dp);
    if (renorm) {
      const Du dn = du_clamp_min(D.qn, DECODE_QEPS);
      D.q[0] = D.q[0] / dn, D.q[1] = D.q[1] / dn, D.q[2] = D.q[2] / dn, D.q[3] = D.q[3] / dn;
    }
    float es = 0.f;
    box_corners_dual(D.q, D.c, D.depth, D.s, Kp, [&](int e, Du v) { es += fabsf(tc[e] - v.v); });
    const float err = es / 24.f;
    // the float path of loss_terms_kernel: the dual decode's value part must be the same number, bit for bit
    const Box3dDecoded d = decode_box3d(pm, C3, c3, lx, ly, Kp, cs, dp);
    float q[4] = {d.q0, d.q1, d.q2, d.q3};
    if (renorm) {
      const float dn = fmaxf(d.qn, DECODE_QEPS);
      q[0] /= dn, q[1] /= dn, q[2] /= dn, q[3] /= dn;
    }
    const float pc[2] = {d.cx, d.cy}, ps[3] = {d.s0, d.s1, d.s2};
    float ec[24];
    box_corners(q, pc, d.depth, ps, Kp, ec);
    float fs = 0.f;
#pragma unroll
    for (int e = 0; e < 24; ++e) fs += fabsf(tc[e] - ec[e]);
    const float errf = fs / 24.f;
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
    Box3dDual D = decode_box3d_dual(pm, C3, c3, dir, lx, ly, Kp, cs, dp);
    if (renorm) {
      const Du dn = du_clamp_min(D.qn, DECODE_QEPS);
      D.q[0] = D.q[0] / dn, D.q[1] = D.q[1] / dn, D.q[2] = D.q[2] / dn, D.q[3] = D.q[3] / dn;
    }
    float acc = 0.f;
#pragma unroll 1
    for (int grp = 0; grp < 4; ++grp) {  // quat, proj_ctr, depth, size: the target with that one component replaced by the prediction
      const bool live = grp == 0 ? (dir < 4 || (dir < 6 && a.allocentric)) : grp == 1 ? (dir == 4 || dir == 5) : grp == 2 ? dir == 6 : dir >= 7;
      if (!live) continue;
      Du q[4], c[2], s[3];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = grp == 0 ? D.q[k] : tq[k];
      c[0] = grp == 1 ? D.c[0] : tctr[0], c[1] = grp == 1 ? D.c[1] : tctr[1];
      const Du dep = grp == 2 ? D.depth : tdep;
#pragma unroll
      for (int k = 0; k < 3; ++k) s[k] = grp == 3 ? D.s[k] : tsz[k];
      float sum = 0.f;
      box_corners_dual(q, c, dep, s, tK, [&](int e, Du v) { sum += smooth_l1_grad(v.v, tc[e], beta) * v.d; });
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
