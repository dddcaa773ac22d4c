// Decode of one predicted 3D box from the box3d head map (fcos3d.py:16-52 predictions_to_boxes3d, geometry.py:15-55
// allocentric_to_egocentric, [ext] pytorch3d quaternion_to_matrix / matrix_to_quaternion 0.5.x-0.6.x).  Stated ONCE, as a template over
// the scalar type: float for the inference select/decode kernel (postproc.hip) and the loss kernels (losses.hip), the dual number Du
// (dual.h) for the forward-mode derivative of loss_grads.hip.  The arithmetic is written in +, -, *, / and the scalar operations op_*
// below, each with a float overload here and a Du overload beside Du.  Every operation and its order matter: the inference path is
// compared bit for bit against the reference through the float instantiation.
// The including translation unit turns floating-point contraction off before this header.
#pragma once
#include <math.h>

namespace dd3d {

struct Box3dDecodeParams {
  int scale_depth_by_focal, depth_is_distance, allocentric;
  float focal_factor, min_depth, max_depth;
};

// One box before the batch-wide renormalisation of the egocentric quaternion: q0..q3 and its norm qn; `bad` = qn is not within
// torch.allclose(qn, 1, atol=1e-3) (geometry.py:48-53: if ANY box of the batch is off, every quaternion is divided by its norm).
template <class T = float>
struct Box3dDecoded {
  T q0, q1, q2, q3, qn;
  int bad;
  T cx, cy, depth, s0, s1, s2;
};

constexpr float DECODE_QEPS = 1e-7f;  // tridet/modeling/dd3d/fcos3d.py:13

// The scalar operations of the decode, the corners and GIoU on float.  op_clamp_min is x.clamp(min=m) and op_max / op_min are
// torch.max / torch.min: the same numbers on float, different gradients at a tie on Du (clamp passes 1, max / min split in halves).
__device__ __forceinline__ float op_value(float x) { return x; }  // the number itself: for comparisons, never differentiated
__device__ __forceinline__ float op_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ float op_sqrt_positive(float x) { return x > 0.f ? sqrtf(x) : 0.f; }  // pytorch3d _sqrt_positive_part
__device__ __forceinline__ float op_clamp_min(float x, float m) { return fmaxf(x, m); }
__device__ __forceinline__ float op_clamp(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
__device__ __forceinline__ float op_max(float x, float m) { return fmaxf(x, m); }
__device__ __forceinline__ float op_min(float x, float m) { return fminf(x, m); }
__device__ __forceinline__ float op_tanh(float x) { return tanhf(x); }

// in: the ten decode inputs of the location and class (quat 0-3, ctr 4-5, depth 6, size 7-9); K: the image's K^-1 (row-major); cs:
// canonical size (W,L,H) of the class; (lx, ly): the location.
template <class T>
__device__ __forceinline__ Box3dDecoded<T> decode_box3d(const T (&in)[10], float lx, float ly, const float* K, const float* cs,
                                                        const Box3dDecodeParams& a) {
  Box3dDecoded<T> o;
  T qa = in[0], qb = in[1], qc = in[2], qd = in[3];
  T cx = in[4], cy = in[5];
  T depth = in[6];
  const T s0 = in[7], s1 = in[8], s2 = in[9];
  T q0{0.f}, q1{0.f}, q2{0.f}, q3{0.f}, qn{1.f};
  int bad = 0;
  // quat / max(|quat|, eps), then / |quat| again  (fcos3d.py:31-34)
  T nrm = op_clamp_min(op_sqrt(qa * qa + qb * qb + qc * qc + qd * qd), DECODE_QEPS);
  qa = qa / nrm, qb = qb / nrm, qc = qc / nrm, qd = qd / nrm;
  nrm = op_sqrt(qa * qa + qb * qb + qc * qc + qd * qd);
  qa = qa / nrm, qb = qb / nrm, qc = qc / nrm, qd = qd / nrm;
  if (a.scale_depth_by_focal) {  // fcos3d.py:36-38
    const float pixel_size = sqrtf(K[0] * K[0] + K[4] * K[4]);
    depth = depth / (pixel_size * a.focal_factor);
  }
  if (a.depth_is_distance) {  // fcos3d.py:40-41, ray through the *location*
    const float rx = K[0] * lx + K[1] * ly + K[2], ry = K[3] * lx + K[4] * ly + K[5], rz = K[6] * lx + K[7] * ly + K[8];
    depth = depth / fmaxf(sqrtf(rx * rx + ry * ry + rz * rz), DECODE_QEPS);
  }
  depth = op_clamp(depth, a.min_depth, a.max_depth);
  cx = cx + lx, cy = cy + ly;  // proj_ctr + locations
  if (a.allocentric) {
    // R_obj_to_local = M(q)  ([ext] pytorch3d quaternion_to_matrix)
    const T two_s = 2.0f / (qa * qa + qb * qb + qc * qc + qd * qd);
    const T o00 = 1.f - two_s * (qc * qc + qd * qd), o01 = two_s * (qb * qc - qd * qa), o02 = two_s * (qb * qd + qc * qa);
    const T o10 = two_s * (qb * qc + qd * qa), o11 = 1.f - two_s * (qb * qb + qd * qd), o12 = two_s * (qc * qd - qb * qa);
    const T o20 = two_s * (qb * qd - qc * qa), o21 = two_s * (qc * qd + qb * qa), o22 = 1.f - two_s * (qb * qb + qc * qc);
    // local frame from the viewing ray through proj_ctr  (geometry.py:30-41)
    T zx = K[0] * cx + K[1] * cy + K[2], zy = K[3] * cx + K[4] * cy + K[5], zz = K[6] * cx + K[7] * cy + K[8];
    const T zn = op_sqrt(zx * zx + zy * zy + zz * zz);
    zx = zx / zn, zy = zy / zn, zz = zz / zn;
    T yx = 0.f - zy * zx, yy = 1.f - zy * zy, yz = 0.f - zy * zz;
    const T yn = op_sqrt(yx * yx + yy * yy + yz * yz);
    yx = yx / yn, yy = yy / yn, yz = yz / yn;
    const T xx = yy * zz - yz * zy, xy = yz * zx - yx * zz, xz = yx * zy - yy * zx;  // cross(y, z)
    // R = [x y z] (columns) * R_obj
    const T m00 = xx * o00 + yx * o10 + zx * o20, m01 = xx * o01 + yx * o11 + zx * o21, m02 = xx * o02 + yx * o12 + zx * o22;
    const T m10 = xy * o00 + yy * o10 + zy * o20, m11 = xy * o01 + yy * o11 + zy * o21, m12 = xy * o02 + yy * o12 + zy * o22;
    const T m20 = xz * o00 + yz * o10 + zz * o20, m21 = xz * o01 + yz * o11 + zz * o21, m22 = xz * o02 + yz * o12 + zz * o22;
    // [ext] pytorch3d matrix_to_quaternion (0.5.x/0.6.x): candidate of the largest |component|, no sign canonicalisation
    const T t0 = 1.f + m00 + m11 + m22, t1 = 1.f + m00 - m11 - m22, t2 = 1.f - m00 + m11 - m22, t3 = 1.f - m00 - m11 + m22;
    const T a0 = op_sqrt_positive(t0), a1 = op_sqrt_positive(t1), a2 = op_sqrt_positive(t2), a3 = op_sqrt_positive(t3);
    int best = 0;
    T am = a0;
    if (op_value(a1) > op_value(am)) best = 1, am = a1;
    if (op_value(a2) > op_value(am)) best = 2, am = a2;
    if (op_value(a3) > op_value(am)) best = 3, am = a3;
    const T den = 2.0f * op_max(am, 0.1f);
    if (best == 0) q0 = a0 * a0, q1 = m21 - m12, q2 = m02 - m20, q3 = m10 - m01;
    else if (best == 1) q0 = m21 - m12, q1 = a1 * a1, q2 = m10 + m01, q3 = m02 + m20;
    else if (best == 2) q0 = m02 - m20, q1 = m10 + m01, q2 = a2 * a2, q3 = m12 + m21;
    else q0 = m10 - m01, q1 = m20 + m02, q2 = m21 + m12, q3 = a3 * a3;
    q0 = q0 / den, q1 = q1 / den, q2 = q2 / den, q3 = q3 / den;
    qn = op_sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    bad = !(fabsf(op_value(qn) - 1.0f) <= 1e-3f + 1e-5f);  // torch.allclose(qn, 1, atol=1e-3) with the default rtol
  } else {
    q0 = qa, q1 = qb, q2 = qc, q3 = qd;
  }
  o.q0 = q0, o.q1 = q1, o.q2 = q2, o.q3 = q3, o.qn = qn, o.bad = bad;
  o.cx = cx, o.cy = cy, o.depth = depth;
  o.s0 = (op_tanh(s0) + 1.0f) * cs[0];
  o.s1 = (op_tanh(s1) + 1.0f) * cs[1];
  o.s2 = (op_tanh(s2) + 1.0f) * cs[2];
  return o;
}

// p: the location's row of the box3d map (channel = component * C3 + class)
__device__ __forceinline__ Box3dDecoded<float> decode_box3d(const float* p, int C3, int c3, float lx, float ly, const float* K, const float* cs,
                                                            const Box3dDecodeParams& a) {
  float in[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) in[k] = p[k * C3 + c3];
  return decode_box3d(in, lx, ly, K, cs, a);
}

}  // namespace dd3d
