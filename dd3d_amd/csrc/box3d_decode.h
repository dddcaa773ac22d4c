// Decode of one predicted 3D box from the box3d head map (fcos3d.py:16-52 predictions_to_boxes3d, geometry.py:15-55
// allocentric_to_egocentric, [ext] pytorch3d quaternion_to_matrix / matrix_to_quaternion 0.5.x-0.6.x).  Shared by the inference
// select/decode kernel (postproc.hip) and the loss kernel (losses.hip), so both decode with the same operations in the same order.
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
struct Box3dDecoded {
  float q0, q1, q2, q3, qn;
  int bad;
  float cx, cy, depth, s0, s1, s2;
};

constexpr float DECODE_QEPS = 1e-7f;  // tridet/modeling/dd3d/fcos3d.py:13

// p: the location's row of the box3d map (channel = component * C3 + class); K: the image's K^-1 (row-major); cs: canonical size (W,L,H)
// of the class; (lx, ly): the location.
__device__ __forceinline__ Box3dDecoded decode_box3d(const float* p, int C3, int c3, float lx, float ly, const float* K, const float* cs,
                                                     const Box3dDecodeParams& a) {
  Box3dDecoded o;
  float qa = p[0 * C3 + c3], qb = p[1 * C3 + c3], qc = p[2 * C3 + c3], qd = p[3 * C3 + c3];
  float cx = p[4 * C3 + c3], cy = p[5 * C3 + c3];
  float depth = p[6 * C3 + c3];
  const float s0 = p[7 * C3 + c3], s1 = p[8 * C3 + c3], s2 = p[9 * C3 + c3];
  float q0 = 0, q1 = 0, q2 = 0, q3 = 0, qn = 1.f;
  int bad = 0;
  // quat / max(|quat|, eps), then / |quat| again  (fcos3d.py:31-34)
  float nrm = fmaxf(sqrtf(qa * qa + qb * qb + qc * qc + qd * qd), DECODE_QEPS);
  qa /= nrm, qb /= nrm, qc /= nrm, qd /= nrm;
  nrm = sqrtf(qa * qa + qb * qb + qc * qc + qd * qd);
  qa /= nrm, qb /= nrm, qc /= nrm, qd /= nrm;
  if (a.scale_depth_by_focal) {  // fcos3d.py:36-38
    const float pixel_size = sqrtf(K[0] * K[0] + K[4] * K[4]);
    depth = depth / (pixel_size * a.focal_factor);
  }
  if (a.depth_is_distance) {  // fcos3d.py:40-41, ray through the *location*
    const float rx = K[0] * lx + K[1] * ly + K[2], ry = K[3] * lx + K[4] * ly + K[5], rz = K[6] * lx + K[7] * ly + K[8];
    depth = depth / fmaxf(sqrtf(rx * rx + ry * ry + rz * rz), DECODE_QEPS);
  }
  depth = fminf(fmaxf(depth, a.min_depth), a.max_depth);
  cx += lx, cy += ly;  // proj_ctr + locations
  if (a.allocentric) {
    // R_obj_to_local = M(q)  ([ext] pytorch3d quaternion_to_matrix)
    const float two_s = 2.0f / (qa * qa + qb * qb + qc * qc + qd * qd);
    const float o00 = 1 - two_s * (qc * qc + qd * qd), o01 = two_s * (qb * qc - qd * qa), o02 = two_s * (qb * qd + qc * qa);
    const float o10 = two_s * (qb * qc + qd * qa), o11 = 1 - two_s * (qb * qb + qd * qd), o12 = two_s * (qc * qd - qb * qa);
    const float o20 = two_s * (qb * qd - qc * qa), o21 = two_s * (qc * qd + qb * qa), o22 = 1 - two_s * (qb * qb + qc * qc);
    // local frame from the viewing ray through proj_ctr  (geometry.py:30-41)
    float zx = K[0] * cx + K[1] * cy + K[2], zy = K[3] * cx + K[4] * cy + K[5], zz = K[6] * cx + K[7] * cy + K[8];
    const float zn = sqrtf(zx * zx + zy * zy + zz * zz);
    zx /= zn, zy /= zn, zz /= zn;
    float yx = 0.f - zy * zx, yy = 1.f - zy * zy, yz = 0.f - zy * zz;
    const float yn = sqrtf(yx * yx + yy * yy + yz * yz);
    yx /= yn, yy /= yn, yz /= yn;
    const float xx = yy * zz - yz * zy, xy = yz * zx - yx * zz, xz = yx * zy - yy * zx;  // cross(y, z)
    // R = [x y z] (columns) * R_obj
    const float m00 = xx * o00 + yx * o10 + zx * o20, m01 = xx * o01 + yx * o11 + zx * o21, m02 = xx * o02 + yx * o12 + zx * o22;
    const float m10 = xy * o00 + yy * o10 + zy * o20, m11 = xy * o01 + yy * o11 + zy * o21, m12 = xy * o02 + yy * o12 + zy * o22;
    const float m20 = xz * o00 + yz * o10 + zz * o20, m21 = xz * o01 + yz * o11 + zz * o21, m22 = xz * o02 + yz * o12 + zz * o22;
    // [ext] pytorch3d matrix_to_quaternion (0.5.x/0.6.x): candidate of the largest |component|, no sign canonicalisation
    const float t0 = 1.f + m00 + m11 + m22, t1 = 1.f + m00 - m11 - m22, t2 = 1.f - m00 + m11 - m22, t3 = 1.f - m00 - m11 + m22;
    const float a0 = t0 > 0.f ? sqrtf(t0) : 0.f, a1 = t1 > 0.f ? sqrtf(t1) : 0.f;
    const float a2 = t2 > 0.f ? sqrtf(t2) : 0.f, a3 = t3 > 0.f ? sqrtf(t3) : 0.f;
    int best = 0;
    float am = a0;
    if (a1 > am) best = 1, am = a1;
    if (a2 > am) best = 2, am = a2;
    if (a3 > am) best = 3, am = a3;
    const float den = 2.0f * fmaxf(am, 0.1f);
    if (best == 0) q0 = a0 * a0, q1 = m21 - m12, q2 = m02 - m20, q3 = m10 - m01;
    else if (best == 1) q0 = m21 - m12, q1 = a1 * a1, q2 = m10 + m01, q3 = m02 + m20;
    else if (best == 2) q0 = m02 - m20, q1 = m10 + m01, q2 = a2 * a2, q3 = m12 + m21;
    else q0 = m10 - m01, q1 = m20 + m02, q2 = m21 + m12, q3 = a3 * a3;
    q0 /= den, q1 /= den, q2 /= den, q3 /= den;
    qn = sqrtf(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    bad = !(fabsf(qn - 1.0f) <= 1e-3f + 1e-5f);  // torch.allclose(qn, 1, atol=1e-3) with the default rtol
  } else {
    q0 = qa, q1 = qb, q2 = qc, q3 = qd;
  }
  o.q0 = q0, o.q1 = q1, o.q2 = q2, o.q3 = q3, o.qn = qn, o.bad = bad;
  o.cx = cx, o.cy = cy, o.depth = depth;
  o.s0 = (tanhf(s0) + 1.0f) * cs[0];
  o.s1 = (tanhf(s1) + 1.0f) * cs[1];
  o.s2 = (tanhf(s2) + 1.0f) * cs[2];
  return o;
}

}  // namespace dd3d
