// Batch-statistics BatchNorm of a head-tower layer for gfx950, forward and backward (include/dd3d_hip.h states the mathematics and the
// order of every sum).  A segment is one (tower, level) pair of the layer; one call serves all segments of a layer.
//
//   bn_slice_kernel<KIND>   block = one slice of DD3D_BN_SLICE pixels of one segment, 256 threads = (C / 4 channel quads) x (P pixel lanes);
//                           a thread walks its lane's pixels with 16-byte loads and keeps one (KIND 2: two) running sum per channel; the
//                           lanes meet in LDS and are added in lane order: one scratch row per slice.  KIND 0: sum c; KIND 1: sum
//                           (c - mu)^2; KIND 2: q = sum ghat and p = sum ghat * xhat.
//   bn_finish_kernel<KIND>  block = (32 channels, segment), 8 lanes per channel over the slice rows, added in lane order.  KIND 0 writes mu;
//                           KIND 1 the variance, rstd, s, t and the running-statistics read-outs; KIND 2 q and p.
//   bn_apply_kernel<MODE>   thread = (pixel, 8 channels): y = relu(fmaf(c - mu, s, beta)) as split planes of MODE (the store of
//                           conv_planes.hip::split_planes_kernel) or as f32.
//   bn_dapply_kernel        thread = (pixel, 4 channels): G_c = s * (ghat - q / N - xhat * p / N).
// All of them are streaming kernels: every element of c (and g, y) is read once per pass.  No float atomics.
#include "bn_common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

template <int MODE>
__global__ __launch_bounds__(BN_T) void bn_apply_kernel(const BnK k) {
  const dd3d_tower_bn_args& a = k.a;
  const int s = blockIdx.y, C = a.C, C8 = C >> 3, M = a.N[s];
  const float* sv = a.stats[s] + DD3D_BN_ROW_S * C;
  const float* mv = a.stats[s] + DD3D_BN_ROW_MU * C;
  const float* bv = a.beta[s];
  const float* in = a.c[s];
  const long total = (long)M * C8;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int m = (int)(t / C8);
    const int c8 = (int)(t - (long)m * C8);
    const float* src = in + (long)m * a.c_pitch + c8 * 8;
    f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 4);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sv + c8 * 8), s1 = *reinterpret_cast<const f32x4*>(sv + c8 * 8 + 4);
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(mv + c8 * 8), m1 = *reinterpret_cast<const f32x4*>(mv + c8 * 8 + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bv + c8 * 8), b1 = *reinterpret_cast<const f32x4*>(bv + c8 * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) x0[e] = fmaxf(fmaf(x0[e] - m0[e], s0[e], b0[e]), 0.f), x1[e] = fmaxf(fmaf(x1[e] - m1[e], s1[e], b1[e]), 0.f);
    bn_store8<MODE>(a, s, M, m, c8, x0, x1);
  }
}

}  // namespace dd3d

extern "C" int64_t dd3d_bn_slices(const dd3d_tower_bn_args* args) {
  using namespace dd3d;
  if (check_bn_shape(args, "dd3d_bn_slices") != DD3D_OK) return -1;
  BnK k;
  k.a = *args;
  plan_bn(k);
  return k.slice_off[args->num_segs];
}

extern "C" int dd3d_bn_batch_stats(const dd3d_tower_bn_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_bn_args(args, "dd3d_bn_batch_stats", 8 | 16);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(args->eps > 0.f && args->momentum >= 0.f && args->momentum <= 1.f, "dd3d_bn_batch_stats: eps = %g, momentum = %g", (double)args->eps,
               (double)args->momentum);
  BnK k;
  k.a = *args;
  plan_bn(k);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 slices((unsigned)k.slice_off[args->num_segs]), fin((unsigned)(args->C / 32), (unsigned)args->num_segs);
  int e;
  hipLaunchKernelGGL(bn_slice_kernel<0>, slices, dim3(BN_T), 0, s, k);
  if ((e = check_launch("bn_slice_kernel<0>")) != DD3D_OK) return e;
  hipLaunchKernelGGL(bn_finish_kernel<0>, fin, dim3(BN_T), 0, s, k);
  if ((e = check_launch("bn_finish_kernel<0>")) != DD3D_OK) return e;
  hipLaunchKernelGGL(bn_slice_kernel<1>, slices, dim3(BN_T), 0, s, k);
  if ((e = check_launch("bn_slice_kernel<1>")) != DD3D_OK) return e;
  hipLaunchKernelGGL(bn_finish_kernel<1>, fin, dim3(BN_T), 0, s, k);
  return check_launch("bn_finish_kernel<1>");
}

extern "C" int dd3d_bn_apply_relu_split(const dd3d_tower_bn_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_bn_args(args, "dd3d_bn_apply_relu_split", 32);
  if (rc != DD3D_OK) return rc;
  if (args->math_mode == DD3D_MATH_F32)
    DD3D_REQUIRE(args->y_pitch % 4 == 0 && args->y_pitch >= args->C, "dd3d_bn_apply_relu_split: y_pitch = %d must be a multiple of 4 and hold %d channels",
                 args->y_pitch, args->C);
  if (args->math_mode == DD3D_MATH_F16X2) DD3D_REQUIRE(args->plane_scale > 0.f, "dd3d_bn_apply_relu_split: plane_scale = %g", (double)args->plane_scale);
  BnK k;
  k.a = *args;
  plan_bn(k);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(stream_blocks((long)max_pixels(args) * (args->C / 8)), (unsigned)args->num_segs);
  switch (args->math_mode) {
    case DD3D_MATH_F32: hipLaunchKernelGGL(bn_apply_kernel<DD3D_MATH_F32>, grid, dim3(BN_T), 0, s, k); break;
    case DD3D_MATH_BF16X3: hipLaunchKernelGGL(bn_apply_kernel<DD3D_MATH_BF16X3>, grid, dim3(BN_T), 0, s, k); break;
    case DD3D_MATH_BF16X2: hipLaunchKernelGGL(bn_apply_kernel<DD3D_MATH_BF16X2>, grid, dim3(BN_T), 0, s, k); break;
    case DD3D_MATH_BF16: hipLaunchKernelGGL(bn_apply_kernel<DD3D_MATH_BF16>, grid, dim3(BN_T), 0, s, k); break;
    case DD3D_MATH_F16X2: hipLaunchKernelGGL(bn_apply_kernel<DD3D_MATH_F16X2>, grid, dim3(BN_T), 0, s, k); break;
    default: DD3D_REQUIRE(false, "dd3d_bn_apply_relu_split: math mode %d", args->math_mode);
  }
  return check_launch("bn_apply_kernel");
}

extern "C" int dd3d_bn_backward_reduce(const dd3d_tower_bn_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_bn_args(args, "dd3d_bn_backward_reduce", 1 | 4 | 16);
  if (rc != DD3D_OK) return rc;
  BnK k;
  k.a = *args;
  plan_bn(k);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(bn_slice_kernel<2>, dim3((unsigned)k.slice_off[args->num_segs]), dim3(BN_T), 0, s, k);
  const int e = check_launch("bn_slice_kernel<2>");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(bn_finish_kernel<2>, dim3((unsigned)(args->C / 32), (unsigned)args->num_segs), dim3(BN_T), 0, s, k);
  return check_launch("bn_finish_kernel<2>");
}

extern "C" int dd3d_bn_backward_apply(const dd3d_tower_bn_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_bn_args(args, "dd3d_bn_backward_apply", 1 | 2 | 4);
  if (rc != DD3D_OK) return rc;
  BnK k;
  k.a = *args;
  plan_bn(k);
  const dim3 grid(stream_blocks((long)max_pixels(args) * (args->C / 4)), (unsigned)args->num_segs);
  hipLaunchKernelGGL(bn_dapply_kernel<true>, grid, dim3(BN_T), 0, reinterpret_cast<hipStream_t>(stream), k);
  return check_launch("bn_dapply_kernel");
}

extern "C" int dd3d_tower_bn_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 32, "dd3d_tower_bn_layout: need 32 slots");
#define OFF(f) (int64_t) offsetof(dd3d_tower_bn_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_tower_bn_args), OFF(c), OFF(gamma), OFF(beta), OFF(run_mean), OFF(run_var), OFF(stats), OFF(y), OFF(g), OFF(qp),
                       OFF(gc), OFF(part), OFF(status), OFF(N), OFF(num_segs), OFF(C), OFF(c_pitch), OFF(g_pitch), OFF(math_mode), OFF(y_mode),
                       OFF(y_pitch), OFF(n_slices), OFF(eps), OFF(momentum), OFF(plane_scale), OFF(reserved)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}