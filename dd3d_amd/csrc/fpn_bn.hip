// Batch-statistics BatchNorm of the FPN's lateral and output convolutions for gfx950 (include/dd3d_hip.h states the mathematics and the
// order of every sum).  A segment is one pyramid stage; one call serves all stages.  The statistics are tower_bn.hip's
// dd3d_bn_batch_stats; this file adds what the towers lack: a norm without a ReLU, and the nearest-x2 top-down sum behind it.
//
//   bn_apply_topdown_kernel<MODE>  thread = (pixel, 8 channels) of one segment: n = fmaf(c - mu, s, beta) of the segment's own pixel, and
//                                  before it the same expression of every linked coarser segment at (y >> k, x >> k), recomputed from
//                                  that segment's raw c, added coarsest first.  The store is bn_common.h's bn_store8 (split planes of
//                                  MODE or f32), plus an optional f32 copy.  A finest-stage thread reads 32 bytes per chain member --
//                                  the coarser ones shared by 4, 16, 64 neighbours, i.e. cache hits -- and writes 32 (f16x2) or 48.
//   bn_slice_kernel<2, false>, bn_finish_kernel<2>, bn_dapply_kernel<false>
//                                  bn_common.h's backward kernels with the mask compiled out: no y is loaded.
// All of them are streaming kernels with 16-byte accesses and one writer per word.  No float atomics.
#include "bn_common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

template <int MODE>
__global__ __launch_bounds__(BN_T) void bn_apply_topdown_kernel(const dd3d_fpn_bn_args f) {
  const dd3d_tower_bn_args& a = f.bn;
  const int s = blockIdx.y, C = a.C, C8 = C >> 3, M = a.N[s];
  const int H = f.H[s], W = f.W[s];
  int depth = 0;  // links above this segment (uniform over the block)
  for (int u = f.up[s]; u >= 0; u = f.up[u]) ++depth;
  const long total = (long)M * C8;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int m = (int)(t / C8);
    const int c8 = (int)(t - (long)m * C8);
    const int x = m % W, r = m / W, y = r % H, b = r / H;
    f32x4 x0 = {0.f, 0.f, 0.f, 0.f}, x1 = x0;
    for (int k = depth; k >= 0; --k) {  // coarsest term first
      int u = s;
      for (int j = 0; j < k; ++j) u = f.up[u];
      const int hk = H >> k, wk = W >> k;
      const long mk = ((long)b * hk + (y >> k)) * wk + (x >> k);
      const float* src = a.c[u] + mk * a.c_pitch + c8 * 8;
      const float* sv = a.stats[u] + DD3D_BN_ROW_S * C + c8 * 8;
      const float* mv = a.stats[u] + DD3D_BN_ROW_MU * C + c8 * 8;
      const float* bv = a.beta[u] + c8 * 8;
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(src), v1 = *reinterpret_cast<const f32x4*>(src + 4);
      const f32x4 s0 = *reinterpret_cast<const f32x4*>(sv), s1 = *reinterpret_cast<const f32x4*>(sv + 4);
      const f32x4 m0 = *reinterpret_cast<const f32x4*>(mv), m1 = *reinterpret_cast<const f32x4*>(mv + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(bv), b1 = *reinterpret_cast<const f32x4*>(bv + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float n0 = fmaf(v0[e] - m0[e], s0[e], b0[e]), n1 = fmaf(v1[e] - m1[e], s1[e], b1[e]);
        x0[e] = k == depth ? n0 : x0[e] + n0;
        x1[e] = k == depth ? n1 : x1[e] + n1;
      }
    }
    if constexpr (MODE != DD3D_MATH_F32) {
      if (f.y32[s]) {
        float* dst = f.y32[s] + (long)m * f.y32_pitch + c8 * 8;
        *reinterpret_cast<f32x4*>(dst) = x0;
        *reinterpret_cast<f32x4*>(dst + 4) = x1;
      }
    }
    bn_store8<MODE>(a, s, M, m, c8, x0, x1);
  }
}

}  // namespace dd3d

extern "C" int dd3d_bn_apply_topdown_split(const dd3d_fpn_bn_args* args, void* stream) {
  using namespace dd3d;
  const char* who = "dd3d_bn_apply_topdown_split";
  DD3D_REQUIRE(args != nullptr, "%s: null args", who);
  const dd3d_tower_bn_args* a = &args->bn;
  const int rc = check_bn_args(a, who, 32);
  if (rc != DD3D_OK) return rc;
  if (a->math_mode == DD3D_MATH_F32)
    DD3D_REQUIRE(a->y_pitch % 4 == 0 && a->y_pitch >= a->C, "%s: y_pitch = %d must be a multiple of 4 and hold %d channels", who, a->y_pitch, a->C);
  if (a->math_mode == DD3D_MATH_F16X2) DD3D_REQUIRE(a->plane_scale > 0.f, "%s: plane_scale = %g", who, (double)a->plane_scale);
  for (int l = 0; l < a->num_segs; ++l)
    DD3D_REQUIRE(args->B[l] >= 1 && args->H[l] >= 1 && args->W[l] >= 1 && (long)args->B[l] * args->H[l] * args->W[l] == (long)a->N[l],
                 "%s: segment %d has N = %d for %d x %d x %d", who, l, a->N[l], args->B[l], args->H[l], args->W[l]);
  for (int l = 0; l < a->num_segs; ++l) {
    const int u = args->up[l];
    DD3D_REQUIRE(u == -1 || (u > l && u < a->num_segs), "%s: segment %d links to %d (-1, or above it and below %d)", who, l, u, a->num_segs);
    if (u >= 0)
      DD3D_REQUIRE(args->B[u] == args->B[l] && 2 * args->H[u] == args->H[l] && 2 * args->W[u] == args->W[l],
                   "%s: segment %d (%d x %d x %d) is not twice its coarser segment %d (%d x %d x %d)", who, l, args->B[l], args->H[l], args->W[l], u,
                   args->B[u], args->H[u], args->W[u]);
    if (args->y32[l] && a->math_mode != DD3D_MATH_F32)
      DD3D_REQUIRE(args->y32_pitch % 4 == 0 && args->y32_pitch >= a->C, "%s: y32_pitch = %d must be a multiple of 4 and hold %d channels", who,
                   args->y32_pitch, a->C);
  }
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(stream_blocks((long)max_pixels(a) * (a->C / 8)), (unsigned)a->num_segs);
  switch (a->math_mode) {
    case DD3D_MATH_F32: hipLaunchKernelGGL(bn_apply_topdown_kernel<DD3D_MATH_F32>, grid, dim3(BN_T), 0, s, *args); break;
    case DD3D_MATH_BF16X3: hipLaunchKernelGGL(bn_apply_topdown_kernel<DD3D_MATH_BF16X3>, grid, dim3(BN_T), 0, s, *args); break;
    case DD3D_MATH_F16X2: hipLaunchKernelGGL(bn_apply_topdown_kernel<DD3D_MATH_F16X2>, grid, dim3(BN_T), 0, s, *args); break;
    default: DD3D_REQUIRE(false, "%s: math mode %d", who, a->math_mode);
  }
  return check_launch("bn_apply_topdown_kernel");
}

extern "C" int dd3d_bn_backward_reduce_linear(const dd3d_tower_bn_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_bn_args(args, "dd3d_bn_backward_reduce_linear", 1 | 16);
  if (rc != DD3D_OK) return rc;
  BnK k;
  k.a = *args;
  plan_bn(k);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL((bn_slice_kernel<2, false>), dim3((unsigned)k.slice_off[args->num_segs]), dim3(BN_T), 0, s, k);
  const int e = check_launch("bn_slice_kernel<2, false>");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(bn_finish_kernel<2>, dim3((unsigned)(args->C / 32), (unsigned)args->num_segs), dim3(BN_T), 0, s, k);
  return check_launch("bn_finish_kernel<2>");
}

extern "C" int dd3d_bn_backward_apply_linear(const dd3d_tower_bn_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_bn_args(args, "dd3d_bn_backward_apply_linear", 1 | 2);
  if (rc != DD3D_OK) return rc;
  BnK k;
  k.a = *args;
  plan_bn(k);
  const dim3 grid(stream_blocks((long)max_pixels(args) * (args->C / 4)), (unsigned)args->num_segs);
  hipLaunchKernelGGL(bn_dapply_kernel<false>, grid, dim3(BN_T), 0, reinterpret_cast<hipStream_t>(stream), k);
  return check_launch("bn_dapply_kernel<false>");
}

extern "C" int dd3d_fpn_bn_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 16, "dd3d_fpn_bn_layout: need 16 slots");
#define OFF(f) (int64_t) offsetof(dd3d_fpn_bn_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_fpn_bn_args), OFF(bn), OFF(y32), OFF(up), OFF(B), OFF(H), OFF(W), OFF(y32_pitch), OFF(reserved)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
