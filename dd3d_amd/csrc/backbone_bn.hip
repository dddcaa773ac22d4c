// Batch-statistics BatchNorm of the DLA-34 bottom-up network for gfx950, forward and backward (include/dd3d_hip.h states the mathematics
// and the order of every sum).  A segment is one norm.  The reductions and the backward apply are bn_common.h's kernels -- the ones the
// head towers and the FPN run, so the sums keep their order and, at the widths those take, their bits -- behind argument checks of their
// own: C = 16 (the stem: 64 one-pixel lanes per slice), multiples of 32 up to 256, and 512 (level5: two chunks of 256 channels on
// blockIdx.y).  This file adds the apply:
//
//   bbn_apply_kernel<MODE, ACT>  thread = (pixel, 8 channels): n = fmaf(c - mu, s, beta), then relu(n), n or relu(n + r) with r the stored
//                                residual (f32 NHWC or split planes, eight channels in two / two / three 16-byte loads), stored as split
//                                planes of MODE (bn_store8) and / or f32 NHWC, either of them a channel slice of a wider buffer.  At
//                                C = 16 two threads share a pixel: every lane of a wave works.  Per thread 32 bytes of c are read, 32 of
//                                an f32 residual (16 / 24 of a split one) and 32 (f16x2) to 80 (bf16x3 + f32) written.
// All of them are streaming kernels with 16-byte accesses and one writer per word.  No float atomics.
#include "bn_common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

typedef unsigned bbn_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bbn_half_lo(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
__device__ __forceinline__ float bbn_half_hi(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }

// Channels c0 .. c0 + 7 (c0 a multiple of 8) of pixel m of a stored tensor with M pixels, decoded as act_load.h::load_act decodes one value.
__device__ __forceinline__ void bbn_load_res8(int mode, const void* base, long M, long m, int c0, int pitch, float inv_scale, float (&r)[8]) {
  if (mode == DD3D_PG_ACT_F32) {
    const float* p = reinterpret_cast<const float*>(base) + m * pitch + c0;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = a[e], r[4 + e] = b[e];
  } else if (mode == DD3D_PG_ACT_F16X2) {  // [c / 32][pixel][hi, lo][32] halves of value * plane_scale
    const unsigned char* p = reinterpret_cast<const unsigned char*>(base) + ((long)(c0 >> 5) * M + m) * 128 + (c0 & 31) * 2;
    const bbn_u32x4 hi = *reinterpret_cast<const bbn_u32x4*>(p), lo = *reinterpret_cast<const bbn_u32x4*>(p + 64);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[2 * e] = (bbn_half_lo(hi[e]) + bbn_half_lo(lo[e])) * inv_scale;
      r[2 * e + 1] = (bbn_half_hi(hi[e]) + bbn_half_hi(lo[e])) * inv_scale;
    }
  } else {  // [c / 32][pixel][hi, mid, lo][32] bf16 terms: (hi + mid) + lo
    const unsigned char* p = reinterpret_cast<const unsigned char*>(base) + ((long)(c0 >> 5) * M + m) * 192 + (c0 & 31) * 2;
    const bbn_u32x4 hi = *reinterpret_cast<const bbn_u32x4*>(p), mid = *reinterpret_cast<const bbn_u32x4*>(p + 64),
                    lo = *reinterpret_cast<const bbn_u32x4*>(p + 128);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      r[2 * e] = (__uint_as_float(hi[e] << 16) + __uint_as_float(mid[e] << 16)) + __uint_as_float(lo[e] << 16);
      r[2 * e + 1] = (__uint_as_float(hi[e] & 0xffff0000u) + __uint_as_float(mid[e] & 0xffff0000u)) + __uint_as_float(lo[e] & 0xffff0000u);
    }
  }
}

template <int MODE, int ACT>
__global__ __launch_bounds__(BN_T) void bbn_apply_kernel(const dd3d_backbone_bn_args f) {
  const dd3d_tower_bn_args& a = f.bn;
  const int s = blockIdx.y, C = a.C, C8 = C >> 3, M = a.N[s];
  const float* sv = a.stats[s] + DD3D_BN_ROW_S * C;
  const float* mv = a.stats[s] + DD3D_BN_ROW_MU * C;
  const float* bv = a.beta[s];
  const float* in = a.c[s];
  const float res_inv = f.res_mode == DD3D_PG_ACT_F16X2 ? 1.0f / f.res_plane_scale : 1.0f;
  const long total = (long)M * C8;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int m = (int)(t / C8);
    const int c8 = (int)(t - (long)m * C8);
    const float* src = in + (long)m * a.c_pitch + c8 * 8;
    f32x4 x0 = *reinterpret_cast<const f32x4*>(src), x1 = *reinterpret_cast<const f32x4*>(src + 4);
    float r[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if constexpr (ACT == DD3D_BBN_RESIDUAL) bbn_load_res8(f.res_mode, f.res[s], M, m, c8 * 8, f.res_pitch, res_inv, r);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sv + c8 * 8), s1 = *reinterpret_cast<const f32x4*>(sv + c8 * 8 + 4);
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(mv + c8 * 8), m1 = *reinterpret_cast<const f32x4*>(mv + c8 * 8 + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(bv + c8 * 8), b1 = *reinterpret_cast<const f32x4*>(bv + c8 * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float n0 = fmaf(x0[e] - m0[e], s0[e], b0[e]), n1 = fmaf(x1[e] - m1[e], s1[e], b1[e]);
      if constexpr (ACT == DD3D_BBN_RESIDUAL) n0 += r[e], n1 += r[4 + e];
      if constexpr (ACT != DD3D_BBN_LINEAR) n0 = fmaxf(n0, 0.f), n1 = fmaxf(n1, 0.f);
      x0[e] = n0, x1[e] = n1;
    }
    if constexpr (MODE != DD3D_MATH_F32) {
      if (f.y32[s]) {
        float* dst = f.y32[s] + (long)m * f.y32_pitch + c8 * 8;
        *reinterpret_cast<f32x4*>(dst) = x0;
        *reinterpret_cast<f32x4*>(dst + 4) = x1;
      }
      if (a.y[s]) bn_store8<MODE>(a, s, M, m, c8, x0, x1);
    } else {
      bn_store8<MODE>(a, s, M, m, c8, x0, x1);
    }
  }
}

template <int MODE>
static void launch_bbn_apply(const dd3d_backbone_bn_args& f, dim3 grid, hipStream_t s) {
  switch (f.act) {
    case DD3D_BBN_RELU: hipLaunchKernelGGL((bbn_apply_kernel<MODE, DD3D_BBN_RELU>), grid, dim3(BN_T), 0, s, f); break;
    case DD3D_BBN_LINEAR: hipLaunchKernelGGL((bbn_apply_kernel<MODE, DD3D_BBN_LINEAR>), grid, dim3(BN_T), 0, s, f); break;
    default: hipLaunchKernelGGL((bbn_apply_kernel<MODE, DD3D_BBN_RESIDUAL>), grid, dim3(BN_T), 0, s, f); break;
  }
}

// the slice launches of a wide call: one block per (slice, chunk of up to 256 channels)
static dim3 bbn_slice_grid(const BnK& k) { return dim3((unsigned)k.slice_off[k.a.num_segs], (unsigned)ceil_div(k.a.C, BN_T)); }
static dim3 bbn_finish_grid(const BnK& k) { return dim3((unsigned)ceil_div(k.a.C, 32), (unsigned)k.a.num_segs); }

template <bool MASK>
static int bbn_backward_reduce(const dd3d_tower_bn_args* args, void* stream, const char* who) {
  const int rc = check_bn_args(args, who, MASK ? (1 | 4 | 16) : (1 | 16), true);
  if (rc != DD3D_OK) return rc;
  if (MASK && args->y_mode != DD3D_PG_ACT_F32) DD3D_REQUIRE(args->C % 32 == 0, "%s: a stored y in split planes needs C %% 32 == 0 (C = %d)", who, args->C);
  BnK k;
  k.a = *args;
  plan_bn(k);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL((bn_slice_kernel<2, MASK>), bbn_slice_grid(k), dim3(BN_T), 0, s, k);
  const int e = check_launch("bn_slice_kernel<2>");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(bn_finish_kernel<2>, bbn_finish_grid(k), dim3(BN_T), 0, s, k);
  return check_launch("bn_finish_kernel<2>");
}

template <bool MASK>
static int bbn_backward_apply(const dd3d_tower_bn_args* args, void* stream, const char* who) {
  const int rc = check_bn_args(args, who, MASK ? (1 | 2 | 4) : (1 | 2), true);
  if (rc != DD3D_OK) return rc;
  if (MASK && args->y_mode != DD3D_PG_ACT_F32) DD3D_REQUIRE(args->C % 32 == 0, "%s: a stored y in split planes needs C %% 32 == 0 (C = %d)", who, args->C);
  BnK k;
  k.a = *args;
  plan_bn(k);
  const dim3 grid(stream_blocks((long)max_pixels(args) * (args->C / 4)), (unsigned)args->num_segs);
  hipLaunchKernelGGL(bn_dapply_kernel<MASK>, grid, dim3(BN_T), 0, reinterpret_cast<hipStream_t>(stream), k);
  return check_launch("bn_dapply_kernel");
}

}  // namespace dd3d

extern "C" int64_t dd3d_backbone_bn_slices(const dd3d_tower_bn_args* args) {
  using namespace dd3d;
  if (check_bn_shape(args, "dd3d_backbone_bn_slices", true) != DD3D_OK) return -1;
  BnK k;
  k.a = *args;
  plan_bn(k);
  return k.slice_off[args->num_segs];
}

extern "C" int dd3d_backbone_bn_batch_stats(const dd3d_tower_bn_args* args, void* stream) {
  using namespace dd3d;
  const char* who = "dd3d_backbone_bn_batch_stats";
  const int rc = check_bn_args(args, who, 8 | 16, true);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(args->eps > 0.f && args->momentum >= 0.f && args->momentum <= 1.f, "%s: eps = %g, momentum = %g", who, (double)args->eps,
               (double)args->momentum);
  BnK k;
  k.a = *args;
  plan_bn(k);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 slices = bbn_slice_grid(k), fin = bbn_finish_grid(k);
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

extern "C" int dd3d_backbone_bn_apply(const dd3d_backbone_bn_args* args, void* stream) {
  using namespace dd3d;
  const char* who = "dd3d_backbone_bn_apply";
  DD3D_REQUIRE(args != nullptr, "%s: null args", who);
  const dd3d_tower_bn_args* a = &args->bn;
  const int rc = check_bn_args(a, who, 0, true);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(args->act == DD3D_BBN_RELU || args->act == DD3D_BBN_LINEAR || args->act == DD3D_BBN_RESIDUAL, "%s: act = %d", who, args->act);
  const bool f32 = a->math_mode == DD3D_MATH_F32;
  DD3D_REQUIRE(f32 || a->math_mode == DD3D_MATH_F16X2 || a->math_mode == DD3D_MATH_BF16X3, "%s: math mode %d (f32, f16x2 or bf16x3)", who, a->math_mode);
  if (f32) DD3D_REQUIRE(a->y_pitch % 4 == 0 && a->y_pitch >= a->C, "%s: y_pitch = %d must be a multiple of 4 and hold %d channels", who, a->y_pitch, a->C);
  if (a->math_mode == DD3D_MATH_F16X2) DD3D_REQUIRE(a->plane_scale > 0.f, "%s: plane_scale = %g", who, (double)a->plane_scale);
  if (args->act == DD3D_BBN_RESIDUAL) {
    DD3D_REQUIRE(args->res_mode == DD3D_PG_ACT_F32 || args->res_mode == DD3D_PG_ACT_F16X2 || args->res_mode == DD3D_PG_ACT_BF16X3, "%s: res_mode = %d", who,
                 args->res_mode);
    if (args->res_mode == DD3D_PG_ACT_F32)
      DD3D_REQUIRE(args->res_pitch % 4 == 0 && args->res_pitch >= a->C, "%s: res_pitch = %d must be a multiple of 4 and hold %d channels", who, args->res_pitch,
                   a->C);
    else
      DD3D_REQUIRE(a->C % 32 == 0, "%s: a residual in split planes needs C %% 32 == 0 (C = %d)", who, a->C);
    if (args->res_mode == DD3D_PG_ACT_F16X2) DD3D_REQUIRE(args->res_plane_scale > 0.f, "%s: res_plane_scale = %g", who, (double)args->res_plane_scale);
  }
  for (int l = 0; l < a->num_segs; ++l) {
    DD3D_REQUIRE(a->beta[l], "%s: segment %d has no norm bias", who, l);
    if (args->act == DD3D_BBN_RESIDUAL) DD3D_REQUIRE(args->res[l], "%s: segment %d has no residual", who, l);
    if (f32) {
      DD3D_REQUIRE(a->y[l], "%s: segment %d has no layer output", who, l);
    } else {
      DD3D_REQUIRE(a->y[l] || args->y32[l], "%s: segment %d has neither split planes nor an f32 output", who, l);
      if (a->y[l]) DD3D_REQUIRE(a->C % 32 == 0, "%s: split planes need C %% 32 == 0 (C = %d)", who, a->C);
      if (args->y32[l])
        DD3D_REQUIRE(args->y32_pitch % 4 == 0 && args->y32_pitch >= a->C, "%s: y32_pitch = %d must be a multiple of 4 and hold %d channels", who,
                     args->y32_pitch, a->C);
    }
  }
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(stream_blocks((long)max_pixels(a) * (a->C / 8)), (unsigned)a->num_segs);
  switch (a->math_mode) {
    case DD3D_MATH_F32: launch_bbn_apply<DD3D_MATH_F32>(*args, grid, s); break;
    case DD3D_MATH_BF16X3: launch_bbn_apply<DD3D_MATH_BF16X3>(*args, grid, s); break;
    default: launch_bbn_apply<DD3D_MATH_F16X2>(*args, grid, s); break;
  }
  return check_launch("bbn_apply_kernel");
}

extern "C" int dd3d_backbone_bn_backward_reduce(const dd3d_tower_bn_args* args, void* stream) {
  return dd3d::bbn_backward_reduce<true>(args, stream, "dd3d_backbone_bn_backward_reduce");
}

extern "C" int dd3d_backbone_bn_backward_apply(const dd3d_tower_bn_args* args, void* stream) {
  return dd3d::bbn_backward_apply<true>(args, stream, "dd3d_backbone_bn_backward_apply");
}

extern "C" int dd3d_backbone_bn_backward_reduce_linear(const dd3d_tower_bn_args* args, void* stream) {
  return dd3d::bbn_backward_reduce<false>(args, stream, "dd3d_backbone_bn_backward_reduce_linear");
}

extern "C" int dd3d_backbone_bn_backward_apply_linear(const dd3d_tower_bn_args* args, void* stream) {
  return dd3d::bbn_backward_apply<false>(args, stream, "dd3d_backbone_bn_backward_apply_linear");
}

extern "C" int dd3d_backbone_bn_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 16, "dd3d_backbone_bn_layout: need 16 slots");
#define OFF(f) (int64_t) offsetof(dd3d_backbone_bn_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_backbone_bn_args), OFF(bn), OFF(y32), OFF(res), OFF(act), OFF(res_mode), OFF(res_pitch), OFF(y32_pitch),
                       OFF(res_plane_scale), OFF(reserved)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
