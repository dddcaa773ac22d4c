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
#include "act_load.h"
#include "conv_common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

constexpr int BN_T = 256;
constexpr int BN_LANES = 8;  // bn_finish_kernel: running sums per channel over the slice rows

struct BnK {
  dd3d_tower_bn_args a;
  int slice_off[DD3D_BN_MAX_SEGS + 1];  // first scratch row of every segment
};

static void plan_bn(BnK& k) {
  k.slice_off[0] = 0;
  for (int s = 0; s < DD3D_BN_MAX_SEGS; ++s)
    k.slice_off[s + 1] = k.slice_off[s] + (s < k.a.num_segs ? ceil_div(k.a.N[s], DD3D_BN_SLICE) : 0);
}

template <int KIND>
__global__ __launch_bounds__(BN_T) void bn_slice_kernel(const BnK k) {
  __shared__ float red[2][1024];  // [sum][lane * C + channel]: P * C <= 1024
  const dd3d_tower_bn_args& a = k.a;
  const int slice = blockIdx.x;
  int s = 0;
  while (s + 1 < a.num_segs && slice >= k.slice_off[s + 1]) ++s;
  const int C = a.C, CQ = C >> 2, P = BN_T / CQ;
  const int tid = threadIdx.x, cq = tid % CQ, lane = tid / CQ;
  const int N = a.N[s];
  const int p0 = (slice - k.slice_off[s]) * DD3D_BN_SLICE;
  const int p1 = min(p0 + DD3D_BN_SLICE, N);
  if (lane < P) {
    const float* c = a.c[s] + cq * 4;
    const float* st = a.stats[s] + cq * 4;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f}, mu = acc0, rstd = acc0;
    if constexpr (KIND >= 1) mu = *reinterpret_cast<const f32x4*>(st + DD3D_BN_ROW_MU * C);
    if constexpr (KIND == 2) rstd = *reinterpret_cast<const f32x4*>(st + DD3D_BN_ROW_RSTD * C);
    const float inv = a.y_mode == DD3D_PG_ACT_F16X2 ? 1.0f / a.plane_scale : 1.0f;
    for (int p = p0 + lane; p < p1; p += P) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(c + (long)p * a.c_pitch);
      if constexpr (KIND == 0) {
        acc0 += v;
      } else if constexpr (KIND == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = v[e] - mu[e];
          acc0[e] = fmaf(d, d, acc0[e]);
        }
      } else {
        const f32x4 g = *reinterpret_cast<const f32x4*>(a.g[s] + (long)p * a.g_pitch + cq * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float y = load_act_any(a.y_mode, a.y[s], N, p, cq * 4 + e, a.y_pitch, inv);
          const float gh = y > 0.f ? g[e] : 0.f;
          acc0[e] += gh;
          acc1[e] = fmaf(gh, (v[e] - mu[e]) * rstd[e], acc1[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[0][lane * C + cq * 4 + e] = acc0[e];
      if constexpr (KIND == 2) red[1][lane * C + cq * 4 + e] = acc1[e];
    }
  }
  __syncthreads();
  if (tid < C) {
    float* row = a.part + (long)slice * 2 * C;
    float t0 = 0.f, t1 = 0.f;
    for (int j = 0; j < P; ++j) {
      t0 += red[0][j * C + tid];
      if constexpr (KIND == 2) t1 += red[1][j * C + tid];
    }
    if constexpr (KIND == 1) {
      row[C + tid] = t0;
    } else {
      row[tid] = t0;
      if constexpr (KIND == 2) row[C + tid] = t1;
    }
  }
}

template <int KIND>
__global__ __launch_bounds__(BN_T) void bn_finish_kernel(const BnK k) {
  __shared__ float red[2][BN_LANES][32];
  const dd3d_tower_bn_args& a = k.a;
  const int s = blockIdx.y, C = a.C;
  const int tid = threadIdx.x, ci = tid & 31, lane = tid >> 5, c = blockIdx.x * 32 + ci;
  const int sl0 = k.slice_off[s], sl1 = k.slice_off[s + 1];
  float t0 = 0.f, t1 = 0.f;
  // four of the lane's rows are fetched before they are added, in the lane's order (a row past the end adds an exact zero)
  for (int sl = sl0 + lane; sl < sl1; sl += 4 * BN_LANES) {
    float v0[4], v1[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int r = sl + u * BN_LANES;
      const float* row = a.part + (long)(r < sl1 ? r : sl) * 2 * C;
      v0[u] = r < sl1 ? row[KIND == 1 ? C + c : c] : 0.f;
      v1[u] = (KIND == 2 && r < sl1) ? row[C + c] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) t0 += v0[u], t1 += v1[u];
  }
  red[0][lane][ci] = t0;
  red[1][lane][ci] = t1;
  __syncthreads();
  if (tid >= 32) return;
  t0 = t1 = 0.f;
  for (int j = 0; j < BN_LANES; ++j) t0 += red[0][j][ci], t1 += red[1][j][ci];
  const float n = (float)a.N[s];
  float* st = a.stats[s];
  if constexpr (KIND == 0) {
    st[DD3D_BN_ROW_MU * C + c] = t0 / n;
  } else if constexpr (KIND == 1) {
    const float mu = st[DD3D_BN_ROW_MU * C + c];
    const float v = t0 / n;
    const float rstd = 1.0f / sqrtf(v + a.eps);
    const float sc = a.gamma[s][c] * rstd;
    st[DD3D_BN_ROW_VAR * C + c] = v;
    st[DD3D_BN_ROW_S * C + c] = sc;
    st[DD3D_BN_ROW_T * C + c] = a.beta[s][c] - mu * sc;
    st[DD3D_BN_ROW_RSTD * C + c] = rstd;
    st[DD3D_BN_ROW_RUN_MEAN * C + c] = (1.0f - a.momentum) * a.run_mean[s][c] + a.momentum * mu;
    st[DD3D_BN_ROW_RUN_VAR * C + c] = (1.0f - a.momentum) * a.run_var[s][c] + a.momentum * (v * (n / (n - 1.0f)));
  } else {
    a.qp[s][c] = t0;
    a.qp[s][C + c] = t1;
  }
}

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
    if constexpr (MODE == DD3D_MATH_F32) {
      float* dst = reinterpret_cast<float*>(a.y[s]) + (long)m * a.y_pitch + c8 * 8;
      *reinterpret_cast<f32x4*>(dst) = x0;
      *reinterpret_cast<f32x4*>(dst + 4) = x1;
    } else {
      constexpr int NP = Planes<MODE>::NP;
      if constexpr (Planes<MODE>::F16) {
        int ovf = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          x0[e] *= a.plane_scale, x1[e] *= a.plane_scale;
          ovf |= !(fabsf(x0[e]) <= 65504.f) | !(fabsf(x1[e]) <= 65504.f);
        }
        if (ovf && a.status) atomicOr(a.status, DD3D_STATUS_F16_OVERFLOW);
      }
      unsigned w[4][NP];
      split_pack<MODE>(x0[0], x0[1], w[0]);
      split_pack<MODE>(x0[2], x0[3], w[1]);
      split_pack<MODE>(x1[0], x1[1], w[2]);
      split_pack<MODE>(x1[2], x1[3], w[3]);
      unsigned char* dst = reinterpret_cast<unsigned char*>(a.y[s]) + ((long)(c8 >> 2) * M + m) * (NP * 64) + (c8 & 3) * 16;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        *reinterpret_cast<u32x4*>(dst + p * 64) = u32x4{w[0][p], w[1][p], w[2][p], w[3][p]};
      }
    }
  }
}

__global__ __launch_bounds__(BN_T) void bn_dapply_kernel(const BnK k) {
  const dd3d_tower_bn_args& a = k.a;
  const int s = blockIdx.y, C = a.C, CQ = C >> 2, N = a.N[s];
  const float* st = a.stats[s];
  const float n = (float)N;
  const float inv = a.y_mode == DD3D_PG_ACT_F16X2 ? 1.0f / a.plane_scale : 1.0f;
  const long total = (long)N * CQ;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const int m = (int)(t / CQ);
    const int c0 = (int)(t - (long)m * CQ) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(a.c[s] + (long)m * a.c_pitch + c0);
    const f32x4 g = *reinterpret_cast<const f32x4*>(a.g[s] + (long)m * a.g_pitch + c0);
    const f32x4 mu = *reinterpret_cast<const f32x4*>(st + DD3D_BN_ROW_MU * C + c0);
    const f32x4 rstd = *reinterpret_cast<const f32x4*>(st + DD3D_BN_ROW_RSTD * C + c0);
    const f32x4 sc = *reinterpret_cast<const f32x4*>(st + DD3D_BN_ROW_S * C + c0);
    const f32x4 q = *reinterpret_cast<const f32x4*>(a.qp[s] + c0), p = *reinterpret_cast<const f32x4*>(a.qp[s] + C + c0);
    f32x4 o;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float y = load_act_any(a.y_mode, a.y[s], N, m, c0 + e, a.y_pitch, inv);
      const float gh = y > 0.f ? g[e] : 0.f;
      const float xh = (v[e] - mu[e]) * rstd[e];
      o[e] = sc[e] * ((gh - q[e] / n) - xh * (p[e] / n));
    }
    *reinterpret_cast<f32x4*>(a.gc[s] + (long)m * C + c0) = o;
  }
}

static int check_bn_shape(const dd3d_tower_bn_args* a, const char* who) {
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->num_segs >= 1 && a->num_segs <= DD3D_BN_MAX_SEGS, "%s: %d segments (1 .. %d)", who, a->num_segs, DD3D_BN_MAX_SEGS);
  DD3D_REQUIRE(a->C >= 32 && a->C % 32 == 0 && a->C <= DD3D_BN_MAX_C, "%s: C = %d is not a multiple of 32 up to %d", who, a->C, DD3D_BN_MAX_C);
  long rows = 0;
  for (int s = 0; s < a->num_segs; ++s) {
    DD3D_REQUIRE(a->N[s] >= 2, "%s: segment %d has N = %d (batch statistics need more than 1 value per channel)", who, s, a->N[s]);
    rows += ceil_div(a->N[s], DD3D_BN_SLICE);
  }
  DD3D_REQUIRE(rows < (1l << 24), "%s: %ld slices", who, rows);
  return DD3D_OK;
}

// `need`: bit 0 g / qp, bit 1 gc, bit 2 the stored y as a DD3D_PG_ACT_* storage, bit 3 the statistics' inputs, bit 4 the scratch rows
static int check_bn_args(const dd3d_tower_bn_args* a, const char* who, int need) {
  const int rc = check_bn_shape(a, who);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(a->c_pitch % 4 == 0 && a->c_pitch >= a->C, "%s: c_pitch = %d must be a multiple of 4 and hold %d channels", who, a->c_pitch, a->C);
  if (need & 1) DD3D_REQUIRE(a->g_pitch % 4 == 0 && a->g_pitch >= a->C, "%s: g_pitch = %d must be a multiple of 4 and hold %d channels", who, a->g_pitch, a->C);
  if (need & 4) {
    DD3D_REQUIRE(a->y_mode == DD3D_PG_ACT_F32 || a->y_mode == DD3D_PG_ACT_F16X2 || a->y_mode == DD3D_PG_ACT_BF16X3, "%s: y_mode = %d", who, a->y_mode);
    if (a->y_mode == DD3D_PG_ACT_F32)
      DD3D_REQUIRE(a->y_pitch % 4 == 0 && a->y_pitch >= a->C, "%s: y_pitch = %d must be a multiple of 4 and hold %d channels", who, a->y_pitch, a->C);
    if (a->y_mode == DD3D_PG_ACT_F16X2) DD3D_REQUIRE(a->plane_scale > 0.f, "%s: plane_scale = %g", who, (double)a->plane_scale);
  }
  if (need & 16) {
    BnK k;
    k.a = *a;
    plan_bn(k);
    DD3D_REQUIRE(a->part && a->n_slices >= k.slice_off[a->num_segs], "%s: part (%d scratch rows for %d)", who, a->n_slices, k.slice_off[a->num_segs]);
  }
  for (int s = 0; s < a->num_segs; ++s) {
    DD3D_REQUIRE(a->c[s] && a->stats[s], "%s: segment %d has no convolution output / statistics", who, s);
    if (need & 1) DD3D_REQUIRE(a->g[s] && a->qp[s], "%s: segment %d has no gradient / q, p", who, s);
    if (need & 2) DD3D_REQUIRE(a->gc[s], "%s: segment %d has no output gradient buffer", who, s);
    if (need & (4 | 32)) DD3D_REQUIRE(a->y[s], "%s: segment %d has no layer output", who, s);
    if (need & 32) DD3D_REQUIRE(a->beta[s], "%s: segment %d has no norm bias", who, s);
    if (need & 8) DD3D_REQUIRE(a->gamma[s] && a->beta[s] && a->run_mean[s] && a->run_var[s], "%s: segment %d has no norm parameters / running statistics", who, s);
  }
  return DD3D_OK;
}

static int max_pixels(const dd3d_tower_bn_args* a) {
  int n = 0;
  for (int s = 0; s < a->num_segs; ++s) n = a->N[s] > n ? a->N[s] : n;
  return n;
}

static unsigned stream_blocks(long threads) {
  const long b = (threads + BN_T - 1) / BN_T;
  return (unsigned)(b > 4096 ? 4096 : b);
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
  hipLaunchKernelGGL(bn_dapply_kernel, grid, dim3(BN_T), 0, reinterpret_cast<hipStream_t>(stream), k);
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
