// What the batch-statistics BatchNorm translation units share (tower_bn.hip: the head towers, behind a ReLU; fpn_bn.hip: the FPN,
// without one; backbone_bn.hip: the DLA-34 bottom-up network, widths 16 .. 512 -- `wide` in the checks): the slice / finish reductions, the backward apply, the split-plane store of an 8-channel group and the argument
// checks.  MASK = true gates the gradient with the sign of the stored output y; MASK = false reads no y at all and computes what
// MASK = true computes for a y of ones, bit for bit.  include/dd3d_hip.h states the mathematics and the order of every sum.
#pragma once
#include "act_load.h"
#include "conv_common.h"

namespace dd3d {
namespace {

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

// Stores 8 consecutive channels (c8 * 8 ...) of pixel m of segment s, M pixels: MODE DD3D_MATH_F32 as f32 NHWC of pitch y_pitch, else as the
// split planes of MODE -- the store of conv_planes.hip::split_planes_kernel, its overflow bit included.
template <int MODE>
__device__ __forceinline__ void bn_store8(const dd3d_tower_bn_args& a, int s, int M, int m, int c8, f32x4 x0, f32x4 x1) {
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

template <int KIND, bool MASK = true>
__global__ __launch_bounds__(BN_T) void bn_slice_kernel(const BnK k) {
  __shared__ float red[2][1024];  // [sum][lane * C + channel]: P * C <= 1024
  const dd3d_tower_bn_args& a = k.a;
  const int slice = blockIdx.x;
  int s = 0;
  while (s + 1 < a.num_segs && slice >= k.slice_off[s + 1]) ++s;
  // a block takes min(C, 256) channels: C <= 256 is one chunk (blockIdx.y = 0), the backbone's C = 512 two (backbone_bn.hip)
  const int C = a.C, CB = C < BN_T ? C : BN_T, ch0 = (int)blockIdx.y * CB, CQ = CB >> 2, P = BN_T / CQ;
  const int tid = threadIdx.x, cq = tid % CQ, lane = tid / CQ;
  const int N = a.N[s];
  const int p0 = (slice - k.slice_off[s]) * DD3D_BN_SLICE;
  const int p1 = min(p0 + DD3D_BN_SLICE, N);
  if (lane < P) {
    const float* c = a.c[s] + ch0 + cq * 4;
    const float* st = a.stats[s] + ch0 + cq * 4;
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
        const f32x4 g = *reinterpret_cast<const f32x4*>(a.g[s] + (long)p * a.g_pitch + ch0 + cq * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          float gh = g[e];
          if constexpr (MASK) gh = load_act_any(a.y_mode, a.y[s], N, p, ch0 + cq * 4 + e, a.y_pitch, inv) > 0.f ? gh : 0.f;
          acc0[e] += gh;
          acc1[e] = fmaf(gh, (v[e] - mu[e]) * rstd[e], acc1[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      red[0][lane * CB + cq * 4 + e] = acc0[e];
      if constexpr (KIND == 2) red[1][lane * CB + cq * 4 + e] = acc1[e];
    }
  }
  __syncthreads();
  if (tid < CB) {
    float* row = a.part + (long)slice * 2 * C + ch0;
    float t0 = 0.f, t1 = 0.f;
    for (int j = 0; j < P; ++j) {
      t0 += red[0][j * CB + tid];
      if constexpr (KIND == 2) t1 += red[1][j * CB + tid];
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
  const int tid = threadIdx.x, ci = tid & 31, lane = tid >> 5;
  const bool live = (int)blockIdx.x * 32 + ci < C;  // (C = 16, backbone_bn.hip: the upper half of the block reads channel 0 and stores nothing)
  const int c = live ? blockIdx.x * 32 + ci : 0;
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
  if (tid >= 32 || !live) return;
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

template <bool MASK = true>
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
      float gh = g[e];
      if constexpr (MASK) gh = load_act_any(a.y_mode, a.y[s], N, m, c0 + e, a.y_pitch, inv) > 0.f ? gh : 0.f;
      const float xh = (v[e] - mu[e]) * rstd[e];
      o[e] = sc[e] * ((gh - q[e] / n) - xh * (p[e] / n));
    }
    *reinterpret_cast<f32x4*>(a.gc[s] + (long)m * C + c0) = o;
  }
}

// `wide`: the widths of backbone_bn.hip (DD3D_BBN_*) in place of the towers' / the FPN's
static bool bn_width_ok(int C, bool wide) {
  if (!wide) return C >= 32 && C % 32 == 0 && C <= DD3D_BN_MAX_C;
  return C == DD3D_BBN_MIN_C || (C >= 32 && C % 32 == 0 && C <= BN_T) || (C % BN_T == 0 && C > 0 && C <= DD3D_BBN_MAX_C);
}

static int check_bn_shape(const dd3d_tower_bn_args* a, const char* who, bool wide = false) {
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->num_segs >= 1 && a->num_segs <= DD3D_BN_MAX_SEGS, "%s: %d segments (1 .. %d)", who, a->num_segs, DD3D_BN_MAX_SEGS);
  if (wide)
    DD3D_REQUIRE(bn_width_ok(a->C, true), "%s: C = %d is not %d, a multiple of 32 up to %d or a multiple of %d up to %d", who, a->C, DD3D_BBN_MIN_C, BN_T, BN_T,
                 DD3D_BBN_MAX_C);
  else
    DD3D_REQUIRE(bn_width_ok(a->C, false), "%s: C = %d is not a multiple of 32 up to %d", who, a->C, DD3D_BN_MAX_C);
  long rows = 0;
  for (int s = 0; s < a->num_segs; ++s) {
    DD3D_REQUIRE(a->N[s] >= 2, "%s: segment %d has N = %d (batch statistics need more than 1 value per channel)", who, s, a->N[s]);
    rows += ceil_div(a->N[s], DD3D_BN_SLICE);
  }
  DD3D_REQUIRE(rows < (1l << 24), "%s: %ld slices", who, rows);
  return DD3D_OK;
}

// `need`: bit 0 g / qp, bit 1 gc, bit 2 the stored y as a DD3D_PG_ACT_* storage, bit 3 the statistics' inputs, bit 4 the scratch rows
static int check_bn_args(const dd3d_tower_bn_args* a, const char* who, int need, bool wide = false) {
  const int rc = check_bn_shape(a, who, wide);
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

}  // namespace
}  // namespace dd3d
