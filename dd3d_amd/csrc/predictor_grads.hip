// Backward of the predictor layer (fcos2d.py:143-152, fcos3d.py:175-180, nuscenes_dd3d.py:371-374) for gfx950: the gradients of the 3x3,
// Cin -> n predictor convolutions of ONE predictor group (the predictors ForwardPlan._heads fuses into one head map; each group reads
// one tower), their per-level Scale / Offset parameters and the tower output they read.  include/dd3d_hip.h states the mathematics.
//
// Weight gradient -- a GEMM with M = n, N = 9 * Cin, K = every pixel of every level and image:
//   pred_wgrad_kernel   block = (slice, 32-channel chunk of the activations, 32-row tile of n), three waves, wave ky owns the taps
//                       (ky, 0..2).  A slice is a run of "units" of one level; a unit is up to 64 pixels of one image row.  Per unit the
//                       block stages the masked gradient rows [64][32] and the three activation rows [3][66][32] (decoded to f32 from
//                       whichever storage the plan keeps them in) in LDS once and runs v_mfma_f32_32x32x2_f32 over pixel pairs:
//                       A = g^T (32 channels of n x 2 pixels), B = a (2 pixels x 32 input channels), one accumulator per tap.  The f32
//                       MFMA is an fmaf chain in k order, so a slice's partial is a fixed-order f32 sum of exact f32 products.  A unit
//                       whose gradient rows are all zero (the box2d / box3d groups off the positives) adds nothing and is skipped.
//   pred_wreduce_kernel thread = (n, k): sums the slices of each level in slice order (the per-level unscaled partial, stored), then
//                       the levels that share a filter, each times its s_l[n], in level order.
//   pred_rsum_kernel    block = (level, n): r = sum_k partial * W (+ bias * q), the exact conv + b contracted with g; q = sum of g.
//   pred_small_kernel   one block: bias gradients, and the Scale / Offset sums over the channels of a slot.
// No float atomics: every sum has one writer and a fixed order, two runs agree bit for bit.
//
// Input gradient -- pred_dgrad_kernel: block = up to 16 pixels of one image row, thread = input channel.  The block stages the masked,
// scaled gradient rows [3][18][n] in LDS; every thread walks (tap, n) with its 16 accumulators, reading the filter row-coalesced from
// L2 and the gradient as LDS broadcasts (plain fmaf: K = 9 n is short and the kernel is bound by its store).  A block whose staged
// gradient is all zero stores zeros.
#include "act_load.h"
#include "common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int PG_UNIT = DD3D_PG_UNIT;  // pixels of an image row per weight-gradient unit
constexpr int PG_WT = 192;             // threads of a weight-gradient block: one wave per filter row
constexpr int PG_DP = 16;              // pixels of an image row per input-gradient block
constexpr int PG_DT = 256;
constexpr int PG_TARGET_SLICES = 48;

struct PredK {
  dd3d_pred_grad_args a;
  int32_t slice_off[DD3D_MAX_LEVELS + 1];  // first slice of a level
  int32_t units_per_slice;
  int32_t dunit_off[DD3D_MAX_LEVELS + 1];  // first input-gradient block of a level
};

inline int wgrad_units(const dd3d_pred_grad_args& a, int l) { return a.B * a.H[l] * ceil_div(a.W[l], PG_UNIT); }

inline void plan_slices(const dd3d_pred_grad_args& a, PredK& k) {
  long total = 0;
  for (int l = 0; l < a.num_levels; ++l) total += wgrad_units(a, l);
  k.units_per_slice = (int)((total + PG_TARGET_SLICES - 1) / PG_TARGET_SLICES);
  if (k.units_per_slice < 1) k.units_per_slice = 1;
  k.slice_off[0] = 0;
  k.dunit_off[0] = 0;
  for (int l = 0; l < a.num_levels; ++l) {
    k.slice_off[l + 1] = k.slice_off[l] + ceil_div(wgrad_units(a, l), k.units_per_slice);
    k.dunit_off[l + 1] = k.dunit_off[l] + a.B * a.H[l] * ceil_div(a.W[l], PG_DP);
  }
  for (int l = a.num_levels; l < DD3D_MAX_LEVELS; ++l) k.slice_off[l + 1] = k.slice_off[l], k.dunit_off[l + 1] = k.dunit_off[l];
}

// g_l of the header: the head-map gradient, 0 where a clamped channel's stored map sits on its clamp
__device__ __forceinline__ float masked_g(const dd3d_pred_grad_args& a, int l, long pix, int n) {
  const long i = pix * a.g_pitch + n;
  const float g = a.g[l][i];
  if (a.lo != nullptr) {
    const float lo = a.lo[n];
    if (lo > -INFINITY && !(a.map[l][i] > lo)) return 0.f;
  }
  return g;
}

__device__ __forceinline__ int level_of(const int32_t* off, int nl, int i) {
  int l = 0;
  while (l + 1 < nl && i >= off[l + 1]) ++l;
  return l;
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
template <int MODE>
__global__ __launch_bounds__(PG_WT) void pred_wgrad_kernel(const PredK K) {
  const dd3d_pred_grad_args& a = K.a;
  __shared__ float gs[PG_UNIT][32];          // masked gradient: [pixel of the unit][channel of the n tile]
  __shared__ float as[3][PG_UNIT + 2][32];   // activation rows y - 1, y, y + 1: [row][pixel x0 - 1 ..][channel of the chunk]
  const int slice = blockIdx.x, chunk = blockIdx.y, n0 = blockIdx.z * 32;
  const int tid = threadIdx.x, lane = tid & 63, ky = tid >> 6;
  const int l = level_of(K.slice_off, a.num_levels, slice);
  const int H = a.H[l], W = a.W[l];
  const int upr = ceil_div(W, PG_UNIT);
  const int nunits = a.B * H * upr;
  const int u0 = (slice - K.slice_off[l]) * K.units_per_slice;
  const int u1 = min(u0 + K.units_per_slice, nunits);
  const long npix = (long)a.B * H * W;
  const float inv_scale = 1.f / a.plane_scale;
  const int K9 = 9 * a.Cin;

  f32x16 acc[3];
#pragma unroll
  for (int t = 0; t < 3; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float qacc = 0.f;

  for (int u = u0; u < u1; ++u) {
    const int row = u / upr, x0 = (u - row * upr) * PG_UNIT;
    const int b = row / H, y = row - b * H;
    const int len = min(PG_UNIT, W - x0);
    const long rowpix = ((long)b * H + y) * W;
    __syncthreads();  // the previous unit's reads are done
    int nz = 0;
    for (int i = tid; i < PG_UNIT * 32; i += PG_WT) {
      const int px = i >> 5, n = n0 + (i & 31);
      float v = 0.f;
      if (px < len && n < a.n) v = masked_g(a, l, rowpix + x0 + px, n);
      gs[px][i & 31] = v;
      nz |= (v != 0.f);
    }
    if (!__syncthreads_or(nz)) continue;  // (block-uniform) nothing to add from this unit
    for (int i = tid; i < 3 * (PG_UNIT + 2) * 32; i += PG_WT) {
      const int r = i / ((PG_UNIT + 2) * 32), rem = i - r * ((PG_UNIT + 2) * 32);
      const int px = rem >> 5, c = rem & 31;
      const int yy = y + r - 1, xx = x0 + px - 1;
      float v = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W && px <= len + 1) v = load_act<MODE>(a.act[l], npix, ((long)b * H + yy) * W + xx, chunk * 32 + c, a.act_pitch, inv_scale);
      as[r][px][c] = v;
    }
    __syncthreads();
    const int steps = (len + 1) >> 1;
    for (int s = 0; s < steps; ++s) {
      const int px = 2 * s + (lane >> 5);  // (an odd len: pixel `len` holds a zero gradient row)
      const float ga = gs[px][lane & 31];
      if (ky == 1) qacc += ga;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) acc[kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, as[ky][px + kx][lane & 31], acc[kx], 0, 0, 0);
    }
  }

  // the partial of this slice: part[slice][n][tap * Cin + c]; accumulator register r of a lane is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* part = a.part + (long)slice * a.n * K9;
#pragma unroll
  for (int kx = 0; kx < 3; ++kx)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = n0 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      if (n < a.n) part[(long)n * K9 + (ky * 3 + kx) * a.Cin + chunk * 32 + (lane & 31)] = acc[kx][r];
    }
  if (ky == 1 && chunk == 0) {  // the gradient's own sum over the slice: the two pixel halves of a channel
    const float q = qacc + __shfl_down(qacc, 32);
    if (lane < 32 && n0 + lane < a.n) a.qpart[(long)slice * a.n + n0 + lane] = q;
  }
}

__global__ __launch_bounds__(256) void pred_wreduce_kernel(const PredK K) {
  const dd3d_pred_grad_args& a = K.a;
  const int K9 = 9 * a.Cin;
  const int k = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
  if (k >= K9) return;
  const long e = (long)n * K9 + k, lv = (long)a.n * K9;
  float P[DD3D_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < DD3D_MAX_LEVELS; ++l) {
    P[l] = 0.f;
    if (l < a.num_levels) {
      float s = 0.f;
      for (int sl = K.slice_off[l]; sl < K.slice_off[l + 1]; ++sl) s += a.part[(long)sl * lv + e];
      P[l] = s;
      a.dw_level[(long)l * lv + e] = s;
    }
  }
#pragma unroll
  for (int l = 0; l < DD3D_MAX_LEVELS; ++l) {
    if (l >= a.num_levels) continue;
    bool owner = true;
#pragma unroll
    for (int m = 0; m < DD3D_MAX_LEVELS; ++m)
      if (m < l && a.w[m] == a.w[l]) owner = false;
    if (!owner) continue;
    float s = 0.f;
#pragma unroll
    for (int m = 0; m < DD3D_MAX_LEVELS; ++m)
      if (m >= l && m < a.num_levels && a.w[m] == a.w[l]) s = fmaf(a.scale[m][n], P[m], s);
    a.dw[(long)l * lv + e] = s;
  }
}

__global__ __launch_bounds__(256) void pred_rsum_kernel(const PredK K) {
  const dd3d_pred_grad_args& a = K.a;
  __shared__ float red[256];
  const int K9 = 9 * a.Cin;
  const int n = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  const float* P = a.dw_level + ((long)l * a.n + n) * K9;
  const float* w = a.w[l] + (long)n * K9;
  float s = 0.f;
  for (int k = tid; k < K9; k += 256) s = fmaf(P[k], w[k], s);
  red[tid] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    float q = 0.f;
    for (int sl = K.slice_off[l]; sl < K.slice_off[l + 1]; ++sl) q += a.qpart[(long)sl * a.n + n];
    a.q[l * a.n + n] = q;
    a.r[l * a.n + n] = fmaf(a.bias[l][n], q, red[0]);
  }
}

__global__ __launch_bounds__(256) void pred_small_kernel(const PredK K) {
  const dd3d_pred_grad_args& a = K.a;
  const int tid = threadIdx.x;
  for (int i = tid; i < a.num_levels * a.n; i += 256) {
    const int l = i / a.n, n = i - l * a.n;
    bool owner = true;
    for (int m = 0; m < l; ++m)
      if (a.w[m] == a.w[l]) owner = false;
    if (!owner) continue;
    float s = 0.f;
    for (int m = l; m < a.num_levels; ++m)
      if (a.w[m] == a.w[l]) s = fmaf(a.scale[m][n], a.q[m * a.n + n], s);
    a.db[i] = s;
  }
  for (int i = tid; i < a.num_levels * DD3D_PG_MAX_SLOTS; i += 256) {
    const int l = i / DD3D_PG_MAX_SLOTS, slot = i - l * DD3D_PG_MAX_SLOTS;
    float sr = 0.f, sq = 0.f;
    if (a.slot != nullptr)
      for (int n = 0; n < a.n; ++n)
        if (a.slot[n] == slot) sr += a.r[l * a.n + n], sq += a.q[l * a.n + n];
    a.dscale[i] = sr;
    a.doffset[i] = sq;
  }
}

// ------------------------------------------------------------------------------------------------------------------- input gradient
__global__ __launch_bounds__(PG_DT) void pred_dgrad_kernel(const PredK K) {
  const dd3d_pred_grad_args& a = K.a;
  extern __shared__ __align__(16) float dg[];  // [3][PG_DP + 2][n4]: s_l[n] * g_l at rows y - 1 .. y + 1, pixels x0 - 1 .. x0 + 16
  const int n4 = (a.n + 3) & ~3;
  const int tid = threadIdx.x;
  const int l = level_of(K.dunit_off, a.num_levels, blockIdx.x);
  const int H = a.H[l], W = a.W[l];
  const int upr = ceil_div(W, PG_DP);
  const int u = blockIdx.x - K.dunit_off[l];
  const int row = u / upr, x0 = (u - row * upr) * PG_DP;
  const int b = row / H, y = row - b * H;
  const int len = min(PG_DP, W - x0);
  int nz = 0;
  for (int i = tid; i < 3 * (PG_DP + 2) * n4; i += PG_DT) {
    const int r = i / ((PG_DP + 2) * n4), rem = i - r * ((PG_DP + 2) * n4);
    const int px = rem / n4, n = rem - px * n4;
    const int yy = y + r - 1, xx = x0 + px - 1;
    float v = 0.f;
    if (n < a.n && yy >= 0 && yy < H && xx >= 0 && xx < W) {
      const float g = masked_g(a, l, ((long)b * H + yy) * W + xx, n);
      if (g != 0.f) v = a.scale[l][n] * g;  // (a masked or zero gradient stays an exact zero whatever the scale holds)
    }
    dg[i] = v;
    nz |= (v != 0.f);
  }
  const bool any = __syncthreads_or(nz) != 0;
  const int K9 = 9 * a.Cin;
  float* out = a.da[l] + (((long)b * H + y) * W + x0) * a.Cin;
  for (int c = tid; c < a.Cin; c += PG_DT) {
    float acc[PG_DP];
#pragma unroll
    for (int i = 0; i < PG_DP; ++i) acc[i] = 0.f;
    if (any) {
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
          // da[y][x] += g[y - ky + 1][x - kx + 1] * W[n][ky][kx][c]: staged row 2 - ky, staged pixel i - kx + 2
          const float* grow = dg + ((2 - ky) * (PG_DP + 2) + (2 - kx)) * n4;
          const float* wp = a.w[l] + (ky * 3 + kx) * a.Cin + c;
          for (int n = 0; n < n4; n += 4) {
            float w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = n + j < a.n ? wp[(long)(n + j) * K9] : 0.f;
#pragma unroll
            for (int i = 0; i < PG_DP; ++i) {
              const float4 g = *reinterpret_cast<const float4*>(grow + i * n4 + n);
              acc[i] = fmaf(g.x, w[0], acc[i]);
              acc[i] = fmaf(g.y, w[1], acc[i]);
              acc[i] = fmaf(g.z, w[2], acc[i]);
              acc[i] = fmaf(g.w, w[3], acc[i]);
            }
          }
        }
    }
#pragma unroll
    for (int i = 0; i < PG_DP; ++i)
      if (i < len) out[(long)i * a.Cin + c] = acc[i];
  }
}

static int check_pred_args(const dd3d_pred_grad_args* a, const char* who, bool wgrad) {
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->num_levels >= 1 && a->num_levels <= DD3D_MAX_LEVELS && a->B >= 1, "%s: %d levels, B = %d", who, a->num_levels, a->B);
  DD3D_REQUIRE(a->Cin >= 32 && a->Cin % 32 == 0, "%s: Cin = %d is not a multiple of 32", who, a->Cin);
  DD3D_REQUIRE(a->n >= 1 && a->n <= DD3D_PG_MAX_N, "%s: n = %d output channels (1 .. %d)", who, a->n, DD3D_PG_MAX_N);
  DD3D_REQUIRE(a->g_pitch % 4 == 0 && a->g_pitch >= a->n, "%s: g_pitch = %d must be a multiple of 4 and hold %d channels", who, a->g_pitch, a->n);
  DD3D_REQUIRE(a->act_mode == DD3D_PG_ACT_F32 || a->act_mode == DD3D_PG_ACT_F16X2 || a->act_mode == DD3D_PG_ACT_BF16X3, "%s: act_mode = %d", who, a->act_mode);
  if (a->act_mode == DD3D_PG_ACT_F32)
    DD3D_REQUIRE(a->act_pitch % 4 == 0 && a->act_pitch >= a->Cin, "%s: act_pitch = %d must be a multiple of 4 and hold %d channels", who, a->act_pitch, a->Cin);
  if (a->act_mode == DD3D_PG_ACT_F16X2) DD3D_REQUIRE(a->plane_scale > 0.f, "%s: plane_scale = %g", who, (double)a->plane_scale);
  long pixels = 0;
  for (int l = 0; l < a->num_levels; ++l) {
    DD3D_REQUIRE(a->H[l] >= 1 && a->W[l] >= 1, "%s: level %d is %d x %d", who, l, a->H[l], a->W[l]);
    DD3D_REQUIRE(a->g[l] && a->w[l] && a->scale[l], "%s: level %d has no gradient / filter / scale", who, l);
    DD3D_REQUIRE(!a->lo || a->map[l], "%s: level %d has a clamp vector and no stored map", who, l);
    if (wgrad) DD3D_REQUIRE(a->act[l] && a->bias[l], "%s: level %d has no activations / bias", who, l);
    else DD3D_REQUIRE(a->da[l], "%s: level %d has no input-gradient buffer", who, l);
    pixels += (long)a->B * a->H[l] * a->W[l];
  }
  DD3D_REQUIRE(pixels < (1l << 31) / 1024, "%s: %ld pixels", who, pixels);
  return DD3D_OK;
}

}  // namespace dd3d

extern "C" int64_t dd3d_predictor_grad_slices(const dd3d_pred_grad_args* args) {
  using namespace dd3d;
  if (check_pred_args(args, "dd3d_predictor_grad_slices", true) != DD3D_OK) return -1;
  PredK k;
  k.a = *args;
  plan_slices(k.a, k);
  return k.slice_off[args->num_levels];
}

extern "C" int dd3d_predictor_wgrad(const dd3d_pred_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_pred_args(args, "dd3d_predictor_wgrad", true);
  if (rc != DD3D_OK) return rc;
  PredK k;
  k.a = *args;
  plan_slices(k.a, k);
  const int nslices = k.slice_off[args->num_levels];
  DD3D_REQUIRE(args->part && args->qpart && args->n_slices >= nslices, "dd3d_predictor_wgrad: part / qpart (%d slices for %d)", args->n_slices, nslices);
  DD3D_REQUIRE(args->dw_level && args->dw && args->db && args->q && args->r && args->dscale && args->doffset, "dd3d_predictor_wgrad: null output");
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)nslices, (unsigned)(args->Cin / 32), (unsigned)ceil_div(args->n, 32));
  switch (args->act_mode) {
    case DD3D_PG_ACT_F32: hipLaunchKernelGGL(pred_wgrad_kernel<DD3D_PG_ACT_F32>, grid, dim3(PG_WT), 0, s, k); break;
    case DD3D_PG_ACT_F16X2: hipLaunchKernelGGL(pred_wgrad_kernel<DD3D_PG_ACT_F16X2>, grid, dim3(PG_WT), 0, s, k); break;
    default: hipLaunchKernelGGL(pred_wgrad_kernel<DD3D_PG_ACT_BF16X3>, grid, dim3(PG_WT), 0, s, k); break;
  }
  int e = check_launch("pred_wgrad_kernel");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(pred_wreduce_kernel, dim3((unsigned)ceil_div(9 * args->Cin, 256), (unsigned)args->n), dim3(256), 0, s, k);
  if ((e = check_launch("pred_wreduce_kernel")) != DD3D_OK) return e;
  hipLaunchKernelGGL(pred_rsum_kernel, dim3((unsigned)args->n, (unsigned)args->num_levels), dim3(256), 0, s, k);
  if ((e = check_launch("pred_rsum_kernel")) != DD3D_OK) return e;
  hipLaunchKernelGGL(pred_small_kernel, dim3(1), dim3(256), 0, s, k);
  return check_launch("pred_small_kernel");
}

extern "C" int dd3d_predictor_dgrad(const dd3d_pred_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_pred_args(args, "dd3d_predictor_dgrad", false);
  if (rc != DD3D_OK) return rc;
  PredK k;
  k.a = *args;
  plan_slices(k.a, k);
  const size_t lds = (size_t)3 * (PG_DP + 2) * ((args->n + 3) & ~3) * sizeof(float);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(pred_dgrad_kernel, dim3((unsigned)k.dunit_off[args->num_levels]), dim3(PG_DT), lds, s, k);
  return check_launch("pred_dgrad_kernel");
}

extern "C" int dd3d_pred_grad_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 32, "dd3d_pred_grad_layout: need 32 slots");
#define OFF(f) (int64_t) offsetof(dd3d_pred_grad_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_pred_grad_args), OFF(act), OFF(g), OFF(map), OFF(w), OFF(bias), OFF(scale), OFF(da), OFF(lo), OFF(slot),
                       OFF(part), OFF(qpart), OFF(dw_level), OFF(dw), OFF(db), OFF(q), OFF(r), OFF(dscale), OFF(doffset), OFF(H), OFF(W),
                       OFF(num_levels), OFF(B), OFF(Cin), OFF(n), OFF(g_pitch), OFF(act_mode), OFF(act_pitch), OFF(n_slices), OFF(plane_scale)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
