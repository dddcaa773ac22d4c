// Backward of the FPN's convolutions (detectron2 FPN.forward, LastLevelP6P7 / LastLevelP6) for gfx950: the gradients of a k x k, stride s,
// Cin -> Cout convolution with a folded norm and NO ReLU on its output, k in {1, 3}, s in {1, 2}, padding (k - 1) / 2, one filter per
// level of a call.  include/dd3d_hip.h states the mathematics.  Both gradients are dense GEMMs on v_mfma_f32_32x32x2_f32, built like the
// towers' (tower_grads.hip) with the differences the FPN brings: strides, Cin up to 1024, a filter per level, no mask on the incoming
// gradient, and an epilogue on the input gradient (mask by a stored tensor, add a tensor, add the 2x2 sum of a finer level's tensor).
// The levels of a call run as separate launches in level order on the stream: level l may read what level l - 1 wrote (the top-down
// transpose), and all levels share one slab of partials.
//
// Weight gradient -- M = Cout, N = k * k * Cin, K = the output pixels of a level:
//   fpn_wgrad_kernel<KS, S>  block = (slice, 32-channel chunk of Cin, 128-row tile of Cout), four waves, wave w owns rows 32 w .. 32 w + 31
//                        of the tile and all k * k taps.  A slice is a run of units; a unit is up to 64 (s = 1) or 32 (s = 2) output
//                        pixels of one output row.  Per unit the block stages the gradient rows [unit][128] and the k input rows
//                        [k][(unit - 1) s + k][32] (decoded to f32 from the plan's storage, rectified when in_relu) in LDS once.
//   fpn_wreduce_kernel   thread = (n, k): the slices in slice order -> dw_level, times scale[n] -> dw.
//   fpn_rsum_kernel      block = n: r = sum_k dw_level * W, q = the slices' gradient sums in slice order.
// Input gradient -- M = input pixels, N = Cin, K = k * k * Cout:
//   fpn_dgrad_kernel<KS, MT> block = (a tile of (2 MT) x 16 input pixels of one image, a group of 256 input channels), four waves, wave w
//                        owns the channel chunks w and w + 4 of the group.  Per 32-channel chunk of Cout the block stages the scaled
//                        gradient of the output pixels the tile's taps reach; a (pixel, tap) pair whose parity does not match the stride
//                        feeds an exact zero.  A chunk's k * k * 32 terms go into a fresh accumulator that is then added to the running
//                        one (short chains, as tower_dgrad_kernel).  Epilogue per element, in this order: mask, + add, + pool.
// No float atomics: every sum has one writer and a fixed order, two runs agree bit for bit.
#include "act_load.h"
#include "common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

typedef float fg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int FG_TN = 128;  // rows of Cout per weight-gradient block
constexpr int FG_T = 256;   // threads of every block here
constexpr int FG_DX = 16;   // width of an input-gradient tile
constexpr int FG_DS = 33;   // floats per staged gradient pixel (32 channels + 1)
constexpr int FG_CG = 256;  // input channels per input-gradient block

struct FpnLevelK {  // one level of a call
  const void* x;
  const float* g;
  const float* w;
  const float* scale;
  const void* mask;
  const float* add;
  const float* pool;
  float *da, *dw_level, *dw, *q, *r, *part, *qpart;
  int32_t B, H, W, Ho, Wo, Cin, Cout, g_pitch, stride, in_relu, x_mode, x_pitch, mask_mode, mask_pitch;
  float x_inv, mask_inv;
  int32_t nslices, units_per_slice, mt;
};

inline int fg_out(int n, int s) { return (n + s - 1) / s; }  // k = 1 or 3 with padding (k - 1) / 2: ceil(n / s)
inline int fg_unit(int s) { return s == 2 ? DD3D_FG_UNIT / 2 : DD3D_FG_UNIT; }

inline void plan_fpn_level(const dd3d_fpn_grad_args& a, int l, FpnLevelK& k) {
  k.B = a.B, k.H = a.H[l], k.W = a.W[l], k.Ho = fg_out(a.H[l], a.stride), k.Wo = fg_out(a.W[l], a.stride);
  k.Cin = a.Cin, k.Cout = a.Cout, k.stride = a.stride;
  const long units = (long)a.B * k.Ho * ceil_div(k.Wo, fg_unit(a.stride));
  const long slice_bytes = (long)a.Cout * a.ksize * a.ksize * a.Cin * (long)sizeof(float);
  long max_slices = DD3D_FG_SLAB_BYTES / slice_bytes;
  if (max_slices < 1) max_slices = 1;
  long ups = (units + max_slices - 1) / max_slices;
  if (ups < DD3D_FG_MIN_UNITS_PER_SLICE) ups = DD3D_FG_MIN_UNITS_PER_SLICE;
  k.units_per_slice = (int)ups;
  k.nslices = (int)((units + ups - 1) / ups);
  k.mt = a.dgrad_rows ? a.dgrad_rows / 2 : 1;
  if (!a.dgrad_rows)
    for (int mt = 4; mt > 1; mt >>= 1)
      if ((long)a.B * ceil_div(k.H, 2 * mt) * ceil_div(k.W, FG_DX) * ceil_div(a.Cin, FG_CG) >= DD3D_FG_MIN_TILES) {
        k.mt = mt;
        break;
      }
}

inline void fill_fpn_level(const dd3d_fpn_grad_args& a, int l, FpnLevelK& k) {
  plan_fpn_level(a, l, k);
  const long kk = (long)a.ksize * a.ksize * a.Cin;
  k.x = a.x[l], k.g = a.g[l], k.w = a.w[l], k.scale = a.scale[l], k.mask = a.mask[l], k.add = a.add[l], k.pool = a.pool[l], k.da = a.da[l];
  k.dw_level = a.dw_level ? a.dw_level + l * a.Cout * kk : nullptr;
  k.dw = a.dw ? a.dw + l * a.Cout * kk : nullptr;
  k.q = a.q ? a.q + (long)l * a.Cout : nullptr;
  k.r = a.r ? a.r + (long)l * a.Cout : nullptr;
  k.part = a.part, k.qpart = a.qpart;
  k.g_pitch = a.g_pitch, k.in_relu = a.in_relu, k.x_mode = a.x_mode, k.x_pitch = a.x_pitch, k.mask_mode = a.mask_mode, k.mask_pitch = a.mask_pitch;
  k.x_inv = 1.f / a.x_plane_scale, k.mask_inv = 1.f / a.mask_plane_scale;
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
template <int KS, int S>
__global__ __launch_bounds__(FG_T, 2) void fpn_wgrad_kernel(const FpnLevelK K) {
  constexpr int UNIT = S == 2 ? DD3D_FG_UNIT / 2 : DD3D_FG_UNIT, XW = (UNIT - 1) * S + KS, P = (KS - 1) / 2, TAPS = KS * KS;
  __shared__ float gs[UNIT][FG_TN];  // gradient: [output pixel of the unit][row of the Cout tile]
  __shared__ float xs[KS][XW][32];   // input rows oy * S + ky - P: [ky][input pixel x0 * S - P ..][channel of the chunk]
  const int slice = blockIdx.x, chunk = blockIdx.y, n0 = blockIdx.z * FG_TN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = K.H, W = K.W, Ho = K.Ho, Wo = K.Wo;
  const int upr = ceil_div(Wo, UNIT);
  const int nunits = K.B * Ho * upr;
  const int u0 = slice * K.units_per_slice;
  const int u1 = min(u0 + K.units_per_slice, nunits);
  const long npix = (long)K.B * H * W;
  const int KK = TAPS * K.Cin;
  const int nw = n0 + 32 * wave;   // first row of Cout of this wave
  const bool active = nw < K.Cout;  // (Cout is a multiple of 32: a wave has all of its rows or none)

  fg_f32x16 acc[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float qacc = 0.f;

  for (int u = u0; u < u1; ++u) {
    const int row = u / upr, x0 = (u - row * upr) * UNIT;
    const int b = row / Ho, oy = row - b * Ho;
    const int len = min(UNIT, Wo - x0);
    const long rowpix = ((long)b * Ho + oy) * Wo;
    __syncthreads();  // the previous unit's reads are done
    for (int i = tid; i < UNIT * FG_TN; i += FG_T) {
      const int px = i / FG_TN, nn = i - px * FG_TN;
      float v = 0.f;
      if (px < len && n0 + nn < K.Cout) v = K.g[(rowpix + x0 + px) * K.g_pitch + n0 + nn];
      gs[px][nn] = v;
    }
    for (int i = tid; i < KS * XW * 32; i += FG_T) {
      const int r = i / (XW * 32), rem = i - r * (XW * 32);
      const int j = rem >> 5, c = rem & 31;
      const int yy = oy * S + r - P, xx = x0 * S - P + j;
      float v = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        v = load_act_any(K.x_mode, K.x, npix, ((long)b * H + yy) * W + xx, chunk * 32 + c, K.x_pitch, K.x_inv);
        if (K.in_relu) v = fmaxf(v, 0.f);
      }
      xs[r][j][c] = v;
    }
    __syncthreads();
    if (!active) continue;  // (wave-uniform; the wave still takes part in the staging and its barriers)
    const int steps = (len + 1) >> 1;
    for (int s = 0; s < steps; ++s) {
      const int px = 2 * s + (lane >> 5);  // (an odd len: pixel `len` holds a zero gradient row; len < UNIT then, so its inputs are staged)
      const float ga = gs[px][32 * wave + (lane & 31)];
      qacc += ga;
#pragma unroll
      for (int ky = 0; ky < KS; ++ky)
#pragma unroll
        for (int kx = 0; kx < KS; ++kx)
          acc[ky * KS + kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, xs[ky][px * S + kx][lane & 31], acc[ky * KS + kx], 0, 0, 0);
    }
  }
  if (!active) return;
  // the partial of this slice: part[slice][n][tap * Cin + c]; accumulator register r of a lane is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* part = K.part + (long)slice * K.Cout * KK;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = nw + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      part[(long)n * KK + t * K.Cin + chunk * 32 + (lane & 31)] = acc[t][r];
    }
  if (chunk == 0) {  // the gradient's own sum over the slice: the two pixel halves of a row of Cout
    const float q = qacc + __shfl_down(qacc, 32);
    if (lane < 32) K.qpart[(long)slice * K.Cout + nw + lane] = q;
  }
}

__global__ __launch_bounds__(FG_T) void fpn_wreduce_kernel(const FpnLevelK K, const int KK) {
  const int k = blockIdx.x * FG_T + threadIdx.x, n = blockIdx.y;
  if (k >= KK) return;
  const long e = (long)n * KK + k, lv = (long)K.Cout * KK;
  float p = 0.f;
  for (int sl = 0; sl < K.nslices; ++sl) p += K.part[(long)sl * lv + e];
  K.dw_level[e] = p;
  K.dw[e] = K.scale[n] * p;
}

__global__ __launch_bounds__(FG_T) void fpn_rsum_kernel(const FpnLevelK K, const int KK) {
  __shared__ float red[FG_T];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* P = K.dw_level + (long)n * KK;
  const float* w = K.w + (long)n * KK;
  float s = 0.f;
  for (int k = tid; k < KK; k += FG_T) s = fmaf(P[k], w[k], s);
  red[tid] = s;
  __syncthreads();
  for (int h = FG_T / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    float q = 0.f;
    for (int sl = 0; sl < K.nslices; ++sl) q += K.qpart[(long)sl * K.Cout + n];
    K.q[n] = q;
    K.r[n] = red[0];
  }
}

// ------------------------------------------------------------------------------------------------------------------- input gradient
__device__ __forceinline__ int fg_floor_div(int a, int s) { return a >= 0 ? a / s : -((-a + s - 1) / s); }

template <int KS, int MT>
__global__ __launch_bounds__(FG_T, MT == 4 ? 1 : 2) void fpn_dgrad_kernel(const FpnLevelK K) {
  constexpr int TY = 2 * MT, P = (KS - 1) / 2, HY = TY + KS - 1, HX = FG_DX + KS - 1, TAPS = KS * KS;
  // scale[n] * g at the output rows oyb .. oyb + HY - 1 and pixels oxb .. oxb + HX - 1, one 32-channel chunk of Cout (stride 2 uses the
  // first MT + 2 rows and 10 pixels of it)
  __shared__ float sg[HY * HX * FG_DS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = K.H, W = K.W, Ho = K.Ho, Wo = K.Wo, S = K.stride;
  const int tx_n = ceil_div(W, FG_DX), ty_n = ceil_div(H, TY);
  int t = blockIdx.x;
  const int b = t / (ty_n * tx_n);
  t -= b * ty_n * tx_n;
  const int y0 = (t / tx_n) * TY, x0 = (t % tx_n) * FG_DX;
  const int oyb = fg_floor_div(y0 - P, S), oxb = fg_floor_div(x0 - P, S);
  const int KK = TAPS * K.Cin;
  const int c0 = blockIdx.y * FG_CG + 32 * wave, c1 = c0 + 128;  // the wave's channel chunks of Cin
  const bool act0 = c0 < K.Cin, act1 = c1 < K.Cin;
  const int m = lane & 31, kh = lane >> 5;  // A: pixel m of a 2 x 16 sub-tile, k half; B: filter row k half, input channel m
  const int istep = (2 / S) * HX * FG_DS;   // staged rows between two sub-tiles (input rows 2 apart)

  fg_f32x16 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  for (int nc = 0; nc < K.Cout; nc += 32) {
    __syncthreads();  // the previous chunk's reads are done
    for (int i = tid; i < HY * HX * 32; i += FG_T) {
      const int hp = i >> 5, n = nc + (i & 31);
      const int hy = hp / HX, hx = hp - hy * HX;
      const int oy = oyb + hy, ox = oxb + hx;
      float v = 0.f;
      if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) {
        const float g = K.g[(((long)b * Ho + oy) * Wo + ox) * K.g_pitch + n];
        if (g != 0.f) v = K.scale[n] * g;  // (a zero gradient stays an exact zero whatever the scale holds)
      }
      sg[hp * FG_DS + (i & 31)] = v;
    }
    __syncthreads();
    if (!act0) continue;  // (wave-uniform)
    fg_f32x16 part[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[i][j][r] = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < TAPS; ++tap) {
      const int ky = tap / KS, kx = tap - KS * ky;
      // da[y][x] += g[(y + P - ky) / S][(x + P - kx) / S] * W[n][ky][kx][c] where both divisions are exact
      const int ny = y0 + (m >> 4) + P - ky, nx = x0 + (m & 15) + P - kx;
      const bool valid = ny % S == 0 && nx % S == 0;  // (the parity is the same for every sub-tile: they are 2 input rows apart)
      const int sy = valid ? ny / S - oyb : 0, sx = valid ? nx / S - oxb : 0;
      const float* ap = sg + (sy * HX + sx) * FG_DS + kh;
      const float* wp = K.w + (long)(nc + kh) * KK + tap * K.Cin + m;
      // (the filter rows come from L2: with MT <= 2 there are registers to have all 16 steps' loads of a tap in flight at once; the
      // 8-row tile keeps four -- a block is bound by this latency, not by its MFMAs)
#pragma unroll(MT == 4 ? 4 : 16)
      for (int s = 0; s < 16; ++s) {
        const float b0 = wp[(long)(2 * s) * KK + c0];
        const float b1 = act1 ? wp[(long)(2 * s) * KK + c1] : 0.f;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const float av = valid ? ap[i * istep + 2 * s] : 0.f;
          part[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, part[i][0], 0, 0, 0);
          if (act1) part[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, part[i][1], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] += part[i][j];
  }
  if (!act0) return;
  const long npix = (long)K.B * H * W;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int mm = (r & 3) + 8 * (r >> 2) + 4 * kh;  // accumulator register r of a lane: pixel mm of the sub-tile, channel lane & 31
      const int yy = y0 + 2 * i + (mm >> 4), xx = x0 + (mm & 15);
      if (yy >= H || xx >= W) continue;
      const long pix = ((long)b * H + yy) * W + xx;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j == 1 && !act1) continue;
        const int c = (j ? c1 : c0) + m;
        float v = acc[i][j][r];
        if (K.mask && !(load_act_any(K.mask_mode, K.mask, npix, pix, c, K.mask_pitch, K.mask_inv) > 0.f)) v = 0.f;
        if (K.add) v += K.add[pix * K.Cin + c];
        if (K.pool) {  // the four children of the pixel on the finer level, row by row, left before right
          const float* t0 = K.pool + ((((long)b * 2 * H + 2 * yy) * 2 * W) + 2 * xx) * K.Cin + c;
          const float* t1 = t0 + (long)2 * W * K.Cin;
          v = (((v + t0[0]) + t0[K.Cin]) + t1[0]) + t1[K.Cin];
        }
        K.da[pix * K.Cin + c] = v;
      }
    }
}

// what the tiling depends on: the geometry, the channel counts and the convolution's form
static int check_fpn_shape(const dd3d_fpn_grad_args* a, const char* who) {
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->num_levels >= 1 && a->num_levels <= DD3D_MAX_LEVELS && a->B >= 1, "%s: %d levels, B = %d", who, a->num_levels, a->B);
  DD3D_REQUIRE(a->ksize == 1 || a->ksize == 3, "%s: ksize = %d (1 or 3)", who, a->ksize);
  DD3D_REQUIRE(a->stride == 1 || a->stride == 2, "%s: stride = %d (1 or 2)", who, a->stride);
  DD3D_REQUIRE(a->Cin >= 32 && a->Cin % 32 == 0 && a->Cin <= DD3D_FG_MAX_CIN, "%s: Cin = %d is not a multiple of 32 up to %d", who, a->Cin, DD3D_FG_MAX_CIN);
  DD3D_REQUIRE(a->Cout >= 32 && a->Cout % 32 == 0 && a->Cout <= DD3D_FG_MAX_COUT, "%s: Cout = %d is not a multiple of 32 up to %d", who, a->Cout,
               DD3D_FG_MAX_COUT);
  DD3D_REQUIRE(a->dgrad_rows == 0 || a->dgrad_rows == 2 || a->dgrad_rows == 4 || a->dgrad_rows == 8, "%s: dgrad_rows = %d (0, 2, 4 or 8)", who, a->dgrad_rows);
  long pixels = 0;
  for (int l = 0; l < a->num_levels; ++l) {
    DD3D_REQUIRE(a->H[l] >= 1 && a->W[l] >= 1, "%s: level %d is %d x %d", who, l, a->H[l], a->W[l]);
    pixels += (long)a->B * a->H[l] * a->W[l];
  }
  DD3D_REQUIRE(pixels < (1l << 31) / 1024, "%s: %ld pixels", who, pixels);
  return DD3D_OK;
}

static int check_fpn_args(const dd3d_fpn_grad_args* a, const char* who, bool wgrad) {
  const int rc = check_fpn_shape(a, who);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(a->g_pitch % 4 == 0 && a->g_pitch >= a->Cout, "%s: g_pitch = %d must be a multiple of 4 and hold %d channels", who, a->g_pitch, a->Cout);
  bool any_mask = false;
  for (int l = 0; l < a->num_levels; ++l) any_mask = any_mask || a->mask[l] != nullptr;
  const int modes[2] = {a->x_mode, a->mask_mode}, pitches[2] = {a->x_pitch, a->mask_pitch};
  const float scales[2] = {a->x_plane_scale, a->mask_plane_scale};
  for (int i = 0; i < 2; ++i) {
    if (i == 0 ? !wgrad : (wgrad || !any_mask)) continue;
    const char* nm = i ? "mask" : "x";
    DD3D_REQUIRE(modes[i] == DD3D_PG_ACT_F32 || modes[i] == DD3D_PG_ACT_F16X2 || modes[i] == DD3D_PG_ACT_BF16X3, "%s: %s_mode = %d", who, nm, modes[i]);
    if (modes[i] == DD3D_PG_ACT_F32)
      DD3D_REQUIRE(pitches[i] % 4 == 0 && pitches[i] >= a->Cin, "%s: %s_pitch = %d must be a multiple of 4 and hold %d channels", who, nm, pitches[i], a->Cin);
    if (modes[i] == DD3D_PG_ACT_F16X2) DD3D_REQUIRE(scales[i] > 0.f, "%s: %s_plane_scale = %g", who, nm, (double)scales[i]);
  }
  for (int l = 0; l < a->num_levels; ++l) {
    DD3D_REQUIRE(a->g[l] && a->w[l] && a->scale[l], "%s: level %d has no gradient / filter / scale", who, l);
    if (wgrad) DD3D_REQUIRE(a->x[l], "%s: level %d has no input", who, l);
    if (!wgrad) {
      DD3D_REQUIRE(a->da[l], "%s: level %d has no input-gradient buffer", who, l);
      if (a->pool[l])
        DD3D_REQUIRE(a->pool_H[l] == 2 * a->H[l] && a->pool_W[l] == 2 * a->W[l], "%s: level %d adds the 2x2 sums of a %d x %d tensor to %d x %d pixels",
                     who, l, a->pool_H[l], a->pool_W[l], a->H[l], a->W[l]);
    }
  }
  return DD3D_OK;
}

template <int KS>
static void launch_fpn_dgrad(const FpnLevelK& k, hipStream_t s) {
  const dim3 grid((unsigned)(k.B * ceil_div(k.H, 2 * k.mt) * ceil_div(k.W, FG_DX)), (unsigned)ceil_div(k.Cin, FG_CG));
  switch (k.mt) {
    case 4: hipLaunchKernelGGL((fpn_dgrad_kernel<KS, 4>), grid, dim3(FG_T), 0, s, k); break;
    case 2: hipLaunchKernelGGL((fpn_dgrad_kernel<KS, 2>), grid, dim3(FG_T), 0, s, k); break;
    default: hipLaunchKernelGGL((fpn_dgrad_kernel<KS, 1>), grid, dim3(FG_T), 0, s, k); break;
  }
}

}  // namespace dd3d

extern "C" int64_t dd3d_fpn_grad_slices(const dd3d_fpn_grad_args* args) {
  using namespace dd3d;
  if (check_fpn_shape(args, "dd3d_fpn_grad_slices") != DD3D_OK) return -1;
  int n = 0;
  for (int l = 0; l < args->num_levels; ++l) {
    FpnLevelK k;
    plan_fpn_level(*args, l, k);
    n = k.nslices > n ? k.nslices : n;
  }
  return n;
}

extern "C" int dd3d_fpn_wgrad(const dd3d_fpn_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_fpn_args(args, "dd3d_fpn_wgrad", true);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(args->dw_level && args->dw && args->q && args->r, "dd3d_fpn_wgrad: null output");
  const int64_t need = dd3d_fpn_grad_slices(args);
  DD3D_REQUIRE(args->part && args->qpart && args->n_slices >= need, "dd3d_fpn_wgrad: part / qpart (%d slices for %ld)", args->n_slices, (long)need);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int KK = args->ksize * args->ksize * args->Cin;
  for (int l = 0; l < args->num_levels; ++l) {
    FpnLevelK k;
    fill_fpn_level(*args, l, k);
    const dim3 grid((unsigned)k.nslices, (unsigned)(args->Cin / 32), (unsigned)ceil_div(args->Cout, FG_TN));
    if (args->ksize == 3 && args->stride == 1) hipLaunchKernelGGL((fpn_wgrad_kernel<3, 1>), grid, dim3(FG_T), 0, s, k);
    else if (args->ksize == 3) hipLaunchKernelGGL((fpn_wgrad_kernel<3, 2>), grid, dim3(FG_T), 0, s, k);
    else if (args->stride == 1) hipLaunchKernelGGL((fpn_wgrad_kernel<1, 1>), grid, dim3(FG_T), 0, s, k);
    else hipLaunchKernelGGL((fpn_wgrad_kernel<1, 2>), grid, dim3(FG_T), 0, s, k);
    int e = check_launch("fpn_wgrad_kernel");
    if (e != DD3D_OK) return e;
    hipLaunchKernelGGL(fpn_wreduce_kernel, dim3((unsigned)ceil_div(KK, FG_T), (unsigned)args->Cout), dim3(FG_T), 0, s, k, KK);
    if ((e = check_launch("fpn_wreduce_kernel")) != DD3D_OK) return e;
    hipLaunchKernelGGL(fpn_rsum_kernel, dim3((unsigned)args->Cout), dim3(FG_T), 0, s, k, KK);
    if ((e = check_launch("fpn_rsum_kernel")) != DD3D_OK) return e;
  }
  return DD3D_OK;
}

extern "C" int dd3d_fpn_dgrad(const dd3d_fpn_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_fpn_args(args, "dd3d_fpn_dgrad", false);
  if (rc != DD3D_OK) return rc;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  for (int l = 0; l < args->num_levels; ++l) {
    FpnLevelK k;
    fill_fpn_level(*args, l, k);
    if (args->ksize == 3) launch_fpn_dgrad<3>(k, s);
    else launch_fpn_dgrad<1>(k, s);
    const int e = check_launch("fpn_dgrad_kernel");
    if (e != DD3D_OK) return e;
  }
  return DD3D_OK;
}

extern "C" int dd3d_fpn_grad_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 40, "dd3d_fpn_grad_layout: need 40 slots");
#define OFF(f) (int64_t) offsetof(dd3d_fpn_grad_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_fpn_grad_args), OFF(x), OFF(g), OFF(w), OFF(scale), OFF(mask), OFF(add), OFF(pool), OFF(da), OFF(part), OFF(qpart),
                       OFF(dw_level), OFF(dw), OFF(q), OFF(r), OFF(H), OFF(W), OFF(pool_H), OFF(pool_W), OFF(num_levels), OFF(B), OFF(Cin), OFF(Cout),
                       OFF(g_pitch), OFF(ksize), OFF(stride), OFF(in_relu), OFF(x_mode), OFF(x_pitch), OFF(mask_mode), OFF(mask_pitch), OFF(n_slices),
                       OFF(dgrad_rows), OFF(x_plane_scale), OFF(mask_plane_scale)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
