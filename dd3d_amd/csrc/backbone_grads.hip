// Backward of the DLA-34 backbone's convolutions and 2x2 max-pools (dla.py:24-62, 206-247; BackboneLowering._tree) for gfx950: the
// gradients of ONE k x k, stride s, Cin -> Cout convolution with a folded norm per call, k in {1, 3}, s in {1, 2}, padding (k - 1) / 2,
// and the backward of the 2x2 max-pool on the residual and level_root paths.  include/dd3d_hip.h states the mathematics.  Both
// convolution gradients are dense GEMMs on v_mfma_f32_32x32x2_f32, built like the FPN's (fpn_grads.hip) with what the backbone brings:
// the incoming gradient is masked by the layer's STORED output while it is staged (as the towers do), Cin up to 1280 and Cout up to
// 512, every operand may be a channel slice of a wider buffer (the root's concat buffer and its gradient), and the input gradient's
// epilogue adds the two other contributions a backbone tensor receives: a plain tensor and a residual gradient masked by ITS stored
// output.
//
// Weight gradient -- M = Cout, N = k * k * Cin, K = the output pixels:
//   bb_wgrad_kernel<KS, S>   block = (slice, 32-channel chunk of Cin, 128-row tile of Cout), four waves, wave w owns rows 32 w .. 32 w + 31
//                        of the tile and all k * k taps.  A slice is a run of units; a unit is up to 64 (s = 1) or 32 (s = 2) output
//                        pixels of one output row.  Per unit the block stages the masked gradient rows [unit][128] and the k input rows
//                        [k][(unit - 1) s + k][32] (decoded to f32 from the plan's storage) in LDS once.
//   bb_wreduce_kernel    thread = (n, k): the slices in slice order -> dw_level, times scale[n] -> dw.
//   bb_rsum_kernel       block = n: r = sum_k dw_level * W, q = the slices' gradient sums in slice order.
// Input gradient -- M = input pixels, N = Cin, K = k * k * Cout:
//   bb_dgrad_kernel<KS, MT, NJ> block = (a tile of (2 MT) x 16 input pixels of one image, a group of 128 NJ input channels), four waves,
//                        wave w owns the channel chunks w (and w + 4 with NJ = 2) of the group.  The coarse levels have few pixels
//                        (480 at level5 of one KITTI image): the call picks the largest (MT, NJ) that still gives DD3D_BG_MIN_TILES
//                        blocks, down to 2 x 16 pixels x 128 channels.  Per 32-channel chunk of Cout the block stages the masked,
//                        scaled gradient of the output pixels the tile's taps reach; a (pixel, tap) pair whose parity does not match
//                        the stride feeds an exact zero.  A chunk's k * k * 32 terms go into a fresh accumulator that is then added to
//                        the running one (short chains, as tower_dgrad_kernel: K reaches 4608 here).  Epilogue: ((add) + res) + sum.
// Max-pool backward:
//   bb_pool_backward_kernel  thread = (pooled pixel, channel): the window's arg-max from the stored input, first maximum wins; the
//                        pooled tensor's gradient may come in two parts, the second masked by a stored tensor (a residual).
// No float atomics: every sum has one writer and a fixed order, two runs agree bit for bit, whichever tile is picked.
#include "act_load.h"
#include "common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

typedef float bg_f32x16 __attribute__((ext_vector_type(16)));

constexpr int BG_TN = 128;  // rows of Cout per weight-gradient block
constexpr int BG_T = 256;   // threads of every block here
constexpr int BG_DX = 16;   // width of an input-gradient tile
constexpr int BG_DS = 33;   // floats per staged gradient pixel (32 channels + 1)

struct BackK {
  dd3d_backbone_grad_args a;
  int32_t Ho, Wo, nslices, units_per_slice, mt, nj;
  float x_inv, y_inv, res_inv;
};

inline int bg_out(int n, int s) { return (n + s - 1) / s; }  // k = 1 or 3 with padding (k - 1) / 2: ceil(n / s)
inline int bg_unit(int s) { return s == 2 ? DD3D_BG_UNIT / 2 : DD3D_BG_UNIT; }

inline void plan_backbone(const dd3d_backbone_grad_args& a, BackK& k) {
  k.a = a;
  k.Ho = bg_out(a.H, a.stride), k.Wo = bg_out(a.W, a.stride);
  const long units = (long)a.B * k.Ho * ceil_div(k.Wo, bg_unit(a.stride));
  const long slice_bytes = (long)a.Cout * a.ksize * a.ksize * a.Cin * (long)sizeof(float);
  long max_slices = DD3D_TG_SLAB_BYTES / slice_bytes;
  if (max_slices < 1) max_slices = 1;
  long ups = (units + max_slices - 1) / max_slices;
  if (ups < DD3D_BG_MIN_UNITS_PER_SLICE) ups = DD3D_BG_MIN_UNITS_PER_SLICE;
  k.units_per_slice = (int)ups;
  k.nslices = (int)((units + ups - 1) / ups);
  // the input gradient's block, (rows, input channels): forced values first; otherwise the first candidate that gives
  // DD3D_BG_MIN_TILES blocks, else the smallest
  static const int cand[4][2] = {{8, 256}, {4, 256}, {2, 256}, {2, 128}};
  int rows = 2, group = 128;
  for (int i = 0; i < 4; ++i) {
    if (a.dgrad_rows && cand[i][0] != a.dgrad_rows) continue;
    if (a.dgrad_group && cand[i][1] != a.dgrad_group) continue;
    rows = cand[i][0], group = cand[i][1];  // (the last candidate that matches the forced values stays when none reaches the count)
    if ((long)a.B * ceil_div(a.H, rows) * ceil_div(a.W, BG_DX) * ceil_div(a.Cin, group) >= DD3D_BG_MIN_TILES) break;
  }
  if (a.dgrad_rows) rows = a.dgrad_rows;     // (a forced pair outside the table, e.g. (8, 128), is taken as it is)
  if (a.dgrad_group) group = a.dgrad_group;
  k.mt = rows / 2, k.nj = group / 128;
  k.x_inv = 1.f / a.x_plane_scale, k.y_inv = 1.f / a.y_plane_scale, k.res_inv = 1.f / a.res_y_plane_scale;
}

// the gradient that crosses the layer's ReLU at one output pixel and channel: g where the stored output is positive, else an exact
// zero; a layer without a ReLU (y null) passes g
__device__ __forceinline__ float bg_masked_g(const BackK& K, long npix, long pix, int n) {
  const float g = K.a.g[pix * K.a.g_pitch + n];
  if (!K.a.y) return g;
  return load_act_any(K.a.y_mode, K.a.y, npix, pix, n, K.a.y_pitch, K.y_inv) > 0.f ? g : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
template <int KS, int S>
__global__ __launch_bounds__(BG_T, 2) void bb_wgrad_kernel(const BackK K) {
  const dd3d_backbone_grad_args& a = K.a;
  constexpr int UNIT = S == 2 ? DD3D_BG_UNIT / 2 : DD3D_BG_UNIT, XW = (UNIT - 1) * S + KS, P = (KS - 1) / 2, TAPS = KS * KS;
  __shared__ float gs[UNIT][BG_TN];  // masked gradient: [output pixel of the unit][row of the Cout tile]
  __shared__ float xs[KS][XW][32];   // input rows oy * S + ky - P: [ky][input pixel x0 * S - P ..][channel of the chunk]
  const int slice = blockIdx.x, chunk = blockIdx.y, n0 = blockIdx.z * BG_TN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, W = a.W, Ho = K.Ho, Wo = K.Wo;
  const int upr = ceil_div(Wo, UNIT);
  const int nunits = a.B * Ho * upr;
  const int u0 = slice * K.units_per_slice;
  const int u1 = min(u0 + K.units_per_slice, nunits);
  const long npix = (long)a.B * H * W, nopix = (long)a.B * Ho * Wo;
  const int KK = TAPS * a.Cin;
  const int nw = n0 + 32 * wave;   // first row of Cout of this wave
  const bool active = nw < a.Cout;  // (Cout is a multiple of 32: a wave has all of its rows or none)

  bg_f32x16 acc[TAPS];
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
    for (int i = tid; i < UNIT * BG_TN; i += BG_T) {
      const int px = i / BG_TN, nn = i - px * BG_TN;
      float v = 0.f;
      if (px < len && n0 + nn < a.Cout) v = bg_masked_g(K, nopix, rowpix + x0 + px, n0 + nn);
      gs[px][nn] = v;
    }
    for (int i = tid; i < KS * XW * 32; i += BG_T) {
      const int r = i / (XW * 32), rem = i - r * (XW * 32);
      const int j = rem >> 5, c = rem & 31;
      const int yy = oy * S + r - P, xx = x0 * S - P + j;
      float v = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) v = load_act_any(a.x_mode, a.x, npix, ((long)b * H + yy) * W + xx, chunk * 32 + c, a.x_pitch, K.x_inv);
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
  float* part = a.part + (long)slice * a.Cout * KK;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = nw + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      part[(long)n * KK + t * a.Cin + chunk * 32 + (lane & 31)] = acc[t][r];
    }
  if (chunk == 0) {  // the gradient's own sum over the slice: the two pixel halves of a row of Cout
    const float q = qacc + __shfl_down(qacc, 32);
    if (lane < 32) a.qpart[(long)slice * a.Cout + nw + lane] = q;
  }
}

__global__ __launch_bounds__(BG_T) void bb_wreduce_kernel(const BackK K, const int KK) {
  const dd3d_backbone_grad_args& a = K.a;
  const int k = blockIdx.x * BG_T + threadIdx.x, n = blockIdx.y;
  if (k >= KK) return;
  const long e = (long)n * KK + k, lv = (long)a.Cout * KK;
  float p = 0.f;
  for (int sl = 0; sl < K.nslices; ++sl) p += a.part[(long)sl * lv + e];
  a.dw_level[e] = p;
  a.dw[e] = a.scale[n] * p;
}

__global__ __launch_bounds__(BG_T) void bb_rsum_kernel(const BackK K, const int KK) {
  const dd3d_backbone_grad_args& a = K.a;
  __shared__ float red[BG_T];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* P = a.dw_level + (long)n * KK;
  const float* w = a.w + (long)n * KK;
  float s = 0.f;
  for (int k = tid; k < KK; k += BG_T) s = fmaf(P[k], w[k], s);
  red[tid] = s;
  __syncthreads();
  for (int h = BG_T / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    float q = 0.f;
    for (int sl = 0; sl < K.nslices; ++sl) q += a.qpart[(long)sl * a.Cout + n];
    a.q[n] = q;
    a.r[n] = red[0];
  }
}

// ------------------------------------------------------------------------------------------------------------------- input gradient
__device__ __forceinline__ int bg_floor_div(int a, int s) { return a >= 0 ? a / s : -((-a + s - 1) / s); }

template <int KS, int MT, int NJ>
__global__ __launch_bounds__(BG_T, MT * NJ == 8 ? 1 : 2) void bb_dgrad_kernel(const BackK K) {
  const dd3d_backbone_grad_args& a = K.a;
  constexpr int TY = 2 * MT, P = (KS - 1) / 2, HY = TY + KS - 1, HX = BG_DX + KS - 1, TAPS = KS * KS, CG = 128 * NJ;
  // scale[n] * (masked g) at the output rows oyb .. oyb + HY - 1 and pixels oxb .. oxb + HX - 1, one 32-channel chunk of Cout (stride 2
  // uses the first MT + 2 rows and 10 pixels of it)
  __shared__ float sg[HY * HX * BG_DS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.H, W = a.W, Ho = K.Ho, Wo = K.Wo, S = a.stride;
  const int tx_n = ceil_div(W, BG_DX), ty_n = ceil_div(H, TY);
  int t = blockIdx.x;
  const int b = t / (ty_n * tx_n);
  t -= b * ty_n * tx_n;
  const int y0 = (t / tx_n) * TY, x0 = (t % tx_n) * BG_DX;
  const int oyb = bg_floor_div(y0 - P, S), oxb = bg_floor_div(x0 - P, S);
  const int KK = TAPS * a.Cin;
  const int c0 = blockIdx.y * CG + 32 * wave, c1 = c0 + 128;  // the wave's channel chunks of Cin
  const bool act0 = c0 < a.Cin, act1 = NJ == 2 && c1 < a.Cin;
  const int m = lane & 31, kh = lane >> 5;  // A: pixel m of a 2 x 16 sub-tile, k half; B: filter row k half, input channel m
  const int istep = (2 / S) * HX * BG_DS;   // staged rows between two sub-tiles (input rows 2 apart)
  const long nopix = (long)a.B * Ho * Wo;

  bg_f32x16 acc[MT][NJ];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  for (int nc = 0; nc < a.Cout; nc += 32) {
    __syncthreads();  // the previous chunk's reads are done
    for (int i = tid; i < HY * HX * 32; i += BG_T) {
      const int hp = i >> 5, n = nc + (i & 31);
      const int hy = hp / HX, hx = hp - hy * HX;
      const int oy = oyb + hy, ox = oxb + hx;
      float v = 0.f;
      if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo) {
        const float g = bg_masked_g(K, nopix, ((long)b * Ho + oy) * Wo + ox, n);
        if (g != 0.f) v = a.scale[n] * g;  // (a masked or zero gradient stays an exact zero whatever the scale holds)
      }
      sg[hp * BG_DS + (i & 31)] = v;
    }
    __syncthreads();
    if (!act0) continue;  // (wave-uniform)
    bg_f32x16 part[MT][NJ];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[i][j][r] = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < TAPS; ++tap) {
      const int ky = tap / KS, kx = tap - KS * ky;
      // da[y][x] += g[(y + P - ky) / S][(x + P - kx) / S] * W[n][ky][kx][c] where both divisions are exact
      const int ny = y0 + (m >> 4) + P - ky, nx = x0 + (m & 15) + P - kx;
      const bool valid = ny % S == 0 && nx % S == 0;  // (the parity is the same for every sub-tile: they are 2 input rows apart)
      const int sy = valid ? ny / S - oyb : 0, sx = valid ? nx / S - oxb : 0;
      const float* ap = sg + (sy * HX + sx) * BG_DS + kh;
      const float* wp = a.w + (long)(nc + kh) * KK + tap * a.Cin + m;
      // (the filter rows come from L2, as in fpn_dgrad_kernel: the small tiles have the registers to keep a tap's loads in flight)
#pragma unroll(MT * NJ == 8 ? 4 : 16)
      for (int s = 0; s < 16; ++s) {
        const float b0 = wp[(long)(2 * s) * KK + c0];
        const float b1 = act1 ? wp[(long)(2 * s) * KK + c1] : 0.f;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const float av = valid ? ap[i * istep + 2 * s] : 0.f;
          part[i][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b0, part[i][0], 0, 0, 0);
          if (NJ == 2 && act1) part[i][NJ - 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b1, part[i][NJ - 1], 0, 0, 0);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[i][j] += part[i][j];
  }
  if (!act0) return;
  const long npix = (long)a.B * H * W;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int mm = (r & 3) + 8 * (r >> 2) + 4 * kh;  // accumulator register r of a lane: pixel mm of the sub-tile, channel lane & 31
      const int yy = y0 + 2 * i + (mm >> 4), xx = x0 + (mm & 15);
      if (yy >= H || xx >= W) continue;
      const long pix = ((long)b * H + yy) * W + xx;
#pragma unroll
      for (int j = 0; j < NJ; ++j) {
        if (j == 1 && !act1) continue;
        const int c = (j ? c1 : c0) + m;
        // the contributions in their order: the plain tensor, the residual gradient masked by ITS stored output, this convolution's
        float v = acc[i][j][r];
        if (a.res_g) {
          const float rg = load_act_any(a.res_y_mode, a.res_y, npix, pix, c, a.res_y_pitch, K.res_inv) > 0.f ? a.res_g[pix * a.res_pitch + c] : 0.f;
          v = (a.add ? a.add[pix * a.add_pitch + c] + rg : rg) + v;
        } else if (a.add) {
          v = a.add[pix * a.add_pitch + c] + v;
        }
        a.da[pix * a.da_pitch + c] = v;
      }
    }
}

// --------------------------------------------------------------------------------------------------------------- max-pool backward
struct PoolK {
  dd3d_pool_grad_args a;
  float x_inv, res_inv;
};

__global__ __launch_bounds__(BG_T) void bb_pool_backward_kernel(const PoolK K) {
  const dd3d_pool_grad_args& a = K.a;
  const int Ho = a.H / 2, Wo = a.W / 2;
  const long total = (long)a.B * Ho * Wo * a.C;
  const long i = (long)blockIdx.x * BG_T + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % a.C);
  long p = i / a.C;
  const int ox = (int)(p % Wo);
  p /= Wo;
  const int oy = (int)(p % Ho), b = (int)(p / Ho);
  const long npix = (long)a.B * a.H * a.W;
  long pix[4];
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    pix[k] = ((long)b * a.H + 2 * oy + (k >> 1)) * a.W + 2 * ox + (k & 1);
    v[k] = load_act_any(a.x_mode, a.x, npix, pix[k], c, a.x_pitch, K.x_inv);
  }
  int best = 0;  // the first maximum in the order (0,0), (0,1), (1,0), (1,1): a later entry wins only when it is larger
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (v[k] > v[best]) best = k;
  const long opix = ((long)b * Ho + oy) * Wo + ox;
  float g = a.g ? a.g[opix * a.g_pitch + c] : 0.f;
  if (a.res_g) {  // a strided tree without a project: the pooled tensor is the residual, its gradient arrives masked by the block's output
    const float rg = load_act_any(a.res_y_mode, a.res_y, (long)a.B * Ho * Wo, opix, c, a.res_y_pitch, K.res_inv) > 0.f ? a.res_g[opix * a.res_pitch + c] : 0.f;
    g = a.g ? g + rg : rg;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float s = k == best ? g : 0.f;
    a.da[pix[k] * a.da_pitch + c] = a.add ? a.add[pix[k] * a.add_pitch + c] + s : s;
  }
}

// ------------------------------------------------------------------------------------------------------------------------ host side
static int check_mode(const char* who, const char* nm, int mode, int pitch, int chans, float scale) {
  DD3D_REQUIRE(mode == DD3D_PG_ACT_F32 || mode == DD3D_PG_ACT_F16X2 || mode == DD3D_PG_ACT_BF16X3, "%s: %s_mode = %d", who, nm, mode);
  if (mode == DD3D_PG_ACT_F32) DD3D_REQUIRE(pitch % 4 == 0 && pitch >= chans, "%s: %s_pitch = %d must be a multiple of 4 and hold %d channels", who, nm, pitch, chans);
  if (mode == DD3D_PG_ACT_F16X2) DD3D_REQUIRE(scale > 0.f, "%s: %s_plane_scale = %g", who, nm, (double)scale);
  return DD3D_OK;
}

// what the tiling depends on: the geometry, the channel counts and the convolution's form
static int check_backbone_shape(const dd3d_backbone_grad_args* a, const char* who, int max_cin = DD3D_BG_MAX_CIN, int max_cout = DD3D_BG_MAX_COUT) {
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->B >= 1 && a->H >= 1 && a->W >= 1, "%s: B = %d, %d x %d", who, a->B, a->H, a->W);
  DD3D_REQUIRE(a->ksize == 1 || a->ksize == 3, "%s: ksize = %d (1 or 3)", who, a->ksize);
  DD3D_REQUIRE(a->stride == 1 || a->stride == 2, "%s: stride = %d (1 or 2)", who, a->stride);
  DD3D_REQUIRE(a->Cin >= 32 && a->Cin % 32 == 0 && a->Cin <= max_cin, "%s: Cin = %d is not a multiple of 32 up to %d", who, a->Cin, max_cin);
  DD3D_REQUIRE(a->Cout >= 32 && a->Cout % 32 == 0 && a->Cout <= max_cout, "%s: Cout = %d is not a multiple of 32 up to %d", who, a->Cout, max_cout);
  DD3D_REQUIRE(a->dgrad_rows == 0 || a->dgrad_rows == 2 || a->dgrad_rows == 4 || a->dgrad_rows == 8, "%s: dgrad_rows = %d (0, 2, 4 or 8)", who, a->dgrad_rows);
  DD3D_REQUIRE(a->dgrad_group == 0 || a->dgrad_group == 128 || a->dgrad_group == 256, "%s: dgrad_group = %d (0, 128 or 256)", who, a->dgrad_group);
  // (every pixel and word index is a long; what is an int is a count of pixels, units or blocks: below 2^26 pixels all of them fit)
  DD3D_REQUIRE((long)a->B * a->H * a->W <= DD3D_BG_MAX_PIXELS, "%s: %ld input pixels (at most %ld)", who, (long)a->B * a->H * a->W, (long)DD3D_BG_MAX_PIXELS);
  return DD3D_OK;
}

static int check_backbone_args(const dd3d_backbone_grad_args* a, const char* who, bool wgrad, int max_cin = DD3D_BG_MAX_CIN,
                               int max_cout = DD3D_BG_MAX_COUT) {
  int rc = check_backbone_shape(a, who, max_cin, max_cout);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(a->g_pitch % 4 == 0 && a->g_pitch >= a->Cout, "%s: g_pitch = %d must be a multiple of 4 and hold %d channels", who, a->g_pitch, a->Cout);
  DD3D_REQUIRE(a->g && a->w && a->scale, "%s: no gradient / filter / scale", who);
  if (a->y && (rc = check_mode(who, "y", a->y_mode, a->y_pitch, a->Cout, a->y_plane_scale)) != DD3D_OK) return rc;
  if (wgrad) {
    DD3D_REQUIRE(a->x, "%s: no input", who);
    if ((rc = check_mode(who, "x", a->x_mode, a->x_pitch, a->Cin, a->x_plane_scale)) != DD3D_OK) return rc;
  } else {
    DD3D_REQUIRE(a->da, "%s: no input-gradient buffer", who);
    DD3D_REQUIRE(a->da_pitch % 4 == 0 && a->da_pitch >= a->Cin, "%s: da_pitch = %d must be a multiple of 4 and hold %d channels", who, a->da_pitch, a->Cin);
    if (a->add) DD3D_REQUIRE(a->add_pitch % 4 == 0 && a->add_pitch >= a->Cin, "%s: add_pitch = %d must be a multiple of 4 and hold %d channels", who, a->add_pitch, a->Cin);
    DD3D_REQUIRE((a->res_g != nullptr) == (a->res_y != nullptr), "%s: res_g and res_y come together", who);
    if (a->res_g) {
      DD3D_REQUIRE(a->res_pitch % 4 == 0 && a->res_pitch >= a->Cin, "%s: res_pitch = %d must be a multiple of 4 and hold %d channels", who, a->res_pitch, a->Cin);
      if ((rc = check_mode(who, "res_y", a->res_y_mode, a->res_y_pitch, a->Cin, a->res_y_plane_scale)) != DD3D_OK) return rc;
    }
  }
  return DD3D_OK;
}

template <int KS, int MT>
static void launch_bb_dgrad_nj(const BackK& k, dim3 grid, hipStream_t s) {
  if (k.nj == 2) hipLaunchKernelGGL((bb_dgrad_kernel<KS, MT, 2>), grid, dim3(BG_T), 0, s, k);
  else hipLaunchKernelGGL((bb_dgrad_kernel<KS, MT, 1>), grid, dim3(BG_T), 0, s, k);
}

template <int KS>
static void launch_bb_dgrad(const BackK& k, hipStream_t s) {
  const dim3 grid((unsigned)(k.a.B * ceil_div(k.a.H, 2 * k.mt) * ceil_div(k.a.W, BG_DX)), (unsigned)ceil_div(k.a.Cin, 128 * k.nj));
  switch (k.mt) {
    case 4: launch_bb_dgrad_nj<KS, 4>(k, grid, s); break;
    case 2: launch_bb_dgrad_nj<KS, 2>(k, grid, s); break;
    default: launch_bb_dgrad_nj<KS, 1>(k, grid, s); break;
  }
}

}  // namespace dd3d

extern "C" int64_t dd3d_backbone_grad_slices(const dd3d_backbone_grad_args* args) {
  using namespace dd3d;
  if (check_backbone_shape(args, "dd3d_backbone_grad_slices") != DD3D_OK) return -1;
  BackK k;
  plan_backbone(*args, k);
  return k.nslices;
}

namespace dd3d {
// the three launches of a weight gradient and the one of an input gradient, behind the argument checks of their entry points
static int run_wgrad(const dd3d_backbone_grad_args* args, const char* who, void* stream) {
  DD3D_REQUIRE(args->dw_level && args->dw && args->q && args->r, "%s: null output", who);
  BackK k;
  plan_backbone(*args, k);
  DD3D_REQUIRE(args->part && args->qpart && args->n_slices >= k.nslices, "%s: part / qpart (%d slices for %d)", who, args->n_slices, k.nslices);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int KK = args->ksize * args->ksize * args->Cin;
  const dim3 grid((unsigned)k.nslices, (unsigned)(args->Cin / 32), (unsigned)ceil_div(args->Cout, BG_TN));
  if (args->ksize == 3 && args->stride == 1) hipLaunchKernelGGL((bb_wgrad_kernel<3, 1>), grid, dim3(BG_T), 0, s, k);
  else if (args->ksize == 3) hipLaunchKernelGGL((bb_wgrad_kernel<3, 2>), grid, dim3(BG_T), 0, s, k);
  else if (args->stride == 1) hipLaunchKernelGGL((bb_wgrad_kernel<1, 1>), grid, dim3(BG_T), 0, s, k);
  else hipLaunchKernelGGL((bb_wgrad_kernel<1, 2>), grid, dim3(BG_T), 0, s, k);
  int e = check_launch("bb_wgrad_kernel");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(bb_wreduce_kernel, dim3((unsigned)ceil_div(KK, BG_T), (unsigned)args->Cout), dim3(BG_T), 0, s, k, KK);
  if ((e = check_launch("bb_wreduce_kernel")) != DD3D_OK) return e;
  hipLaunchKernelGGL(bb_rsum_kernel, dim3((unsigned)args->Cout), dim3(BG_T), 0, s, k, KK);
  return check_launch("bb_rsum_kernel");
}

static int run_dgrad(const dd3d_backbone_grad_args* args, void* stream) {
  BackK k;
  plan_backbone(*args, k);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (args->ksize == 3) launch_bb_dgrad<3>(k, s);
  else launch_bb_dgrad<1>(k, s);
  return check_launch("bb_dgrad_kernel");
}
}  // namespace dd3d

extern "C" int dd3d_backbone_wgrad(const dd3d_backbone_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_backbone_args(args, "dd3d_backbone_wgrad", true);
  if (rc != DD3D_OK) return rc;
  return run_wgrad(args, "dd3d_backbone_wgrad", stream);
}

extern "C" int dd3d_backbone_dgrad(const dd3d_backbone_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_backbone_args(args, "dd3d_backbone_dgrad", false);
  if (rc != DD3D_OK) return rc;
  return run_dgrad(args, stream);
}

// ---- the VoVNet backbone's convolutions (include/dd3d_hip.h, the VoVNet section): the same kernels under wider limits.  Nothing in the
// kernels' indexing depends on the DLA limits: every word index is a long, the LDS tiles are sized by the unit and the 32-channel chunk
// alone, and the grids grow with Cin / 32 and Cout / 128.
extern "C" int64_t dd3d_vovnet_conv_grad_slices(const dd3d_backbone_grad_args* args) {
  using namespace dd3d;
  if (check_backbone_shape(args, "dd3d_vovnet_conv_grad_slices", DD3D_VG_MAX_CIN, DD3D_VG_MAX_COUT) != DD3D_OK) return -1;
  BackK k;
  plan_backbone(*args, k);
  return k.nslices;
}

extern "C" int dd3d_vovnet_conv_wgrad(const dd3d_backbone_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_backbone_args(args, "dd3d_vovnet_conv_wgrad", true, DD3D_VG_MAX_CIN, DD3D_VG_MAX_COUT);
  if (rc != DD3D_OK) return rc;
  return run_wgrad(args, "dd3d_vovnet_conv_wgrad", stream);
}

extern "C" int dd3d_vovnet_conv_dgrad(const dd3d_backbone_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_backbone_args(args, "dd3d_vovnet_conv_dgrad", false, DD3D_VG_MAX_CIN, DD3D_VG_MAX_COUT);
  if (rc != DD3D_OK) return rc;
  return run_dgrad(args, stream);
}

extern "C" int dd3d_maxpool2x2_backward(const dd3d_pool_grad_args* a, void* stream) {
  using namespace dd3d;
  const char* who = "dd3d_maxpool2x2_backward";
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->B >= 1 && a->H >= 2 && a->W >= 2 && a->H % 2 == 0 && a->W % 2 == 0, "%s: B = %d, %d x %d (even sizes)", who, a->B, a->H, a->W);
  DD3D_REQUIRE(a->C >= 32 && a->C % 32 == 0 && a->C <= DD3D_BG_MAX_CIN, "%s: C = %d is not a multiple of 32 up to %d", who, a->C, DD3D_BG_MAX_CIN);
  DD3D_REQUIRE((long)a->B * a->H * a->W <= DD3D_BG_MAX_PIXELS, "%s: %ld input pixels (at most %ld)", who, (long)a->B * a->H * a->W, (long)DD3D_BG_MAX_PIXELS);
  DD3D_REQUIRE(a->x && (a->g || a->res_g) && a->da, "%s: no input / gradient / output", who);
  int rc = check_mode(who, "x", a->x_mode, a->x_pitch, a->C, a->x_plane_scale);
  if (rc != DD3D_OK) return rc;
  if (a->g) DD3D_REQUIRE(a->g_pitch % 4 == 0 && a->g_pitch >= a->C, "%s: g_pitch = %d must be a multiple of 4 and hold %d channels", who, a->g_pitch, a->C);
  DD3D_REQUIRE((a->res_g != nullptr) == (a->res_y != nullptr), "%s: res_g and res_y come together", who);
  if (a->res_g) {
    DD3D_REQUIRE(a->res_pitch % 4 == 0 && a->res_pitch >= a->C, "%s: res_pitch = %d must be a multiple of 4 and hold %d channels", who, a->res_pitch, a->C);
    if ((rc = check_mode(who, "res_y", a->res_y_mode, a->res_y_pitch, a->C, a->res_y_plane_scale)) != DD3D_OK) return rc;
  }
  DD3D_REQUIRE(a->da_pitch % 4 == 0 && a->da_pitch >= a->C, "%s: da_pitch = %d must be a multiple of 4 and hold %d channels", who, a->da_pitch, a->C);
  if (a->add) DD3D_REQUIRE(a->add_pitch % 4 == 0 && a->add_pitch >= a->C, "%s: add_pitch = %d must be a multiple of 4 and hold %d channels", who, a->add_pitch, a->C);
  PoolK k;
  k.a = *a;
  k.x_inv = 1.f / a->x_plane_scale, k.res_inv = a->res_g ? 1.f / a->res_y_plane_scale : 1.f;
  const long total = (long)a->B * (a->H / 2) * (a->W / 2) * a->C;
  hipLaunchKernelGGL(bb_pool_backward_kernel, dim3((unsigned)((total + BG_T - 1) / BG_T)), dim3(BG_T), 0, reinterpret_cast<hipStream_t>(stream), k);
  return check_launch("bb_pool_backward_kernel");
}

extern "C" int dd3d_backbone_grad_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 64, "dd3d_backbone_grad_layout: need 64 slots");
#define OFF(f) (int64_t) offsetof(dd3d_backbone_grad_args, f)
#define POFF(f) (int64_t) offsetof(dd3d_pool_grad_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_backbone_grad_args), OFF(x), OFF(y), OFF(g), OFF(w), OFF(scale), OFF(add), OFF(res_g), OFF(res_y), OFF(da), OFF(part),
                       OFF(qpart), OFF(dw_level), OFF(dw), OFF(q), OFF(r), OFF(B), OFF(H), OFF(W), OFF(Cin), OFF(Cout), OFF(ksize), OFF(stride), OFF(g_pitch),
                       OFF(add_pitch), OFF(res_pitch), OFF(da_pitch), OFF(x_mode), OFF(x_pitch), OFF(y_mode), OFF(y_pitch), OFF(res_y_mode), OFF(res_y_pitch),
                       OFF(n_slices), OFF(dgrad_rows), OFF(dgrad_group), OFF(x_plane_scale), OFF(y_plane_scale), OFF(res_y_plane_scale),
                       (int64_t)sizeof(dd3d_pool_grad_args), POFF(x), POFF(g), POFF(res_g), POFF(res_y), POFF(add), POFF(da), POFF(B), POFF(H), POFF(W), POFF(C),
                       POFF(x_mode), POFF(x_pitch), POFF(res_y_mode), POFF(res_y_pitch), POFF(g_pitch), POFF(res_pitch), POFF(add_pitch), POFF(da_pitch),
                       POFF(x_plane_scale), POFF(res_y_plane_scale)};
#undef OFF
#undef POFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
