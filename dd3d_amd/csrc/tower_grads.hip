// Backward of one head-tower layer (fcos2d.py:130-141, fcos3d.py:160-173) for gfx950: the gradients of a 3x3, Cin -> Cout tower
// convolution with its per-level folded norm and ReLU, over all pyramid levels.  include/dd3d_hip.h states the mathematics.  After the
// predictor layer nothing is sparse any more: both gradients are dense GEMMs on v_mfma_f32_32x32x2_f32.
//
// Weight gradient -- M = Cout, N = 9 * Cin, K = every pixel of every level and image:
//   tower_wgrad_kernel   block = (slice, 32-channel chunk of Cin, 128-row tile of Cout), four waves, wave w owns rows 32 w .. 32 w + 31 of
//                        the tile and all nine taps: nine accumulators, a 128 x 288 output tile per block.  A slice is a run of "units" of
//                        one level; a unit is up to 64 pixels of one image row.  Per unit the block stages the masked gradient rows
//                        [64][128] and the three input rows [3][66][32] (decoded to f32 from the plan's storage) in LDS ONCE and every
//                        wave runs 32 pixel pairs x 9 taps of MFMA over them: A = g^T (32 rows of Cout x 2 pixels), B = x (2 pixels x 32
//                        channels).  One LDS read of A and nine of B feed nine MFMAs (576 issue cycles).
//   tower_wreduce_kernel thread = (n, k): the slices of each level in slice order (dw_level), then the levels, each times s_l[n].
//   tower_rsum_kernel    block = (n, level): r = sum_k dw_level * W, q = the slices' gradient sums.
// Input gradient -- M = pixels, N = Cin, K = 9 * Cout:
//   tower_dgrad_kernel   block = a tile of (2 MT) x 16 pixels of one image x all of Cin (MT = 1, 2 or 4: the largest that still fills
//                        the chip), four waves, wave w owns the channel chunks w and w + 4 and all pixels of the tile: 2 MT
//                        accumulators.  Per 32-channel chunk of Cout the block stages the masked, scaled gradient halo
//                        [(2 MT + 2)][18][32] in LDS; A = a pixel's two gradient channels (LDS), B = two filter rows x 32 input
//                        channels read straight from L2 (the 2.4 MB filter stays resident there).  A chunk's 288 terms go into a
//                        fresh accumulator that is then added to the running one: eight short chains instead of one of 2304 terms.
// No float atomics: every sum has one writer and a fixed order, two runs agree bit for bit.
#include "act_load.h"
#include "common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int TG_UNIT = DD3D_TG_UNIT;  // pixels of an image row per weight-gradient unit
constexpr int TG_TN = 128;             // rows of Cout per weight-gradient block
constexpr int TG_T = 256;              // threads of every block here
constexpr int TG_DX = 16;              // width of an input-gradient tile
constexpr int TG_DS = 33;              // floats per staged halo pixel (32 channels + 1: the pixels of a half wave fall on different banks)

struct TowerK {
  dd3d_tower_grad_args a;
  int32_t slice_off[DD3D_MAX_LEVELS + 1];  // first slice of a level
  int32_t units_per_slice;
  int32_t tile_off[DD3D_MAX_LEVELS + 1];   // first input-gradient block of a level
  int32_t mt;                              // input-gradient tile: 2 * mt rows
};

inline long tg_units(const dd3d_tower_grad_args& a, int l) { return (long)a.B * a.H[l] * ceil_div(a.W[l], TG_UNIT); }
inline long tg_tiles(const dd3d_tower_grad_args& a, int l, int mt) { return (long)a.B * ceil_div(a.H[l], 2 * mt) * ceil_div(a.W[l], TG_DX); }

inline void plan_tower(const dd3d_tower_grad_args& a, TowerK& k) {
  long total = 0;
  for (int l = 0; l < a.num_levels; ++l) total += tg_units(a, l);
  const long slice_bytes = (long)a.Cout * 9 * a.Cin * (long)sizeof(float);
  long max_slices = DD3D_TG_SLAB_BYTES / slice_bytes;
  if (max_slices < 1) max_slices = 1;
  long ups = (total + max_slices - 1) / max_slices;
  if (ups < DD3D_TG_MIN_UNITS_PER_SLICE) ups = DD3D_TG_MIN_UNITS_PER_SLICE;
  k.units_per_slice = (int)ups;
  k.mt = a.dgrad_rows ? a.dgrad_rows / 2 : 1;
  if (!a.dgrad_rows)
    for (int mt = 4; mt > 1; mt >>= 1) {
      long tiles = 0;
      for (int l = 0; l < a.num_levels; ++l) tiles += tg_tiles(a, l, mt);
      if (tiles >= DD3D_TG_MIN_TILES) {
        k.mt = mt;
        break;
      }
    }
  k.slice_off[0] = 0;
  k.tile_off[0] = 0;
  for (int l = 0; l < a.num_levels; ++l) {
    k.slice_off[l + 1] = k.slice_off[l] + (int)((tg_units(a, l) + ups - 1) / ups);
    k.tile_off[l + 1] = k.tile_off[l] + (int)tg_tiles(a, l, k.mt);
  }
  for (int l = a.num_levels; l < DD3D_MAX_LEVELS; ++l) k.slice_off[l + 1] = k.slice_off[l], k.tile_off[l + 1] = k.tile_off[l];
}

__device__ __forceinline__ int tg_level_of(const int32_t* off, int nl, int i) {
  int l = 0;
  while (l + 1 < nl && i >= off[l + 1]) ++l;
  return l;
}

// g_l of the header at one pixel and output channel: the incoming gradient where the stored output is positive, else an exact zero
__device__ __forceinline__ float tg_masked_g(const dd3d_tower_grad_args& a, int l, long npix, long pix, int n, float y_inv_scale) {
  const float g = a.g[l][pix * a.g_pitch + n];
  return load_act_any(a.y_mode, a.y[l], npix, pix, n, a.y_pitch, y_inv_scale) > 0.f ? g : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
__global__ __launch_bounds__(TG_T, 2) void tower_wgrad_kernel(const TowerK K) {
  const dd3d_tower_grad_args& a = K.a;
  __shared__ float gs[TG_UNIT][TG_TN];       // masked gradient: [pixel of the unit][row of the Cout tile]
  __shared__ float xs[3][TG_UNIT + 2][32];   // input rows y - 1, y, y + 1: [row][pixel x0 - 1 ..][channel of the chunk]
  const int slice = blockIdx.x, chunk = blockIdx.y, n0 = blockIdx.z * TG_TN;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l = tg_level_of(K.slice_off, a.num_levels, slice);
  const int H = a.H[l], W = a.W[l];
  const int upr = ceil_div(W, TG_UNIT);
  const int nunits = a.B * H * upr;
  const int u0 = (slice - K.slice_off[l]) * K.units_per_slice;
  const int u1 = min(u0 + K.units_per_slice, nunits);
  const long npix = (long)a.B * H * W;
  const float x_inv = 1.f / a.x_plane_scale, y_inv = 1.f / a.y_plane_scale;
  const int K9 = 9 * a.Cin;
  const int nw = n0 + 32 * wave;             // first row of Cout of this wave
  const bool active = nw < a.Cout;           // (Cout is a multiple of 32: a wave has all of its rows or none)

  f32x16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float qacc = 0.f;

  for (int u = u0; u < u1; ++u) {
    const int row = u / upr, x0 = (u - row * upr) * TG_UNIT;
    const int b = row / H, y = row - b * H;
    const int len = min(TG_UNIT, W - x0);
    const long rowpix = ((long)b * H + y) * W;
    __syncthreads();  // the previous unit's reads are done
    for (int i = tid; i < TG_UNIT * TG_TN; i += TG_T) {
      const int px = i / TG_TN, nn = i - px * TG_TN;
      float v = 0.f;
      if (px < len && n0 + nn < a.Cout) v = tg_masked_g(a, l, npix, rowpix + x0 + px, n0 + nn, y_inv);
      gs[px][nn] = v;
    }
    for (int i = tid; i < 3 * (TG_UNIT + 2) * 32; i += TG_T) {
      const int r = i / ((TG_UNIT + 2) * 32), rem = i - r * ((TG_UNIT + 2) * 32);
      const int px = rem >> 5, c = rem & 31;
      const int yy = y + r - 1, xx = x0 + px - 1;
      float v = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W && px <= len + 1)
        v = load_act_any(a.x_mode, a.x[l], npix, ((long)b * H + yy) * W + xx, chunk * 32 + c, a.x_pitch, x_inv);
      xs[r][px][c] = v;
    }
    __syncthreads();
    if (!active) continue;  // (wave-uniform; the wave still takes part in the staging and its barriers)
    const int steps = (len + 1) >> 1;
    for (int s = 0; s < steps; ++s) {
      const int px = 2 * s + (lane >> 5);  // (an odd len: pixel `len` holds a zero gradient row)
      const float ga = gs[px][32 * wave + (lane & 31)];
      qacc += ga;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
          acc[ky * 3 + kx] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga, xs[ky][px + kx][lane & 31], acc[ky * 3 + kx], 0, 0, 0);
    }
  }
  if (!active) return;
  // the partial of this slice: part[slice][n][tap * Cin + c]; accumulator register r of a lane is row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  float* part = a.part + (long)slice * a.Cout * K9;
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = nw + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      part[(long)n * K9 + t * a.Cin + chunk * 32 + (lane & 31)] = acc[t][r];
    }
  if (chunk == 0) {  // the gradient's own sum over the slice: the two pixel halves of a row of Cout
    const float q = qacc + __shfl_down(qacc, 32);
    if (lane < 32) a.qpart[(long)slice * a.Cout + nw + lane] = q;
  }
}

__global__ __launch_bounds__(TG_T) void tower_wreduce_kernel(const TowerK K) {
  const dd3d_tower_grad_args& a = K.a;
  const int K9 = 9 * a.Cin;
  const int k = blockIdx.x * TG_T + threadIdx.x, n = blockIdx.y;
  if (k >= K9) return;
  const long e = (long)n * K9 + k, lv = (long)a.Cout * K9;
  float s = 0.f;
  for (int l = 0; l < a.num_levels; ++l) {
    float p = 0.f;
    for (int sl = K.slice_off[l]; sl < K.slice_off[l + 1]; ++sl) p += a.part[(long)sl * lv + e];
    a.dw_level[(long)l * lv + e] = p;
    s = fmaf(a.scale[l][n], p, s);
  }
  a.dw[e] = s;
}

__global__ __launch_bounds__(TG_T) void tower_rsum_kernel(const TowerK K) {
  const dd3d_tower_grad_args& a = K.a;
  __shared__ float red[TG_T];
  const int K9 = 9 * a.Cin;
  const int n = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  const float* P = a.dw_level + ((long)l * a.Cout + n) * K9;
  const float* w = a.w + (long)n * K9;
  float s = 0.f;
  for (int k = tid; k < K9; k += TG_T) s = fmaf(P[k], w[k], s);
  red[tid] = s;
  __syncthreads();
  for (int h = TG_T / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    float q = 0.f;
    for (int sl = K.slice_off[l]; sl < K.slice_off[l + 1]; ++sl) q += a.qpart[(long)sl * a.Cout + n];
    a.q[l * a.Cout + n] = q;
    a.r[l * a.Cout + n] = red[0];
  }
}

// ------------------------------------------------------------------------------------------------------------------- input gradient
template <int MT>
__global__ __launch_bounds__(TG_T, MT == 4 ? 1 : 2) void tower_dgrad_kernel(const TowerK K) {
  const dd3d_tower_grad_args& a = K.a;
  constexpr int TY = 2 * MT, HY = TY + 2, HX = TG_DX + 2;
  __shared__ float sg[HY * HX * TG_DS];  // s_l[n] * g_l at rows y0 - 1 .. y0 + TY, pixels x0 - 1 .. x0 + 16, one 32-channel chunk of Cout
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l = tg_level_of(K.tile_off, a.num_levels, blockIdx.x);
  const int H = a.H[l], W = a.W[l];
  const int tx_n = ceil_div(W, TG_DX), ty_n = ceil_div(H, TY);
  int t = blockIdx.x - K.tile_off[l];
  const int b = t / (ty_n * tx_n);
  t -= b * ty_n * tx_n;
  const int y0 = (t / tx_n) * TY, x0 = (t % tx_n) * TG_DX;
  const long npix = (long)a.B * H * W;
  const float y_inv = 1.f / a.y_plane_scale;
  const int K9 = 9 * a.Cin;
  const int c0 = 32 * wave, c1 = 32 * (wave + 4);  // the wave's channel chunks of Cin
  const bool act0 = c0 < a.Cin, act1 = c1 < a.Cin;
  const int m = lane & 31, kh = lane >> 5;         // A: pixel m of a 2 x 16 sub-tile, k half; B: filter row k half, input channel m

  f32x16 acc[MT][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  for (int nc = 0; nc < a.Cout; nc += 32) {
    __syncthreads();  // the previous chunk's reads are done
    for (int i = tid; i < HY * HX * 32; i += TG_T) {
      const int hp = i >> 5, n = nc + (i & 31);
      const int hy = hp / HX, hx = hp - hy * HX;
      const int yy = y0 + hy - 1, xx = x0 + hx - 1;
      float v = 0.f;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const float g = tg_masked_g(a, l, npix, ((long)b * H + yy) * W + xx, n, y_inv);
        if (g != 0.f) v = a.scale[l][n] * g;  // (a masked or zero gradient stays an exact zero whatever the scale holds)
      }
      sg[hp * TG_DS + (i & 31)] = v;
    }
    __syncthreads();
    if (!act0) continue;  // (wave-uniform: Cin <= 96 leaves the last waves without a chunk)
    f32x16 part[MT][2];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) part[i][j][r] = 0.f;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - 3 * ky;
      // da[y][x] += g[y - ky + 1][x - kx + 1] * W[n][ky][kx][c]: staged row (y - y0) - ky + 2, staged pixel (x - x0) - kx + 2
      const float* ap = sg + (((m >> 4) + 2 - ky) * HX + (m & 15) + 2 - kx) * TG_DS + kh;
      const float* wp = a.w + (long)(nc + kh) * K9 + tap * a.Cin + m;
#pragma unroll 4
      for (int s = 0; s < 16; ++s) {
        const float b0 = wp[(long)(2 * s) * K9 + c0];
        const float b1 = act1 ? wp[(long)(2 * s) * K9 + c1] : 0.f;
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const float av = ap[(2 * i * HX) * TG_DS + 2 * s];
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
  const bool add = a.da_add[l] != nullptr;
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int mm = (r & 3) + 8 * (r >> 2) + 4 * kh;  // accumulator register r of a lane: pixel mm of the sub-tile, channel lane & 31
      const int yy = y0 + 2 * i + (mm >> 4), xx = x0 + (mm & 15);
      if (yy >= H || xx >= W) continue;
      const long o = (((long)b * H + yy) * W + xx) * a.Cin + m;
      a.da[l][o + c0] = add ? a.da_add[l][o + c0] + acc[i][0][r] : acc[i][0][r];
      if (act1) a.da[l][o + c1] = add ? a.da_add[l][o + c1] + acc[i][1][r] : acc[i][1][r];
    }
}

// what the tiling depends on: the geometry and the channel counts
static int check_tower_shape(const dd3d_tower_grad_args* a, const char* who) {
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->num_levels >= 1 && a->num_levels <= DD3D_MAX_LEVELS && a->B >= 1, "%s: %d levels, B = %d", who, a->num_levels, a->B);
  DD3D_REQUIRE(a->Cin >= 32 && a->Cin % 32 == 0 && a->Cin <= DD3D_TG_MAX_C, "%s: Cin = %d is not a multiple of 32 up to %d", who, a->Cin, DD3D_TG_MAX_C);
  DD3D_REQUIRE(a->Cout >= 32 && a->Cout % 32 == 0 && a->Cout <= DD3D_TG_MAX_C, "%s: Cout = %d is not a multiple of 32 up to %d", who, a->Cout, DD3D_TG_MAX_C);
  DD3D_REQUIRE(a->dgrad_rows == 0 || a->dgrad_rows == 2 || a->dgrad_rows == 4 || a->dgrad_rows == 8, "%s: dgrad_rows = %d (0, 2, 4 or 8)", who, a->dgrad_rows);
  long pixels = 0;
  for (int l = 0; l < a->num_levels; ++l) {
    DD3D_REQUIRE(a->H[l] >= 1 && a->W[l] >= 1, "%s: level %d is %d x %d", who, l, a->H[l], a->W[l]);
    pixels += (long)a->B * a->H[l] * a->W[l];
  }
  DD3D_REQUIRE(pixels < (1l << 31) / 1024, "%s: %ld pixels", who, pixels);
  return DD3D_OK;
}

static int check_tower_args(const dd3d_tower_grad_args* a, const char* who, bool wgrad) {
  const int rc = check_tower_shape(a, who);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(a->g_pitch % 4 == 0 && a->g_pitch >= a->Cout, "%s: g_pitch = %d must be a multiple of 4 and hold %d channels", who, a->g_pitch, a->Cout);
  const int modes[2] = {a->x_mode, a->y_mode}, pitches[2] = {a->x_pitch, a->y_pitch}, chans[2] = {a->Cin, a->Cout};
  const float scales[2] = {a->x_plane_scale, a->y_plane_scale};
  for (int i = wgrad ? 0 : 1; i < 2; ++i) {
    const char* nm = i ? "y" : "x";
    DD3D_REQUIRE(modes[i] == DD3D_PG_ACT_F32 || modes[i] == DD3D_PG_ACT_F16X2 || modes[i] == DD3D_PG_ACT_BF16X3, "%s: %s_mode = %d", who, nm, modes[i]);
    if (modes[i] == DD3D_PG_ACT_F32)
      DD3D_REQUIRE(pitches[i] % 4 == 0 && pitches[i] >= chans[i], "%s: %s_pitch = %d must be a multiple of 4 and hold %d channels", who, nm, pitches[i], chans[i]);
    if (modes[i] == DD3D_PG_ACT_F16X2) DD3D_REQUIRE(scales[i] > 0.f, "%s: %s_plane_scale = %g", who, nm, (double)scales[i]);
  }
  DD3D_REQUIRE(a->w != nullptr, "%s: no filter", who);
  for (int l = 0; l < a->num_levels; ++l) {
    DD3D_REQUIRE(a->g[l] && a->y[l] && a->scale[l], "%s: level %d has no gradient / stored output / scale", who, l);
    if (wgrad) DD3D_REQUIRE(a->x[l], "%s: level %d has no input", who, l);
    else DD3D_REQUIRE(a->da[l], "%s: level %d has no input-gradient buffer", who, l);
    if (!wgrad) DD3D_REQUIRE((a->da_add[l] != nullptr) == (a->da_add[0] != nullptr), "%s: da_add is set on some levels only", who);
  }
  return DD3D_OK;
}

}  // namespace dd3d

extern "C" int64_t dd3d_tower_grad_slices(const dd3d_tower_grad_args* args) {
  using namespace dd3d;
  if (check_tower_shape(args, "dd3d_tower_grad_slices") != DD3D_OK) return -1;
  TowerK k;
  k.a = *args;
  plan_tower(k.a, k);
  return k.slice_off[args->num_levels];
}

extern "C" int dd3d_tower_wgrad(const dd3d_tower_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_tower_args(args, "dd3d_tower_wgrad", true);
  if (rc != DD3D_OK) return rc;
  TowerK k;
  k.a = *args;
  plan_tower(k.a, k);
  const int nslices = k.slice_off[args->num_levels];
  DD3D_REQUIRE(args->part && args->qpart && args->n_slices >= nslices, "dd3d_tower_wgrad: part / qpart (%d slices for %d)", args->n_slices, nslices);
  DD3D_REQUIRE(args->dw_level && args->dw && args->q && args->r, "dd3d_tower_wgrad: null output");
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)nslices, (unsigned)(args->Cin / 32), (unsigned)ceil_div(args->Cout, TG_TN));
  hipLaunchKernelGGL(tower_wgrad_kernel, grid, dim3(TG_T), 0, s, k);
  int e = check_launch("tower_wgrad_kernel");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(tower_wreduce_kernel, dim3((unsigned)ceil_div(9 * args->Cin, TG_T), (unsigned)args->Cout), dim3(TG_T), 0, s, k);
  if ((e = check_launch("tower_wreduce_kernel")) != DD3D_OK) return e;
  hipLaunchKernelGGL(tower_rsum_kernel, dim3((unsigned)args->Cout, (unsigned)args->num_levels), dim3(TG_T), 0, s, k);
  return check_launch("tower_rsum_kernel");
}

extern "C" int dd3d_tower_dgrad(const dd3d_tower_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = check_tower_args(args, "dd3d_tower_dgrad", false);
  if (rc != DD3D_OK) return rc;
  TowerK k;
  k.a = *args;
  plan_tower(k.a, k);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)k.tile_off[args->num_levels]);
  switch (k.mt) {
    case 4: hipLaunchKernelGGL(tower_dgrad_kernel<4>, grid, dim3(TG_T), 0, s, k); break;
    case 2: hipLaunchKernelGGL(tower_dgrad_kernel<2>, grid, dim3(TG_T), 0, s, k); break;
    default: hipLaunchKernelGGL(tower_dgrad_kernel<1>, grid, dim3(TG_T), 0, s, k); break;
  }
  return check_launch("tower_dgrad_kernel");
}

extern "C" int dd3d_tower_grad_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 32, "dd3d_tower_grad_layout: need 32 slots");
#define OFF(f) (int64_t) offsetof(dd3d_tower_grad_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_tower_grad_args), OFF(x), OFF(y), OFF(g), OFF(scale), OFF(da_add), OFF(da), OFF(w), OFF(part), OFF(qpart),
                       OFF(dw_level), OFF(dw), OFF(q), OFF(r), OFF(H), OFF(W), OFF(num_levels), OFF(B), OFF(Cin), OFF(Cout), OFF(g_pitch),
                       OFF(x_mode), OFF(x_pitch), OFF(y_mode), OFF(y_pitch), OFF(n_slices), OFF(dgrad_rows), OFF(x_plane_scale), OFF(y_plane_scale)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
