// Backward of the DLA-34 stem's three convolutions (dla.py base_layer, level0, level1) for gfx950: the gradients of ONE k x k, stride s,
// Cin -> Cout convolution with a folded norm and a ReLU per call, (k, s, Cin, Cout) in {(7, 1, 4, 16), (3, 1, 16, 16), (3, 2, 16, 32)},
// padding (k - 1) / 2.  include/dd3d_hip.h states the mathematics; the quantities are dd3d_backbone_wgrad's / dd3d_backbone_dgrad's.
// These layers run at full resolution with 4, 16 and 32 channels: a 16-channel pixel is one 64-byte line, and both gradients are GEMMs
// on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation), whose 16-wide operands the stem's channel counts fill without
// padding.  No LDS staging: a lane fetches its operand from global memory (a pixel's channels are one line, neighbouring taps hit L1).
//
// Weight gradient -- M = Cout, N = k * k * Cin, K = the output pixels:
//   sg_wgrad_kernel<KS, S, CIN, COUT>  block = one slice (or several, wgrad_blocks), four waves; a slice is a run of units, a unit is up
//                        to 64 output pixels of one output row; wave w takes the units w, w + 4, .. of the slice.  One MFMA step is four
//                        output pixels: A = the masked gradient [n][pixel], B = the input [pixel][column].  With Cin = 16 a column is a
//                        channel and there is one B per tap; with Cin = 4 (the 7 x 7 on the image) a B holds four neighbouring taps
//                        kx of a filter row ([kx][c] is contiguous in an NHWC4 pixel row), two B per filter row, the eighth kx unused.
//                        The four waves' sums meet in LDS in the order (w0 + w2) + (w1 + w3); wave 0 writes the slice's partial.
//   sg_wreduce_kernel    thread = one word of the filter: the slices in slice order, 64 to a sub-sum -> dw_level, times scale[n] -> dw.
//   sg_rsum_kernel       block = n: r = sum_k dw_level * W, q = the slices' gradient sums in the same two-level order.
// Input gradient (the two 3 x 3 shapes) -- M = input pixels, N = Cin = 16, K = 9 * Cout:
//   sg_dgrad_kernel<S, COUT>  wave = a tile of 16 S input pixels of one row, waves go over tiles with a grid stride.  Stride 1: one
//                        16-pixel sub-tile and all nine taps.  Stride 2: two sub-tiles, the even and the odd pixels of the tile, and per
//                        sub-tile only the taps whose parity lands on an output pixel: 1, 2, 2 or 4 of them by (row, column) parity.
//                        The filter (scaled gradient times W: A = scale[n] * masked g, B = W[n][tap][c]) lives in registers for the
//                        whole run of a wave.  One accumulator chain per pixel: at most 9 * 16 or 4 * 32 terms.
// No float atomics: every sum has one writer and a fixed order that depends on the call's shape alone; two runs agree bit for bit,
// whatever wgrad_blocks holds.
//
// The VoVNet-V2 stem's first convolution (vovnet.py stem_1: 3 x 3, stride 2, the four-channel image -> 64 channels) is the same weight
// gradient at (k, s, Cin, Cout) = (3, 2, 4, 64), through entry points of its own (dd3d_vovnet_stem_wgrad / dd3d_vovnet_stem_grad_slices):
// sg_wgrad_kernel<3, 2, 4, 64> -- one B per filter row holds its three taps kx times four channels, the fourth tap slot unused; four
// blocks of 16 rows of Cout share it: twelve accumulator tiles a wave, 25088 bytes of LDS for the waves' meeting.  The image has no
// gradient, so there is no input-gradient call.
#include "act_load.h"
#include "common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

typedef float sg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int SG_T = 256;          // threads of every block here
constexpr int SG_GROUP = 64;       // slices per sub-sum of the reduce
constexpr int SG_DGRAD_BLOCKS = 4096;

struct StemK {
  dd3d_stem_grad_args a;
  int32_t Ho, Wo, nslices, units_per_slice;
  float y_inv;
};

inline int sg_out(int n, int s) { return (n + s - 1) / s; }

inline void plan_stem(const dd3d_stem_grad_args& a, StemK& k) {
  k.a = a;
  k.Ho = sg_out(a.H, a.stride), k.Wo = sg_out(a.W, a.stride);
  const long units = (long)a.B * k.Ho * ceil_div(k.Wo, DD3D_SG_UNIT);
  long ups = (units + DD3D_SG_TARGET_SLICES - 1) / DD3D_SG_TARGET_SLICES;
  if (ups < DD3D_SG_MIN_UNITS_PER_SLICE) ups = DD3D_SG_MIN_UNITS_PER_SLICE;
  if (ups > DD3D_SG_MAX_UNITS_PER_SLICE) ups = DD3D_SG_MAX_UNITS_PER_SLICE;
  const long slice_bytes = (long)a.Cout * a.ksize * a.ksize * a.Cin * (long)sizeof(float);
  const long max_slices = DD3D_TG_SLAB_BYTES / slice_bytes;  // (at least 8738: a stem slice is at most 32 x 196 words)
  if (ups * max_slices < units) ups = (units + max_slices - 1) / max_slices;
  k.units_per_slice = (int)ups;
  k.nslices = (int)((units + ups - 1) / ups);
  k.y_inv = 1.f / a.y_plane_scale;
}

// the gradient that crosses the layer's ReLU at one output pixel and channel: g where the stored output is positive, else an exact zero
__device__ __forceinline__ float sg_masked(const StemK& K, long nopix, long pix, int n, float g) {
  return load_act_any(K.a.y_mode, K.a.y, nopix, pix, n, K.a.y_pitch, K.y_inv) > 0.f ? g : 0.f;
}

// ------------------------------------------------------------------------------------------------------------------ weight gradient
template <int KS, int S, int CIN, int COUT>
__global__ __launch_bounds__(SG_T) void sg_wgrad_kernel(const StemK K) {
  const dd3d_stem_grad_args& a = K.a;
  constexpr int P = (KS - 1) / 2, JP = 16 / CIN, NB = (KS + JP - 1) / JP, MB = COUT / 16, KK = KS * KS * CIN, NACC = KS * NB * MB;
  constexpr int WORDS = NACC * 256 + MB * 16;  // one wave's accumulators and gradient sums
  __shared__ float red[2][WORDS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane & 15, kp = lane >> 4;  // A: row n = col of a 16-block of Cout, pixel kp; B: pixel kp, column col
  const int dxj = col / CIN, c = col - dxj * CIN;
  const int H = a.H, W = a.W, Ho = K.Ho, Wo = K.Wo;
  const int upr = ceil_div(Wo, DD3D_SG_UNIT);
  const int nunits = a.B * Ho * upr;
  const long nopix = (long)a.B * Ho * Wo;

  for (int slice = blockIdx.x; slice < K.nslices; slice += gridDim.x) {
    sg_f32x4 acc[NACC];
    float qacc[MB];
#pragma unroll
    for (int t = 0; t < NACC; ++t) acc[t] = sg_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int m = 0; m < MB; ++m) qacc[m] = 0.f;
    const int u0 = slice * K.units_per_slice;
    const int u1 = min(u0 + K.units_per_slice, nunits);
    for (int u = u0 + wave; u < u1; u += 4) {
      const int row = u / upr, x0 = (u - row * upr) * DD3D_SG_UNIT;
      const int b = row / Ho, oy = row - b * Ho;
      const int len = min(DD3D_SG_UNIT, Wo - x0);
      const long rowpix = ((long)b * Ho + oy) * Wo;
      for (int st = 0; st < len; st += 4) {
        const int ox = x0 + st + kp;
        const bool valid = ox < Wo;  // (the last step of a unit may pass the row's end: those pixels feed exact zeros)
        float ga[MB];
#pragma unroll
        for (int m = 0; m < MB; ++m) {
          ga[m] = valid ? sg_masked(K, nopix, rowpix + ox, 16 * m + col, a.g[(rowpix + ox) * a.g_pitch + 16 * m + col]) : 0.f;
          qacc[m] += ga[m];
        }
#pragma unroll
        for (int ky = 0; ky < KS; ++ky) {
          const int yy = oy * S + ky - P;
          const bool rowok = valid && yy >= 0 && yy < H;
#pragma unroll
          for (int nb = 0; nb < NB; ++nb) {
            const int kx = nb * JP + dxj, xx = ox * S + kx - P;
            // (the address is formed only for a pixel inside the image)
            const float bv = (rowok && kx < KS && xx >= 0 && xx < W) ? a.x[(((long)b * H + yy) * W + xx) * a.x_pitch + c] : 0.f;
#pragma unroll
            for (int m = 0; m < MB; ++m)
              acc[(ky * NB + nb) * MB + m] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[m], bv, acc[(ky * NB + nb) * MB + m], 0, 0, 0);
          }
        }
      }
    }
    // the gradient's own sum: the four pixel lanes of a row of Cout, (0 + 1) + (2 + 3), into lanes 0 .. 15
    float qs[MB];
#pragma unroll
    for (int m = 0; m < MB; ++m) {
      const float v = qacc[m] + __shfl_down(qacc[m], 16);
      qs[m] = v + __shfl_down(v, 32);
    }
    // the four waves' sums in the order (w0 + w2) + (w1 + w3); a lane reads back the words a lane of the same number wrote
    __syncthreads();  // the previous slice's reads of `red` are done
    if (wave >= 2) {
      float* d = red[wave - 2];
#pragma unroll
      for (int t = 0; t < NACC; ++t) *reinterpret_cast<sg_f32x4*>(d + (t * 64 + lane) * 4) = acc[t];
      if (lane < 16)
#pragma unroll
        for (int m = 0; m < MB; ++m) d[NACC * 256 + m * 16 + lane] = qs[m];
    }
    __syncthreads();
    if (wave < 2) {
      const float* d = red[wave];
#pragma unroll
      for (int t = 0; t < NACC; ++t) acc[t] += *reinterpret_cast<const sg_f32x4*>(d + (t * 64 + lane) * 4);
      if (lane < 16)
#pragma unroll
        for (int m = 0; m < MB; ++m) qs[m] += d[NACC * 256 + m * 16 + lane];
    }
    __syncthreads();
    if (wave == 1) {
      float* d = red[0];
#pragma unroll
      for (int t = 0; t < NACC; ++t) *reinterpret_cast<sg_f32x4*>(d + (t * 64 + lane) * 4) = acc[t];
      if (lane < 16)
#pragma unroll
        for (int m = 0; m < MB; ++m) d[NACC * 256 + m * 16 + lane] = qs[m];
    }
    __syncthreads();
    if (wave == 0) {
      const float* d = red[0];
      // the partial of this slice: part[slice][n][(ky * KS + kx) * CIN + c]; register r of a lane is row 4 (lane >> 4) + r, column col
      float* part = a.part + (long)slice * COUT * KK;
#pragma unroll
      for (int t = 0; t < NACC; ++t) {
        const sg_f32x4 v = acc[t] + *reinterpret_cast<const sg_f32x4*>(d + (t * 64 + lane) * 4);
        const int m = t % MB, nb = (t / MB) % NB, ky = t / (MB * NB);
        const int kx = nb * JP + dxj;
        if (kx < KS)
#pragma unroll
          for (int r = 0; r < 4; ++r) part[(long)(16 * m + 4 * kp + r) * KK + (ky * KS + kx) * CIN + c] = v[r];
      }
      if (lane < 16)
#pragma unroll
        for (int m = 0; m < MB; ++m) a.qpart[(long)slice * COUT + 16 * m + lane] = qs[m] + d[NACC * 256 + m * 16 + lane];
    }
  }
}

// the slices in slice order, SG_GROUP to a sub-sum, the sub-sums in their order
__device__ __forceinline__ float sg_sum_slices(const float* p, long stride, int nslices) {
  float total = 0.f;
  for (int s0 = 0; s0 < nslices; s0 += SG_GROUP) {
    const int s1 = min(s0 + SG_GROUP, nslices);
    float sub = 0.f;
    for (int sl = s0; sl < s1; ++sl) sub += p[(long)sl * stride];
    total += sub;
  }
  return total;
}

__global__ __launch_bounds__(SG_T) void sg_wreduce_kernel(const StemK K, const int KK) {
  const dd3d_stem_grad_args& a = K.a;
  const int e = blockIdx.x * SG_T + threadIdx.x, total = a.Cout * KK;
  if (e >= total) return;
  const float p = sg_sum_slices(a.part + e, total, K.nslices);
  a.dw_level[e] = p;
  a.dw[e] = a.scale[e / KK] * p;
}

__global__ __launch_bounds__(SG_T) void sg_rsum_kernel(const StemK K, const int KK) {
  const dd3d_stem_grad_args& a = K.a;
  __shared__ float red[SG_T];
  const int n = blockIdx.x, tid = threadIdx.x;
  red[tid] = tid < KK ? a.dw_level[(long)n * KK + tid] * a.w[(long)n * KK + tid] : 0.f;  // (KK is at most 196)
  __syncthreads();
  for (int h = SG_T / 2; h > 0; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0) {
    a.q[n] = sg_sum_slices(a.qpart + n, a.Cout, K.nslices);
    a.r[n] = red[0];
  }
}

// ------------------------------------------------------------------------------------------------------------------- input gradient
// one sub-tile: the 16 input pixels x0 + S i + PX of row y; S = 2: PY is the row's parity, and only the taps with y + 1 - ky and
// x + 1 - kx even reach an output pixel
template <int S, int COUT, int PY, int PX>
__device__ __forceinline__ void sg_dgrad_subtile(const StemK& K, const float (&breg)[9][COUT / 16][4], const float (&sc)[COUT / 16][4], int b, int y, int x0,
                                                 int lane) {
  const dd3d_stem_grad_args& a = K.a;
  constexpr int MB = COUT / 16;
  const int i = lane & 15, kq = lane >> 4;
  const int x = x0 + S * i + PX;
  const long nopix = (long)a.B * K.Ho * K.Wo;
  sg_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      if (S == 2 && (((PY + 1 + ky) & 1) || ((PX + 1 + kx) & 1))) continue;  // (compile time: the loops are unrolled)
      const int ny = y + 1 - ky, nx = x + 1 - kx;
      const int oy = ny / S, ox = nx / S;
      const bool ok = x < a.W && ny >= 0 && nx >= 0 && oy < K.Ho && ox < K.Wo;
#pragma unroll
      for (int h = 0; h < MB; ++h) {
        const int n0 = 16 * h + 4 * kq;  // this lane's four rows of K in the tap: n0 .. n0 + 3, one per step
        float av[4] = {0.f, 0.f, 0.f, 0.f};
        if (ok) {
          const long opix = ((long)b * K.Ho + oy) * K.Wo + ox;  // (formed only for an output pixel that exists)
          const float4 g4 = *reinterpret_cast<const float4*>(a.g + opix * a.g_pitch + n0);
          const float gv[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            const float gm = sg_masked(K, nopix, opix, n0 + s, gv[s]);
            if (gm != 0.f) av[s] = sc[h][s] * gm;  // (a masked or zero gradient stays an exact zero whatever the scale holds)
          }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], breg[ky * 3 + kx][h][s], acc, 0, 0, 0);
      }
    }
  // register r of a lane: pixel 4 (lane >> 4) + r of the sub-tile, channel lane & 15
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int xo = x0 + S * (4 * kq + r) + PX;
    if (xo < a.W) a.da[(((long)b * a.H + y) * a.W + xo) * a.da_pitch + i] = acc[r];
  }
}

template <int S, int COUT>
__global__ __launch_bounds__(SG_T) void sg_dgrad_kernel(const StemK K) {
  const dd3d_stem_grad_args& a = K.a;
  constexpr int MB = COUT / 16, KK = 9 * 16, TW = 16 * S;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cc = lane & 15, kq = lane >> 4;
  // B: filter row n = 16 h + 4 (lane >> 4) + s at step s of block h of a tap, input channel lane & 15; the scale of the same rows
  float breg[9][MB][4], sc[MB][4];
#pragma unroll
  for (int h = 0; h < MB; ++h)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int n = 16 * h + 4 * kq + s;
      sc[h][s] = a.scale[n];
#pragma unroll
      for (int t = 0; t < 9; ++t) breg[t][h][s] = a.w[(long)n * KK + t * 16 + cc];
    }
  const int xt = ceil_div(a.W, TW);
  const int ntiles = a.B * a.H * xt;
  for (int t = blockIdx.x * 4 + wave; t < ntiles; t += gridDim.x * 4) {
    const int row = t / xt, x0 = (t - row * xt) * TW;
    const int b = row / a.H, y = row - b * a.H;
    if (S == 1) {
      sg_dgrad_subtile<1, COUT, 0, 0>(K, breg, sc, b, y, x0, lane);
    } else if (y & 1) {  // (wave-uniform)
      sg_dgrad_subtile<2, COUT, 1, 0>(K, breg, sc, b, y, x0, lane);
      sg_dgrad_subtile<2, COUT, 1, 1>(K, breg, sc, b, y, x0, lane);
    } else {
      sg_dgrad_subtile<2, COUT, 0, 0>(K, breg, sc, b, y, x0, lane);
      sg_dgrad_subtile<2, COUT, 0, 1>(K, breg, sc, b, y, x0, lane);
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------------ host side
// the shapes of one family of entry points: the DLA stem's three, or (vovnet) stem_1's one
static int sg_check_shape(const dd3d_stem_grad_args* a, const char* who, bool dgrad, bool vovnet = false) {
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->B >= 1 && a->H >= 1 && a->W >= 1, "%s: B = %d, %d x %d", who, a->B, a->H, a->W);
  if (vovnet) {
    DD3D_REQUIRE(a->ksize == 3 && a->stride == 2 && a->Cin == 4 && a->Cout == 64, "%s: (ksize, stride, Cin, Cout) = (%d, %d, %d, %d) is not (3, 2, 4, 64)", who,
                 a->ksize, a->stride, a->Cin, a->Cout);
  } else {
    const bool base = a->ksize == 7 && a->stride == 1 && a->Cin == 4 && a->Cout == 16;
    const bool level0 = a->ksize == 3 && a->stride == 1 && a->Cin == 16 && a->Cout == 16;
    const bool level1 = a->ksize == 3 && a->stride == 2 && a->Cin == 16 && a->Cout == 32;
    DD3D_REQUIRE(base || level0 || level1, "%s: (ksize, stride, Cin, Cout) = (%d, %d, %d, %d) is none of (7, 1, 4, 16), (3, 1, 16, 16), (3, 2, 16, 32)", who,
                 a->ksize, a->stride, a->Cin, a->Cout);
    DD3D_REQUIRE(!(dgrad && base), "%s: the 7 x 7 on the image has no input gradient", who);
  }
  DD3D_REQUIRE((long)a->B * a->H * a->W <= DD3D_BG_MAX_PIXELS, "%s: %ld input pixels (at most %ld)", who, (long)a->B * a->H * a->W, (long)DD3D_BG_MAX_PIXELS);
  return DD3D_OK;
}

static int sg_check_args(const dd3d_stem_grad_args* a, const char* who, bool dgrad, bool vovnet = false) {
  const int rc = sg_check_shape(a, who, dgrad, vovnet);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(a->g && a->w && a->scale && a->y, "%s: no gradient / filter / scale / stored output", who);
  DD3D_REQUIRE(a->g_pitch % 4 == 0 && a->g_pitch >= a->Cout, "%s: g_pitch = %d must be a multiple of 4 and hold %d channels", who, a->g_pitch, a->Cout);
  DD3D_REQUIRE(a->y_mode == DD3D_PG_ACT_F32 || a->y_mode == DD3D_PG_ACT_F16X2 || a->y_mode == DD3D_PG_ACT_BF16X3, "%s: y_mode = %d", who, a->y_mode);
  if (a->y_mode == DD3D_PG_ACT_F32)
    DD3D_REQUIRE(a->y_pitch % 4 == 0 && a->y_pitch >= a->Cout, "%s: y_pitch = %d must be a multiple of 4 and hold %d channels", who, a->y_pitch, a->Cout);
  if (a->y_mode == DD3D_PG_ACT_F16X2) DD3D_REQUIRE(a->y_plane_scale > 0.f, "%s: y_plane_scale = %g", who, (double)a->y_plane_scale);
  if (dgrad) {
    DD3D_REQUIRE(a->da, "%s: no input-gradient buffer", who);
    DD3D_REQUIRE(a->da_pitch % 4 == 0 && a->da_pitch >= a->Cin, "%s: da_pitch = %d must be a multiple of 4 and hold %d channels", who, a->da_pitch, a->Cin);
    DD3D_REQUIRE(reinterpret_cast<uintptr_t>(a->g) % 16 == 0, "%s: g is not 16-byte aligned", who);
  } else {
    DD3D_REQUIRE(a->x, "%s: no input", who);
    DD3D_REQUIRE(a->x_pitch % 4 == 0 && a->x_pitch >= a->Cin, "%s: x_pitch = %d must be a multiple of 4 and hold %d channels", who, a->x_pitch, a->Cin);
  }
  return DD3D_OK;
}

}  // namespace dd3d

extern "C" int64_t dd3d_stem_grad_slices(const dd3d_stem_grad_args* args) {
  using namespace dd3d;
  if (sg_check_shape(args, "dd3d_stem_grad_slices", false) != DD3D_OK) return -1;
  StemK k;
  plan_stem(*args, k);
  return k.nslices;
}

namespace dd3d {

// the weight gradient's three launches for either family of entry points
static int sg_run_wgrad(const dd3d_stem_grad_args* args, void* stream, const char* who, bool vovnet) {
  const int rc = sg_check_args(args, who, false, vovnet);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(args->dw_level && args->dw && args->q && args->r, "%s: null output", who);
  StemK k;
  plan_stem(*args, k);
  DD3D_REQUIRE(args->part && args->qpart && args->n_slices >= k.nslices, "%s: part / qpart (%d slices for %d)", who, args->n_slices, k.nslices);
  DD3D_REQUIRE(args->wgrad_blocks >= 0, "%s: wgrad_blocks = %d", who, args->wgrad_blocks);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int KK = args->ksize * args->ksize * args->Cin;
  const dim3 grid((unsigned)(args->wgrad_blocks > 0 && args->wgrad_blocks < k.nslices ? args->wgrad_blocks : k.nslices));
  if (vovnet) hipLaunchKernelGGL((sg_wgrad_kernel<3, 2, 4, 64>), grid, dim3(SG_T), 0, s, k);
  else if (args->ksize == 7) hipLaunchKernelGGL((sg_wgrad_kernel<7, 1, 4, 16>), grid, dim3(SG_T), 0, s, k);
  else if (args->stride == 1) hipLaunchKernelGGL((sg_wgrad_kernel<3, 1, 16, 16>), grid, dim3(SG_T), 0, s, k);
  else hipLaunchKernelGGL((sg_wgrad_kernel<3, 2, 16, 32>), grid, dim3(SG_T), 0, s, k);
  int e = check_launch("sg_wgrad_kernel");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(sg_wreduce_kernel, dim3((unsigned)ceil_div(args->Cout * KK, SG_T)), dim3(SG_T), 0, s, k, KK);
  if ((e = check_launch("sg_wreduce_kernel")) != DD3D_OK) return e;
  hipLaunchKernelGGL(sg_rsum_kernel, dim3((unsigned)args->Cout), dim3(SG_T), 0, s, k, KK);
  return check_launch("sg_rsum_kernel");
}

}  // namespace dd3d

extern "C" int dd3d_stem_wgrad(const dd3d_stem_grad_args* args, void* stream) { return dd3d::sg_run_wgrad(args, stream, "dd3d_stem_wgrad", false); }

extern "C" int64_t dd3d_vovnet_stem_grad_slices(const dd3d_stem_grad_args* args) {
  using namespace dd3d;
  if (sg_check_shape(args, "dd3d_vovnet_stem_grad_slices", false, true) != DD3D_OK) return -1;
  StemK k;
  plan_stem(*args, k);
  return k.nslices;
}

extern "C" int dd3d_vovnet_stem_wgrad(const dd3d_stem_grad_args* args, void* stream) {
  return dd3d::sg_run_wgrad(args, stream, "dd3d_vovnet_stem_wgrad", true);
}

extern "C" int dd3d_stem_dgrad(const dd3d_stem_grad_args* args, void* stream) {
  using namespace dd3d;
  const int rc = sg_check_args(args, "dd3d_stem_dgrad", true);
  if (rc != DD3D_OK) return rc;
  StemK k;
  plan_stem(*args, k);
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long tiles = (long)args->B * args->H * ceil_div(args->W, 16 * args->stride);
  const long blocks = (tiles + 3) / 4;
  const dim3 grid((unsigned)(blocks < SG_DGRAD_BLOCKS ? blocks : SG_DGRAD_BLOCKS));
  if (args->stride == 1) hipLaunchKernelGGL((sg_dgrad_kernel<1, 16>), grid, dim3(SG_T), 0, s, k);
  else hipLaunchKernelGGL((sg_dgrad_kernel<2, 32>), grid, dim3(SG_T), 0, s, k);
  return check_launch("sg_dgrad_kernel");
}

extern "C" int dd3d_stem_grad_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 32, "dd3d_stem_grad_layout: need 32 slots");
#define OFF(f) (int64_t) offsetof(dd3d_stem_grad_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_stem_grad_args), OFF(x), OFF(y), OFF(g), OFF(w), OFF(scale), OFF(da), OFF(part), OFF(qpart), OFF(dw_level), OFF(dw),
                       OFF(q), OFF(r), OFF(B), OFF(H), OFF(W), OFF(Cin), OFF(Cout), OFF(ksize), OFF(stride), OFF(x_pitch), OFF(g_pitch), OFF(da_pitch),
                       OFF(y_mode), OFF(y_pitch), OFF(n_slices), OFF(wgrad_blocks), OFF(y_plane_scale)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
