// Gradient of the dense-depth training loss (dense_depth_loss.hip) with respect to the raw per-level predictor maps, for gfx950:
//   d_raw[l](b, i, j) = up[l] * weight / (divisor[l] * N * pix_b) * sum over valid p with (i, j) among its taps of tapweight(p; i, j) * s'(v_l(p) - gt(p))
// The derivative passes through the TRANSPOSE of the aligned bilinear up-sampling: every canvas pixel scatters to its four taps.  No
// float atomics and no full-resolution buffer; every sum has a fixed order, so two launches on the same inputs agree bit for bit.
//
// All canvas pixels of one level-l CELL share their four taps: the pixels whose source row and column (after the "half" shift and clamp,
// aligned_bilinear.h) truncate to (ci, cj).  A cell is the rectangle rows [ci*f + f/2, (ci+1)*f + f/2) (no f/2 without "half"; the first
// cell starts at 0, the last ends at Hp), likewise in x; the entry point checks on the host, with the same f32 arithmetic, that this is
// so for every level (it is for every power-of-two stride).  The tap weights separate into a row and a column factor.
//
//   dense_depth_grad_cells_kernel   pass 1.  One WAVE per (level, image, cell, sub-tile): a sub-tile is a run of rows of a cell holding
//                                   at most ~1024 pixels (whole cells up to stride 16, 24 sub-tiles of 8 rows at stride 128 under "half":
//                                   few, large cells still fill the chip).  A lane reads four pixels per iteration (one 16-byte load:
//                                   cell borders are multiples of 4), evaluates the prediction from the cell's four tap values (loaded once
//                                   per wave) with the forward's own blend, and keeps four corner sums of weight * s'; a wave butterfly,
//                                   then lane 0 stores the slab row.  Unscaled: neither 1/N nor `up` enters.  A wave instead of a block
//                                   per sub-tile: no LDS, no barrier, and the level-0 cells (64 .. 144 pixels) do not idle three waves.
//   dense_depth_grad_gather_kernel  pass 2.  One thread per raw pixel adds, in a fixed order, the corner sums that land on it: the cells
//                                   (i-1 .. i) x (j-1 .. j), each corner whose tap index (from aligned_bilinear_taps: the edge replication
//                                   puts both row weights of the last cell row on row h-1) equals (i, j), every sub-tile in turn; then the
//                                   scale, with N read from the forward's count[0], and the store of channel 0 -- zeros included.
// The grid of both passes is exact (no cap, no loop over work items); the entry point checks that the item counts stay below 2^31.
#include <math.h>

#include "aligned_bilinear.h"
#include "common.h"
#include "dense_depth_args.h"
#include "smooth_l1.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

constexpr int GT = 256;                // threads per block
constexpr int GW = GT / 64;            // waves (= pass-1 work items) per block
constexpr int DDG_TILE_PIXELS = 1024;  // pixels of a full-width sub-tile, about (one 16-byte load x 4 per lane)

typedef float f32x4 __attribute__((ext_vector_type(4)));

// rows / columns of the largest cell of a level: the first one under "half" also takes the canvas's first f/2 rows
__host__ __device__ inline int ddg_cell_extent(int f, int half) { return f + (half ? f / 2 : 0); }
__host__ __device__ inline int ddg_tile_rows(int f, int half) {
  const int r = DDG_TILE_PIXELS / f, m = ddg_cell_extent(f, half);
  return r < 1 ? 1 : (r < m ? r : m);
}
// first canvas row (column) of cell c of n: the cells partition [0, n*f)
__host__ __device__ inline int ddg_cell_begin(int c, int n, int f, int half) { return c <= 0 ? 0 : (c >= n ? n * f : c * f + (half ? f / 2 : 0)); }

struct DenseDepthGradK {
  dd3d_dense_depth_loss_args a;
  dd3d_dense_depth_grad_args g;
  int item_off[DD3D_MAX_LEVELS + 1];  // pass-1 work items (= slab rows) before each level
  int pix_off[DD3D_MAX_LEVELS + 1];   // raw pixels before each level
  int tile_rows[DD3D_MAX_LEVELS], nsub[DD3D_MAX_LEVELS];
};

__global__ __launch_bounds__(GT) void dense_depth_grad_cells_kernel(const DenseDepthGradK P) {
  const dd3d_dense_depth_loss_args& a = P.a;
  const int lane = threadIdx.x & 63;
  const int item = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * GW + (threadIdx.x >> 6)));  // wave-uniform
  if (item >= P.item_off[a.num_levels]) return;
  int l = 0;
  while (item >= P.item_off[l + 1]) ++l;
  const int h = a.h[l], w = a.w[l], f = a.stride[l], half = a.offset_half;
  const int nsub = P.nsub[l], trows = P.tile_rows[l];
  int rem = item - P.item_off[l];
  const int s = rem % nsub;
  rem /= nsub;
  const int cj = rem % w;
  rem /= w;
  const int ci = rem % h, b = rem / h;
  const int ya = ddg_cell_begin(ci, h, f, half), yb = ddg_cell_begin(ci + 1, h, f, half);
  const int xa = ddg_cell_begin(cj, w, f, half), xb = ddg_cell_begin(cj + 1, w, f, half);
  const int r0 = ya + s * trows, r1 = min(r0 + trows, yb);  // an empty sub-tile (a short border cell) still writes its zero row
  const int qw = (xb - xa) >> 2, nq = max(r1 - r0, 0) * qw;
  // the cell's taps, from the geometry's one statement, at the cell's first pixel
  const BilinearTaps t0 = aligned_bilinear_taps(ya, xa, h, w, f, half);
  const float* p = a.raw[l] + (long)b * h * w * a.pitch;
  const float v00 = p[((long)t0.y0 * w + t0.x0) * a.pitch], v01 = p[((long)t0.y0 * w + t0.x1) * a.pitch];
  const float v10 = p[((long)t0.y1 * w + t0.x0) * a.pitch], v11 = p[((long)t0.y1 * w + t0.x1) * a.pitch];
  const float factor = a.focal_factor;
  const float pix = aligned_bilinear_pixel_size(a.inv_K, b, factor);
  const float* gt_img = a.gt + (long)b * a.Hp * a.Wp;
  float c00 = 0.f, c01 = 0.f, c10 = 0.f, c11 = 0.f;
  for (int q = lane; q < nq; q += 64) {
    const int y = r0 + q / qw, x = xa + (q % qw) * 4;
    const f32x4 g = *reinterpret_cast<const f32x4*>(gt_img + (long)y * a.Wp + x);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gt = g[e];
      if (!(gt < a.min_depth) && !(gt > a.max_depth)) {  // the forward's validity test
        const BilinearTaps t = aligned_bilinear_taps(y, x + e, h, w, f, half);  // (t.y0, t.x0) == (ci, cj): the host checked
        float v = aligned_bilinear_blend(t, v00, v01, v10, v11);
        if (factor > 0.f) v = v / pix;
        const float d = smooth_l1_grad(v, gt, a.beta);
        const float d0 = (1.f - t.ly) * d, d1 = t.ly * d;
        c00 += (1.f - t.lx) * d0;
        c01 += t.lx * d0;
        c10 += (1.f - t.lx) * d1;
        c11 += t.lx * d1;
      }
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {  // fixed-order butterfly
    c00 += __shfl_xor(c00, o, 64);
    c01 += __shfl_xor(c01, o, 64);
    c10 += __shfl_xor(c10, o, 64);
    c11 += __shfl_xor(c11, o, 64);
  }
  if (lane == 0) {
    f32x4 r;
    r[0] = c00, r[1] = c01, r[2] = c10, r[3] = c11;
    *reinterpret_cast<f32x4*>(P.g.slab + (long)item * DD3D_DDG_ROW) = r;
  }
}

__global__ __launch_bounds__(GT) void dense_depth_grad_gather_kernel(const DenseDepthGradK P) {
  const dd3d_dense_depth_loss_args& a = P.a;
  const int idx = (int)(blockIdx.x * GT + threadIdx.x);
  if (idx >= P.pix_off[a.num_levels]) return;
  int l = 0;
  while (idx >= P.pix_off[l + 1]) ++l;
  const int h = a.h[l], w = a.w[l], f = a.stride[l], half = a.offset_half, nsub = P.nsub[l];
  int rem = idx - P.pix_off[l];
  const int j = rem % w;
  rem /= w;
  const int i = rem % h, b = rem / h;
  float acc = 0.f;
  for (int ci = max(i - 1, 0); ci <= i; ++ci) {
    for (int cj = max(j - 1, 0); cj <= j; ++cj) {
      const BilinearTaps t0 = aligned_bilinear_taps(ddg_cell_begin(ci, h, f, half), ddg_cell_begin(cj, w, f, half), h, w, f, half);
      const float* rows = P.g.slab + ((long)P.item_off[l] + (((long)b * h + ci) * w + cj) * nsub) * DD3D_DDG_ROW;
#pragma unroll
      for (int c = 0; c < 4; ++c) {  // corner c = 2 * (row tap) + (column tap), the order of the slab row
        if (((c >> 1) ? t0.y1 : t0.y0) == i && ((c & 1) ? t0.x1 : t0.x0) == j) {
          for (int s = 0; s < nsub; ++s) acc += rows[s * DD3D_DDG_ROW + c];
        }
      }
    }
  }
  const long long n = a.count[0];
  float scale = 0.f;  // no valid pixel: zeros, what autograd gives the mean of an empty selection
  if (n > 0) {
#pragma clang fp contract(off)
    scale = (P.g.upstream[l] * ((a.loss_weight / (float)n) / a.divisor[l])) / aligned_bilinear_pixel_size(a.inv_K, b, a.focal_factor);
  }
  P.g.d_raw[l][(((long)b * h + i) * w + j) * a.pitch] = acc * scale;
}

// the levels' work tables; DD3D_OK, or the reason the backward cannot run on these args
static int plan_dense_depth_grad(const dd3d_dense_depth_loss_args* a, DenseDepthGradK* K, const char* who) {
  const int ok = check_dense_depth_args(a, who);
  if (ok != DD3D_OK) return ok;
  const int half = a->offset_half ? 1 : 0;
  long items = 0, pix = 0;
  for (int l = 0; l < a->num_levels; ++l) {
    const int f = a->stride[l];
    DD3D_REQUIRE(f % 4 == 0 && (!half || f % 8 == 0), "%s: level %d has stride %d: the gradient needs a multiple of %d (16-byte loads inside a cell)", who,
                 l, f, half ? 8 : 4);
    // The cells must be what ddg_cell_begin says: the first and the last pixel of every run truncate to the run's index, in the kernels'
    // own f32 arithmetic (monotone in between).
    const int n2[2] = {a->h[l], a->w[l]};
    for (int d = 0; d < 2; ++d) {
      for (int c = 0; c < n2[d]; ++c) {
        DD3D_REQUIRE((int)aligned_bilinear_source(c * f, n2[d], f) == c && (int)aligned_bilinear_source(c * f + f - 1, n2[d], f) == c,
                     "%s: level %d, stride %d: the f32 source coordinates of cell %d do not truncate to one index; the gradient needs a stride "
                     "for which they do (any power of two)", who, l, f, c);
      }
    }
    K->tile_rows[l] = ddg_tile_rows(f, half);
    K->nsub[l] = ceil_div(ddg_cell_extent(f, half), K->tile_rows[l]);
    K->item_off[l] = (int)items;
    K->pix_off[l] = (int)pix;
    pix += (long)a->B * a->h[l] * a->w[l];
    items += (long)a->B * a->h[l] * a->w[l] * K->nsub[l];
    DD3D_REQUIRE(items < (1L << 31) - GT && pix < (1L << 31) - GT, "%s: canvas too large", who);
  }
  for (int l = a->num_levels; l <= DD3D_MAX_LEVELS; ++l) K->item_off[l] = (int)items, K->pix_off[l] = (int)pix;
  K->a = *a;
  return DD3D_OK;
}

}  // namespace dd3d

extern "C" int64_t dd3d_dense_depth_grad_rows(const dd3d_dense_depth_loss_args* a) {
  using namespace dd3d;
  DenseDepthGradK K{};
  if (plan_dense_depth_grad(a, &K, "dd3d_dense_depth_grad_rows") != DD3D_OK) return -1;
  return K.item_off[a->num_levels];
}

extern "C" int dd3d_dense_depth_loss_backward(const dd3d_dense_depth_loss_args* a, const dd3d_dense_depth_grad_args* g, void* stream) {
  using namespace dd3d;
  DenseDepthGradK K{};
  const int ok = plan_dense_depth_grad(a, &K, "dd3d_dense_depth_loss_backward");
  if (ok != DD3D_OK) return ok;
  DD3D_REQUIRE(g != nullptr, "dd3d_dense_depth_loss_backward: null grad args");
  DD3D_REQUIRE(g->upstream && g->slab, "dd3d_dense_depth_loss_backward: null upstream or slab");
  DD3D_REQUIRE((reinterpret_cast<uintptr_t>(g->slab) & 15) == 0, "dd3d_dense_depth_loss_backward: the slab must be 16-byte aligned");
  for (int l = 0; l < a->num_levels; ++l) DD3D_REQUIRE(g->d_raw[l] != nullptr, "dd3d_dense_depth_loss_backward: level %d has no gradient map", l);
  const int items = K.item_off[a->num_levels], pix = K.pix_off[a->num_levels];
  DD3D_REQUIRE(g->n_slab >= items, "dd3d_dense_depth_loss_backward: the slab holds %lld rows, the launch writes %d", (long long)g->n_slab, items);
  K.g = *g;
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dense_depth_grad_cells_kernel, dim3((unsigned)ceil_div(items, GW)), dim3(GT), 0, s, K);
  const int e = check_launch("dense_depth_grad_cells_kernel");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(dense_depth_grad_gather_kernel, dim3((unsigned)ceil_div(pix, GT)), dim3(GT), 0, s, K);
  return check_launch("dense_depth_grad_gather_kernel");
}

extern "C" int dd3d_dense_depth_grad_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 8, "dd3d_dense_depth_grad_layout: need 8 slots");
#define OFF(f) (int64_t) offsetof(dd3d_dense_depth_grad_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_dense_depth_grad_args), OFF(d_raw), OFF(upstream), OFF(slab), OFF(n_slab)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
