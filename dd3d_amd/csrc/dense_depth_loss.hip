// Dense-depth training loss of DD3DDenseDepth for gfx950 (dense_depth.py:165-171, dense_depth_loss.py:28-36; the gradient: dense_depth_loss_grads.hip): per pyramid
// level the smooth-L1 mean, over the valid ground-truth pixels, between the ground truth and the level's depth map up-sampled to the
// input resolution -- WITHOUT materialising the up-sampled maps.
//
//   dense_depth_loss_kernel    one pass over the ground-truth canvas, four pixels (one 16-byte load) per thread and iteration.  For a
//                              valid pixel every level's prediction is evaluated in place: four bilinear taps into the level's raw
//                              predictor map (a few hundred KB over all levels: cache resident), aligned_bilinear_at
//                              (aligned_bilinear.h), which aligned_bilinear_scale_kernel (aux_kernels.hip) writes out.  A thread keeps one sum
//                              per level and one integer count; per-block sums in a fixed tree order go to a slab.
//   dense_depth_finalize_kernel one block: the slab summed in a fixed order, then mean, weight and the per-level divisor.
// No float atomics: two runs on the same inputs agree bit for bit.
#include <math.h>

#include "aligned_bilinear.h"
#include "common.h"
#include "dense_depth_args.h"
#include "smooth_l1.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

constexpr int DT = 256;                             // threads per block, four pixels per thread and iteration
constexpr int DDL_MAX_GRID = DD3D_DDL_MAX_BLOCKS;  // capped grid (256 CUs x 4 blocks); larger canvases loop

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct DenseDepthLossK {
  dd3d_dense_depth_loss_args a;
};

__global__ __launch_bounds__(DT) void dense_depth_loss_kernel(const DenseDepthLossK P) {
  const dd3d_dense_depth_loss_args& a = P.a;
  const int L = a.num_levels;
  const int Wq = a.Wp >> 2;  // quads per row (Wp is a multiple of 4: a quad never straddles rows)
  const long nquads = (long)a.B * a.Hp * Wq;
  const float factor = a.focal_factor;
  float sum[DD3D_MAX_LEVELS];
#pragma unroll
  for (int l = 0; l < DD3D_MAX_LEVELS; ++l) sum[l] = 0.f;
  int count = 0;
  for (long q = (long)blockIdx.x * DT + threadIdx.x; q < nquads; q += (long)gridDim.x * DT) {
    const f32x4 g = *reinterpret_cast<const f32x4*>(a.gt + q * 4);
    const int xq = (int)(q % Wq) * 4;
    const long t = q / Wq;
    const int y = (int)(t % a.Hp);
    const int b = (int)(t / a.Hp);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float gt = g[e];
      // dense_depth_loss.py:29-33: valid iff NOT gt < min and NOT gt > max (a NaN passes both and makes the sums NaN, as there)
      if (!(gt < a.min_depth) && !(gt > a.max_depth)) {
        ++count;
#pragma unroll
        for (int l = 0; l < DD3D_MAX_LEVELS; ++l) {
          if (l < L) {
            const float v = aligned_bilinear_at(a.raw[l], a.inv_K, b, y, xq + e, a.h[l], a.w[l], a.pitch, a.stride[l], a.offset_half, factor);
            {  // the running sum rounded on its own, like the smooth-L1's operations (smooth_l1.h) and the reference's tensor ops
#pragma clang fp contract(off)
              sum[l] = sum[l] + smooth_l1(v, gt, a.beta);
            }
          }
        }
      }
    }
  }
  // fixed-order block reduction: wave butterfly, then the four wave sums in order
  __shared__ float ws[DT / 64][DD3D_MAX_LEVELS];
  __shared__ int wc[DT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int l = 0; l < DD3D_MAX_LEVELS; ++l) {
    float v = sum[l];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) ws[wave][l] = v;
  }
  {
    int c = count;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) wc[wave] = c;
  }
  __syncthreads();
  float* row = a.partials + (long)blockIdx.x * DD3D_DDL_ROW;
  if (threadIdx.x < DD3D_MAX_LEVELS) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < DT / 64; ++w) s += ws[w][threadIdx.x];
    row[threadIdx.x] = s;
  } else if (threadIdx.x == DD3D_MAX_LEVELS) {
    int c = 0;
#pragma unroll
    for (int w = 0; w < DT / 64; ++w) c += wc[w];
    reinterpret_cast<int32_t*>(row)[DD3D_MAX_LEVELS] = c;  // (a block sees fewer than 2^31 pixels: the entry point checks)
  }
}

__global__ __launch_bounds__(DT) void dense_depth_finalize_kernel(const DenseDepthLossK P, int nblocks) {
  const dd3d_dense_depth_loss_args& a = P.a;
  __shared__ float red[DT];
  __shared__ long long redc[DT];
  __shared__ float S[DD3D_MAX_LEVELS];
  for (int k = 0; k < a.num_levels; ++k) {
    float s = 0.f;
    for (int r = threadIdx.x; r < nblocks; r += DT) s += a.partials[(long)r * DD3D_DDL_ROW + k];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int h = DT / 2; h > 0; h >>= 1) {
      if (threadIdx.x < h) red[threadIdx.x] += red[threadIdx.x + h];
      __syncthreads();
    }
    if (threadIdx.x == 0) S[k] = red[0];
    __syncthreads();
  }
  long long c = 0;
  for (int r = threadIdx.x; r < nblocks; r += DT) c += reinterpret_cast<const int32_t*>(a.partials + (long)r * DD3D_DDL_ROW)[DD3D_MAX_LEVELS];
  redc[threadIdx.x] = c;
  __syncthreads();
  for (int h = DT / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) redc[threadIdx.x] += redc[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const long long n = redc[0];
  a.count[0] = (int64_t)n;
  for (int l = 0; l < a.num_levels; ++l) {
#pragma clang fp contract(off)
    const float mean = S[l] / (float)n;  // no valid pixel: 0 / 0 = NaN, the mean of an empty selection
    const float weighted = a.loss_weight * mean;  // dense_depth_loss.py:36
    a.out[l] = weighted / a.divisor[l];           // dense_depth.py:169
  }
}

}  // namespace dd3d

extern "C" int dd3d_dense_depth_loss(const dd3d_dense_depth_loss_args* a, void* stream) {
  using namespace dd3d;
  const int ok = check_dense_depth_args(a, "dd3d_dense_depth_loss");
  if (ok != DD3D_OK) return ok;
  const long nquads = (long)a->B * a->Hp * (a->Wp / 4);
  const int grid = (int)((nquads + DT - 1) / DT < DDL_MAX_GRID ? (nquads + DT - 1) / DT : DDL_MAX_GRID);
  DD3D_REQUIRE(a->n_partials >= grid, "dd3d_dense_depth_loss: partials hold %d rows, the launch has %d blocks", a->n_partials, grid);
  DD3D_REQUIRE((nquads * 4 + grid - 1) / grid < (1L << 31), "dd3d_dense_depth_loss: canvas too large");
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dense_depth_loss_kernel, dim3((unsigned)grid), dim3(DT), 0, s, DenseDepthLossK{*a});
  const int e = check_launch("dense_depth_loss_kernel");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(dense_depth_finalize_kernel, dim3(1), dim3(DT), 0, s, DenseDepthLossK{*a}, grid);
  return check_launch("dense_depth_finalize_kernel");
}

extern "C" int dd3d_dense_depth_loss_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 32, "dd3d_dense_depth_loss_layout: need 32 slots");
#define OFF(f) (int64_t) offsetof(dd3d_dense_depth_loss_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_dense_depth_loss_args), OFF(raw), OFF(gt), OFF(inv_K), OFF(partials), OFF(out), OFF(count), OFF(h),
                       OFF(w), OFF(stride), OFF(divisor), OFF(num_levels), OFF(B), OFF(Hp), OFF(Wp), OFF(pitch), OFF(offset_half),
                       OFF(n_partials), OFF(focal_factor), OFF(min_depth), OFF(max_depth), OFF(beta), OFF(loss_weight)};
#undef OFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
