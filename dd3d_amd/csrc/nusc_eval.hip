// nuScenes detection matching for gfx950: the greedy centre-distance matching of the nuScenes devkit's `accumulate`
// (nuscenes/eval/detection/algo.py, detection_cvpr_2019), for every (sample, class) segment and every distance threshold in one launch.
// The reference runs it through the devkit (tridet/evaluators/nuscenes_evaluator.py:249-312): a Python loop over every prediction of
// a class in descending score order and, for each, over every GT box of its sample.  The host (dd3d_amd/evaluators/nuscenes_eval.py)
// sorts the predictions of each class in the devkit's order and cuts them into (sample, class) segments; the matching state (the
// `taken` set) is per sample, so the segments are independent and the global order restricted to one segment is all it needs.
//
// Work unit: one wave64 per (segment, threshold).  GT row 64k + lane of the segment belongs to lane `lane` (chunk k); its `taken`
// flag is bit k of one 64-bit register word per lane, selected by shift and never indexed (no private array, no scratch), which caps
// a segment at 64 x 64 = 4096 GT.  The predictions are processed one after another.  For each, every lane scans its untaken GT in
// ascending index order and keeps the strictly smaller distance; a butterfly then reduces the lexicographic minimum of
// (distance, GT index) across the wave.  The prediction matches iff that distance < threshold, and the lane owning the GT marks it
// taken.  Why this equals the devkit's sequential loop, `for gt_idx, gt in enumerate(gts): if not taken and d < min_dist:
// min_dist, match = d, gt_idx` with min_dist starting at +inf, then `is_match = min_dist < dist_th`:
//   - the strict `<` scan in index order keeps the FIRST index among equal minima: the lowest one.  Each lane's scan visits its
//     GT in ascending order with the same strict `<`, and the butterfly breaks distance ties by the lower index, so the wave ends
//     with the lowest-index GT of the minimum distance over all untaken GT: the same pick;
//   - a NaN distance is never `<` anything, so it is never picked, there or here; +inf is not `< +inf`, so it is never picked
//     either (both start from +inf), and the sentinel (+inf, INT_MAX) loses every comparison against a real candidate;
//   - the match test is the same strict `<` on the same float64 value.
// tests/nuscenes_eval_oracle.py restates the sequential loop and tests/test_nuscenes_eval.py checks it against this rule.
// Numerics: float64 throughout, contraction off (no FMA), no fast-math.  The distance is sqrt(dx * dx + dy * dy) with
// dx = pred.x - gt.x, dy = pred.y - gt.y.  hipcc (the AMDGPU backend's llvm.sqrt.f64 expansion) emits no v_sqrt_f64 on gfx950 (that
// instruction is not correctly rounded): the operand is scaled by v_ldexp_f64 when tiny, a v_rsq_f64 estimate is refined by v_fma_f64
// Newton steps with a final residual correction, scaled back, and zero / inf pass through a v_cmp_class_f64 select.  That is the
// correctly rounded square root of IEEE 754 (numpy's and Python's math.sqrt); the GPU tests check the decisions bit-for-bit against
// them, at distances one float64 step either side of each threshold included.
#include <limits.h>
#include <math.h>

#include "common.h"

DD3D_NOTE_BUILD_FLAGS

#pragma clang fp contract(off)

namespace dd3d {
namespace {

constexpr int NW = 64;      // wave
constexpr int NWAVES = 4;   // waves per block, one (segment, threshold) each

static_assert(DD3D_NUSC_MAX_GT_PER_SEGMENT == 64 * NW, "one 64-bit taken word per lane");

struct Thresholds {  // the distance thresholds travel by value
  double v[DD3D_NUSC_MAX_THRESHOLDS];
  __device__ __forceinline__ double at(int t) const {  // unrolled select: an indexed kernel-argument array would be copied to scratch
    double m = v[0];
#pragma unroll
    for (int i = 1; i < DD3D_NUSC_MAX_THRESHOLDS; ++i) m = i == t ? v[i] : m;
    return m;
  }
};

// Lexicographic minimum of (distance, GT index) over the wave; every lane ends with the same pair.
__device__ __forceinline__ void wave_min_dist(double& d, int& j) {
#pragma unroll
  for (int m = NW / 2; m > 0; m >>= 1) {
    const double od = __shfl_xor(d, m, NW);
    const int oj = __shfl_xor(j, m, NW);
    if (od < d || (od == d && oj < j)) d = od, j = oj;
  }
}

__device__ __forceinline__ double center_dist(double px, double py, double gx, double gy) {
  const double dx = px - gx, dy = py - gy;
  return sqrt(dx * dx + dy * dy);
}

__global__ __launch_bounds__(NW* NWAVES) void nusc_center_match_kernel(const double* __restrict__ pred_xy, const double* __restrict__ gt_xy,
                                                                       const int32_t* __restrict__ pred_begin, const int32_t* __restrict__ gt_begin,
                                                                       int32_t n_seg, int32_t n_pred, int32_t n_gt, Thresholds th,
                                                                       int32_t* __restrict__ match) {
  const int lane = threadIdx.x & (NW - 1);
  const int seg = blockIdx.x * NWAVES + (threadIdx.x / NW);
  const int t = blockIdx.y;
  if (seg >= n_seg) return;
  const int p0 = pred_begin[seg], p1 = pred_begin[seg + 1], g0 = gt_begin[seg], g1 = gt_begin[seg + 1];
  // the host validated its copy of the offsets; a device copy that disagrees skips the segment rather than leave the bounds
  if (p0 < 0 || g0 < 0 || p1 < p0 || g1 < g0 || p1 > n_pred || g1 > n_gt || p1 - p0 > DD3D_NUSC_MAX_PRED_PER_SEGMENT ||
      g1 - g0 > DD3D_NUSC_MAX_GT_PER_SEGMENT)
    return;
  const int ng = g1 - g0, nk = (ng + NW - 1) / NW;
  const double thr = th.at(t);
  int32_t* out = match + (long)t * n_pred;
  // chunk 0 (the whole segment in all but crowded scenes) stays in registers; later chunks are read from L1 / L2 per prediction
  const bool has0 = lane < ng;
  const double gx0 = has0 ? gt_xy[2L * (g0 + lane)] : 0.0, gy0 = has0 ? gt_xy[2L * (g0 + lane) + 1] : 0.0;
  uint64_t taken = 0;  // bit k <-> GT 64k + lane of the segment
  for (int p = p0; p < p1; ++p) {
    const double px = pred_xy[2L * p], py = pred_xy[2L * p + 1];
    double best = INFINITY;
    int bj = INT_MAX;
    if (has0 && !(taken & 1ull)) {
      const double d = center_dist(px, py, gx0, gy0);
      if (d < best) best = d, bj = lane;
    }
    for (int k = 1; k < nk; ++k) {
      const int j = k * NW + lane;
      if (j >= ng || ((taken >> k) & 1ull)) continue;
      const double d = center_dist(px, py, gt_xy[2L * (g0 + j)], gt_xy[2L * (g0 + j) + 1]);
      if (d < best) best = d, bj = j;  // j grows with k: strict < keeps the lowest index
    }
    wave_min_dist(best, bj);
    const bool hit = best < thr;  // false for the sentinel (+inf) and for a NaN threshold
    if (hit && lane == (bj & (NW - 1))) taken |= 1ull << (bj / NW);
    if (lane == 0) out[p] = hit ? g0 + bj : -1;
  }
}

}  // namespace
}  // namespace dd3d

extern "C" int dd3d_nusc_center_match(const dd3d_nusc_match_args* a, int32_t* match, void* stream) {
  using namespace dd3d;
  const char* who = "dd3d_nusc_center_match";
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->n_seg >= 0 && a->n_pred >= 0 && a->n_gt >= 0, "%s: negative size", who);
  DD3D_REQUIRE(a->n_thr >= 1 && a->n_thr <= DD3D_NUSC_MAX_THRESHOLDS, "%s: n_thr = %d outside [1, %d]", who, a->n_thr, DD3D_NUSC_MAX_THRESHOLDS);
  DD3D_REQUIRE(a->n_seg <= 65535 * NWAVES, "%s: %d segments, more than %d", who, a->n_seg, 65535 * NWAVES);
  if (a->n_seg == 0 || a->n_pred == 0) return DD3D_OK;
  DD3D_REQUIRE(a->pred_begin_host != nullptr && a->gt_begin_host != nullptr, "%s: null host offsets", who);
  DD3D_REQUIRE(a->pred_xy != nullptr && a->pred_begin != nullptr && a->gt_begin != nullptr && match != nullptr, "%s: null pointer", who);
  DD3D_REQUIRE(a->n_gt == 0 || a->gt_xy != nullptr, "%s: null gt_xy", who);
  const int32_t* pb = a->pred_begin_host;
  const int32_t* gb = a->gt_begin_host;
  DD3D_REQUIRE(pb[0] >= 0 && gb[0] >= 0, "%s: negative first offset", who);
  DD3D_REQUIRE(pb[a->n_seg] <= a->n_pred && gb[a->n_seg] <= a->n_gt, "%s: offsets end at %d / %d, past n_pred = %d / n_gt = %d", who, pb[a->n_seg],
               gb[a->n_seg], a->n_pred, a->n_gt);
  for (int s = 0; s < a->n_seg; ++s) {
    DD3D_REQUIRE(pb[s + 1] >= pb[s] && gb[s + 1] >= gb[s], "%s: offsets decrease at segment %d", who, s);
    DD3D_REQUIRE(pb[s + 1] - pb[s] <= DD3D_NUSC_MAX_PRED_PER_SEGMENT, "%s: segment %d has %d predictions, more than %d", who, s, pb[s + 1] - pb[s],
                 DD3D_NUSC_MAX_PRED_PER_SEGMENT);
    DD3D_REQUIRE(gb[s + 1] - gb[s] <= DD3D_NUSC_MAX_GT_PER_SEGMENT, "%s: segment %d has %d ground-truth boxes, more than %d", who, s, gb[s + 1] - gb[s],
                 DD3D_NUSC_MAX_GT_PER_SEGMENT);
  }
  Thresholds th{};
  for (int t = 0; t < a->n_thr; ++t) th.v[t] = a->thr[t];
  hipLaunchKernelGGL(nusc_center_match_kernel, dim3((unsigned)ceil_div(a->n_seg, NWAVES), (unsigned)a->n_thr), dim3(NW * NWAVES), 0,
                     reinterpret_cast<hipStream_t>(stream), a->pred_xy, a->gt_xy, a->pred_begin, a->gt_begin, a->n_seg, a->n_pred, a->n_gt, th, match);
  return check_launch("nusc_center_match_kernel");
}
