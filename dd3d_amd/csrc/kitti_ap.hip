// KITTI 3D / BEV AP statistics for gfx950: the two greedy matchings of tridet/evaluators/kitti_3d_evaluator.py
// (KITTIEvaluationEngine.eval_metric :413-513), which the reference runs as numba CPU code one image at a time.
//   kitti_tp_scores_kernel   compute_threshold_jit :749-810   (pass 1: the scores of the true positives, for get_thresholds)
//   kitti_pr_counts_kernel   compute_statistics_jit :910-1038 with compute_fp=True (pass 2: tp / fp / fn per score threshold)
// Only tp / fp / fn reach KITTIEvaluationEngine.evaluate (:386-403); the other `pr` columns (yaw, similarity, match degree,
// confidence and scale errors) are discarded there and are not computed.  The DontCare boxes do not change a count (nstuff = 0,
// :1020-1021).
//
// Work unit: one wave64 per (image, class x difficulty, overlap threshold[, score threshold]).  The loop over GT stays sequential,
// because a detection assigned to one GT is not a candidate for the next.  The loop over the image's detections is split across
// the lanes (detection 64k + lane belongs to lane `lane`, chunk k), and the reference's sequential choice becomes a wave-wide
// argmax.  The equivalence, for one GT, over the candidates C = {j unassigned, ign_dt[j] != -1, overlap[j] > min_overlap, and in
// pass 2 score[j] >= thresh}:
//   pass 1 (:777-785)  `score > valid_detection` with valid_detection starting at -FLT_MAX is a running strict maximum: the result
//                      is the candidate of largest score (among those > -FLT_MAX), lowest index on ties.  NaN scores compare false
//                      and are never picked.
//   pass 2 (:965-991)  with max_overlap starting at -FLT_MAX and assigned_ignored_det:
//                      - the first branch takes an ign_dt == 0 candidate when its overlap beats max_overlap, or when the current
//                        pick is an ign_dt == 1 one (assigned_ignored_det); max_overlap only moves in this branch, so over the
//                        ign_dt == 0 candidates it is a running strict maximum of the overlap (every candidate's overlap is
//                        > min_overlap >= -FLT_MAX, so the first one always passes);
//                      - the second branch takes an ign_dt == 1 candidate only while nothing is picked (valid_detection ==
//                        NO_DETECTION): the first such candidate, which any later ign_dt == 0 candidate replaces;
//                      so the pick is the ign_dt == 0 candidate of largest overlap, lowest index on ties, and when there is none the
//                      lowest-index ign_dt == 1 candidate.  Codes other than 0 / 1 / -1 are never picked in pass 2, as there.
//                      Both are keys (rank, overlap, -index) reduced with a butterfly, so every lane ends with the same pick.
//   tests/kitti_ap_oracle.py restates both state machines and tests/test_kitti_ap.py checks them against these rules.
// Numerics: overlaps are the float32 values of the overlap kernels, compared against min_overlap in float64 (the reference casts
// them to float64, :560); scores and thresholds are float64.  The score cut of :947-950 (`score < thresh` drops a detection) is
// applied as `!(score >= thresh)`: identical for every number, and a NaN score is dropped rather than matched or counted (the
// reference's fastmath build leaves NaN comparisons undefined).  No fast-math: plain IEEE comparisons, NaN overlaps never pass.
// The per-lane `assigned` flags are two 64-bit words in registers (bit k = chunk k), so a wave handles up to 8192 detections with
// no private array (no scratch).  Counts are integers: per-block LDS sums, then one 64-bit atomic per nonzero (threshold, field),
// so every run gives the same result.
#include <float.h>
#include <limits.h>
#include <math.h>

#include "common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {
namespace {

constexpr int KW = 64;          // wave
constexpr int KWAVES = 4;       // waves per block
constexpr int P2_IMGS = 8;      // pass 2: images per block (the block's waves take (image, threshold) tasks image by image)
constexpr double NO_DETECTION = -(double)FLT_MAX;  // np.finfo(np.float32).min, compared in float64 (:771, :955)

static_assert(DD3D_KITTI_MAX_DT_PER_IMAGE == 2 * 64 * KW, "two 64-bit flag words per lane");

struct MinOverlaps {  // min_overlap travels by value: the host validates it before the launch
  double v[DD3D_KITTI_MAX_OVERLAPS];
  __device__ __forceinline__ double at(int o) const {  // unrolled select: an indexed kernel-argument array would be copied to scratch
    double m = v[0];
#pragma unroll
    for (int i = 1; i < DD3D_KITTI_MAX_OVERLAPS; ++i) m = i == o ? v[i] : m;
    return m;
  }
};

// Per-lane detection flags: bit k <-> detection 64k + lane.  Selected by comparison, never indexed (an indexed array goes to scratch).
struct LaneBits {
  uint64_t lo = 0, hi = 0;
  __device__ __forceinline__ bool get(int k) const { return ((k < 64 ? lo : hi) >> (k & 63)) & 1ull; }
  __device__ __forceinline__ void set(int k) {
    if (k < 64) lo |= 1ull << k;
    else hi |= 1ull << (k & 63);
  }
};

struct Image {  // one image's slice of the inputs for one class x difficulty
  const float* ov;
  const int8_t* igd;
  const int8_t* igg;
  const double* sc;
  int nd, ng, nk, d0, g0;
};

// False when image `img`'s offsets break the bounds the host declared: the task is skipped instead of reading out of range.
__device__ __forceinline__ bool load_image(const dd3d_kitti_match_args& a, int img, int cd, Image& im) {
  const int d0 = a.dt_begin[img], d1 = a.dt_begin[img + 1], g0 = a.gt_begin[img], g1 = a.gt_begin[img + 1];
  const long nd = (long)d1 - d0, ng = (long)g1 - g0;
  if (d0 < 0 || g0 < 0 || nd < 0 || ng < 0 || nd > a.max_dt || ng > a.max_gt || d1 > a.n_dt || g1 > a.n_gt) return false;
  const int64_t off = a.ov_off[img];
  if (nd * ng > 0 && (off < 0 || off > a.n_ov - nd * ng)) return false;
  im.ov = a.ov + (nd * ng > 0 ? off : 0);
  im.igd = a.ign_dt + (long)cd * a.n_dt + d0;
  im.igg = a.ign_gt + (long)cd * a.n_gt + g0;
  im.sc = a.dt_score + d0;
  im.nd = (int)nd, im.ng = (int)ng, im.nk = (int)((nd + KW - 1) / KW), im.d0 = d0, im.g0 = g0;
  return true;
}

// Pass 1 key: larger score, then lower index.  Sentinel (NO_DETECTION, INT_MAX) loses to every candidate (score > NO_DETECTION).
__device__ __forceinline__ void wave_max_score(double& s, int& j) {
#pragma unroll
  for (int m = KW / 2; m > 0; m >>= 1) {
    const double os = __shfl_xor(s, m, KW);
    const int oj = __shfl_xor(j, m, KW);
    if (os > s || (os == s && oj < j)) s = os, j = oj;
  }
}

// Pass 2 key: rank (2 = ign_dt 0, 1 = ign_dt 1, 0 = none), then larger overlap (rank 2 only; 0 otherwise), then lower index.
__device__ __forceinline__ void wave_max_overlap(int& r, float& v, int& j) {
#pragma unroll
  for (int m = KW / 2; m > 0; m >>= 1) {
    const int orr = __shfl_xor(r, m, KW);
    const float ov = __shfl_xor(v, m, KW);
    const int oj = __shfl_xor(j, m, KW);
    if (orr > r || (orr == r && (ov > v || (ov == v && oj < j)))) r = orr, v = ov, j = oj;
  }
}

__global__ __launch_bounds__(KW* KWAVES) void kitti_tp_scores_kernel(dd3d_kitti_match_args a, MinOverlaps mo, double* __restrict__ tp_score) {
  const int lane = threadIdx.x & (KW - 1);
  const int img = blockIdx.x * KWAVES + (threadIdx.x / KW);
  const int cdo = blockIdx.y, cd = cdo / a.n_o;
  if (img >= a.n_img) return;
  Image im;
  if (!load_image(a, img, cd, im)) return;
  const double min_ov = mo.at(cdo - cd * a.n_o);
  double* out = tp_score + (long)cdo * a.n_gt + im.g0;
  LaneBits taken;  // ign_dt == -1, or assigned to an earlier GT
  for (int k = 0; k < im.nk; ++k) {
    const int j = k * KW + lane;
    if (j >= im.nd || im.igd[j] == -1) taken.set(k);
  }
  for (int g = 0; g < im.ng; ++g) {
    const int ig = im.igg[g];
    double rec = -INFINITY;
    if (ig != -1) {
      double best = NO_DETECTION;
      int bj = INT_MAX;
      for (int k = 0; k < im.nk; ++k) {
        if (taken.get(k)) continue;
        const int j = k * KW + lane;
        const double v = (double)im.ov[(long)j * im.ng + g];
        const double s = im.sc[j];
        if (v > min_ov && s > best) best = s, bj = j;  // j grows with k: strict > keeps the lowest index
      }
      wave_max_score(best, bj);
      if (bj != INT_MAX) {
        if (lane == (bj & (KW - 1))) taken.set(bj / KW);
        if (!(ig == 1 || im.igd[bj] == 1)) rec = best;  // :799-808: a true positive records its score
      }
    }
    if (lane == 0) out[g] = rec;
  }
}

// (tp, fp, fn) of one image at one score threshold.  Uniform across the wave.
struct Counts {
  int tp, fp, fn;
};

__device__ __forceinline__ Counts pr_counts_one(const Image& im, double min_ov, double th, int lane) {
  LaneBits taken;  // ign_dt == -1, score below the threshold, or assigned to an earlier GT
  for (int k = 0; k < im.nk; ++k) {
    const int j = k * KW + lane;
    if (j >= im.nd || im.igd[j] == -1 || !(im.sc[j] >= th)) taken.set(k);
  }
  int tp = 0, fn = 0;
  for (int g = 0; g < im.ng; ++g) {
    const int ig = im.igg[g];
    if (ig == -1) continue;
    int r = 0, bj = INT_MAX;
    float bv = 0.f;
    for (int k = 0; k < im.nk; ++k) {
      if (taken.get(k)) continue;
      const int j = k * KW + lane;
      const float v = im.ov[(long)j * im.ng + g];
      if (!((double)v > min_ov)) continue;
      const int c = im.igd[j];
      if (c == 0) {
        if (r < 2 || v > bv) r = 2, bv = v, bj = j;
      } else if (c == 1 && r == 0) {
        r = 1, bj = j;
      }
    }
    wave_max_overlap(r, bv, bj);
    if (r == 0) {
      fn += ig == 0;  // :994-995
    } else {
      if (lane == (bj & (KW - 1))) taken.set(bj / KW);
      tp += !(ig == 1 || im.igd[bj] == 1);  // :998-1016
    }
  }
  int fp = 0;  // :1017-1020: neither assigned, ign_dt -1 / 1, nor below the threshold
  for (int k = 0; k < im.nk; ++k) {
    const int j = k * KW + lane;
    fp += __popcll(__ballot(j < im.nd && !taken.get(k) && im.igd[j] != 1));
  }
  return Counts{tp, fp, fn};
}

__global__ __launch_bounds__(KW* KWAVES) void kitti_pr_counts_kernel(dd3d_kitti_match_args a, MinOverlaps mo, const double* __restrict__ thresh,
                                                                     const int32_t* __restrict__ n_thresh, int t_max,
                                                                     unsigned long long* __restrict__ tp_fp_fn) {
  __shared__ int cnt[DD3D_KITTI_MAX_THRESHOLDS * 3];
  const int lane = threadIdx.x & (KW - 1), wave = threadIdx.x / KW;
  const int cdo = blockIdx.y, cd = cdo / a.n_o;
  const double min_ov = mo.at(cdo - cd * a.n_o);
  const int nt = max(0, min(n_thresh[cdo], t_max));
  const double* th = thresh + (long)cdo * t_max;
  for (int i = threadIdx.x; i < nt * 3; i += blockDim.x) cnt[i] = 0;
  __syncthreads();
  const int img0 = blockIdx.x * P2_IMGS, nimg = min(P2_IMGS, a.n_img - img0);
  Image im;
  bool ok = false;
  int cur = -1;
  for (int task = wave; task < nimg * nt; task += KWAVES) {
    const int img = img0 + task / nt, t = task - (task / nt) * nt;
    if (img != cur) cur = img, ok = load_image(a, img, cd, im);
    if (!ok) continue;
    const Counts c = pr_counts_one(im, min_ov, th[t], lane);
    if (lane == 0) {
      if (c.tp) atomicAdd(&cnt[t * 3 + 0], c.tp);
      if (c.fp) atomicAdd(&cnt[t * 3 + 1], c.fp);
      if (c.fn) atomicAdd(&cnt[t * 3 + 2], c.fn);
    }
  }
  __syncthreads();
  unsigned long long* out = tp_fp_fn + (long)cdo * t_max * 3;
  for (int i = threadIdx.x; i < nt * 3; i += blockDim.x)
    if (cnt[i]) atomicAdd(&out[i], (unsigned long long)cnt[i]);
}

int check_args(const dd3d_kitti_match_args* a, const char* who, MinOverlaps* mo, bool* empty) {
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->n_img >= 0 && a->n_dt >= 0 && a->n_gt >= 0 && a->n_cd >= 0 && a->n_o >= 0 && a->n_ov >= 0 && a->max_dt >= 0 && a->max_gt >= 0,
               "%s: negative size", who);
  DD3D_REQUIRE(a->max_dt <= DD3D_KITTI_MAX_DT_PER_IMAGE, "%s: %d detections in one image, more than the %d this kernel takes", who, a->max_dt,
               DD3D_KITTI_MAX_DT_PER_IMAGE);
  DD3D_REQUIRE(a->max_gt <= DD3D_KITTI_MAX_GT_PER_IMAGE, "%s: %d ground-truth boxes in one image, more than the %d this kernel takes", who,
               a->max_gt, DD3D_KITTI_MAX_GT_PER_IMAGE);
  DD3D_REQUIRE(a->n_o <= DD3D_KITTI_MAX_OVERLAPS, "%s: %d overlap thresholds, more than %d", who, a->n_o, DD3D_KITTI_MAX_OVERLAPS);
  DD3D_REQUIRE((long)a->n_cd * a->n_o <= 65535, "%s: n_cd * n_o = %ld exceeds 65535", who, (long)a->n_cd * a->n_o);
  *empty = a->n_img == 0 || a->n_cd == 0 || a->n_o == 0;
  if (*empty) return DD3D_OK;
  DD3D_REQUIRE(a->min_overlap != nullptr && a->dt_begin != nullptr && a->gt_begin != nullptr && a->ov_off != nullptr, "%s: null pointer", who);
  DD3D_REQUIRE(a->n_dt == 0 || (a->dt_score != nullptr && a->ign_dt != nullptr), "%s: null detection array", who);
  DD3D_REQUIRE(a->n_gt == 0 || a->ign_gt != nullptr, "%s: null ign_gt", who);
  DD3D_REQUIRE(a->n_ov == 0 || a->ov != nullptr, "%s: null ov", who);
  for (int o = 0; o < a->n_o; ++o) {
    const double m = a->min_overlap[o];
    DD3D_REQUIRE(!(m < NO_DETECTION), "%s: min_overlap[%d] = %g is below -FLT_MAX", who, o, m);
    mo->v[o] = m;
  }
  return DD3D_OK;
}

}  // namespace
}  // namespace dd3d

extern "C" int dd3d_kitti_tp_scores(const dd3d_kitti_match_args* args, double* tp_score, void* stream) {
  using namespace dd3d;
  MinOverlaps mo{};
  bool empty = false;
  const int rc = check_args(args, "dd3d_kitti_tp_scores", &mo, &empty);
  if (rc != DD3D_OK || empty || args->n_gt == 0) return rc;  // no GT: nothing to write
  DD3D_REQUIRE(tp_score != nullptr, "dd3d_kitti_tp_scores: null tp_score");
  hipLaunchKernelGGL(kitti_tp_scores_kernel, dim3((unsigned)ceil_div(args->n_img, KWAVES), (unsigned)(args->n_cd * args->n_o)), dim3(KW * KWAVES), 0,
                     reinterpret_cast<hipStream_t>(stream), *args, mo, tp_score);
  return check_launch("kitti_tp_scores_kernel");
}

extern "C" int dd3d_kitti_pr_counts(const dd3d_kitti_match_args* args, const double* thresh, const int32_t* n_thresh, int32_t t_max, int64_t* tp_fp_fn,
                                    void* stream) {
  using namespace dd3d;
  MinOverlaps mo{};
  bool empty = false;
  const int rc = check_args(args, "dd3d_kitti_pr_counts", &mo, &empty);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(t_max >= 0 && t_max <= DD3D_KITTI_MAX_THRESHOLDS, "dd3d_kitti_pr_counts: t_max = %d outside [0, %d]", t_max, DD3D_KITTI_MAX_THRESHOLDS);
  if (empty || t_max == 0) return DD3D_OK;
  DD3D_REQUIRE(thresh != nullptr && n_thresh != nullptr && tp_fp_fn != nullptr, "dd3d_kitti_pr_counts: null thresh / n_thresh / tp_fp_fn");
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const hipError_t e = hipMemsetAsync(tp_fp_fn, 0, sizeof(int64_t) * 3 * (size_t)t_max * args->n_cd * args->n_o, s);
  if (e != hipSuccess) {
    set_error("dd3d_kitti_pr_counts: clearing tp_fp_fn: %s", hipGetErrorString(e));
    return DD3D_E_LAUNCH;
  }
  hipLaunchKernelGGL(kitti_pr_counts_kernel, dim3((unsigned)ceil_div(args->n_img, P2_IMGS), (unsigned)(args->n_cd * args->n_o)), dim3(KW * KWAVES), 0, s,
                     *args, mo, thresh, n_thresh, t_max, reinterpret_cast<unsigned long long*>(tp_fp_fn));
  return check_launch("kitti_pr_counts_kernel");
}
