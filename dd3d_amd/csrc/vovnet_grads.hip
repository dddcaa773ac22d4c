// Backward of the VoVNet-V2 backbone's eSE gate and 3x3 stride-2 ceil-mode max-pool (vovnet.py:164-185, 241-249; BackboneLowering._vovnet)
// for gfx950.  include/dd3d_hip.h states the mathematics.  The backbone's convolutions (3x3 up to Cin 1024, the concat 1x1 up to
// 2144 -> 1024) run on the backbone kernels through dd3d_vovnet_conv_wgrad / dd3d_vovnet_conv_dgrad (backbone_grads.hip).
//
// eSE gate backward -- out = xt * s (+ identity), s = hsigmoid(fc_w . mean_hw(xt) + fc_b):
//   ese_bwd_partial_kernel  block = (32 channels, row split, image), eight row lanes: sum xt and sum g * xt over the split's rows, the
//                           lanes added in lane order -> part[b][rs][2][C].  xt is decoded from the plan's storage.
//   ese_bwd_gate_kernel     block = (four channels co, image), a wave per co: the splits in split order -> mean; z in the forward gate's
//                           order (lanes of every 64th ci, then a butterfly); s, ds, dz.
//   ese_bwd_fc_kernel       thread = (co, ci): d fc_w over the images; thread = (b, c): u = fc_w^T dz / HW in chunks of 32 co; thread = co:
//                           d fc_b.
//   ese_bwd_apply_kernel    thread = (pixel, four channels): g_xt = g * s + u.
// The module input's third term: vovnet_add_kernel, thread = (pixel, four channels): out = a + b.
// Max-pool backward as a gather:
//   pool3_backward_kernel   thread = (input pixel, channel): the at most 2 x 2 windows that contain the pixel in ascending (oy, ox); each
//                           window's arg-max recomputed from the stored input, the first maximum in row-major order wins.
// No float atomics: every sum has one writer and a fixed order, two runs agree bit for bit.
#include "act_load.h"
#include "common.h"

DD3D_NOTE_BUILD_FLAGS

namespace dd3d {

typedef float vg_f32x4 __attribute__((ext_vector_type(4)));

constexpr int VG_T = 256;     // threads of every block here
constexpr int VG_LANES = 8;   // row lanes of the pooling pass

struct EseGK {
  dd3d_ese_grad_args a;
  float x_inv, inv_hw;
};

__global__ __launch_bounds__(VG_T) void ese_bwd_partial_kernel(const EseGK K) {
  const dd3d_ese_grad_args& a = K.a;
  __shared__ float red[2][VG_LANES][32];
  const int rs = blockIdx.y, b = blockIdx.z;
  const int rl = threadIdx.x >> 5, cl = threadIdx.x & 31;
  const int c = blockIdx.x * 32 + cl;  // (C is a multiple of 32)
  const int rows_per = ceil_div(a.HW, a.rsplit);
  const int r0 = rs * rows_per, r1 = min(a.HW, r0 + rows_per);
  const long npix = (long)a.B * a.HW;
  float sx = 0.f, sgx = 0.f;
  for (int r = r0 + rl; r < r1; r += VG_LANES) {
    const long pix = (long)b * a.HW + r;
    const float x = load_act_any(a.xt_mode, a.xt, npix, pix, c, a.xt_pitch, K.x_inv);
    sx += x;
    sgx = fmaf(a.g[pix * a.g_pitch + c], x, sgx);
  }
  red[0][rl][cl] = sx, red[1][rl][cl] = sgx;
  __syncthreads();
  if (rl < 2) {  // row lane 0 adds the sums of xt, row lane 1 those of g * xt, both in lane order
    float s = red[rl][0][cl];
#pragma unroll
    for (int k = 1; k < VG_LANES; ++k) s += red[rl][k][cl];
    a.part[(((long)b * a.rsplit + rs) * 2 + rl) * a.C + c] = s;
  }
}

__global__ __launch_bounds__(VG_T) void ese_bwd_gate_kernel(const EseGK K) {
  const dd3d_ese_grad_args& a = K.a;
  const int b = blockIdx.y, co = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;  // (C is a multiple of 4: co < C)
  const int C = a.C, RS = a.rsplit;
  const float* P = a.part + (long)b * RS * 2 * C;
  float acc = 0.f;
  for (int ci = lane; ci < C; ci += 64) {
    float m = 0.f;
    for (int r = 0; r < RS; ++r) m += P[(long)r * 2 * C + ci];
    m *= K.inv_hw;
    if (blockIdx.x == 0 && threadIdx.x < 64) a.m[(long)b * C + ci] = m;  // (every wave holds the same means: one of them stores)
    acc += a.fc_w[(long)co * C + ci] * m;
  }
  for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d, 64);
  if (lane == 0) {
    const float z = acc + a.fc_b[co];
    float ds = 0.f;
    for (int r = 0; r < RS; ++r) ds += P[((long)r * 2 + 1) * C + co];
    const long o = (long)b * C + co;
    a.z[o] = z;
    a.s[o] = fminf(fmaxf(z + 3.0f, 0.f), 6.0f) / 6.0f;
    a.dz[o] = (z > -3.0f && z < 3.0f) ? ds / 6.0f : 0.f;
  }
}

__global__ __launch_bounds__(VG_T) void ese_bwd_fc_kernel(const EseGK K) {
  const dd3d_ese_grad_args& a = K.a;
  const int C = a.C, B = a.B;
  long i = (long)blockIdx.x * VG_T + threadIdx.x;
  if (i < (long)C * C) {  // d fc_w[co][ci]: the images in image order
    const int co = (int)(i / C), ci = (int)(i - (long)co * C);
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc = fmaf(a.dz[(long)b * C + co], a.m[(long)b * C + ci], acc);
    a.d_fc_w[i] = acc;
    return;
  }
  i -= (long)C * C;
  if (i < (long)B * C) {  // u[b][c]: a fresh sum per chunk of 32 co, the chunks in chunk order
    const int b = (int)(i / C), c = (int)(i - (long)b * C);
    float total = 0.f;
    for (int c0 = 0; c0 < C; c0 += 32) {
      float p = 0.f;
#pragma unroll 8
      for (int co = c0; co < c0 + 32; ++co) p = fmaf(a.fc_w[(long)co * C + c], a.dz[(long)b * C + co], p);
      total += p;
    }
    a.u[i] = total * K.inv_hw;
    return;
  }
  i -= (long)B * C;
  if (i < C) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) acc += a.dz[(long)b * C + i];
    a.d_fc_b[i] = acc;
  }
}

__global__ __launch_bounds__(VG_T) void ese_bwd_apply_kernel(const EseGK K) {
  const dd3d_ese_grad_args& a = K.a;
  const int C4 = a.C / 4;
  const long total = (long)a.B * a.HW * C4;
  const long i = (long)blockIdx.x * VG_T + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C4) * 4;
  const long pix = i / C4;
  const int b = (int)(pix / a.HW);
  const vg_f32x4 g = *reinterpret_cast<const vg_f32x4*>(a.g + pix * a.g_pitch + c);
  const vg_f32x4 s = *reinterpret_cast<const vg_f32x4*>(a.s + (long)b * a.C + c);
  const vg_f32x4 u = *reinterpret_cast<const vg_f32x4*>(a.u + (long)b * a.C + c);
  vg_f32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = fmaf(g[e], s[e], u[e]);
  *reinterpret_cast<vg_f32x4*>(a.g_xt + pix * a.gxt_pitch + c) = o;
}

__global__ __launch_bounds__(VG_T) void vovnet_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, long npix,
                                                          int C4, int a_pitch, int b_pitch, int out_pitch) {
  const long i = (long)blockIdx.x * VG_T + threadIdx.x;
  if (i >= npix * C4) return;
  const int c = (int)(i % C4) * 4;
  const long pix = i / C4;
  *reinterpret_cast<vg_f32x4*>(out + pix * out_pitch + c) =
      *reinterpret_cast<const vg_f32x4*>(a + pix * a_pitch + c) + *reinterpret_cast<const vg_f32x4*>(b + pix * b_pitch + c);
}

// --------------------------------------------------------------------------------------------------------------- max-pool backward
struct Pool3K {
  dd3d_pool3_grad_args a;
  int32_t Ho, Wo;
  float x_inv;
};

inline int pool3_out(int n) {  // dd3d_maxpool3x3s2_ceil_nhwc's rule: ceil((n - 3) / 2) + 1, the last window must start inside the map
  int o = (n - 3 + 1) / 2 + 1;
  if ((o - 1) * 2 >= n) --o;
  return o;
}

__global__ __launch_bounds__(VG_T) void pool3_backward_kernel(const Pool3K K) {
  const dd3d_pool3_grad_args& a = K.a;
  const int H = a.H, W = a.W, Ho = K.Ho, Wo = K.Wo;
  const long total = (long)a.B * H * W * a.C;
  const long i = (long)blockIdx.x * VG_T + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % a.C);
  const long pix = i / a.C;
  const int x = (int)(pix % W);
  const long t = pix / W;
  const int y = (int)(t % H), b = (int)(t / H);
  const long npix = (long)a.B * H * W, img = (long)b * H;
  // the windows that contain (y, x): oy in ceil((y - 2) / 2) .. floor(y / 2), inside 0 .. Ho - 1
  const int oy0 = y >= 2 ? (y - 1) >> 1 : 0, oy1 = min(Ho - 1, y >> 1);
  const int ox0 = x >= 2 ? (x - 1) >> 1 : 0, ox1 = min(Wo - 1, x >> 1);
  float v = a.add ? a.add[pix * a.add_pitch + c] : 0.f;
  for (int oy = oy0; oy <= oy1; ++oy)
    for (int ox = ox0; ox <= ox1; ++ox) {
      int by = 2 * oy, bx = 2 * ox;  // the first maximum in row-major order: a later entry wins only when it is larger
      float best = load_act_any(a.x_mode, a.x, npix, (img + by) * W + bx, c, a.x_pitch, K.x_inv);
      for (int dy = 0; dy < 3; ++dy) {
        const int yy = 2 * oy + dy;
        if (yy >= H) break;
        for (int dx = 0; dx < 3; ++dx) {
          const int xx = 2 * ox + dx;
          if (xx >= W) break;
          const float w = load_act_any(a.x_mode, a.x, npix, (img + yy) * W + xx, c, a.x_pitch, K.x_inv);
          if (w > best) best = w, by = yy, bx = xx;
        }
      }
      if (by == y && bx == x) v += a.g[(((long)b * Ho + oy) * Wo + ox) * a.g_pitch + c];
    }
  a.da[pix * a.da_pitch + c] = v;
}

static int check_storage(const char* who, const char* nm, int mode, int pitch, int chans, float scale) {
  DD3D_REQUIRE(mode == DD3D_PG_ACT_F32 || mode == DD3D_PG_ACT_F16X2 || mode == DD3D_PG_ACT_BF16X3, "%s: %s_mode = %d", who, nm, mode);
  if (mode == DD3D_PG_ACT_F32) DD3D_REQUIRE(pitch % 4 == 0 && pitch >= chans, "%s: %s_pitch = %d must be a multiple of 4 and hold %d channels", who, nm, pitch, chans);
  if (mode == DD3D_PG_ACT_F16X2) DD3D_REQUIRE(scale > 0.f, "%s: %s_plane_scale = %g", who, nm, (double)scale);
  return DD3D_OK;
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace dd3d

extern "C" int dd3d_ese_backward(const dd3d_ese_grad_args* a, void* stream) {
  using namespace dd3d;
  const char* who = "dd3d_ese_backward";
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->B >= 1 && a->B <= 65535 && a->HW >= 1, "%s: B = %d, HW = %d", who, a->B, a->HW);
  DD3D_REQUIRE(a->C >= 32 && a->C % 32 == 0 && a->C <= DD3D_VG_MAX_COUT, "%s: C = %d is not a multiple of 32 up to %d", who, a->C, DD3D_VG_MAX_COUT);
  DD3D_REQUIRE(a->rsplit >= 1 && a->rsplit <= DD3D_EG_MAX_RSPLIT, "%s: rsplit = %d (1 .. %d)", who, a->rsplit, DD3D_EG_MAX_RSPLIT);
  DD3D_REQUIRE((long)a->B * a->HW <= DD3D_BG_MAX_PIXELS, "%s: %ld pixels (at most %ld)", who, (long)a->B * a->HW, (long)DD3D_BG_MAX_PIXELS);
  DD3D_REQUIRE(a->xt && a->g && a->fc_w && a->fc_b, "%s: no input / gradient / fc", who);
  DD3D_REQUIRE(a->part && a->m && a->z && a->s && a->dz && a->u && a->g_xt && a->d_fc_w && a->d_fc_b, "%s: null output", who);
  const int rc = check_storage(who, "xt", a->xt_mode, a->xt_pitch, a->C, a->xt_plane_scale);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(a->g_pitch % 4 == 0 && a->g_pitch >= a->C, "%s: g_pitch = %d must be a multiple of 4 and hold %d channels", who, a->g_pitch, a->C);
  DD3D_REQUIRE(a->gxt_pitch % 4 == 0 && a->gxt_pitch >= a->C, "%s: gxt_pitch = %d must be a multiple of 4 and hold %d channels", who, a->gxt_pitch, a->C);
  DD3D_REQUIRE(aligned16(a->g) && aligned16(a->g_xt) && aligned16(a->s) && aligned16(a->u), "%s: g, g_xt, s and u must be 16-byte aligned", who);
  EseGK k;
  k.a = *a;
  k.x_inv = 1.f / a->xt_plane_scale, k.inv_hw = 1.0f / (float)a->HW;
  const hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ese_bwd_partial_kernel, dim3((unsigned)(a->C / 32), (unsigned)a->rsplit, (unsigned)a->B), dim3(VG_T), 0, st, k);
  int e = check_launch("ese_bwd_partial_kernel");
  if (e != DD3D_OK) return e;
  hipLaunchKernelGGL(ese_bwd_gate_kernel, dim3((unsigned)(a->C / 4), (unsigned)a->B), dim3(VG_T), 0, st, k);
  if ((e = check_launch("ese_bwd_gate_kernel")) != DD3D_OK) return e;
  const long fc = (long)a->C * a->C + (long)a->B * a->C + a->C;
  hipLaunchKernelGGL(ese_bwd_fc_kernel, dim3((unsigned)((fc + VG_T - 1) / VG_T)), dim3(VG_T), 0, st, k);
  if ((e = check_launch("ese_bwd_fc_kernel")) != DD3D_OK) return e;
  const long total = (long)a->B * a->HW * (a->C / 4);
  hipLaunchKernelGGL(ese_bwd_apply_kernel, dim3((unsigned)((total + VG_T - 1) / VG_T)), dim3(VG_T), 0, st, k);
  return check_launch("ese_bwd_apply_kernel");
}

extern "C" int dd3d_vovnet_add(const float* a, const float* b, float* out, int64_t npix, int32_t C, int32_t a_pitch, int32_t b_pitch, int32_t out_pitch,
                               void* stream) {
  using namespace dd3d;
  const char* who = "dd3d_vovnet_add";
  DD3D_REQUIRE(a && b && out, "%s: null operand", who);
  DD3D_REQUIRE(npix >= 1 && npix <= DD3D_BG_MAX_PIXELS, "%s: %ld pixels (1 .. %ld)", who, (long)npix, (long)DD3D_BG_MAX_PIXELS);
  DD3D_REQUIRE(C >= 4 && C % 4 == 0 && C <= DD3D_VG_MAX_CIN, "%s: C = %d is not a multiple of 4 up to %d", who, C, DD3D_VG_MAX_CIN);
  DD3D_REQUIRE(a_pitch % 4 == 0 && a_pitch >= C && b_pitch % 4 == 0 && b_pitch >= C && out_pitch % 4 == 0 && out_pitch >= C,
               "%s: pitches %d, %d, %d must be multiples of 4 and hold %d channels", who, a_pitch, b_pitch, out_pitch, C);
  DD3D_REQUIRE(aligned16(a) && aligned16(b) && aligned16(out), "%s: operands must be 16-byte aligned", who);
  const long total = (long)npix * (C / 4);
  hipLaunchKernelGGL(vovnet_add_kernel, dim3((unsigned)((total + VG_T - 1) / VG_T)), dim3(VG_T), 0, reinterpret_cast<hipStream_t>(stream), a, b, out, (long)npix,
                     C / 4, a_pitch, b_pitch, out_pitch);
  return check_launch("vovnet_add_kernel");
}

extern "C" int dd3d_maxpool3x3s2_ceil_backward(const dd3d_pool3_grad_args* a, void* stream) {
  using namespace dd3d;
  const char* who = "dd3d_maxpool3x3s2_ceil_backward";
  DD3D_REQUIRE(a != nullptr, "%s: null args", who);
  DD3D_REQUIRE(a->B >= 1 && a->H >= 3 && a->W >= 3, "%s: B = %d, %d x %d (at least 3 x 3)", who, a->B, a->H, a->W);
  DD3D_REQUIRE(a->C >= 32 && a->C % 32 == 0 && a->C <= DD3D_VG_MAX_COUT, "%s: C = %d is not a multiple of 32 up to %d", who, a->C, DD3D_VG_MAX_COUT);
  DD3D_REQUIRE((long)a->B * a->H * a->W <= DD3D_BG_MAX_PIXELS, "%s: %ld input pixels (at most %ld)", who, (long)a->B * a->H * a->W, (long)DD3D_BG_MAX_PIXELS);
  DD3D_REQUIRE(a->x && a->g && a->da, "%s: no input / gradient / output", who);
  const int rc = check_storage(who, "x", a->x_mode, a->x_pitch, a->C, a->x_plane_scale);
  if (rc != DD3D_OK) return rc;
  DD3D_REQUIRE(a->g_pitch % 4 == 0 && a->g_pitch >= a->C, "%s: g_pitch = %d must be a multiple of 4 and hold %d channels", who, a->g_pitch, a->C);
  DD3D_REQUIRE(a->da_pitch % 4 == 0 && a->da_pitch >= a->C, "%s: da_pitch = %d must be a multiple of 4 and hold %d channels", who, a->da_pitch, a->C);
  if (a->add) DD3D_REQUIRE(a->add_pitch % 4 == 0 && a->add_pitch >= a->C, "%s: add_pitch = %d must be a multiple of 4 and hold %d channels", who, a->add_pitch, a->C);
  Pool3K k;
  k.a = *a;
  k.Ho = pool3_out(a->H), k.Wo = pool3_out(a->W);
  k.x_inv = 1.f / a->x_plane_scale;
  const long total = (long)a->B * a->H * a->W * a->C;  // (at most 2^26 pixels x 1024 channels / 256 threads: the block count fits 32 bits)
  hipLaunchKernelGGL(pool3_backward_kernel, dim3((unsigned)((total + VG_T - 1) / VG_T)), dim3(VG_T), 0, reinterpret_cast<hipStream_t>(stream), k);
  return check_launch("pool3_backward_kernel");
}

extern "C" int dd3d_vovnet_grad_layout(int64_t* out, int32_t n) {
  using namespace dd3d;
  DD3D_REQUIRE(out && n >= 48, "dd3d_vovnet_grad_layout: need 48 slots");
#define EOFF(f) (int64_t) offsetof(dd3d_ese_grad_args, f)
#define POFF(f) (int64_t) offsetof(dd3d_pool3_grad_args, f)
  const int64_t v[] = {(int64_t)sizeof(dd3d_ese_grad_args), EOFF(xt), EOFF(g), EOFF(fc_w), EOFF(fc_b), EOFF(part), EOFF(m), EOFF(z), EOFF(s), EOFF(dz), EOFF(u),
                       EOFF(g_xt), EOFF(d_fc_w), EOFF(d_fc_b), EOFF(B), EOFF(HW), EOFF(C), EOFF(rsplit), EOFF(xt_mode), EOFF(xt_pitch), EOFF(g_pitch),
                       EOFF(gxt_pitch), EOFF(xt_plane_scale), EOFF(reserved),
                       (int64_t)sizeof(dd3d_pool3_grad_args), POFF(x), POFF(g), POFF(add), POFF(da), POFF(B), POFF(H), POFF(W), POFF(C), POFF(x_mode),
                       POFF(x_pitch), POFF(g_pitch), POFF(add_pitch), POFF(da_pitch), POFF(x_plane_scale)};
#undef EOFF
#undef POFF
  const int k = (int)(sizeof(v) / sizeof(v[0]));
  for (int i = 0; i < n; ++i) out[i] = i < k ? v[i] : -1;
  return k;
}
