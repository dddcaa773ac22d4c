/*
 * dd3d_hip.h -- C ABI of the MI355X (gfx950) DD3D forward-path library  (libdd3d_hip.so): the forward, the evaluators' kernels and the
 * training losses (detector: dd3d_loss_*, with the head-map gradients of dd3d_loss_backward and the predictor layer's backward below them,
 * dd3d_predictor_wgrad / dd3d_predictor_dgrad, and the head towers' below those, dd3d_tower_wgrad / dd3d_tower_dgrad, and the FPN's below those, dd3d_fpn_wgrad / dd3d_fpn_dgrad; depth pre-training: dd3d_dense_depth_loss, with the gradient at the head's per-level maps
 * of dd3d_dense_depth_loss_backward)
 *
 * The reference (TRI-ML/dd3d) has no FFI of its own for this path: it is pure Python and reaches
 * native code only through third-party wheels (cuDNN via torch, torchvision.ops.nms,
 * detectron2._C.nms_rotated, pytorch3d).  The entry points below are what a maintainer would bind
 * INSTEAD of those calls; each one cites the reference call site(s) it replaces.  See
 * INTEGRATION.md for the ctypes stub on the reference side.
 *
 * Conventions
 *   - plain C, no torch types: device pointers, int sizes, an opaque hipStream_t passed as void*.
 *   - every buffer is owned by the caller (PyTorch caching allocator); the library allocates no
 *     persistent device memory and never synchronises the device.
 *   - kernels are enqueued asynchronously on `stream`; calls are safe under hipGraph stream capture.
 *   - return value: 0 = ok, <0 = error (DD3D_E_*); dd3d_last_error() gives a message (thread-local).
 *   - activations are NHWC fp32 with an explicit per-pixel pitch, so a conv can read / write a
 *     channel slice of a wider buffer (this is how torch.cat in dla.py:161 disappears), and / or
 *     "split planes": [channel chunk c/32][pixel (b,h,w)][plane][32] 16-bit terms of the arithmetic
 *     mode (DD3D_MATH_*), the form in which one convolution hands its output to the next so that
 *     the consumer streams it into LDS by LDS-DMA with no conversion work (a channel slice of a
 *     wider buffer = a run of whole chunk images, so the concat-by-placement carries over).
 */
#ifndef DD3D_HIP_H
#define DD3D_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DD3D_ABI_VERSION 7

#define DD3D_OK 0
#define DD3D_E_INVALID (-1)  /* bad argument (shape / alignment / enum) */
#define DD3D_E_LAUNCH (-2)   /* hip launch error */
#define DD3D_E_UNSUPPORTED (-3)

#define DD3D_MAX_LEVELS 8
#define DD3D_CAND_FIELDS 22 /* SoA fields of a decoded candidate, see dd3d_fcos_select_decode */
#define DD3D_DET_FIELDS 32  /* AoS fields of a final detection, see dd3d_nms_finalize / dd3d_bev_nms_aggregate */

int dd3d_abi_version(void);
const char* dd3d_last_error(void);
/* "gfx950" -- the only architecture the code objects are built for. */
const char* dd3d_arch(void);
/* "" for the product build.  Otherwise the -DDD3D_...=... knobs the library's translation units were compiled with ("file: KNOB=value; ..."):
 * an A/B variant (tests/tools/build_variant.sh; every knob still computes correct results).  dd3d_amd/hip.py refuses such a library unless the
 * caller selected it explicitly. */
const char* dd3d_build_flags(void);

/* ------------------------------------------------------------------------------------------------
 * Implicit-GEMM convolution on f32 MFMA (v_mfma_f32_32x32x2_f32), fused epilogue.
 * Replaces: every nn.Conv2d / detectron2 Conv2d(+FrozenBN/BN +ReLU) on the path --
 *   tridet/modeling/feature_extractor/dla.py:50-62,160-167,233-247,346-355 (DLA blocks, roots),
 *   detectron2 FPN lateral/output/top-block convs [ext] (built at dla.py:550-557),
 *   tridet/modeling/dd3d/fcos2d.py:137-152 and fcos3d.py:163-180 (towers, predictors, Scale/Offset),
 *   plus the residual add (dla.py:59-60) and torch.cat before a Root (dla.py:161), which are folded
 *   into the epilogue / the pitch addressing.
 *
 * One launch processes `nsegs` segments that share the filter geometry (KH,KW,stride,pad,Cin,N) but
 * have their own tensors: e.g. the 5 FPN levels x 3 head towers of one tower layer = 15 segments.
 *
 *   out[m, n] = max( lo[n],  relu?( sum_k A[m,k] * Wp[n,k] * scale[n] + bias[n] + res[...] ) )
 *
 * K ordering of the packed filter Wp[Npad][Kpad] (n-major, k contiguous):
 *   k = (c / CC) * (KH*KW*CC) + (kh*KW + kw) * CC + (c % CC),   CC = min(Cin, 32),
 * zero-padded to Kpad (multiple of 32) and Npad (multiple of 32).  Cin must be 4, 16 or a multiple of 32.
 * ------------------------------------------------------------------------------------------------ */
typedef struct dd3d_conv_seg {  /* array lives in DEVICE memory */
  const float* in;     /* NHWC input, already offset to the first input channel                  */
  const float* w;      /* packed filter [Npad][Kpad]                                             */
  const float* scale;  /* [N] folded-norm / Scale multiplier                                     */
  const float* bias;   /* [N] folded-norm shift / conv bias / Offset                             */
  const float* lo;     /* [N] per-channel lower clamp (0 => ReLU on that channel, -inf => none), or NULL */
  const float* res;    /* residual source or NULL: f32 NHWC (res_mode 1) or split planes (res_mode 2 / 3, ABI 4) */
  float* out;          /* NHWC output, already offset to the first output channel                */
  int32_t B, H, W;     /* input batch / height / width                                           */
  int32_t Ho, Wo;      /* output height / width                                                   */
  int32_t in_pitch, out_pitch, res_pitch; /* floats per pixel of the respective buffers          */
  int32_t M;           /* B*Ho*Wo                                                                */
  int32_t res_mode;    /* 0 none; 1 add the f32 value res[m * res_pitch + n] (same pixel) before the clamp;
                          ABI 4, split-plane-input kernels only: the residual is read from SPLIT PLANES of the launch's arithmetic mode,
                          `res` = first chunk of the slice, [ceil(N/32)][pixels][NP][32] terms of value * out_plane_scale:
                          2 same pixel (pixels = M) -- dla.py:59-60 without an f32 twin of the residual source;
                          3 the map at HALF the resolution, pixel (b, ho/2, wo/2) of B x Ho/2 x Wo/2 (Ho, Wo even): the FPN top-down
                            path's F.interpolate(scale 2, nearest) + add [ext d2 FPN.forward] fused into the lateral convolution.
                          DD3D_TILE_256x256_W8 carries no residual (its waves have no registers left for one). */
  const void* in_planes; /* split-plane input [Cin/32][B*H*W][NP][32], first chunk of the slice; read instead of `in` when
                            dd3d_conv_launch.in_planes is set                                    */
  int32_t n_limit;     /* > 0: this segment stores only output channels < n_limit (<= launch N); 0: all N  */
  int32_t reserved;    /* 0; ignored */
  void* out_planes;    /* split-plane output [ceil(N/32)][M][NP][32] (first chunk of the slice) or NULL; `out` may then be NULL.
                          Channels N .. 32*ceil(N/32)-1 of the last chunk are written as zeros.  Split-operand modes only. */
} dd3d_conv_seg;

typedef struct dd3d_conv_launch {  /* host memory */
  const dd3d_conv_seg* segs; /* device */
  const int32_t* tiles;      /* device, ntiles x {seg, m0} */
  float* workspace;          /* device, splitk * ntiles * ceil(N/BN) * BM * BN floats (raw accumulator slabs) when splitk > 1, else NULL */
  int32_t nsegs, ntiles;
  int32_t KH, KW, stride, pad;
  int32_t Cin, N, Kpad, Npad;
  int32_t relu;      /* 1: clamp every output channel at 0 */
  int32_t splitk;    /* >= 1 */
  int32_t math_mode; /* DD3D_MATH_* */
  int32_t tile_cfg;  /* DD3D_TILE_* */
  const float* zero_page; /* device, >= 128 B of zeros, 16-B aligned: source of padded taps for the LDS-DMA kernel
                             (NULL selects the register-staged kernel) */
  int32_t* tile_counters; /* device, ceil(N/BN) * ntiles int32, ZERO on entry when splitk > 1 (else NULL).  The slice of an
                             output tile that arrives last sums the partial slabs in slice order and applies the epilogue
                             inside the same launch; the counters are zero again when the launch has completed. */
  const dd3d_conv_seg* seg0_host; /* HOST copy of segs[0 .. nsegs-1], or NULL.  With nsegs == 1 the descriptor then travels in the kernel
                                     arguments (tiles are taken as m0 = i * BM) and the device copies are not read.  With a host copy the
                                     library VALIDATES every segment's residual contract before launching (ABI 5); without one (NULL) the
                                     caller vouches for the device-side descriptors:
                                       res_mode in 0..3 and res != NULL unless 0; res_mode 2 / 3 only with in_planes;
                                       res_mode 3: even Ho, Wo;  DD3D_TILE_256x256_W8: res_mode 0 (its waves hold no residual);
                                       res_mode 1 with in_planes: res_pitch % 4 == 0 and res_pitch >= (channels stored rounded up to 4)
                                       -- the epilogue reads the residual row in 16-byte pieces. */
  int32_t in_relu; /* 1: the input is rectified on the fly, out = epilogue(conv(max(in, 0))) -- LastLevelP6P7: p7 = conv(relu(p6)).
                      DD3D_MATH_BF16X3 with f32 input only */
  int32_t in_planes; /* 1: every segment reads its split-plane input (seg.in_planes) instead of the f32 one; Cin % 32 == 0 and a
                        split-operand math mode */
  float out_plane_scale; /* DD3D_MATH_F16X2: the split-plane outputs hold value * out_plane_scale (a power of two; 0 = 1) */
  int32_t* status;       /* device int32 OR-ed with DD3D_STATUS_* bits by the kernels, or NULL */
  float* amax;           /* DD3D_MATH_F16X2, split-plane outputs: 16 device floats, 32 floats apart (amax[32 * j], j < 16), or NULL.  The
                            launch folds max |value * out_plane_scale| over a sample of its stored outputs (one wave tile per block) into
                            them (atomic max; non-negative floats compare like their bit patterns).  The caller zeroes them before a forward
                            and reads their maximum afterwards: a tensor whose LARGEST scaled entry is below 2^-5 has lost more than four
                            of its 24 bits to the absolute floor 2^-25 of the half pair (the "underflow" side of the range guard). */
} dd3d_conv_launch;

/* Arithmetic of the implicit GEMM (results agree to f32 rounding level; both accumulate in f32):
 *   DD3D_MATH_F32     v_mfma_f32_32x32x2_f32 on f32 operands; segment.w = Wp[Npad][Kpad] f32
 *   DD3D_MATH_BF16X3  each f32 operand split exactly into 3 bf16 terms, 6 cross products on v_mfma_f32_32x32x16_bf16;
 *                     segment.w = Wp3[Npad][Kpad/32][3][32] bf16 (planes hi, mid, lo of the same k order); Cin % 32 == 0,
 *                     tiles 256x128 / 128x128 / 128x64 / 64x128 */
#define DD3D_MATH_F32 0
#define DD3D_MATH_BF16X3 1
/* Reduced split-operand modes (what BASELINE.json's "bf16 inference" configurations name); split-plane inputs only
 * (dd3d_split_planes converts an f32 tensor), f32 accumulate, filters split the same way, round-to-nearest-even terms:
 *   DD3D_MATH_BF16X2  x ~ hi + lo (two bf16 terms, ~17 significand bits), 3 cross products: half the matrix work of BF16X3
 *   DD3D_MATH_BF16    x ~ bf16(x), one product: plain bf16 operands */
#define DD3D_MATH_BF16X2 2
#define DD3D_MATH_BF16 3
/*   DD3D_MATH_F16X2   x * S = hi + lo, two IEEE half terms by round-to-nearest (2 x 11 significand bits: the pair carries the 24 bits
 *                     of an f32 wherever lo is a normal half), 3 cross products on v_mfma_f32_32x32x16_f16; the dropped lo*lo term is
 *                     <= 2^-24 |a*b| like the dropped terms of DD3D_MATH_BF16X3 -> f32-equivalent at HALF its matrix work, inside the
 *                     half format's exponent range.  S: activations carry the power-of-two `plane_scale` of the launch / of
 *                     dd3d_split_planes (|x * S| <= 65504 or the status word is set; terms below 2^-24 / S are lost); filters are
 *                     scaled per output row by the caller, who divides the products of the scales out of `scale[n]`. */
#define DD3D_MATH_F16X2 4
#define DD3D_STATUS_F16_OVERFLOW 1 /* bit set in *status when a value left the half range while being split */
/* DD3D_MATH_F16X2 range guard, for the multi-GPU exchange: out[0] = *status (may be NULL: 0), out[1] = 1 when one of the n_launches
 * watched launches stored a nonzero sampled maximum below `floor` (amax: [n_launches][16][32] floats, see dd3d_conv_launch.amax).  The
 * two words travel in a rank's record; after the all_gather every rank sees every rank's verdict and all act on the same step. */
int dd3d_fold_range_flags(const int32_t* status, const float* amax, int32_t n_launches, float floor, int32_t* out, void* stream);
/* What the host reads after a forward, packed into ONE contiguous run of 4-byte words so that a single asynchronous device-to-host
 * copy (into pinned memory, enqueued behind the forward) replaces one blocking read per field -- the reference's forward ends by
 * returning Instances (tridet/modeling/dd3d/core.py:153-164), which needs the detection counts on the host:
 *   out[0] = *status (NULL: 0), out[1] = G, out[2] = n_launches, out[3] = n_flag_recs, out[4 .. 4 + G) = det_count[0 .. G),
 *   then n_launches floats: max over the 16 sub-maxima of every watched launch (amax as in dd3d_conv_launch.amax),
 *   then 2 * n_flag_recs words: flags[r * flag_stride + {0, 1}] (every rank's dd3d_fold_range_flags words inside the gathered records).
 * `out` holds 4 + G + n_launches + 2 * n_flag_recs words.  One block; ordered on `stream` behind the forward's last launch. */
int dd3d_pack_readback(const int32_t* det_count, int32_t G, const int32_t* status, const float* amax, int32_t n_launches,
                       const int32_t* flags, int32_t n_flag_recs, int64_t flag_stride, int32_t* out, void* stream);
/* planes per value of a math mode (0 for DD3D_MATH_F32) */
int dd3d_math_planes(int32_t math_mode);

#define DD3D_TILE_128x128 0
#define DD3D_TILE_128x64 1
#define DD3D_TILE_64x64 2
#define DD3D_TILE_128x32 3
#define DD3D_TILE_64x128 4
#define DD3D_TILE_256x128 5    /* DD3D_MATH_BF16X3 only, like the three below */
#define DD3D_TILE_128x128_W4 6 /* 4-wave blocks (256 threads) small enough in LDS for two per CU */
#define DD3D_TILE_64x64_W4 7
#define DD3D_TILE_128x64_W4 8
#define DD3D_TILE_128x64_K2 9  /* 8 waves, two K-tiles (64 k) per barrier */
#define DD3D_TILE_64x128_K2 10
#define DD3D_TILE_64x64_W4K2 11
/* split-plane kernels only: wave tiles of 128 x 64 / 64 x 128 outputs (8 accumulator blocks per wave) -- one ds_read_b128 per two MFMAs
 * in the two-term modes instead of two per three; 4-wave blocks hold one wave per SIMD (up to 512 registers each) */
#define DD3D_TILE_256x128_T42 12 /* 4 waves (2 x 2), wave tile 128 x 64 */
#define DD3D_TILE_128x256_T24 13 /* 4 waves (2 x 2), wave tile 64 x 128 */
#define DD3D_TILE_256x256_W8 14  /* 8 waves (2 x 4), wave tile 128 x 64; one- and two-term modes only */
#define DD3D_TILE_128x32_W4 15   /* split-plane kernels: 4 waves (4 x 1), 32 output columns -- the narrow predictors (N <= 32: fcos2d.py:96-110) */
#define DD3D_TILE_192x256_W8 16  /* row-shared 3 x 3 kernel only: 8 waves (2 x 4), wave tile 96 x 64 -- launches whose 256-row tiles fill only part of the chip
                                  * (the merged FPN output convolutions: 210 blocks instead of 158 on 256 CUs); no residual, no split-K, like DD3D_TILE_256x256_W8 */
#define DD3D_TILE_COUNT 17
/* rows (M) and columns (N) of a block tile for a DD3D_TILE_* id; returns 0 on success */
int dd3d_conv_tile_shape(int32_t tile_cfg, int32_t* bm, int32_t* bn);
/* B / A ring depths (NSB, NSA) of the row-shared split-plane kernel instantiation that `tile_cfg` launches in `math_mode` -- the 5th and
 * 8th template arguments rocprofv3 prints for `conv_igemm_planes_row_kernel<...>` (profile bookkeeping; DD3D_E_UNSUPPORTED when the pair
 * has no such kernel) */
int dd3d_conv_row_rings(int32_t tile_cfg, int32_t math_mode, int32_t* nsb, int32_t* nsa);
int dd3d_conv2d_igemm_f32(const dd3d_conv_launch* launch, void* stream);

/* f32 NHWC -> split planes of `math_mode` (the entry into the plane format for tensors a non-convolution kernel produced: pooled
 * maps, the FPN top-down sums, eSE outputs, the stem), optionally rectified (LastLevelP6P7: p7 = conv(relu(p6)) [ext]).
 *   in [M][in_pitch] f32, channels [0, C), C % 32 == 0;  out [C/32][M][NP][32] 16-bit terms of in * plane_scale (plane_scale: see
 *   DD3D_MATH_F16X2; ignored by the bf16 modes); status: see dd3d_conv_launch */
int dd3d_split_planes(const float* in, void* out, int32_t M, int32_t C, int32_t in_pitch, int32_t math_mode, int32_t relu, float plane_scale,
                      int32_t* status, void* stream);

/* dd3d_maxpool2x2_nhwc / dd3d_upsample2x_add_nhwc that ALSO write the split planes of their result (one launch instead of the kernel
 * followed by dd3d_split_planes): out_planes / fine_planes = [C/32][pixels][NP][32] terms of `math_mode` (first chunk of the slice),
 * C % 32 == 0.  dd3d_maxpool2x2_planes: `out` (f32) may be NULL.  plane_scale / status as in dd3d_split_planes. */
int dd3d_maxpool2x2_planes(const float* in, float* out, void* out_planes, int32_t B, int32_t H, int32_t W, int32_t C, int32_t in_pitch,
                           int32_t out_pitch, int32_t math_mode, float plane_scale, int32_t* status, void* stream);
/* ABI 4: 2x2 / stride 2 max-pool (dla.py:228-231 Tree.downsample) of a map held as split planes ONLY: in_planes [C/32][B*H*W][NP][32] ->
 * out_planes [C/32][B*(H/2)*(W/2)][NP][32]; per channel the terms of the largest of the four values are copied (no re-split). */
int dd3d_maxpool2x2_planes_in(const void* in_planes, void* out_planes, int32_t B, int32_t H, int32_t W, int32_t C, int32_t math_mode, void* stream);
int dd3d_upsample2x_add_planes(float* fine, const float* coarse, void* fine_planes, int32_t B, int32_t H, int32_t W, int32_t C, int32_t fine_pitch,
                               int32_t coarse_pitch, int32_t math_mode, float plane_scale, int32_t* status, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Small-channel convolution (the full-resolution stem: dla.py:271-280,327-344 base_layer / level0 / level1,
 * vovnet.py stem_1), DD3D_MATH_BF16X3 arithmetic, + per-channel scale/bias (+ lower clamp / ReLU).
 * The block stages the input patch of its output tile once (f32 -> bf16 hi/mid/lo planes) and feeds
 * v_mfma_f32_16x16x32_bf16 straight from it; no im2col K loop.
 *   in  f32 NHWC [B][H][W] rows of in_pitch floats, channels [0, Cin) used, Cin in {4, 16}
 *   w3  bf16 [chunk][plane][Npad16][32]: 32-k chunks of the k order
 *         Cin 4 : k = (dh*8 + dw)*4 + c      (one chunk per filter row, tap slots >= KW zero)
 *         Cin 16: k = (dh*KW + dw)*16 + c    (two taps per chunk, an odd tap count zero-padded)
 *       planes hi / mid / lo of the exact 3-way bf16 split, Npad16 = round_up(N, 16)
 *   out f32 NHWC rows of out_pitch floats, channels [0, N)
 * Instantiated: (Cin 4, 7x7, s1, p3, N<=16) (Cin 16, 3x3, s1, p1, N<=16) (Cin 16, 3x3, s2, p1, N<=32) (Cin 4, 3x3, s2, p1, N<=64);
 * dd3d_conv2d_smallc_supported() tells.
 * ------------------------------------------------------------------------------------------------ */
typedef struct dd3d_smallc_args {  /* host memory */
  const float* in;
  float* out;
  const void* w3;
  const float* scale;
  const float* bias;
  const float* lo; /* optional per-channel lower clamp */
  int32_t B, H, W, Ho, Wo;
  int32_t in_pitch, out_pitch;
  int32_t Cin, KH, KW, stride, pad, N;
  int32_t relu;
} dd3d_smallc_args;
int dd3d_conv2d_smallc_supported(int32_t Cin, int32_t KH, int32_t KW, int32_t stride, int32_t pad, int32_t N);

/* ------------------------------------------------------------------------------------------------
 * The DLA stem in one launch (ABI 3): uint8 image -> (x - mean) / std (core.py:61-66, zero outside the real image as
 * ImageList.from_tensors pads, image_list.py:120-142) -> base_layer 7x7 3->16 -> level0 3x3 16->16 -> level1 3x3 stride 2 16->32,
 * each + folded norm + ReLU (dla.py:271-280,327-344), DD3D_MATH_F16X2 arithmetic.  Intermediate maps never leave the LDS.
 *   src    uint8 [B][3][Hp][Wp] planar; sizes int32 [B][2] = real (h, w) of each image; mean / stdv per input channel
 *   wK     halves [chunk][plane hi, lo][Npad16][32] of filter K in the k order of dd3d_conv2d_smallc_bf16x3 (w1: Cin 4, 7 chunks,
 *          16 rows; w2: Cin 16, 5 chunks, 16 rows; w3: Cin 16, 5 chunks, 32 rows), every row n scaled by a power of two s_K[n]
 *   scaleK / biasK  per output channel: out = relu(acc * scaleK + biasK); the caller folds 1 / (s_K[n] * plane_scale) into scaleK
 *   out    f32 NHWC [B][Hp/2][Wp/2] rows of out_pitch floats, channels [0, 32) (may be NULL)
 *   out_planes  [pixel][plane][32] halves of value * plane_scale: the one 32-channel chunk image of the split-plane form (may be NULL)
 *   status: the word dd3d_conv_launch.status names -- DD3D_STATUS_F16_OVERFLOW is set when an intermediate or output value leaves the half range)
 * ------------------------------------------------------------------------------------------------ */
typedef struct dd3d_stem_args {  /* host memory; all pointers device */
  const uint8_t* src;
  const int32_t* sizes;
  float mean[3], stdv[3];
  const void* w1;
  const float* scale1;
  const float* bias1;
  const void* w2;
  const float* scale2;
  const float* bias2;
  const void* w3;
  const float* scale3;
  const float* bias3;
  float* out;
  void* out_planes;
  int32_t B, Hp, Wp, out_pitch;
  float plane_scale;
  int32_t* status;
  /* ABI 5 -- start-of-forward chores the launch can take along (block (0, 0, 0) does them; each may be NULL / 0), so that a DLA plan needs no
   * separate launches for them:  inv_K[b] = inverse(K[b]) for b < B (what dd3d_invert_intrinsics computes: core.py:93), and zero_f32[0 .. zero_count)
   * = 0.f (the per-launch range-guard maxima dd3d_conv_launch.amax points into, which are per forward). */
  const float* K;
  float* inv_K;
  float* zero_f32;
  int32_t zero_count;
} dd3d_stem_args;
int dd3d_stem_fused_f16x2(const dd3d_stem_args* args, void* stream);
/* The same launch for a plan that runs the stem's backward (dd3d_stem_wgrad / dd3d_stem_dgrad below): `stem` is dd3d_stem_args as above
 * and produces the same bits in out / out_planes; each block also stores the part of its base_layer and level0 tiles it owns -- the
 * canvas pixels [2 oh0, 2 oh0 + 16) x [2 ow0, 2 ow0 + 64) of its 8 x 32 level1 tile at (oh0, ow0), clipped to the canvas -- as f32 NHWC,
 * [B][Hp][Wp][pitch], channels 0 .. 15: the decoded value (hi + lo) / plane_scale of the LDS planes, exactly what the next layer
 * consumed.  Every pixel has one writer.  Rejected like dd3d_stem_fused_f16x2, and: a NULL or misaligned (16 bytes) keep pointer, a
 * pitch below 16 or not a multiple of 4. */
typedef struct dd3d_stem_keep_args {
  dd3d_stem_args stem;
  float* keep_base;
  float* keep_level0;
  int32_t keep_base_pitch, keep_level0_pitch;
} dd3d_stem_keep_args;
int dd3d_stem_fused_keep_f16x2(const dd3d_stem_keep_args* args, void* stream);
int dd3d_conv2d_smallc_bf16x3(const dd3d_smallc_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Pre-processing.  Replaces DD3D.preprocess_image + ImageList.from_tensors
 * (tridet/modeling/dd3d/core.py:61-72, tridet/structures/image_list.py:120-142):
 * (u8 - mean)/std per channel inside the (h_i, w_i) image, 0.0 in the right/bottom padding.
 *   src  : uint8 [B][3][Hp][Wp] (CHW planes, canvas already at the padded size)
 *   sizes: int32 [B][2] = (h_i, w_i), device
 *   dst  : fp32 NHWC [B][Hp][Wp][4], channel 3 = 0
 * ------------------------------------------------------------------------------------------------ */
int dd3d_preprocess_u8_nhwc4(const uint8_t* src, const int32_t* sizes, float* dst, int32_t B, int32_t Hp, int32_t Wp,
                             const float mean[3], const float std[3], void* stream);

/* 2x2 stride-2 max pooling, NHWC with pitches.  Replaces nn.MaxPool2d(2, 2) = Tree.downsample
 * (tridet/modeling/feature_extractor/dla.py:224-225,235).  H, W even; C % 4 == 0. */
int dd3d_maxpool2x2_nhwc(const float* in, float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t in_pitch,
                         int32_t out_pitch, void* stream);

/* 3x3 stride-2 max pooling, no padding, ceil_mode=True.  Replaces nn.MaxPool2d(3, 2, ceil_mode=True) in front of
 * VoVNet stages 3-5 (tridet/modeling/feature_extractor/vovnet.py:248-249).  Output size = ceil((H-3)/2)+1 (PyTorch rule). */
int dd3d_maxpool3x3s2_ceil_nhwc(const float* in, float* out, int32_t B, int32_t H, int32_t W, int32_t C, int32_t in_pitch,
                                int32_t out_pitch, void* stream);

/* effective Squeeze-Excitation + OSA identity: out = x * hsigmoid(fc(mean_hw(x))) (+ identity).
 * Replaces eSEModule.forward and the identity add of _OSA_module.forward (vovnet.py:180-185,233-236).
 *   x [B*HW][x_pitch] (C channels), fc_w [C][C] row-major (= the 1x1 conv weight), fc_b [C],
 *   workspaces: partial [B][rsplit][C], gate [B][C].  Deterministic (two-pass sum, no atomics). */
int dd3d_ese_nhwc(const float* x, const float* identity, float* out, const float* fc_w, const float* fc_b, float* partial,
                  float* gate, int32_t B, int32_t HW, int32_t C, int32_t x_pitch, int32_t id_pitch, int32_t out_pitch,
                  int32_t rsplit, void* stream);

/* The same module in two launches that also write the split planes of the result (pool + per-image mean; gate + scale (+ identity)
 * -> f32 NHWC `out` (may be NULL) and / or the split planes of `math_mode` in `out_planes` (may be NULL; C % 32 == 0; layout and
 * plane_scale as dd3d_split_planes)): 5 passes over the map instead of the 7 of dd3d_ese_nhwc + dd3d_split_planes.  Same summation
 * order as dd3d_ese_nhwc.  C % 8 == 0, C <= 4096.
 *   workspaces: partial [B][rsplit][C], mean [B][C], counters int32 [B] -- zero before the first launch, left zero by the kernel
 *   status OR-ed with DD3D_STATUS_F16_OVERFLOW as dd3d_split_planes; may be NULL */
int dd3d_ese_fused(const float* x, const float* identity, float* out, void* out_planes, const float* fc_w, const float* fc_b, float* partial,
                   float* mean, int32_t* counters, int32_t B, int32_t HW, int32_t C, int32_t x_pitch, int32_t id_pitch, int32_t out_pitch,
                   int32_t rsplit, int32_t math_mode, float plane_scale, int32_t* status, void* stream);

/* fine[b,y,x,:] += coarse[b,y/2,x/2,:].  Replaces the FPN top-down step of detectron2 FPN.forward [ext]:
 * prev = lateral + F.interpolate(prev, scale_factor=2, mode="nearest").  H, W (of `fine`) even; C % 4 == 0. */
int dd3d_upsample2x_add_nhwc(float* fine, const float* coarse, int32_t B, int32_t H, int32_t W, int32_t C,
                             int32_t fine_pitch, int32_t coarse_pitch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fused per-(image, level) candidate selection + 2D/3D decode.
 * Replaces FCOS2DInference.forward_for_single_feature_map (fcos2d.py:270-344),
 * FCOS3DInference.forward_for_single_feature_map (fcos3d.py:328-399), predictions_to_boxes3d
 * (fcos3d.py:16-52), allocentric_to_egocentric / unproject_points2d (tridet/utils/geometry.py:15-112),
 * pytorch3d quaternion_to_matrix / matrix_to_quaternion [ext], compute_features_locations
 * (tridet/utils/tensor2d.py:6-25).
 *
 * Head maps are NHWC with these channel layouts (C = num classes, C3 = 1 if class-agnostic else C):
 *   cls  [B*HW][cls_pitch]  : logits 0..C-1
 *   box2d[B*HW][b2d_pitch]  : relu(scale*reg) 0..3, centerness logit 4
 *   box3d[B*HW][b3d_pitch]  : quat 4*C3 (comp*C3+cls), ctr 2*C3, depth C3, size 3*C3, conf C3
 * Output (per image b): cand[b][f][slot_off[level] + j], f < DD3D_CAND_FIELDS:
 *   0-3 box x1,y1,x2,y2 | 4 score=sqrt(cls*ctr) | 5 score_3d | 6 class (int bits) | 7 loc*C+class (int bits)
 *   8-9 location x,y | 10-13 quat wxyz (egocentric) | 14-15 proj_ctr | 16 depth | 17-19 size WLH
 *   20 argmax attribute (int bits) | 21 speed      (nuScenes; NuscenesInference, nuscenes_dd3d.py:268-296)
 * counts[b][level] = number of valid slots (<= topk); npass[b][level] = #scores over threshold.
 * Candidate order inside a level = ascending (loc, class), i.e. torch.nonzero order.
 * ------------------------------------------------------------------------------------------------ */
typedef struct dd3d_select_args {  /* host memory */
  const float* cls[DD3D_MAX_LEVELS];
  const float* box2d[DD3D_MAX_LEVELS];
  const float* box3d[DD3D_MAX_LEVELS]; /* NULL entries => 2D only (MODEL.BOX3D_ON false) */
  int32_t H[DD3D_MAX_LEVELS], W[DD3D_MAX_LEVELS], stride[DD3D_MAX_LEVELS];
  int32_t cls_pitch, b2d_pitch, b3d_pitch;
  int32_t num_levels, B, num_classes;
  int32_t class_agnostic_3d;
  int32_t loc_offset_half;       /* DD3D.FEATURE_LOCATIONS_OFFSET == "half" */
  int32_t thresh_with_ctr;       /* DD3D.FCOS2D.INFERENCE.THRESH_WITH_CTR */
  int32_t topk;                  /* PRE_NMS_TOPK */
  int32_t attr_off, num_attr;    /* nuScenes: cls-map channels [attr_off, attr_off+num_attr) = attribute logits (0 attrs: none) */
  int32_t speed_off;             /* nuScenes: cls-map channel of relu(speed), or -1 */
  float pre_nms_thresh;
  float min_depth, max_depth, focal_factor;
  int32_t scale_depth_by_focal, allocentric, depth_is_distance;
  const float* inv_K;            /* [B][9] row-major inverse intrinsics, device */
  const float* canon_sizes;      /* [>=num_classes][3] (W,L,H), device */
  int32_t* scratch_idx;          /* device, per (b,level) region; offsets below  */
  float* scratch_score;
  int64_t scratch_off[DD3D_MAX_LEVELS]; /* element offset of level l's region for image 0 */
  int64_t scratch_img_stride;           /* elements per image */
  float* cand;                   /* [B][DD3D_CAND_FIELDS][slots per image] */
  int32_t* counts;               /* [B][num_levels] */
  int32_t* npass;                /* [B][num_levels] */
  int32_t slot_off[DD3D_MAX_LEVELS + 1]; /* first slot of level l in an image's candidate row; slot_off[num_levels] = slots per image.
                                    Level l needs min(topk, H*W*C) slots, so the exchanged buffer carries no slot a level can never
                                    fill.  All zero: the dense layout l * topk (num_levels * topk slots per image). */
} dd3d_select_args;
int dd3d_fcos_select_decode(const dd3d_select_args* args, void* stream);

/* Closed-form inverse of the (B,3,3) intrinsics.  Replaces images.intrinsics.inverse() (core.py:93). */
int dd3d_invert_intrinsics(const float* K, float* inv_K, int32_t B, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Class-aware 2D NMS + top-k + resize.  Replaces FCOS2DInference.nms_and_top_k (fcos2d.py:346-367) =
 * detectron2.layers.batched_nms -> torchvision.ops.batched_nms / nms [ext] (rank by score_3d,
 * coordinate trick when 4*n <= 4000 else per-class), torch.kthvalue top-k on the 2D score with >=,
 * and detectron2 detector_postprocess [ext] (core.py:153-160).
 *   cand/counts as written by dd3d_fcos_select_decode for G images (after the RCCL gather: G = all images)
 *   out_size [G][4] = (in_h, in_w, out_h, out_w) float, device
 *   det [G][det_cap][DD3D_DET_FIELDS]:
 *     0-3 box | 4 score | 5 score_3d | 6 class | 7 fpn level | 8-9 location | 10-13 quat | 14-15 proj_ctr
 *     | 16 depth | 17-19 size | 20 attribute | 21 speed | 22-25 global quat | 26-28 global tvec (filled by
 *     dd3d_bev_nms_aggregate) | 29-31 unused       (class / level / attribute stored as float-valued integers)
 *   det_count [G]; order = descending score_3d (torchvision keep order).
 * Workspaces (device): sort_idx int32 [G][ncap], sbox float [G][ncap][4], scls int32 [G][ncap],
 *   mask uint64 [G][ncap][ncap/64], nvalid int32 [G][2], where ncap = round_up(num_levels*topk, 64).
 * ------------------------------------------------------------------------------------------------ */
typedef struct dd3d_nms_args {  /* host memory */
  const float* cand;
  const int32_t* counts;
  int32_t G, num_levels, topk;
  int32_t do_nms;          /* DD3D.INFERENCE.DO_NMS */
  int32_t use_score3d;     /* rank by score_3d (BOX3D_ON) else score */
  float nms_thresh;        /* <= 0 disables suppression (fcos2d.py:349) */
  int32_t post_topk;       /* POST_NMS_TOPK */
  int32_t do_postprocess;  /* DD3D.INFERENCE.DO_POSTPROCESS */
  const float* out_size;
  int32_t* sort_idx;
  float* sbox;
  int32_t* scls;
  uint64_t* mask;
  int32_t* nvalid;
  float* det;
  int32_t* det_count;
  int32_t det_cap;
  int32_t slot_off[DD3D_MAX_LEVELS + 1]; /* same table as the producer of `cand` used (the select args) */
  /* Reading the images out of the all-gathered records of several ranks (ABI 3).  img_per_rec = 0: `cand`, `counts`, `out_size` are
   * dense [G] arrays (above).  img_per_rec = P > 0: they point INTO RECORD 0 of a buffer of records rec_stride 4-byte words apart,
   * each holding P images; image g of this call is global image img_first + g = image (img_first + g) % P of record
   * (img_first + g) / P.  This is how the owner of a nuScenes sample finalises cameras that other ranks decoded. */
  int32_t img_first, img_per_rec;
  int64_t rec_stride;
} dd3d_nms_args;
int dd3d_nms_finalize(const dd3d_nms_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * nuScenes sample aggregation = camera->global box transform + BEV rotated-box NMS.
 * Replaces nuscenes_sample_aggregate / sample_bev_nms (tridet/modeling/dd3d/postprocessing.py:22-108),
 * boxes3d_to_rotated_boxes / bev_nms (tridet/layers/bev_nms.py:51-133), GenericBoxes3D.corners
 * (tridet/structures/boxes3d.py:47-64), pytorch3d Transform3d / rotation conversions [ext] and detectron2
 * batched_nms_rotated -> nms_rotated / box_iou_rotated [ext].
 *   det_in [G][det_cap][DD3D_DET_FIELDS], count_in [G]      as written by dd3d_nms_finalize
 *   inv_K [G][9] inverse intrinsics (as written by dd3d_invert_intrinsics)
 *   pose [G][7] (quat wxyz, tvec) camera->global; group [G] sample index of each image (category id =
 *   class + group*num_classes); out_size as in dd3d_nms_finalize (used when do_postprocess)
 *   max_dets: cap on the batch-global, score-ordered keep list (0 = none; the reference truncates the whole batch,
 *   postprocessing.py:93-94).  det_out / count_out: survivors per image in their original order, fields 22-28 = the
 *   global-frame box when write_global.  count_out = -1 everywhere if more than 8192 boxes arrive.
 * Workspaces (device): work float [G*det_cap][16], sbox float [G*det_cap][8], mask uint64 [mcap][mcap/64]
 *   (mcap = min(round_up(G*det_cap, 64), 8192): rows and columns are positions in the SORTED list, which never holds more than the
 *   8192 boxes of the LDS sorter -- ABI 6; ABI 5 strode the rows by round_up(G*det_cap, 64)/64 words), meta int32 [4].
 * ------------------------------------------------------------------------------------------------ */
typedef struct dd3d_bev_args {  /* host memory */
  const float* det_in;
  const int32_t* count_in;
  const float* inv_K;
  const float* pose;
  const int32_t* group;
  const float* out_size;
  int32_t G, det_cap, num_classes;
  float iou_thresh;
  int32_t max_dets;
  int32_t write_global;
  int32_t do_postprocess;
  float* work;
  float* sbox;
  uint64_t* mask;
  int32_t* meta;
  float* det_out;
  int32_t* count_out;
  /* same record addressing as the NMS arguments above, ABI 3: with img_per_rec > 0, `inv_K`, `pose` and `out_size` point into record 0 of the gathered buffer
   * ([P][9], [P][7], [P][4] blocks of a record) and image g is global image img_first + g; `group`, `det_in`, `count_in` stay dense. */
  int32_t img_first, img_per_rec;
  int64_t rec_stride;
} dd3d_bev_args;
int dd3d_bev_nms_aggregate(const dd3d_bev_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Input side (the step right before the path): the test-time resize of the uint8 image.
 * Replaces detectron2 ResizeTransform.apply_image [ext] = PIL Image.resize(BILINEAR) behind ResizeShortestEdge
 * (tridet/data/augmentations/resize_transform.py:85-88, dataset_mapper.py:118-127): Pillow's separable 8-bit resampling --
 * horizontal pass, 8-bit intermediate, vertical pass -- with the per-coordinate bounds and 22-bit fixed-point coefficients
 * computed by the caller (dd3d_amd/inputs.py resample_coeffs).  Bit-identical to PIL.
 *   src  uint8 planar [C][H][W] with strides (src_plane, src_row); dst planar with (dst_plane, dst_row) -- e.g. one image
 *        slot of the forward plan's input canvas; tmp uint8 [C][H][new_w], needed when both sizes change
 *   lo_* / cnt_* int32 [new size], kk_* int32 [new size][ksize_*]
 * ------------------------------------------------------------------------------------------------ */
typedef struct dd3d_resize_args {  /* host memory; all pointers device */
  const uint8_t* src;
  uint8_t* dst;
  uint8_t* tmp;
  int32_t C, H, W, new_h, new_w;
  int64_t src_plane, dst_plane;
  int32_t src_row, dst_row;
  const int32_t *lo_w, *cnt_w, *kk_w;
  const int32_t *lo_h, *cnt_h, *kk_h;
  int32_t ksize_w, ksize_h;
} dd3d_resize_args;
int dd3d_resize_bilinear_u8(const dd3d_resize_args* args, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DD3DDenseDepth tail (tridet/modeling/dd3d/dense_depth.py:140-151): aligned_bilinear(x, factor, offset)
 * (tridet/utils/tensor2d.py:28-47) of channel 0 of an NHWC map [B][h][w] (rows of `pitch` floats) to out [B][factor*h][factor*w],
 * then, when focal_factor > 0, out /= norm(inv_K[b][0][0], inv_K[b][1][1]) * focal_factor  (SCALE_DEPTH_BY_FOCAL_LENGTHS).
 * ------------------------------------------------------------------------------------------------ */
int dd3d_aligned_bilinear_scale(const float* src, float* out, const float* inv_K, int32_t B, int32_t h, int32_t w, int32_t pitch,
                                int32_t factor, int32_t offset_half, float focal_factor, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Evaluator-side overlaps (the step right after the path).  Replace the reference's own numba.cuda / numba
 * kernels in tridet/evaluators/rotate_iou.py (called at kitti_3d_evaluator.py:622-632):
 *   dd3d_rotate_iou_eval    rotate_iou_gpu_eval :292-327: boxes [N][5], qboxes [K][5] = (x, y, x_d, y_d, angle clockwise) ->
 *                           out [N][K]; criterion -1 IoU, 0 / 1 intersection over the query's / box's area, 2 intersection area
 *   dd3d_d3_box_overlap     d3_box_overlap_kernel :330-357: boxes [N][7], qboxes [K][7]; rinc [N][K] holds BEV intersection areas
 *                           on entry (criterion 2 above) and 3D overlaps on return; camera_coordinate picks the vertical axis
 *   dd3d_image_box_overlap  image_box_overlap :360-381: XYXY boxes [N][4], [K][4] -> out [N][K]
 * All pointers device memory, float32, row-major.
 * ------------------------------------------------------------------------------------------------ */
int dd3d_rotate_iou_eval(const float* boxes, const float* qboxes, float* out, int32_t N, int32_t K, int32_t criterion, void* stream);
int dd3d_d3_box_overlap(const float* boxes, const float* qboxes, float* rinc, int32_t N, int32_t K, int32_t criterion,
                        int32_t camera_coordinate, void* stream);
int dd3d_image_box_overlap(const float* boxes, const float* qboxes, float* out, int32_t N, int32_t K, int32_t criterion, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Result formatting for the evaluators.  Replaces the per-box host loops of
 * tridet/evaluators/kitti_3d_evaluator.py:205-264 (convert_3d_box_to_kitti, called once per detection at :120 and per annotation
 * at :145) and tridet/evaluators/nuscenes_evaluator.py:196-198 (global velocity = speed * first column of R(quat_global)).
 *   box3d        [n][10] float32 = Boxes3D.vectorize(): quat (w,x,y,z), tvec (3), size (W,L,H)   (boxes3d.py:142-144)
 *   quat_global  [n][4] float32 and speed [n] float32, or both NULL (KITTI)
 *   out          [n][10] float64 = (W, L, H, x, y, z, rot_y, alpha, vx, vy); alpha rounded to 2 decimals like the reference
 * Arithmetic is float64 (the reference's numpy / pyquaternion path), x / y / z stay float32 values like the reference's in-place add.
 * ------------------------------------------------------------------------------------------------ */
int dd3d_format_boxes3d(const float* box3d, const float* quat_global, const float* speed, double* out, int32_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * KITTI 3D / BEV AP statistics (tridet/evaluators/kitti_3d_evaluator.py, KITTIEvaluationEngine.eval_metric :413-513).  The two
 * greedy matchings of the reference's numba CPU code, over every (image, class x difficulty, overlap threshold[, score threshold])
 * in one launch each:
 *   dd3d_kitti_tp_scores  compute_threshold_jit :749-810 (pass 1): tp_score [n_cd][n_o][n_gt] float64 = the score of the detection
 *                         a GT is matched to as a true positive, -inf for every other GT (ignored, unmatched, matched to an
 *                         ignored detection).  The host collects the finite ones per (cd, o) for get_thresholds :813-847.
 *   dd3d_kitti_pr_counts  compute_statistics_jit :910-1038 with compute_fp=True (pass 2), once per score threshold:
 *                         tp_fp_fn [n_cd][n_o][t_max][3] int64 = (tp, fp, fn) summed over the images for thresh[cd][o][t],
 *                         t < n_thresh[cd][o]; entries t >= n_thresh are 0.  The entry point zeroes the buffer on `stream`
 *                         (hipMemsetAsync) before the launch.
 * Inputs, all device memory except min_overlap:
 *   ov          float32 overlap blocks, as dd3d_rotate_iou_eval / dd3d_d3_box_overlap leave them: image i's block is
 *               [n_dt_i][n_gt_i] row-major at element ov_off[i] (detection rows, GT columns); n_ov = elements of `ov`
 *   dt_begin / gt_begin  [n_img + 1] prefix offsets of each image's detections / GT in the per-box arrays
 *   dt_score    [n_dt] float64 (compared in float64 throughout)
 *   ign_dt / ign_gt  [n_cd][n_dt] / [n_cd][n_gt] int8 codes of clean_kitti_data :653-746 (-1 other class, 0 valid, 1 ignored)
 *   min_overlap [n_o] float64, HOST memory, each >= -FLT_MAX; overlaps are compared against it in float64
 *   max_dt / max_gt  upper bounds of the per-image counts (n_dt_i <= max_dt, n_gt_i <= max_gt)
 * Caps: max_dt <= DD3D_KITTI_MAX_DT_PER_IMAGE, max_gt <= DD3D_KITTI_MAX_GT_PER_IMAGE, n_o <= DD3D_KITTI_MAX_OVERLAPS,
 * t_max <= DD3D_KITTI_MAX_THRESHOLDS, n_cd * n_o <= 65535; larger inputs are rejected.  An image whose offsets break the declared
 * bounds is skipped by the kernels (its outputs are left as they were) rather than read out of range.  Work with no image, no
 * class x difficulty or no overlap threshold (or t_max = 0) returns 0 with nothing enqueued.  Results are deterministic: the
 * counts are integers.
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_KITTI_MAX_DT_PER_IMAGE 8192
#define DD3D_KITTI_MAX_GT_PER_IMAGE 1024
#define DD3D_KITTI_MAX_OVERLAPS 8
#define DD3D_KITTI_MAX_THRESHOLDS 256
typedef struct dd3d_kitti_match_args {  /* host memory */
  const float* ov;
  const int64_t* ov_off;
  const int32_t* dt_begin;
  const int32_t* gt_begin;
  const double* dt_score;
  const int8_t* ign_dt;
  const int8_t* ign_gt;
  const double* min_overlap;
  int64_t n_ov;
  int32_t n_img, n_dt, n_gt, n_cd, n_o, max_dt, max_gt;
} dd3d_kitti_match_args;
int dd3d_kitti_tp_scores(const dd3d_kitti_match_args* args, double* tp_score, void* stream);
int dd3d_kitti_pr_counts(const dd3d_kitti_match_args* args, const double* thresh, const int32_t* n_thresh, int32_t t_max, int64_t* tp_fp_fn,
                         void* stream);

/* ------------------------------------------------------------------------------------------------
 * nuScenes detection matching (the nuScenes devkit's `accumulate`, detection_cvpr_2019, driven by
 * tridet/evaluators/nuscenes_evaluator.py:249-312).  The greedy centre-distance matching of every (sample, class) segment at every
 * distance threshold, in one launch:
 *   match [n_thr][n_pred] int32 = the GT row (index into gt_xy) that prediction row p is matched to at threshold t, or -1.
 * Inputs (device memory unless marked HOST):
 *   pred_xy     [n_pred][2] float64 prediction centres (x, y); each segment's rows are in matching order (the host sorts them)
 *   gt_xy       [n_gt][2] float64 GT centres (x, y); each segment's rows are its sample's GT of the class, in the sample's order
 *   pred_begin / gt_begin            [n_seg + 1] int32 offsets of each segment's rows (CSR)
 *   pred_begin_host / gt_begin_host  HOST copies of the same offsets, validated before the launch
 *   thr         n_thr distance thresholds, by value
 * For each prediction in order, the untaken GT of its segment at the smallest distance sqrt(dx*dx + dy*dy) (float64, correctly
 * rounded, lowest row on ties; NaN never matches) is matched iff that distance < thr[t], and is then taken.
 * Caps: n_thr in [1, DD3D_NUSC_MAX_THRESHOLDS], at most DD3D_NUSC_MAX_PRED_PER_SEGMENT predictions and DD3D_NUSC_MAX_GT_PER_SEGMENT GT
 * per segment, n_seg <= 262140, offsets monotone within [0, n_pred] / [0, n_gt]; anything else is rejected.  Rows outside every segment
 * are not written.  No segment or no prediction returns 0 with nothing enqueued.
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_NUSC_MAX_PRED_PER_SEGMENT 500
#define DD3D_NUSC_MAX_GT_PER_SEGMENT 4096
#define DD3D_NUSC_MAX_THRESHOLDS 8
typedef struct dd3d_nusc_match_args {  /* host memory */
  const double* pred_xy;
  const double* gt_xy;
  const int32_t* pred_begin;
  const int32_t* gt_begin;
  const int32_t* pred_begin_host;
  const int32_t* gt_begin_host;
  int32_t n_seg, n_pred, n_gt, n_thr;
  double thr[DD3D_NUSC_MAX_THRESHOLDS];
} dd3d_nusc_match_args;
int dd3d_nusc_center_match(const dd3d_nusc_match_args* args, int32_t* match, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training losses of DD3D / NuscenesDD3D (csrc/losses.hip; their head-map gradients: dd3d_loss_backward below).
 * Replaces DD3DTargetPreparer / NuscenesDD3DTargetPreparer (prepare_targets.py:28-235, nuscenes_dd3d.py:24-196), FCOS2DLoss
 * (fcos2d.py:159-239), FCOS3DLoss (fcos3d.py:191-299), DisentangledBox3DLoss (disentangled_box3d_loss.py) and NuscenesLoss
 * (nuscenes_dd3d.py:199-265), single process.
 *
 * Ground truth: image b owns records gt[gt_off[b] .. gt_off[b+1]) of DD3D_LOSS_GT_FIELDS words, at most max_gt (<= DD3D_LOSS_MAX_GT)
 * per image: the assignment reads only the first max_gt records of an image (the caller rejects larger images; dd3d_amd raises).
 * Classes must lie in [0, num_classes] (num_classes = background) and attributes in [0, num_attr]: they index the head-map rows and
 * the canonical sizes (dd3d_amd checks them before packing):
 *   0-3 box x1,y1,x2,y2 | 4 class (int bits) | 5 attribute (int bits) | 6 speed | 7-10 quat wxyz | 11-12 proj_ctr | 13 depth
 *   14-16 size WLH | 17-25 K^-1 row-major | 26-27 unused
 * Targets are flattened level-first, then image, then H*W (prepare_targets.py:49-63): location n of the N = B * loc_off[L] targets.
 * `locations` holds the loc_off[L] (x, y) of one image, level-major.
 *
 * dd3d_loss_assign: one thread per (image, location), the image's boxes in LDS.  Writes labels (num_classes = background),
 *   target_inds (-1 for an image without GT), box2d_reg [N][4], ctr_target [N] (0 off the positives), box3d_t [N][19]
 *   (quat 4, proj_ctr 2, depth 1, size 3, K^-1 9) and, when `attributes` is set, attributes [N] / speeds [N].  With box3d head maps
 *   it also ORs into flags[0] whether an allocentric decode of a positive is off unit norm (the batch-wide renormalisation of
 *   geometry.py:48-53, which the loss stage needs before it can decode);
 *   a one-thread launch in front clears flags[0] (a kernel, not hipMemsetAsync: a captured memset node did not keep its fill bytes
 *   over the replays of the larger training graphs).
 * dd3d_loss_terms: one thread per target reads the head maps (layouts of dd3d_select_args), writes per-block partial sums of
 *   DD3D_LOSS_TERMS terms to `partials` (>= ceil(N / 256) rows), then one single-block launch sums them in a fixed order and writes
 *   out[DD3D_LOSS_OUT] and num_pos[0].  No float atomics: the result is the same bit for bit on every run.
 *   out: 0 loss_cls | 1 loss_box2d_reg | 2 loss_centerness | 3 loss_box3d_quat | 4 loss_box3d_proj_ctr | 5 loss_box3d_depth
 *        6 loss_box3d_size | 7 loss_conf3d | 8 loss_attr | 9 loss_speed | 10 num_pos | 11 loss_denom | 12-15 unused
 * dd3d_loss_layout: sizeof(dd3d_loss_args) and the byte offsets of its fields (layout check of the bindings; host only).
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_LOSS_GT_FIELDS 28
#define DD3D_LOSS_MAX_GT 512
#define DD3D_LOSS_BOX3D_FIELDS 19
#define DD3D_LOSS_TERMS 16
#define DD3D_LOSS_OUT 16
typedef struct dd3d_loss_args {  /* host memory */
  const float* cls[DD3D_MAX_LEVELS];   /* head maps, device (dd3d_loss_assign: may be NULL) */
  const float* box2d[DD3D_MAX_LEVELS];
  const float* box3d[DD3D_MAX_LEVELS]; /* NULL entries => 2D only */
  const float* locations;              /* [loc_off[num_levels]][2] */
  const int32_t* gt_off;               /* [B + 1] */
  const float* gt;                     /* [gt_off[B]][DD3D_LOSS_GT_FIELDS] */
  const float* inv_K;                  /* [B][9] K^-1 of the images (the prediction decode) */
  const float* canon_sizes;            /* [num_classes][3] */
  int32_t* labels;
  int32_t* target_inds;
  float* box2d_reg;
  float* ctr_target;
  float* box3d_t;                      /* [N][DD3D_LOSS_BOX3D_FIELDS] or NULL */
  int32_t* attributes;                 /* nuScenes targets or NULL */
  float* speeds;
  int32_t* flags;                      /* [1] */
  float* partials;                     /* [n_partials][DD3D_LOSS_TERMS] */
  float* out;                          /* [DD3D_LOSS_OUT] */
  int32_t* num_pos;                    /* [1] */
  int32_t H[DD3D_MAX_LEVELS], W[DD3D_MAX_LEVELS];
  int32_t loc_off[DD3D_MAX_LEVELS + 1];
  float soi_lo[DD3D_MAX_LEVELS], soi_hi[DD3D_MAX_LEVELS]; /* sizes of interest, both ends inclusive */
  float radius[DD3D_MAX_LEVELS];       /* stride * POS_RADIUS */
  int32_t num_levels, B, num_classes, max_gt, n_partials;
  int32_t cls_pitch, b2d_pitch, b3d_pitch, attr_off, num_attr, speed_off;
  int32_t center_sample, class_agnostic_3d, scale_depth_by_focal, allocentric, depth_is_distance;
  float min_depth, max_depth, focal_factor;
  float focal_alpha, focal_gamma, smooth_l1_beta, conf3d_temperature;
  float weight_box3d, weight_conf3d, weight_attr, weight_speed;
} dd3d_loss_args;
int dd3d_loss_assign(const dd3d_loss_args* args, void* stream);
int dd3d_loss_terms(const dd3d_loss_args* args, void* stream);
int dd3d_loss_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Head-map gradients of the losses above (csrc/loss_grads.hip): d (sum_k upstream[k] * out[k]) / d (cls, box2d, box3d) as
 * dd3d_loss_terms reads the maps -- logits (+ attr, speed on nuScenes), post-ReLU box2d_reg and centerness, quat / ctr / depth / size /
 * conf.  The derivative is the one torch autograd gives the reference's FCOS2DLoss, FCOS3DLoss, DisentangledBox3DLoss and NuscenesLoss
 * (loss_conf3d through the BCE only: the reference detaches its target), with torch's conventions at the non-smooth points: min / max
 * split a tie in halves, clamp passes 1 on its closed interval, sign(0) = 0, the norms and square roots have derivative 0 at 0.
 *
 * dd3d_loss_backward runs after dd3d_loss_assign and dd3d_loss_terms on the same `args` and stream; it reads the labels, the targets,
 *   flags, out[10] (positive count), out[11] (loss_denom) and the partials slab (the attribute and speed denominators, recomputed in the
 *   finalize launch's summation order into denoms[0..2]).  One thread per target writes the complete rows of its location in the three
 *   gradient maps, channels [0, nch): zeros for a background row and for the 3D channels of classes other than the label; the pad words
 *   up to the pitch stay untouched.  No word has two writers: no memset is needed, there is no atomic on a float, and two runs agree
 *   bit for bit.  denoms: 4 words of device scratch; after the call the int32 at denoms[3] is 0 unless the value part of the
 *   backward's decode differed from the forward's in some positive (it never should: a self-check of the two statements).
 * dd3d_loss_grad_layout: sizeof(dd3d_loss_grad_args) and the byte offsets of its fields (layout check of the bindings; host only).
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_LOSS_GRAD_DENOMS 4
typedef struct dd3d_loss_grad_args {      /* host memory */
  float* d_cls[DD3D_MAX_LEVELS];          /* same NHWC layout and pitch as dd3d_loss_args.cls / box2d / box3d */
  float* d_box2d[DD3D_MAX_LEVELS];
  float* d_box3d[DD3D_MAX_LEVELS];        /* NULL where box3d[l] is NULL */
  const float* upstream;                  /* device, DD3D_LOSS_OUT floats: d total / d out[k], k as in out[] (0..9 used) */
  float* denoms;                          /* device scratch, DD3D_LOSS_GRAD_DENOMS words */
} dd3d_loss_grad_args;
int dd3d_loss_backward(const dd3d_loss_args* args, const dd3d_loss_grad_args* grads, void* stream);
int dd3d_loss_grad_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Dense-depth training loss of DD3DDenseDepth (csrc/dense_depth_loss.hip); its gradient follows below.
 * Replaces the training branch of DD3DDenseDepth.forward after the head (tridet/modeling/dd3d/dense_depth.py:153-171: aligned_bilinear
 * of every level, the focal-length scaling, DenseDepthL1Loss per level and the / sqrt(2)^level) and DenseDepthL1Loss.forward
 * (dense_depth_loss.py:28-36) with tridet/layers/smooth_l1_loss.py.
 *
 * One pass over the ground-truth canvas gt [B][Hp][Wp] (f32, images in the top-left corner, 0 elsewhere, 16-byte aligned, Wp a multiple
 * of 4).  A pixel is valid iff NOT gt < min_depth and NOT gt > max_depth (a NaN is valid and makes every level NaN).  For a valid pixel
 * and every level l the prediction is the value dd3d_aligned_bilinear_scale(raw[l], ..., h[l], w[l], pitch, stride[l], offset_half,
 * focal_factor) would write at that pixel -- the same arithmetic, bit for bit; the up-sampled maps are never stored.  The per-pixel term
 * is 0.5 n^2 for n = |pred - gt| < beta (not divided by beta), n - 0.5 beta otherwise, plain n for beta < 1e-5.
 *   out[l]   = (loss_weight * (sum_l / count)) / divisor[l]     (f32, in that order; count == 0 gives NaN)
 *   count[0] = number of valid pixels (exact)
 * partials: >= min(ceil(B * Hp * Wp / 4 / 256), DD3D_DDL_MAX_BLOCKS) rows of DD3D_DDL_ROW words (per-block sums of the levels, then the
 * block's count as int32).  Per-block sums in a fixed order, then one single-block launch: no float atomics, the result is the same
 * bit for bit on every run.  h[l] * stride[l] == Hp and w[l] * stride[l] == Wp for every level, or the call is rejected.
 * dd3d_dense_depth_loss_layout: sizeof(dd3d_dense_depth_loss_args) and the byte offsets of its fields (layout check of the bindings).
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_DDL_ROW 12
#define DD3D_DDL_MAX_BLOCKS 1024
typedef struct dd3d_dense_depth_loss_args {  /* host memory */
  const float* raw[DD3D_MAX_LEVELS];  /* per level: NHWC f32 predictor map [B][h][w][pitch], channel 0 used (device) */
  const float* gt;                    /* [B][Hp][Wp] */
  const float* inv_K;                 /* [B][9] K^-1 of the images; may be NULL when focal_factor <= 0 */
  float* partials;                    /* [n_partials][DD3D_DDL_ROW] */
  float* out;                         /* [num_levels] */
  int64_t* count;                     /* [1] */
  int32_t h[DD3D_MAX_LEVELS], w[DD3D_MAX_LEVELS], stride[DD3D_MAX_LEVELS];
  float divisor[DD3D_MAX_LEVELS];     /* f32(sqrt(2)^l), the power taken in float64 on the host */
  int32_t num_levels, B, Hp, Wp, pitch;
  int32_t offset_half;                /* FEATURE_LOCATIONS_OFFSET == "half" */
  int32_t n_partials;
  float focal_factor;                 /* SCALE_DEPTH_BY_FOCAL_LENGTHS_FACTOR, or <= 0: no focal scaling */
  float min_depth, max_depth, beta, loss_weight;
} dd3d_dense_depth_loss_args;
int dd3d_dense_depth_loss(const dd3d_dense_depth_loss_args* args, void* stream);
int dd3d_dense_depth_loss_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Gradient of the dense-depth loss above with respect to the raw per-level maps (csrc/dense_depth_loss_grads.hip):
 *   d_raw[l] = d (sum_l upstream[l] * out[l]) / d raw[l]
 * the derivative torch autograd gives DenseDepthL1Loss behind aligned_bilinear and the focal-length division.  With N = count[0],
 *   d_raw[l](b, i, j) = upstream[l] * loss_weight / (divisor[l] * N * pix_b)
 *                       * sum over the valid pixels p of image b whose taps include (i, j) of tapweight(p; i, j) * s'(pred_l(p) - gt(p))
 * pix_b = |(invK00, invK11)| * focal_factor (1 without focal scaling); s'(d) = d for |d| < beta, sign(d) otherwise and everywhere for
 * beta < 1e-5, sign(0) = 0.  N == 0: every gradient is 0 (the losses are NaN).  A NaN ground-truth pixel counts in N and adds 0 (its
 * difference compares false both ways); a NaN or infinite prediction makes the four taps of its cell NaN at that level, nothing else.
 *
 * dd3d_dense_depth_loss_backward runs after dd3d_dense_depth_loss on the same `args` and stream and reads the count[0] that call wrote;
 *   nothing is read back to the host.  The transposed interpolation is a scatter; it is done without float atomics in two launches:
 *   (1) the pixels that share their four taps at a level (a "cell": stride x stride pixels, shifted by stride / 2 under offset_half,
 *   the border cells larger or smaller) are cut into sub-tiles of at most ~1024 pixels; one wave per sub-tile sums
 *   tapweight * s' for the four corners in a fixed order into one slab row; (2) one thread per raw pixel adds the rows of the up to
 *   four cells around it (up to nine corner sums at the replicated last row / column) in a fixed order, scales and stores.  No
 *   full-resolution map is stored; two runs agree bit for bit.
 * d_raw[l]: NHWC f32 with the pitch of raw[l]; channel 0 of EVERY raw pixel is written (zeros included: no memset is needed), the
 *   other channels are untouched.
 * slab: >= dd3d_dense_depth_grad_rows(args) rows of DD3D_DDG_ROW floats, 16-byte aligned; n_slab says how many there are.
 * Beyond the forward's conditions every stride must be a multiple of 4 (of 8 under offset_half: a 16-byte load never straddles two
 *   cells) and such that the f32 source coordinates of one cell's pixels truncate to one index (every power of two does); the call is
 *   rejected otherwise, before anything is launched.
 * dd3d_dense_depth_grad_rows: the slab rows one backward call on `args` writes (host only; -1 and dd3d_last_error on bad args).
 * dd3d_dense_depth_grad_layout: sizeof(dd3d_dense_depth_grad_args) and the byte offsets of its fields (layout check of the bindings).
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_DDG_ROW 4
typedef struct dd3d_dense_depth_grad_args {  /* host memory */
  float* d_raw[DD3D_MAX_LEVELS];      /* per level: [B][h][w][pitch], the layout of dd3d_dense_depth_loss_args.raw (device) */
  const float* upstream;              /* device, num_levels floats: d total / d out[l] */
  float* slab;                        /* device scratch, [n_slab][DD3D_DDG_ROW] */
  int64_t n_slab;
} dd3d_dense_depth_grad_args;
int dd3d_dense_depth_loss_backward(const dd3d_dense_depth_loss_args* args, const dd3d_dense_depth_grad_args* grads, void* stream);
int64_t dd3d_dense_depth_grad_rows(const dd3d_dense_depth_loss_args* args);
int dd3d_dense_depth_grad_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Backward of the predictor layer (csrc/predictor_grads.hip): the 3x3, Cin -> n convolutions below the head maps (fcos2d.py:143-152,
 * fcos3d.py:175-180, nuscenes_dd3d.py:371-374) with their per-level Scale / Offset.  One call covers one predictor GROUP: the predictors
 * whose outputs share a head map (channels concatenated along n) and therefore one tower.  Forward, per level l:
 *   map_l = clamp_lo((conv3x3(a_l, W_l) + b_l) * s_l + o_l)          W_l, b_l: the same arrays on every level that shares the module
 * With G_l the head-map gradient dd3d_loss_backward wrote and g_l = G_l * [map_l > lo] on the channels with a finite lo (from the STORED
 * map: an entry on its clamp gives 0, as torch.relu does), g_l = G_l elsewhere:
 *   dw_level[l][n][ky][kx][c] = sum_{b,y,x} g_l[b,y,x,n] * a_l[b, y+ky-1, x+kx-1, c]       (zero padding; not scaled)
 *   q[l][n] = sum_{b,y,x} g_l[b,y,x,n]        r[l][n] = sum_k dw_level[l][n][k] * W_l[n][k] + b_l[n] * q[l][n]   (= sum g_l * (conv + b))
 *   dw[l] = sum_{m: w[m] == w[l]} s_m[n] * dw_level[m],   db[l][n] = sum_{m: w[m] == w[l]} s_m[n] * q[m][n]
 *           written for the FIRST level l of each distinct filter pointer; the rows of the other levels are not touched
 *   dscale[l][j] = sum_{n: slot[n] == j} r[l][n]   (d / d Scale_l of slot j)     doffset[l][j] = sum_{n: slot[n] == j} q[l][n]
 *   da[l][b,y,x,c] = sum_{n,ky,kx} s_l[n] * g_l[b, y-ky+1, x-kx+1, n] * W_l[n][ky][kx][c]
 * All sums are f32 sums of exact f32 products (the weight gradient on v_mfma_f32_32x32x2_f32, bitwise an fmaf chain) in a fixed order:
 * per-slice partials, then one reducing launch -- no float atomics, two runs agree bit for bit.  Every word of the outputs named above
 * is written (no memset needed); nothing beyond them is.
 *
 * act: the tower output as the plan holds it -- DD3D_PG_ACT_F32: f32 NHWC [B][H][W][act_pitch], pointer at the first channel;
 *   DD3D_PG_ACT_F16X2 / _BF16X3: split planes [Cin/32][B*H*W][2 or 3][32] 16-bit terms (first chunk of the slice), halves of
 *   value * plane_scale resp. bf16 terms, decoded as the convolutions decode them.
 * dd3d_predictor_wgrad: dw_level, q, r, dw, db, dscale, doffset (four launches).  dd3d_predictor_dgrad: da (one launch; reads g, map,
 *   lo, scale, w only).  Both after dd3d_loss_backward on the same stream; safe under stream capture.
 * dd3d_predictor_grad_slices: rows of `part` / `qpart` a weight-gradient call on `args` needs (host only; -1 on bad args).
 * dd3d_pred_grad_layout: sizeof(dd3d_pred_grad_args) and the byte offsets of its fields (layout check of the bindings; host only).
 * Rejected: Cin not a multiple of 32, pitches not a multiple of 4 or too small, n outside 1 .. DD3D_PG_MAX_N, null pointers.
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_PG_MAX_SLOTS 8
#define DD3D_PG_MAX_N 256
#define DD3D_PG_UNIT 64
#define DD3D_PG_ACT_F32 0
#define DD3D_PG_ACT_F16X2 1
#define DD3D_PG_ACT_BF16X3 2
typedef struct dd3d_pred_grad_args {        /* host memory; every pointer is device memory */
  const void* act[DD3D_MAX_LEVELS];
  const float* g[DD3D_MAX_LEVELS];          /* [B][H][W][g_pitch] */
  const float* map[DD3D_MAX_LEVELS];        /* the stored head map, layout of g; read where lo is finite; may be NULL when lo is */
  const float* w[DD3D_MAX_LEVELS];          /* [n][3][3][Cin] */
  const float* bias[DD3D_MAX_LEVELS];       /* [n]; zeros where a module has no bias */
  const float* scale[DD3D_MAX_LEVELS];      /* [n] s_l */
  float* da[DD3D_MAX_LEVELS];               /* [B][H][W][Cin] f32 */
  const float* lo;                          /* [n] lower clamp of the forward (-inf: none), or NULL */
  const int32_t* slot;                      /* [n] Scale / Offset slot of a channel, 0 .. DD3D_PG_MAX_SLOTS - 1, or -1; or NULL */
  float* part;                              /* scratch [n_slices][n][9 * Cin] */
  float* qpart;                             /* scratch [n_slices][n] */
  float* dw_level;                          /* [num_levels][n][9 * Cin] */
  float* dw;                                /* [num_levels][n][9 * Cin] */
  float* db;                                /* [num_levels][n] */
  float* q;                                 /* [num_levels][n] */
  float* r;                                 /* [num_levels][n] */
  float* dscale;                            /* [num_levels][DD3D_PG_MAX_SLOTS] */
  float* doffset;                           /* [num_levels][DD3D_PG_MAX_SLOTS] */
  int32_t H[DD3D_MAX_LEVELS], W[DD3D_MAX_LEVELS];
  int32_t num_levels, B, Cin, n, g_pitch;
  int32_t act_mode;                         /* DD3D_PG_ACT_* */
  int32_t act_pitch;                        /* DD3D_PG_ACT_F32: floats per pixel */
  int32_t n_slices;                         /* rows of part / qpart */
  float plane_scale;                        /* DD3D_PG_ACT_F16X2: the planes hold value * plane_scale (a power of two) */
} dd3d_pred_grad_args;
int dd3d_predictor_wgrad(const dd3d_pred_grad_args* args, void* stream);
int dd3d_predictor_dgrad(const dd3d_pred_grad_args* args, void* stream);
int64_t dd3d_predictor_grad_slices(const dd3d_pred_grad_args* args);
int dd3d_pred_grad_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Backward of one head-tower layer over all pyramid levels (csrc/tower_grads.hip): the 3x3, Cin -> Cout convolution of a tower
 * (fcos2d.py:130-141, fcos3d.py:160-173) with its per-level folded norm and ReLU.  Forward, per level l, W shared by the levels:
 *   y_l = relu(s_l * conv3x3(x_l, W) + t_l)                     (s_l, t_l): layers.fold_norm of the level's norm, running statistics
 * With G_l the gradient at y_l and g_l = G_l * [y_l > 0], the mask taken from the STORED y_l (an entry on the clamp gives 0):
 *   dw_level[l][n][ky][kx][c] = sum_{b,y,x} g_l[b,y,x,n] * x_l[b, y+ky-1, x+kx-1, c]        (zero padding; not scaled)
 *   dw[n][k] = sum_l s_l[n] * dw_level[l][n][k]                  one fmaf per level, in level order
 *   q[l][n] = sum_{b,y,x} g_l[b,y,x,n]          r[l][n] = sum_k dw_level[l][n][k] * W[n][k]     (= sum g_l * conv; no division by s_l)
 *   da[l][b,y,x,c] = da_add[l][b,y,x,c] + sum_{n,ky,kx} s_l[n] * g_l[b, y-ky+1, x-kx+1, n] * W[n][ky][kx][c]
 * Both are GEMMs on v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation, bitwise an fmaf chain in k order): the weight
 * gradient with M = Cout, N = 9 Cin, K = the pixels of a slice, per-slice partials summed in slice order by a second launch; the input
 * gradient with M = pixels, N = Cin, K = 9 Cout, one accumulator per 32-channel chunk of Cout (its 288 terms in (tap, n) order), the
 * chunks added in chunk order.  A zero or masked g_l entry enters both as an exact zero whatever s_l holds.  No float atomics: every sum
 * has one writer and a fixed order, two runs agree bit for bit, whichever pixel tile the input gradient picks.  Every word of dw_level,
 * dw, q, r and da is written (no memset needed); nothing beyond them and the scratch rows in use is.
 *
 * x, y: the layer's input and stored output as the plan holds them, each in its own storage (DD3D_PG_ACT_*: f32 NHWC with a pitch, or
 *   split planes of the slice's first chunk; f16x2 planes hold value * plane_scale).  g, da, da_add: f32 NHWC, pitches g_pitch / Cin / Cin.
 * part / qpart: dd3d_tower_grad_slices(args) rows (host only; it reads B, H, W, num_levels, Cin and Cout alone, no pointer needs to
 *   be set).  The count grows with the pixel count (four 64-pixel units per slice at least) until the slab reaches DD3D_TG_SLAB_BYTES
 *   (+ at most one row per level), from where the units per slice grow instead.
 * dgrad_rows: rows of the input gradient's 16-pixel-wide tile, 2, 4 or 8; 0 lets the call choose (the largest that still gives
 *   DD3D_TG_MIN_TILES blocks).  The result does not depend on it.
 * dd3d_tower_wgrad: dw_level, dw, q, r (three launches).  dd3d_tower_dgrad: da (one launch; reads g, y, scale, w, da_add only).  Safe
 *   under stream capture.  dd3d_tower_grad_layout: sizeof and field offsets (layout check of the bindings; host only).
 * Rejected (-1, dd3d_last_error starts with the entry point's name): Cin or Cout not a multiple of 32 or above DD3D_TG_MAX_C, pitches
 *   not a multiple of 4 or too small, unknown storages, null pointers, too few slab rows, dgrad_rows outside {0, 2, 4, 8}.
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_TG_MAX_C 256
#define DD3D_TG_UNIT 64
#define DD3D_TG_MIN_UNITS_PER_SLICE 4
#define DD3D_TG_SLAB_BYTES (160ll << 20)
#define DD3D_TG_MIN_TILES 512
typedef struct dd3d_tower_grad_args {       /* host memory; every pointer is device memory */
  const void* x[DD3D_MAX_LEVELS];           /* layer input, storage x_mode */
  const void* y[DD3D_MAX_LEVELS];           /* stored layer output (after the ReLU), storage y_mode */
  const float* g[DD3D_MAX_LEVELS];          /* gradient at y: [B][H][W][g_pitch] */
  const float* scale[DD3D_MAX_LEVELS];      /* [Cout] s_l */
  const float* da_add[DD3D_MAX_LEVELS];     /* [B][H][W][Cin], or all NULL */
  float* da[DD3D_MAX_LEVELS];               /* [B][H][W][Cin] */
  const float* w;                           /* [Cout][3][3][Cin] */
  float* part;                              /* scratch [n_slices][Cout][9 * Cin] */
  float* qpart;                             /* scratch [n_slices][Cout] */
  float* dw_level;                          /* [num_levels][Cout][9 * Cin] */
  float* dw;                                /* [Cout][9 * Cin] */
  float* q;                                 /* [num_levels][Cout] */
  float* r;                                 /* [num_levels][Cout] */
  int32_t H[DD3D_MAX_LEVELS], W[DD3D_MAX_LEVELS];
  int32_t num_levels, B, Cin, Cout, g_pitch;
  int32_t x_mode, x_pitch;                  /* DD3D_PG_ACT_*; floats per pixel (DD3D_PG_ACT_F32) */
  int32_t y_mode, y_pitch;
  int32_t n_slices;                         /* rows of part / qpart */
  int32_t dgrad_rows;
  float x_plane_scale, y_plane_scale;       /* DD3D_PG_ACT_F16X2 */
} dd3d_tower_grad_args;
int dd3d_tower_wgrad(const dd3d_tower_grad_args* args, void* stream);
int dd3d_tower_dgrad(const dd3d_tower_grad_args* args, void* stream);
int64_t dd3d_tower_grad_slices(const dd3d_tower_grad_args* args);
int dd3d_tower_grad_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Backward of the FPN (csrc/fpn_grads.hip): detectron2's FPN.forward with LastLevelP6P7 (DLA-34) or LastLevelP6 (V2-99), fuse type
 * "sum".  G_s: the gradient at the FPN output p_s (the towers' feature<l>; zero for an output DD3D.IN_FEATURES does not select); t_s: the
 * STORED top-down sum of stage s; f_s: the backbone feature; (a, c): layers.fold_norm of a convolution, running statistics (a = 1,
 * c = bias without a norm).
 *   layer         forward                                    backward
 *   P7            p7 = conv3x3s2(relu(p6); W7) + b7          dW7 = sum G7 (x) patches(relu(p6)), db7 = sum G7,
 *                                                            D6 = G6 + [p6 > 0] * dgrad_s2(G7, W7)      (the mask from the STORED p6)
 *   P6            p6 = conv3x3s2(p5; W6) + b6                dW6 = sum D6 (x) patches(p5), db6 = sum D6, D5 = G5 + dgrad_s2(D6, W6)
 *   output conv   p_s = a_s * conv3x3(t_s; Wo_s) + c_s       dWo_s = a_s * sum D_s (x) patches(t_s), q_s = sum D_s, r_s = sum_k P * Wo_s
 *   top-down sum  t_s = lat_s + up2(t_{s+1})                 finest stage: T_s = dgrad(a_s * D_s, Wo_s);
 *                                                            others: T_s = dgrad(a_s * D_s, Wo_s) + pool2x2sum(T_{s-1})
 *   lateral       lat_s = a'_s * (f_s . Wl_s) + c'_s         dWl_s = a'_s * sum T_s (x) f_s, q, r as above, dF_s = (a'_s * T_s) . Wl_s
 * Without P7 D6 = G6; D_s = G_s except on the coarsest stage (D5 of the top-block chain).  P = the unscaled sum (dw_level), so that the
 * norm read-out is the towers' (rstd * (r + (b_conv - mean) * q)).
 *
 * One call covers one convolution per level: k x k (ksize 1 or 3), stride 1 or 2, padding (k - 1) / 2, output size ceil(H / stride),
 * a filter w[l] and a scale[l] per level.  H, W are the INPUT's sizes.  The levels run as separate launches in level order on the stream
 * and share the slab: level l may read what level l - 1 wrote (pool[l] == da[l - 1]: the transposed top-down path in one call).
 *   dw_level[l][n][ky][kx][c] = sum_{b,oy,ox} g_l[b,oy,ox,n] * X_l[b, oy s + ky - p, ox s + kx - p, c]     X = x, or max(x, 0) with in_relu
 *   dw[l] = scale_l[n] * dw_level[l]       q[l][n] = sum g_l       r[l][n] = sum_k dw_level[l][n][k] * w_l[n][k]
 *   da[l][b,y,x,c] = ((((M * sum_{n,ky,kx} scale_l[n] * g_l[b,(y+p-ky)/s,(x+p-kx)/s,n] * w_l[n][ky][kx][c]) + add) + t00) + t01) + t10) + t11
 *     over the taps for which both divisions are exact; M = [mask_l[b,y,x,c] > 0] when mask[l] is set (a masked entry is an exact zero),
 *     `+ add` when add[l] is set, and t_ij = pool[l][b, 2y + i, 2x + j, c] when pool[l] is set, added in exactly this order.
 * Both are GEMMs on v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation): the weight gradient with K = the output pixels of a
 * slice, per-slice partials summed in slice order by a second launch; the input gradient with one fresh accumulator per 32-channel chunk
 * of Cout (its k k 32 terms in (tap, n) order), the chunks added in chunk order.  A zero g enters the input gradient as an exact zero
 * whatever scale holds.  No float atomics, one writer and a fixed order per sum: two runs agree bit for bit, whichever tile is picked.
 * Every word of dw_level, dw, q, r (wgrad) and da (dgrad) of the levels in use is written; nothing beyond them and the slab rows in use.
 *
 * x, mask: DD3D_PG_ACT_* storages (f32 NHWC with a pitch, or split planes of the slice's first chunk).  g: f32 NHWC, pitch g_pitch;
 *   add, pool, da: f32 NHWC, pitch Cin.  part / qpart: dd3d_fpn_grad_slices(args) rows (host only; reads B, H, W, num_levels, Cin, Cout,
 *   ksize, stride: the largest level's count -- units of 64 (stride 2: 32) output pixels of a row, DD3D_FG_MIN_UNITS_PER_SLICE per slice
 *   at least, more once the slab would pass DD3D_FG_SLAB_BYTES).
 * dd3d_fpn_wgrad: three launches per level (reads x, g, w, scale).  dd3d_fpn_dgrad: one launch per level (reads g, w, scale, mask, add,
 *   pool).  Safe under stream capture.  dd3d_fpn_grad_layout: sizeof and field offsets.
 * Rejected (-1, dd3d_last_error starts with the entry point's name): Cin not a multiple of 32 or above DD3D_FG_MAX_CIN, Cout not a
 *   multiple of 32 or above DD3D_FG_MAX_COUT, ksize outside {1, 3}, stride outside {1, 2}, pitches not a multiple of 4 or too small,
 *   unknown storages, null pointers, too few slab rows, a pool tensor that is not exactly twice the level's size, dgrad_rows outside
 *   {0, 2, 4, 8}.
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_FG_MAX_CIN 1024
#define DD3D_FG_MAX_COUT 256
#define DD3D_FG_UNIT 64
#define DD3D_FG_MIN_UNITS_PER_SLICE 4
#define DD3D_FG_SLAB_BYTES (160ll << 20)
#define DD3D_FG_MIN_TILES 512
typedef struct dd3d_fpn_grad_args {         /* host memory; every pointer is device memory */
  const void* x[DD3D_MAX_LEVELS];           /* convolution input [B][H][W], storage x_mode */
  const float* g[DD3D_MAX_LEVELS];          /* gradient at the convolution's output: [B][ceil(H/stride)][ceil(W/stride)][g_pitch] */
  const float* w[DD3D_MAX_LEVELS];          /* [Cout][ksize][ksize][Cin] */
  const float* scale[DD3D_MAX_LEVELS];      /* [Cout] */
  const void* mask[DD3D_MAX_LEVELS];        /* stored tensor of the input's shape, storage mask_mode; or NULL */
  const float* add[DD3D_MAX_LEVELS];        /* [B][H][W][Cin], or NULL */
  const float* pool[DD3D_MAX_LEVELS];       /* [B][pool_H][pool_W][Cin] with pool_H == 2 H, pool_W == 2 W, or NULL */
  float* da[DD3D_MAX_LEVELS];               /* [B][H][W][Cin] */
  float* part;                              /* scratch [n_slices][Cout][ksize * ksize * Cin] */
  float* qpart;                             /* scratch [n_slices][Cout] */
  float* dw_level;                          /* [num_levels][Cout][ksize * ksize * Cin] */
  float* dw;                                /* [num_levels][Cout][ksize * ksize * Cin] */
  float* q;                                 /* [num_levels][Cout] */
  float* r;                                 /* [num_levels][Cout] */
  int32_t H[DD3D_MAX_LEVELS], W[DD3D_MAX_LEVELS];
  int32_t pool_H[DD3D_MAX_LEVELS], pool_W[DD3D_MAX_LEVELS];
  int32_t num_levels, B, Cin, Cout, g_pitch;
  int32_t ksize, stride;
  int32_t in_relu;                          /* weight gradient: rectify the staged input (P7 reads relu(p6)) */
  int32_t x_mode, x_pitch;                  /* DD3D_PG_ACT_*; floats per pixel (DD3D_PG_ACT_F32) */
  int32_t mask_mode, mask_pitch;
  int32_t n_slices;                         /* rows of part / qpart */
  int32_t dgrad_rows;                       /* rows of the input gradient's 16-pixel-wide tile: 2, 4, 8, or 0 = the call chooses */
  float x_plane_scale, mask_plane_scale;    /* DD3D_PG_ACT_F16X2 */
} dd3d_fpn_grad_args;
int dd3d_fpn_wgrad(const dd3d_fpn_grad_args* args, void* stream);
int dd3d_fpn_dgrad(const dd3d_fpn_grad_args* args, void* stream);
int64_t dd3d_fpn_grad_slices(const dd3d_fpn_grad_args* args);
int dd3d_fpn_grad_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Backward of the DLA-34 backbone, level5 down to level2 (csrc/backbone_grads.hip): BasicBlock trees at most two deep without a
 * residual root (dla.py:24-62, 206-247; BackboneLowering._tree).  n(.): the convolution's folded norm (layers.fold_norm, running
 * statistics); every ReLU mask is [stored output > 0], from the tensor the forward left in the plan, in the storage it was left in.
 * A depth-1 tree with input x and output `out`, G_t the gradient at a tensor t BEFORE t's own ReLU mask:
 *   op            forward                                         backward
 *   root          out = relu(n(root . [x2 | x1 | bottom | ...]))   dWr = wgrad([out > 0] G_out, cat), D_cat = dgrad([out > 0] G_out, Wr),
 *                                                                  written once over the whole concat buffer and read by slices
 *   tree2.conv2   x2 = relu(n(conv3x3(mid2)) + x1)                 g2 = [x2 > 0] D_cat[x2]: dW = wgrad(g2, mid2), G_mid2 = dgrad(g2, W)
 *   tree2.conv1   mid2 = relu(n(conv3x3(x1)))                      dW = wgrad([mid2 > 0] G_mid2, x1),
 *                                                                  G_x1 = (D_cat[x1] + [x2 > 0] D_cat[x2]) + dgrad([mid2 > 0] G_mid2, W)
 *   tree1.conv2   x1 = relu(n(conv3x3(mid1)) + residual)           g1 = [x1 > 0] G_x1: dW = wgrad(g1, mid1), G_mid1 = dgrad(g1, W)
 *   project       residual = n(project . bottom)    (no ReLU)      dWp = wgrad(g1, bottom), G_bottom = D_cat[bottom] + dgrad(g1, Wp)
 *                 (the gradient at `residual` is g1: the call masks G_x1 by the stored x1; D_cat[bottom] only under level_root)
 *   tree1.conv1   mid1 = relu(n(conv3x3_s(x)))                     dW = wgrad([mid1 > 0] G_mid1, x),
 *                                                                  stride 2: C_x = F_x + dgrad_s2([mid1 > 0] G_mid1, W)
 *                                                                  stride 1 (bottom = x): G_x = (A_x + g1) + dgrad([mid1 > 0] G_mid1, W)
 *   max-pool      bottom = maxpool2x2(x)            (stride 2)     G_x = C_x + unpool(G_bottom): the window's arg-max receives it
 * F_x: the FPN's gradient at x where x is a backbone output feature (backbone_level<n>), A_x: the root slice of x in an enclosing
 * tree's concat gradient.  A depth-2 tree is [tree1 (depth 1, stride 2, writes t1 into the concat buffer of tree2) ; tree2 (depth 1,
 * stride 1, input t1, root over [x2 | x1 | bottom | t1])]; under level_root the ONE pooled `bottom` is read by tree2's root and by
 * tree1's project: G_bottom = D_cat2[bottom] + dgrad(g1, Wp) goes through the pool backward once.  The order of every sum is the order
 * written here; none uses float atomics.
 *
 * dd3d_backbone_wgrad / dd3d_backbone_dgrad: ONE convolution per call, k x k (ksize 1 or 3), stride 1 or 2, padding (k - 1) / 2, output
 * size ceil(H / stride); H, W are the INPUT's sizes.  With gm = g * [y > 0] (y NULL: gm = g):
 *   dw_level[n][ky][kx][c] = sum_{b,oy,ox} gm[b,oy,ox,n] * x[b, oy s + ky - p, ox s + kx - p, c]     (zero padding; not scaled)
 *   dw = scale[n] * dw_level        q[n] = sum gm        r[n] = sum_k dw_level[n][k] * w[n][k]
 *   da[b,y,x,c] = (add[b,y,x,c] + res_g[b,y,x,c] * [res_y[b,y,x,c] > 0]) + sum_{n,ky,kx} scale[n] * gm[b,(y+p-ky)/s,(x+p-kx)/s,n] * w[n][ky][kx][c]
 *     over the taps for which both divisions are exact; `add` and the res pair are optional (either alone is added to the sum as is).
 * the same quantities as the towers' and the FPN's: the norm read-out is theirs (rstd * (r + (b_conv - mean) * q)).  Both are GEMMs on
 * v_mfma_f32_32x32x2_f32 (exact f32 products, f32 accumulation): the weight gradient with per-slice partials summed in slice order; the
 * input gradient with one fresh accumulator per 32-channel chunk of Cout (k k 32 terms in (tap, n) order), the chunks added in chunk
 * order.  A zero or masked g enters the input gradient as an exact zero whatever scale holds.  One writer and a fixed order per sum: two
 * runs agree bit for bit, whichever tile is picked.  Every word of dw_level, dw, q, r (wgrad) and of the Cin channels of da (dgrad) is
 * written; nothing beyond them and the slab rows in use -- the other channels of a wider da buffer keep what they held.
 *
 * Every activation and gradient operand may be a channel slice of a wider buffer: f32 NHWC is a pointer at the slice's first channel
 *   and the buffer's pitch; split planes are the pointer at the slice's first 32-channel chunk image (slices start on chunk boundaries).
 *   x, y, res_y: DD3D_PG_ACT_* storages.  g, add, res_g, da: f32 NHWC with pitches g_pitch, add_pitch, res_pitch, da_pitch.
 * part / qpart: dd3d_backbone_grad_slices(args) rows (host only; reads B, H, W, Cin, Cout, ksize, stride): units of 64 (stride 2: 32)
 *   output pixels of a row, DD3D_BG_MIN_UNITS_PER_SLICE per slice at least, more once the slab would pass DD3D_TG_SLAB_BYTES.
 * dgrad_rows / dgrad_group: rows (2, 4, 8) and input channels (128, 256) of the input gradient's block; 0 lets the call choose: the
 *   largest of (8, 256), (4, 256), (2, 256) that gives DD3D_BG_MIN_TILES blocks, else (2, 128).  The result does not depend on them.
 * dd3d_backbone_wgrad: three launches (reads x, y, g, w, scale).  dd3d_backbone_dgrad: one launch (reads y, g, w, scale, add, res_g,
 *   res_y).  Safe under stream capture.
 *
 * dd3d_maxpool2x2_backward: da[b, 2y+i, 2x+j, c] = (add[...] or nothing) + (g'[b,y,x,c] if (i, j) is the window's arg-max else 0) with
 *   g' = g, or g + res_g * [res_y > 0] (res_g alone when g is NULL): a strided tree without a project, whose pooled tensor is the block's
 *   residual (max-pool row of the table: G_bottom = D_cat[bottom] + g1; it does not occur in DLA-34).  The arg-max is recomputed from the stored input x (H x W, both even, any DD3D_PG_ACT_* storage); among equal maxima the first in the
 *   order (0,0), (0,1), (1,0), (1,1) wins (torch's max_pool2d backward on the CPU).  One launch.
 * dd3d_backbone_grad_layout: sizeof and field offsets of both structs.
 * Rejected (-1, dd3d_last_error starts with the entry point's name): Cin not a multiple of 32 or above DD3D_BG_MAX_CIN, Cout not a
 *   multiple of 32 or above DD3D_BG_MAX_COUT, ksize outside {1, 3}, stride outside {1, 2}, pitches not a multiple of 4 or too small,
 *   unknown storages, null pointers, res_g without res_y, too few slab rows, dgrad_rows outside {0, 2, 4, 8}, dgrad_group outside
 *   {0, 128, 256}, more than DD3D_BG_MAX_PIXELS input pixels (B * H * W; the stride-2 level1 tensor of the 6 x 896 x 1600 nuScenes sample
 *   has 2.15 million); the pool: odd sizes, C not a multiple of 32, the same pixel limit.
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_BG_MAX_CIN 1280
#define DD3D_BG_MAX_COUT 512
#define DD3D_BG_UNIT 64
#define DD3D_BG_MIN_UNITS_PER_SLICE 4
#define DD3D_BG_MIN_TILES 512               /* two blocks per CU of 256; chosen like DD3D_FG_MIN_TILES, not measured */
#define DD3D_BG_MAX_PIXELS (1l << 26)       /* B * H * W of a call's input: pixel, unit and block counts stay ints; words are longs */
typedef struct dd3d_backbone_grad_args {    /* host memory; every pointer is device memory */
  const void* x;                            /* convolution input [B][H][W], storage x_mode */
  const void* y;                            /* stored output behind the ReLU [B][Ho][Wo], storage y_mode; NULL: no ReLU (project) */
  const float* g;                           /* gradient at the output: [B][Ho][Wo][g_pitch] */
  const float* w;                           /* [Cout][ksize][ksize][Cin] */
  const float* scale;                       /* [Cout] */
  const float* add;                         /* [B][H][W][add_pitch], or NULL */
  const float* res_g;                       /* [B][H][W][res_pitch], or NULL: a gradient masked by res_y before it is added */
  const void* res_y;                        /* stored tensor of the input's shape, storage res_y_mode (set with res_g) */
  float* da;                                /* [B][H][W][da_pitch] */
  float* part;                              /* scratch [n_slices][Cout][ksize * ksize * Cin] */
  float* qpart;                             /* scratch [n_slices][Cout] */
  float* dw_level;                          /* [Cout][ksize * ksize * Cin] */
  float* dw;                                /* [Cout][ksize * ksize * Cin] */
  float* q;                                 /* [Cout] */
  float* r;                                 /* [Cout] */
  int32_t B, H, W, Cin, Cout, ksize, stride;
  int32_t g_pitch, add_pitch, res_pitch, da_pitch;
  int32_t x_mode, x_pitch;                  /* DD3D_PG_ACT_*; floats per pixel (DD3D_PG_ACT_F32) */
  int32_t y_mode, y_pitch;
  int32_t res_y_mode, res_y_pitch;
  int32_t n_slices;                         /* rows of part / qpart */
  int32_t dgrad_rows, dgrad_group;
  float x_plane_scale, y_plane_scale, res_y_plane_scale;  /* DD3D_PG_ACT_F16X2 */
} dd3d_backbone_grad_args;
typedef struct dd3d_pool_grad_args {        /* host memory; every pointer is device memory */
  const void* x;                            /* the pool's stored input [B][H][W], storage x_mode */
  const float* g;                           /* gradient at the pooled tensor: [B][H/2][W/2][g_pitch]; NULL with res_g alone */
  const float* res_g;                       /* [B][H/2][W/2][res_pitch] or NULL: a second part, masked by res_y before it is added */
  const void* res_y;                        /* stored tensor [B][H/2][W/2], storage res_y_mode (set with res_g) */
  const float* add;                         /* [B][H][W][add_pitch], or NULL */
  float* da;                                /* [B][H][W][da_pitch] */
  int32_t B, H, W, C;
  int32_t x_mode, x_pitch;
  int32_t res_y_mode, res_y_pitch;
  int32_t g_pitch, res_pitch, add_pitch, da_pitch;
  float x_plane_scale, res_y_plane_scale;
} dd3d_pool_grad_args;
int dd3d_backbone_wgrad(const dd3d_backbone_grad_args* args, void* stream);
int dd3d_backbone_dgrad(const dd3d_backbone_grad_args* args, void* stream);
int64_t dd3d_backbone_grad_slices(const dd3d_backbone_grad_args* args);
int dd3d_maxpool2x2_backward(const dd3d_pool_grad_args* args, void* stream);
int dd3d_backbone_grad_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Backward of the DLA-34 stem's convolutions (csrc/stem_grads.hip): base_layer (7 x 7 on the normalised four-channel image), level0.0
 * (3 x 3) and level1.0 (3 x 3, stride 2), each conv + folded norm + ReLU with ONE consumer.  The contract and the quantities are
 * dd3d_backbone_wgrad's / dd3d_backbone_dgrad's above (gm, dw_level, dw, q, r, da, the norm read-out, H and W the INPUT's sizes, padding
 * (k - 1) / 2, output size ceil(H / stride)) with these differences:
 *   shapes   (ksize, stride, Cin, Cout) in {(7, 1, 4, 16), (3, 1, 16, 16), (3, 2, 16, 32)}; dd3d_stem_dgrad takes the two 3 x 3 only (the
 *            image has no gradient).  The 7 x 7 reads four channels per pixel; dw's column of channel 3 is computed like the others.
 *   operands x, g, da: f32 NHWC with pitches x_pitch, g_pitch, da_pitch (dgrad: g 16-byte aligned).  y: any DD3D_PG_ACT_* storage, always
 *            present (every stem layer has a ReLU).
 *   da       = sum_{n,ky,kx} scale[n] * gm * w alone: a stem tensor has one consumer, there is no `add` and no residual pair.
 * Both are GEMMs on v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulation).  The weight gradient: per-slice partials in `part` /
 * `qpart`; a slice is dd3d_stem_grad_slices' run of units of up to DD3D_SG_UNIT output pixels of a row -- as many units as give about
 * DD3D_SG_TARGET_SLICES slices, between DD3D_SG_MIN_UNITS_PER_SLICE and DD3D_SG_MAX_UNITS_PER_SLICE, more once the slab would pass
 * DD3D_TG_SLAB_BYTES; inside a slice four runs of every fourth unit, added as (0 + 2) + (1 + 3); the slices are summed in slice order,
 * 64 to a sub-sum.  The slicing depends on the shape alone.  wgrad_blocks: blocks of the weight gradient's main launch (0: one per slice;
 * fewer: a block walks several slices); the result does not depend on it.  The input gradient: one chain per output word, (tap, n) order
 * within the taps that reach it -- the stride-2 call visits the 4 / 2 / 2 / 1 taps of an input pixel's (row, column) parity only.
 * One writer and a fixed order per sum: two runs agree bit for bit.  Every word of dw_level, dw, q, r (wgrad) and of the Cin channels of
 * da (dgrad) is written; nothing beyond them and the slab rows in use.  dd3d_stem_wgrad: three launches; dd3d_stem_dgrad: one.  Safe
 * under stream capture.  dd3d_stem_grad_slices: host only, reads B, H, W, Cin, Cout, ksize, stride.  dd3d_stem_grad_layout: sizeof and
 * field offsets.
 * Rejected (-1, dd3d_last_error starts with the entry point's name): any other (ksize, stride, Cin, Cout), the 7 x 7 in dgrad, pitches
 *   not a multiple of 4 or too small, an unknown y storage, null pointers, a misaligned g (dgrad), too few slab rows, a negative
 *   wgrad_blocks, more than DD3D_BG_MAX_PIXELS input pixels.
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_SG_UNIT 64
#define DD3D_SG_TARGET_SLICES 512           /* two blocks per CU of 256; not measured */
#define DD3D_SG_MIN_UNITS_PER_SLICE 8
#define DD3D_SG_MAX_UNITS_PER_SLICE 64
typedef struct dd3d_stem_grad_args {        /* host memory; every pointer is device memory */
  const float* x;                           /* convolution input [B][H][W][x_pitch] (wgrad) */
  const void* y;                            /* stored output behind the ReLU [B][Ho][Wo], storage y_mode */
  const float* g;                           /* gradient at the output: [B][Ho][Wo][g_pitch] */
  const float* w;                           /* [Cout][ksize][ksize][Cin] */
  const float* scale;                       /* [Cout] */
  float* da;                                /* [B][H][W][da_pitch] (dgrad) */
  float* part;                              /* scratch [n_slices][Cout][ksize * ksize * Cin] */
  float* qpart;                             /* scratch [n_slices][Cout] */
  float* dw_level;                          /* [Cout][ksize * ksize * Cin] */
  float* dw;                                /* [Cout][ksize * ksize * Cin] */
  float* q;                                 /* [Cout] */
  float* r;                                 /* [Cout] */
  int32_t B, H, W, Cin, Cout, ksize, stride;
  int32_t x_pitch, g_pitch, da_pitch;
  int32_t y_mode, y_pitch;                  /* DD3D_PG_ACT_*; floats per pixel (DD3D_PG_ACT_F32) */
  int32_t n_slices;                         /* rows of part / qpart */
  int32_t wgrad_blocks;
  float y_plane_scale;                      /* DD3D_PG_ACT_F16X2 */
} dd3d_stem_grad_args;
int dd3d_stem_wgrad(const dd3d_stem_grad_args* args, void* stream);
int dd3d_stem_dgrad(const dd3d_stem_grad_args* args, void* stream);
int64_t dd3d_stem_grad_slices(const dd3d_stem_grad_args* args);
int dd3d_stem_grad_layout(int64_t* out, int32_t n);
/* The VoVNet-V2 stem's first convolution (vovnet.py stem_1: 3 x 3, stride 2, padding 1, the normalised four-channel image -> 64 channels,
 * folded norm, ReLU) has the same weight gradient through entry points of its own, on the same struct (layout unchanged):
 *   shape    (ksize, stride, Cin, Cout) = (3, 2, 4, 64) alone.  There is no input gradient: the image has none.
 * The contract is dd3d_stem_wgrad's, word for word: exact f32 products on v_mfma_f32_16x16x4_f32; g masked by the stored output y (any
 * DD3D_PG_ACT_* storage) while it is loaded; per-slice partials in `part` / `qpart`; the slicing depends on the shape alone -- units of up
 * to DD3D_SG_UNIT output pixels of a row, the same target / minimum / maximum / slab rule (dd3d_vovnet_stem_grad_slices); the four waves
 * added as (0 + 2) + (1 + 3); the slices summed in slice order, 64 to a sub-sum; dw_level, dw = scale * dw_level, q and r as above.  A B
 * operand holds the three taps kx of a filter row times four channels, the fourth tap slot unused; dw's column of channel 3 is computed
 * like the others.  No float atomics, one writer per word: two runs agree bit for bit, whatever wgrad_blocks holds.  Every word of
 * dw_level, dw, q and r is written; nothing beyond them and the slab rows in use.  Three launches.  Safe under stream capture.
 * dd3d_vovnet_stem_grad_slices: host only, reads B, H, W, Cin, Cout, ksize, stride.
 * Rejected (-1, dd3d_last_error starts with the entry point's name): any other (ksize, stride, Cin, Cout) -- the DLA stem's three shapes
 *   included, as dd3d_stem_wgrad / dd3d_stem_grad_slices keep rejecting this one --, pitches not a multiple of 4 or too small, an unknown
 *   y storage, null pointers, too few slab rows, a negative wgrad_blocks, more than DD3D_BG_MAX_PIXELS input pixels. */
int dd3d_vovnet_stem_wgrad(const dd3d_stem_grad_args* args, void* stream);
int64_t dd3d_vovnet_stem_grad_slices(const dd3d_stem_grad_args* args);

/* ------------------------------------------------------------------------------------------------
 * Backward of the VoVNet-V2 backbone, stage5 down to stem_1 (csrc/vovnet_grads.hip; stem_1's call: csrc/stem_grads.hip, above; the wide
 * convolution entry points live beside the kernels they launch in csrc/backbone_grads.hip): the specs whose channel counts are multiples of 32 (V-19-eSE, V-39-eSE, V-57-eSE,
 * V-99-eSE; vovnet.py:188-273; BackboneLowering._vovnet).  n(.), the ReLU masks and G_t as in the DLA section.  One OSA module with input
 * x, concat buffer cat = [x | l0 | .. | l(n-1)], pre-eSE tensor xt and output `out`:
 *   op        forward                                       backward
 *   eSE       out = xt * s (+ x under `identity`)           dd3d_ese_backward: G_xt, d fc_w, d fc_b (below); under identity G_out also
 *             s = hsigmoid(fc_w . mean_hw(xt) + fc_b)       reaches x (module input row)
 *   concat    xt = relu(n(concat1x1 . cat))                 dWc = wgrad([xt > 0] G_xt, cat), D_cat = dgrad([xt > 0] G_xt, Wc), written once
 *                                                           over the whole concat width and read by slices
 *   layer i   l_i = relu(n(conv3x3(l_(i-1))))  (l_(-1) = x)  g_i = [l_i > 0] G_li: dW_i = wgrad(g_i, l_(i-1)),
 *                                                           i > 0: G_l(i-1) = D_cat[l_(i-1)] + dgrad(g_i, W_i)        (G_l(n-1) = D_cat[l_(n-1)])
 *   input                                                   G_x = (D_cat[x] + G_out) + dgrad(g_0, W_0) under identity, else D_cat[x] + dgrad(g_0, W_0);
 *                                                           the three terms: one elementwise launch T = D_cat[x] + G_out (dd3d_vovnet_add),
 *                                                           then T is layer 0's `add`
 *   max-pool  x = maxpool3x3s2_ceil(prev stage's out)       G_prev_out = F_prev_out + the gathered window gradients (dd3d_maxpool3x3s2_ceil_backward)
 *   stem_3    cat2[x] = relu(n(conv3x3_s2(stem_2 out)))     dW = wgrad([x > 0] G_x, stem_2 out), G_stem2 = dgrad_s2([x > 0] G_x, W)
 *   stem_2    stem_2 out = relu(n(conv3x3(stem_1 out)))     dW = wgrad([. > 0] G_stem2, stem_1 out), G_stem1 = dgrad(.) -- not masked by stem_1's
 *                                                           own ReLU
 *   stem_1    stem_1 out = relu(n(conv3x3_s2(image)))       dW = wgrad([stem_1 out > 0] G_stem1, image) (dd3d_vovnet_stem_wgrad above); the image
 *                                                           has no gradient
 * F_t: the FPN's gradient at a stage output.  The order of every sum is the order written here; none uses float atomics.
 *
 * dd3d_vovnet_conv_wgrad / dd3d_vovnet_conv_dgrad / dd3d_vovnet_conv_grad_slices: dd3d_backbone_wgrad / dd3d_backbone_dgrad /
 *   dd3d_backbone_grad_slices -- the same arguments, kernels, sums, orders, slab rule, tile choice and rejections -- with the limits
 *   Cin <= DD3D_VG_MAX_CIN and Cout <= DD3D_VG_MAX_COUT (multiples of 32).  The kernels themselves are untouched: a module input's third
 *   term is summed beforehand by
 * dd3d_vovnet_add: out[p][c] = a[p][c] + b[p][c] over npix pixels and C channels (a multiple of 4), f32 NHWC with pitches (multiples of 4,
 *   16-byte aligned pointers); operands may be channel slices of wider buffers.  One launch, thread = (pixel, four channels); every word
 *   of the C channels of out is written.
 *
 * dd3d_ese_backward: with m[b][c] = (sum_hw xt[b,hw,c]) / HW, z[b][c] = sum_ci fc_w[c][ci] * m[b][ci] + fc_b[c], s = clamp(z + 3, 0, 6) / 6:
 *     ds[b][c] = sum_hw g[b,hw,c] * xt[b,hw,c]           dz = ds / 6 where -3 < z < 3, else an exact 0
 *     u[b][c]  = (sum_co fc_w[co][c] * dz[b][co]) / HW    g_xt[b,hw,c] = g[b,hw,c] * s[b][c] + u[b][c]      (not masked by xt's own ReLU)
 *     d_fc_w[co][ci] = sum_b dz[b][co] * m[b][ci]         d_fc_b[co] = sum_b dz[b][co]
 *   m and z are recomputed from the stored xt (any DD3D_PG_ACT_* storage) in the pass that forms ds; nothing of the forward's workspace is
 *   read.  Four launches: (1) block = (32 channels, row split rs of `rsplit`, image): the rows rs * ceil(HW / rsplit) .. of the split, eight
 *   row lanes of every eighth row each, the lanes added in lane order -> part[b][rs][{sum xt, sum g xt}][c]; (2) block = (four channels
 *   co, image), a wave per co: the splits in split order -> m, ds; z over ci by lanes of every 64th ci, then a butterfly over the lanes (the
 *   forward gate's order) -> m, z, s, dz; (3) thread = (co, ci): d_fc_w over b in image order; thread = (b, c): u in chunks of 32 co, a
 *   fresh sum per chunk, the chunks added in chunk order; thread = co: d_fc_b over b; (4) thread = (pixel, four channels): g_xt.  One
 *   writer and a fixed order per sum: two runs agree bit for bit.  Written: every word of part's rows in use, m, z, s, dz, u ([B][C] each),
 *   d_fc_w, d_fc_b and the C channels of g_xt; nothing beyond them.  Safe under stream capture.
 *   Rejected (-1, the message starts with the entry point's name): C not a multiple of 32 or above DD3D_VG_MAX_COUT, rsplit outside
 *   1 .. DD3D_EG_MAX_RSPLIT, pitches not a multiple of 4 or too small, an unknown storage, null pointers, B * HW above DD3D_BG_MAX_PIXELS.
 *
 * dd3d_maxpool3x3s2_ceil_backward: the backward of MaxPool2d(3, 2, ceil_mode=True) (dd3d_maxpool3x3s2_ceil_nhwc) as a gather.  Output
 *   sizes: Ho = ceil((H - 3) / 2) + 1, minus one when the last window would start outside the map ((Ho - 1) * 2 >= H); Wo alike.  Window
 *   (oy, ox) covers the rows 2 oy .. min(2 oy + 2, H - 1) and the columns alike (clipped at the border, no padding); its arg-max is
 *   recomputed from the stored input x (any DD3D_PG_ACT_* storage); among equal maxima the first in row-major window order wins (torch's
 *   max_pool2d on the CPU).  thread = (input pixel, channel): v = add[b,y,x,c] (or nothing), then for the at most 2 x 2 windows that
 *   contain the pixel, in ascending (oy, ox): v += g[b,oy,ox,c] where the pixel is that window's arg-max.  Without `add` the sum starts
 *   at 0: bit for bit torch's CPU backward.  One launch; every word of the C channels of da is written.  H, W >= 3.
 *   Rejected: H or W below 3, C not a multiple of 32 or above DD3D_VG_MAX_COUT, pitches, storages, null pointers, the pixel limit.
 * dd3d_vovnet_grad_layout: sizeof and field offsets of both structs.
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_VG_MAX_CIN 2144                /* the concat 1x1 of stage5: 1024 + 5 * 224 */
#define DD3D_VG_MAX_COUT 1024
#define DD3D_EG_MAX_RSPLIT 64
typedef struct dd3d_ese_grad_args {         /* host memory; every pointer is device memory */
  const void* xt;                           /* the stored pre-eSE tensor [B][HW], storage xt_mode */
  const float* g;                           /* gradient at the module output: [B][HW][g_pitch] */
  const float* fc_w;                        /* [C][C] */
  const float* fc_b;                        /* [C] */
  float* part;                              /* scratch [B][rsplit][2][C] */
  float* m;                                 /* [B][C] */
  float* z;                                 /* [B][C] */
  float* s;                                 /* [B][C] */
  float* dz;                                /* [B][C] */
  float* u;                                 /* [B][C] */
  float* g_xt;                              /* [B][HW][gxt_pitch] */
  float* d_fc_w;                            /* [C][C] */
  float* d_fc_b;                            /* [C] */
  int32_t B, HW, C, rsplit;
  int32_t xt_mode, xt_pitch;                /* DD3D_PG_ACT_*; floats per pixel (DD3D_PG_ACT_F32) */
  int32_t g_pitch, gxt_pitch;
  float xt_plane_scale;                     /* DD3D_PG_ACT_F16X2 */
  int32_t reserved;                         /* 0; ignored */
} dd3d_ese_grad_args;
typedef struct dd3d_pool3_grad_args {       /* host memory; every pointer is device memory */
  const void* x;                            /* the pool's stored input [B][H][W], storage x_mode */
  const float* g;                           /* gradient at the pooled tensor: [B][Ho][Wo][g_pitch] */
  const float* add;                         /* [B][H][W][add_pitch], or NULL */
  float* da;                                /* [B][H][W][da_pitch] */
  int32_t B, H, W, C;
  int32_t x_mode, x_pitch;
  int32_t g_pitch, add_pitch, da_pitch;
  float x_plane_scale;
} dd3d_pool3_grad_args;
int dd3d_vovnet_conv_wgrad(const dd3d_backbone_grad_args* args, void* stream);
int dd3d_vovnet_conv_dgrad(const dd3d_backbone_grad_args* args, void* stream);
int64_t dd3d_vovnet_conv_grad_slices(const dd3d_backbone_grad_args* args);
int dd3d_vovnet_add(const float* a, const float* b, float* out, int64_t npix, int32_t C, int32_t a_pitch, int32_t b_pitch, int32_t out_pitch,
                    void* stream);
int dd3d_ese_backward(const dd3d_ese_grad_args* args, void* stream);
int dd3d_maxpool3x3s2_ceil_backward(const dd3d_pool3_grad_args* args, void* stream);
int dd3d_vovnet_grad_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Batch-statistics BatchNorm of one head-tower layer, forward and backward (csrc/tower_bn.hip): what nn.BatchNorm2d computes in
 * train() behind the tower's shared 3x3 convolution (fcos2d.py:71-93; ModuleListDial: one norm per pyramid level).  A SEGMENT is one
 * (tower, level) pair of the layer: N = B * h * w pixels of the padded canvas, C channels, statistics per channel over the N pixels.
 * With c the raw convolution output (f32 NHWC, conv bias included when the module has one):
 *   mu = sum(c) / N            v = sum((c - mu)^2) / N                   two passes over c, not E[c^2] - mu^2
 *   rstd = 1 / sqrt(v + eps)   s = gamma * rstd      t = beta - mu * s
 *   y = relu(fmaf(c - mu, s, beta))                                        (= c * s + t without the cancellation between c * s and
 *                                                                           mu * s: a channel constant over the batch gives relu(beta))
 *   running_mean' = (1 - momentum) * running_mean + momentum * mu
 *   running_var'  = (1 - momentum) * running_var  + momentum * v * N / (N - 1)       (read-outs: the inputs are never written)
 * and with G the gradient at y, ghat = G * [stored y > 0] and xhat = (c - mu) * rstd:
 *   q = sum(ghat)     p = sum(ghat * xhat)                               (= d beta, d gamma)
 *   G_c = s * (ghat - q / N - xhat * p / N)                              dense: the ReLU mask does not survive
 * Order of every sum (mu, v, q, p alike): the segment's pixels are cut into slices of DD3D_BN_SLICE consecutive pixels.  Inside a slice
 * a channel has P = 256 / (C / 4) running sums (thread lanes); lane j adds pixels j, j + P, j + 2P, ... in that order, the lanes are
 * added in lane order.  The slice partials (one scratch row each, one writer) are added by a second launch: eight lanes, lane j adds
 * slices j, j + 8, ... in that order (fetched four at a time), the lanes are added in lane order.  No float atomics; two runs agree bit for bit.
 *
 * c, g, gc: f32 NHWC, pitches c_pitch, g_pitch, C, pointers at the segment's first channel.  stats: [DD3D_BN_STAT_ROWS][C] per segment, rows
 *   DD3D_BN_ROW_*.  qp: [2][C] per segment (q, then p).  part: scratch [n_slices][2][C], n_slices >= dd3d_bn_slices(args) (host only; it
 *   reads num_segs, C and N alone): sum over the segments of ceil(N / DD3D_BN_SLICE).
 * dd3d_bn_batch_stats (four launches: slice sums, mu, slice sums of squared deviations, the rest): every word of `stats`; reads c, gamma,
 *   beta, run_mean, run_var.
 * dd3d_bn_apply_relu_split (one launch): y from c, beta and stats rows MU, S, as split planes of `math_mode` ([C/32][N][NP][32] 16-bit terms, first
 *   chunk of the slice; DD3D_MATH_F16X2: halves of value * plane_scale, |value * plane_scale| > 65504 or a NaN ORs DD3D_STATUS_F16_OVERFLOW
 *   into `status`, exactly as dd3d_split_planes) or, math_mode DD3D_MATH_F32, as f32 NHWC of pitch y_pitch.
 * dd3d_bn_backward_reduce (two launches): qp; reads c, g, the stored y (storage y_mode, DD3D_PG_ACT_*), stats rows MU, RSTD.
 * dd3d_bn_backward_apply (one launch): gc; reads c, g, y, qp and stats rows MU, RSTD, S.
 * All are safe under stream capture and write nothing beyond the outputs named and the scratch rows in use.
 * dd3d_tower_bn_layout: sizeof and field offsets (layout check of the bindings; host only).
 * Rejected (-1, dd3d_last_error starts with the entry point's name): num_segs outside 1 .. DD3D_BN_MAX_SEGS, C not a multiple of 32 or above
 *   DD3D_BN_MAX_C, pitches not a multiple of 4 or below C, null pointers, N < 2, too few scratch rows, unknown storages.
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_BN_MAX_SEGS 24
#define DD3D_BN_MAX_C 256
#define DD3D_BN_SLICE 64
#define DD3D_BN_STAT_ROWS 7
#define DD3D_BN_ROW_MU 0
#define DD3D_BN_ROW_VAR 1
#define DD3D_BN_ROW_S 2
#define DD3D_BN_ROW_T 3
#define DD3D_BN_ROW_RSTD 4
#define DD3D_BN_ROW_RUN_MEAN 5
#define DD3D_BN_ROW_RUN_VAR 6
typedef struct dd3d_tower_bn_args {         /* host memory; every pointer is device memory */
  const float* c[DD3D_BN_MAX_SEGS];         /* raw convolution output: [N][c_pitch] */
  const float* gamma[DD3D_BN_MAX_SEGS];     /* [C] norm weight */
  const float* beta[DD3D_BN_MAX_SEGS];      /* [C] norm bias */
  const float* run_mean[DD3D_BN_MAX_SEGS];  /* [C] running statistics before the step (read only) */
  const float* run_var[DD3D_BN_MAX_SEGS];
  float* stats[DD3D_BN_MAX_SEGS];           /* [DD3D_BN_STAT_ROWS][C] */
  void* y[DD3D_BN_MAX_SEGS];                /* the layer's output: written by the apply, read by the backward */
  const float* g[DD3D_BN_MAX_SEGS];         /* gradient at y: [N][g_pitch] */
  float* qp[DD3D_BN_MAX_SEGS];              /* [2][C]: q, p */
  float* gc[DD3D_BN_MAX_SEGS];              /* gradient at c: [N][C] */
  float* part;                              /* scratch [n_slices][2][C] */
  int32_t* status;                          /* DD3D_STATUS_* word, or NULL */
  int32_t N[DD3D_BN_MAX_SEGS];              /* pixels of the segment */
  int32_t num_segs, C, c_pitch, g_pitch;
  int32_t math_mode;                        /* apply: DD3D_MATH_* of the planes written, DD3D_MATH_F32: f32 NHWC */
  int32_t y_mode, y_pitch;                  /* backward: DD3D_PG_ACT_* of the stored y; floats per pixel of an f32 y (both directions) */
  int32_t n_slices;                         /* rows of part */
  float eps, momentum, plane_scale;         /* plane_scale: DD3D_MATH_F16X2 / DD3D_PG_ACT_F16X2 */
  int32_t reserved;                         /* 0; ignored */
} dd3d_tower_bn_args;
int dd3d_bn_batch_stats(const dd3d_tower_bn_args* args, void* stream);
int dd3d_bn_apply_relu_split(const dd3d_tower_bn_args* args, void* stream);
int dd3d_bn_backward_reduce(const dd3d_tower_bn_args* args, void* stream);
int dd3d_bn_backward_apply(const dd3d_tower_bn_args* args, void* stream);
int64_t dd3d_bn_slices(const dd3d_tower_bn_args* args);
int dd3d_tower_bn_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Batch-statistics BatchNorm of the FPN's lateral and output convolutions (csrc/fpn_bn.hip): nn.BatchNorm2d in train() behind a
 * convolution WITHOUT a ReLU, and, for the laterals, detectron2's top-down path prev = lateral + interpolate(prev, x2, nearest).  A
 * SEGMENT is one pyramid stage: N = B * H * W pixels of the padded canvas.  The statistics are dd3d_bn_batch_stats' (above), one call
 * over all stages.  With n_l(b, y, x) = fmaf(c_l - mu_l, s_l, beta_l) of segment l at its own pixel:
 *   unlinked segment (up[l] = -1):   y_l = n_l
 *   linked chain l -> u1 = up[l] -> u2 = up[u1] -> ... -> uk (up[uk] = -1), every link an exact halving of H and W:
 *     y_l(b, y, x) = (...((n_uk(b, y >> k, x >> k) + n_u(k-1)(b, y >> (k-1), x >> (k-1))) + ...) + n_u1(b, y >> 1, x >> 1)) + n_l(b, y, x)
 *   the COARSEST term first, every coarser term recomputed from that segment's raw c: the float32 value of the reference's
 *   recurrence (float addition commutes: n4 + up(n5) == n5 + n4), in one launch, with no dependence between segments and without
 *   reading a rounded stored sum.  No ReLU: negative values are stored.
 * and with G the gradient at y_l's norm output (for a lateral: at the stored sum, which passes it on unchanged):
 *   q = sum(G)   p = sum(G * xhat)   G_c = s * (G - q / N - xhat * p / N)            xhat = (c - mu) * rstd
 *   -- dd3d_bn_backward_reduce / _apply (above) without the mask: same slices, same order of every sum, same scratch rows, and the
 *   bits those return for a stored y of ones; y, y_mode, y_pitch and plane_scale are not read.
 * dd3d_bn_apply_topdown_split (one launch, thread = (pixel, 8 channels), 16-byte loads and stores, one writer per word): y of every
 *   segment from bn.c, bn.beta and bn.stats rows MU, S, stored as dd3d_bn_apply_relu_split stores: split planes of bn.math_mode in
 *   bn.y (DD3D_MATH_F16X2: halves of value * plane_scale; |value * plane_scale| > 65504 or a NaN ORs DD3D_STATUS_F16_OVERFLOW into
 *   bn.status) or, DD3D_MATH_F32, f32 NHWC of pitch bn.y_pitch.  y32[l] (optional, split-plane modes): an f32 NHWC copy, pitch y32_pitch.
 *   Segments are ordered finest to coarsest within a chain: up[l] is -1 or an index above l.
 * dd3d_bn_backward_reduce_linear (two launches): qp; reads c, g, stats rows MU, RSTD.
 * dd3d_bn_backward_apply_linear (one launch): gc; reads c, g, qp and stats rows MU, RSTD, S.
 * All are safe under stream capture and write nothing beyond the outputs named and the scratch rows in use.  No float atomics.
 * dd3d_fpn_bn_layout: sizeof and field offsets (layout check of the bindings; host only).
 * Rejected (-1, dd3d_last_error starts with the entry point's name): what the tower entry points reject, and for the apply a segment
 *   whose N is not B * H * W, a link that is not above its segment or below num_segs, a linked segment that is not exactly twice its
 *   coarser one in H and W or differs in B, a y32 pitch that is not a multiple of 4 or below C.
 * ------------------------------------------------------------------------------------------------ */
typedef struct dd3d_fpn_bn_args {     /* host memory; every pointer is device memory */
  dd3d_tower_bn_args bn;              /* c, beta, stats, y, status, N, num_segs, C, c_pitch, math_mode, y_pitch, plane_scale */
  float* y32[DD3D_BN_MAX_SEGS];       /* optional f32 copy of y: [N][y32_pitch] */
  int32_t up[DD3D_BN_MAX_SEGS];       /* the segment's coarser segment, or -1 */
  int32_t B[DD3D_BN_MAX_SEGS], H[DD3D_BN_MAX_SEGS], W[DD3D_BN_MAX_SEGS];
  int32_t y32_pitch;
  int32_t reserved;                   /* 0; ignored */
} dd3d_fpn_bn_args;
int dd3d_bn_apply_topdown_split(const dd3d_fpn_bn_args* args, void* stream);
int dd3d_bn_backward_reduce_linear(const dd3d_tower_bn_args* args, void* stream);
int dd3d_bn_backward_apply_linear(const dd3d_tower_bn_args* args, void* stream);
int dd3d_fpn_bn_layout(int64_t* out, int32_t n);

/* ------------------------------------------------------------------------------------------------
 * Batch-statistics BatchNorm of the DLA-34 bottom-up network (csrc/backbone_bn.hip): nn.BatchNorm2d in train() behind every convolution
 * of base_layer, level0, level1 and the trees (dla.py:24-62, 146-167, 271-280).  A SEGMENT is one norm: N = B * h * w pixels of the
 * padded canvas, C channels.  The mathematics is the towers' (above): mu, v in two passes, rstd, s, t, the running-statistics read-outs,
 * n = fmaf(c - mu, s, beta).  What differs is the width -- C = DD3D_BBN_MIN_C (16: the stem), a multiple of 32 up to 256, or a multiple
 * of 256 up to DD3D_BBN_MAX_C (512: level5) -- and what follows the norm:
 *   act DD3D_BBN_RELU      y = relu(n)                       conv1 of a block, root.conv, the stem layers
 *   act DD3D_BBN_LINEAR    y = n                             project (negative values are stored)
 *   act DD3D_BBN_RESIDUAL  y = relu(n + r)                   conv2 of a BasicBlock; r the stored residual at the same pixel and channel,
 *                                                            decoded from its storage res_mode (DD3D_PG_ACT_*: f32 NHWC of pitch res_pitch,
 *                                                            or split planes of the slice's first chunk: (hi + lo) / res_plane_scale,
 *                                                            (hi + mid) + lo -- what the convolution epilogue's res_mode 1 / 2 add), added
 *                                                            in f32 before the ReLU
 * Backward, with G the gradient at y: ghat = G * [stored y > 0] for RELU and RESIDUAL (y > 0 exactly where n + r > 0), ghat = G for
 *   LINEAR; q = sum(ghat) = d beta, p = sum(ghat * xhat) = d gamma, G_c = s * (ghat - q / N - xhat * p / N).  The residual's own share,
 *   G * [y > 0], is formed by the consumer of G (dd3d_backbone_dgrad's res_g / res_y), not here.
 * Order of every sum: the towers' -- slices of DD3D_BN_SLICE consecutive pixels; inside a slice a channel has P = 256 / (min(C, 256) / 4)
 *   thread lanes, lane j adds pixels j, j + P, ... in that order, the lanes are added in lane order; the slice partials are added by
 *   eight lanes, lane j slices j, j + 8, ..., the lanes in lane order.  The sum ORDER IS KEPT: at C a multiple of 32 up to 256 the
 *   statistics and the backward's q, p, G_c are the bits of dd3d_bn_batch_stats / dd3d_bn_backward_reduce / _apply (they run the same
 *   kernels); C = 16 has P = 64 (one pixel per lane), C = 512 runs as two chunks of 256 channels with P = 4 each.  One writer per word,
 *   no float atomics, the same bits on every run, safe under stream capture.
 * dd3d_backbone_bn_batch_stats (four launches): bn-> every word of stats; reads c, gamma, beta, run_mean, run_var.
 * dd3d_backbone_bn_apply (one launch, thread = (pixel, 8 channels), 16-byte loads and stores; at C = 16 two threads share a pixel, no
 *   lane idles): y from bn.c, bn.beta, bn.stats rows MU, S and the residual.  Stores: bn.math_mode a split-plane mode -- bn.y[s]
 *   (optional) the split planes [C/32][N][NP][32] of the slice's first chunk, bit for bit what dd3d_split_planes makes of the f32 value,
 *   its DD3D_STATUS_F16_OVERFLOW bit in bn.status included; y32[s] (optional) f32 NHWC of pitch y32_pitch; at least one of the two; planes
 *   need C % 32 == 0.  bn.math_mode DD3D_MATH_F32: bn.y[s] is f32 NHWC of pitch bn.y_pitch and y32 is not read.  An output may be a channel
 *   slice of a wider buffer in either storage (f32: the pitch; planes: a run of whole chunk images of N pixels).
 * dd3d_backbone_bn_backward_reduce / _apply: the masked backward (stored y in storage bn.y_mode, a channel slice allowed);
 * dd3d_backbone_bn_backward_reduce_linear / _apply_linear: without the mask, the bits of the masked calls for a y of ones.
 *   gc: f32 [N][C].  part: [n_slices][2][C], n_slices >= dd3d_backbone_bn_slices(args) = sum of ceil(N / DD3D_BN_SLICE).
 * dd3d_backbone_bn_layout: sizeof and field offsets (layout check of the bindings; host only).
 * Rejected (-1, dd3d_last_error starts with the entry point's name): what the tower entry points reject, with the widths above in place
 *   of theirs; for the apply an unknown act, a RESIDUAL segment without res, an unknown res_mode, a res_pitch that is not a multiple of 4
 *   or below C (f32 residual), a residual in planes at C % 32 != 0, a split-plane math_mode other than f16x2 / bf16x3, planes asked
 *   for at C % 32 != 0, a segment with neither output, a y32 pitch that is not a multiple of 4 or below C.
 * ------------------------------------------------------------------------------------------------ */
#define DD3D_BBN_MIN_C 16
#define DD3D_BBN_MAX_C 512
#define DD3D_BBN_RELU 0
#define DD3D_BBN_LINEAR 1
#define DD3D_BBN_RESIDUAL 2
typedef struct dd3d_backbone_bn_args { /* host memory; every pointer is device memory */
  dd3d_tower_bn_args bn;               /* c, beta, stats, y, status, N, num_segs, C, c_pitch, math_mode, y_pitch, plane_scale */
  float* y32[DD3D_BN_MAX_SEGS];        /* optional f32 copy of y beside the planes: [N][y32_pitch] */
  const void* res[DD3D_BN_MAX_SEGS];   /* DD3D_BBN_RESIDUAL: the stored residual, first channel / first chunk of its slice */
  int32_t act;                         /* DD3D_BBN_* */
  int32_t res_mode, res_pitch;         /* DD3D_PG_ACT_*; floats per pixel of an f32 residual */
  int32_t y32_pitch;
  float res_plane_scale;               /* DD3D_PG_ACT_F16X2 */
  int32_t reserved;                    /* 0; ignored */
} dd3d_backbone_bn_args;
int dd3d_backbone_bn_batch_stats(const dd3d_tower_bn_args* args, void* stream);
int dd3d_backbone_bn_apply(const dd3d_backbone_bn_args* args, void* stream);
int dd3d_backbone_bn_backward_reduce(const dd3d_tower_bn_args* args, void* stream);
int dd3d_backbone_bn_backward_apply(const dd3d_tower_bn_args* args, void* stream);
int dd3d_backbone_bn_backward_reduce_linear(const dd3d_tower_bn_args* args, void* stream);
int dd3d_backbone_bn_backward_apply_linear(const dd3d_tower_bn_args* args, void* stream);
int64_t dd3d_backbone_bn_slices(const dd3d_tower_bn_args* args);
int dd3d_backbone_bn_layout(int64_t* out, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* DD3D_HIP_H */
