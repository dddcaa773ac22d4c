"""Inputs and plain references for the seam tests of the forward path's glue kernels (tests/test_glue_kernels_gpu.py): the pooling /
top-down / split kernels, input normalisation, aligned bilinear upsampling, the intrinsics inverse and the device side of the f16x2
range guard.  No GPU and no pytest marks here: numpy float64 / torch CPU only, so the references themselves are checked on a machine
without a device (tests/test_glue_cases.py)."""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0**-24  # unit roundoff of f32 (round to nearest)
FLT_MAX = float(np.finfo(np.float32).max)
DENORMALS = (1e-40, -1e-40, 1.4e-45)  # f32 subnormals (the last one is the smallest)

PAD = 64                    # sentinel elements each side of every output buffer
SENT_F32 = -1.2345678e20    # no kernel under test produces these from the inputs built here
SENT_I32 = 0x5A5A5A5A
SENT_I16 = 0x0777
POISON = 3.0e30             # fills what a kernel must not read (neighbouring channels, the floats between two sub-maxima)

# ------------------------------------------------------------------------------------------------------------ pooling / top-down
POOL3_SIZES = [(3, 3), (4, 4), (5, 5), (6, 6), (7, 7), (8, 8), (9, 9), (3, 9), (8, 3)]
POOL2_SHAPES = [  # (B, H, W): one window, one row of windows, one column, B * Ho * Wo = 45 (not a multiple of 64)
    (1, 2, 2), (3, 2, 14), (1, 10, 2), (3, 6, 10)]


def signed_map(kind, B, C, H, W, seed):
    """NCHW f32 map: 'neg' is negative everywhere (the pools of the models only ever see rectified data), 'mixed' has both signs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=g)
    if kind == "neg":
        return -(x.abs() + 0.01)
    assert kind == "mixed"
    return x


def special_map(B, C, H, W, seed, denormals=True, k=2):
    """Mixed-sign map with one special value planted per k x k block of image 0 / channel 0; the blocks are the windows of a k x k /
    stride 2 pool whose top-left corners are listed in the returned dict (k = 2: H >= 8, W >= 12; k = 3: H >= 9, W >= 13): +inf, a
    block of -inf only, FLT_MAX, -FLT_MAX among -inf, +0.0 and -0.0 over negatives, and f32 subnormals over negatives.
    Returns (map, {name: (y, x) of the block's top-left corner})."""
    assert k in (2, 3) and H >= 6 + k and W >= 10 + k
    x = signed_map("mixed", B, C, H, W, seed)
    where = {"+inf": (0, 0), "-inf": (0, 4), "fltmax": (0, 8), "-fltmax": (4, 0), "zeros": (4, 4), "denormal": (4, 8)}
    negatives = -1.0 - torch.arange(k * k, dtype=torch.float32).view(k, k)

    def block(name):
        y0, x0 = where[name]
        return x[0, 0, y0:y0 + k, x0:x0 + k]

    block("+inf")[0, 1] = float("inf")
    block("-inf")[:] = float("-inf")
    block("fltmax")[1, 0] = FLT_MAX
    block("-fltmax")[:] = float("-inf")
    block("-fltmax")[1, 1] = -FLT_MAX
    block("zeros")[:] = negatives
    block("zeros")[0, 1], block("zeros")[1, 0] = 0.0, -0.0
    if denormals:
        block("denormal")[:] = negatives
        block("denormal")[0, 1], block("denormal")[1, 0] = DENORMALS[1], DENORMALS[2]
    else:
        where.pop("denormal")
    return x, where


def big_map(B, C, H, W, seed):
    """randn NCHW map stored channels-last (what the kernels read), so that large cases are laid out once."""
    return torch.randn(B, H, W, C, generator=torch.Generator().manual_seed(seed)).permute(0, 3, 1, 2)


def maxpool2x2(x):
    return F.max_pool2d(x, 2, 2)


def maxpool3x3s2_ceil(x):
    return F.max_pool2d(x, 3, 2, ceil_mode=True)


def upsample2x_add(fine, coarse):
    return fine + F.interpolate(coarse, scale_factor=2, mode="nearest")


def pool3_overhang(H, W):
    """Boolean [Ho, Wo]: the 3x3 / stride 2 window of this output reaches past the bottom or the right edge of an H x W map."""
    Ho, Wo = maxpool3x3s2_ceil(torch.zeros(1, 1, H, W)).shape[2:]
    oy = (2 * torch.arange(Ho) + 2 >= H).view(-1, 1)
    ox = (2 * torch.arange(Wo) + 2 >= W).view(1, -1)
    return oy | ox


# (input H, W, C, output H, W) of the 3x3 / stride 2 / ceil pools of DD3D-V2-99 at the KITTI geometry 384 x 1280, as the launch plan
# allocates them: tests/test_glue_cases.py holds this list against v99_kitti_pool_shapes(), so the GPU module need not build a plan
V99_KITTI_POOLS = [(96, 320, 256, 48, 160), (48, 160, 512, 24, 80), (24, 80, 768, 12, 40)]


def v99_kitti_pool_shapes():
    """[(input H, W, C, allocated output H, W)] of the 3x3 / stride 2 / ceil pools of DD3D-V2-99 at the KITTI geometry 384 x 1280, read
    off a launch plan built without a device (engine/backbones.py sizes the output buffers)."""
    from dd3d_amd import META_ARCH_REGISTRY
    from dd3d_amd.engine import ForwardPlan
    from tests.util import bundle
    cfg, sd = bundle("dd3d_kitti_v99", "v99_kitti", None)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
    model.load_state_dict(sd, strict=True)
    plan = ForwardPlan(model, 1, 384, 1280, device="cpu", dry_run=True)
    pools = [op.desc for op in plan.ops if getattr(op, "desc", None) and op.desc.get("kind") == "maxpool3x3s2_ceil"]
    assert pools
    return [(p["vin"].H, p["vin"].W, p["vin"].C, p["vout"].H, p["vout"].W) for p in pools]


# ------------------------------------------------------------------------------------------------------------ layouts
def nhwc_slice(x, pitch, c0, fill):
    """NCHW map -> [B, H, W, pitch] f32 holding it at channels c0 .. c0 + C, `fill` elsewhere."""
    B, C, H, W = x.shape
    assert c0 + C <= pitch
    if pitch == C:
        return x.permute(0, 2, 3, 1).contiguous()
    t = torch.full((B, H, W, pitch), float(fill), dtype=torch.float32)
    t[..., c0:c0 + C] = x.permute(0, 2, 3, 1)
    return t


def decode_planes(p, f16, scale):
    """int16 [chunks][M][NP][32] split planes -> f32 [M, chunks * 32]: the terms summed in plane order, as the kernels that read
    planes rebuild a value (IEEE halves of value * scale for the f16x2 mode, bf16 terms otherwise)."""
    if f16:
        terms = p.view(torch.float16).float() / scale
    else:
        terms = (p.to(torch.int32) << 16).view(torch.float32)
    x = terms[:, :, 0]
    for q in range(1, p.shape[2]):
        x = x + terms[:, :, q]
    return x.permute(1, 0, 2).reshape(p.shape[1], p.shape[0] * 32)


def rows_to_nchw(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------------------ preprocess
def byte_image(B, Hp, Wp):
    """uint8 [B, 3, Hp, Wp] (Hp * Wp >= 256): every channel of every image runs through all 256 byte values, each channel in its own
    order, so no two channels and no two neighbouring pixels agree."""
    assert Hp * Wp >= 256
    i = torch.arange(Hp * Wp).view(1, 1, -1)
    step = torch.tensor([1, 7, 201]).view(1, 3, 1)
    off = torch.tensor([0, 85, 170]).view(1, 3, 1)
    b = torch.arange(B).view(-1, 1, 1)
    return ((i * step + off + 31 * b) % 256).to(torch.uint8).view(B, 3, Hp, Wp)


def preprocess_ref(img, sizes, mean, std):
    """(x - mean) / std in f32 inside each image's (h, w), zero outside; -> [B, Hp, Wp, 4] with channel 3 zero."""
    B, _, Hp, Wp = img.shape
    ref = (img.float() - torch.tensor(mean, dtype=torch.float32).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float32).view(1, 3, 1, 1)
    for b, (h, w) in enumerate(sizes):
        ref[b, :, h:, :] = 0
        ref[b, :, :, w:] = 0
    out = torch.zeros(B, Hp, Wp, 4)
    out[..., :3] = ref.permute(0, 2, 3, 1)
    return out


# ------------------------------------------------------------------------------------------------------------ aligned bilinear
BILINEAR_FACTORS = [1, 2, 3, 8, 16, 128]
BILINEAR_MAPS = [(1, 1), (1, 7), (5, 1), (3, 10), (12, 40)]
BLEND_ROUNDINGS = 8  # 1 - l, a product, a sum of two products, the product by the row weight, the final sum: six, rounded up


def _axis64(n, f, half):
    o = np.arange(n * f)
    s = np.maximum(o - f // 2, 0) if half else o
    scale = np.float32(n) / np.float32(f * n)  # the coordinate as torch computes it: in float32
    r = (scale * s.astype(np.float32)).astype(np.float32)
    i0 = r.astype(np.int64)
    l = (r - i0.astype(np.float32)).astype(np.float32)
    return i0, np.minimum(i0 + 1, n - 1), l.astype(np.float64)


def aligned_bilinear64(src, f, half, inv_K=None, focal_factor=0.0):
    """tensor2d.py:28-47 (replicate-pad by one, bilinear with align_corners=True to (f h + 1, f w + 1), crop; offset 'half' shifts by
    f // 2 with edge replication) + the focal scaling of dense_depth.py:159-163, on f32 `src` [B, h, w]: the source coordinate in
    float32 as torch takes it, the four-point blend and the division in float64.  -> float64 [B, f h, f w]."""
    src = np.asarray(src, dtype=np.float32)
    B, h, w = src.shape
    y0, y1, ly = _axis64(h, f, half)
    x0, x1, lx = _axis64(w, f, half)
    s = src.astype(np.float64)
    rows_ = (1 - lx[None, None, :]) * s[:, :, x0] + lx[None, None, :] * s[:, :, x1]  # [B, h, f w]: the blend along x of every source row
    out = (1 - ly[None, :, None]) * rows_[:, y0] + ly[None, :, None] * rows_[:, y1]
    if focal_factor > 0:
        out = out / focal_divisor(inv_K, focal_factor).reshape(B, 1, 1)
    return out


def focal_divisor(inv_K, focal_factor):
    k = np.asarray(inv_K, dtype=np.float32).reshape(-1, 9).astype(np.float64)
    return np.sqrt(k[:, 0]**2 + k[:, 4]**2) * float(np.float32(focal_factor))


def bilinear_bar_terms(src, inv_K=None, focal_factor=0.0):
    """(lead [B], rel): |got - ref| <= lead[b] + rel * |ref|.  lead = BLEND_ROUNDINGS * 2^-24 of the image's largest source entry, divided
    by the focal divisor when the scaling is on; rel = 2 * 2^-24 for the divisor's square root and the division, else 0."""
    src = np.asarray(src, dtype=np.float64)
    lead = BLEND_ROUNDINGS * EPS * np.abs(src).reshape(src.shape[0], -1).max(1)
    if focal_factor > 0:
        return lead / focal_divisor(inv_K, focal_factor), 2 * EPS
    return lead, 0.0


def bilinear_bar(src, ref, inv_K=None, focal_factor=0.0):
    """Per-element bound [B, H, W] on |got - ref| (bilinear_bar_terms)."""
    lead, rel = bilinear_bar_terms(src, inv_K, focal_factor)
    return lead.reshape(-1, 1, 1) + rel * np.abs(ref)


# ------------------------------------------------------------------------------------------------------------ intrinsics inverse
INV_REL = 8 * EPS      # zero-skew pinhole: every non-zero entry is a product of at most two inputs times a reciprocal of a product
INV_RESIDUAL = 16 * EPS


def invert64(K):
    """Cofactor inverse in float64 of float32 3x3 matrices [B, 3, 3]."""
    m = np.asarray(K, dtype=np.float32).astype(np.float64).reshape(-1, 3, 3)
    a, b, c, d, e, f, g, h, i = [m[:, r, s] for r in range(3) for s in range(3)]
    A, Bc, Cc = e * i - f * h, -(d * i - f * g), d * h - e * g
    det = a * A + b * Bc + c * Cc
    adj = np.stack([A, -(b * i - c * h), b * f - c * e, Bc, a * i - c * g, -(a * f - c * d), Cc, -(a * h - b * g), a * e - b * d], 1)
    return (adj / det[:, None]).reshape(-1, 3, 3)


def pinhole(fx, fy, cx, cy):
    return [[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]]


def pinhole_matrices(n, seed=0):
    """n distinct zero-skew pinhole matrices: the focal sweep 2^k * 700 (k = -3 .. 3) first, then random ones."""
    rng = np.random.default_rng(seed)
    out = [pinhole(2.0**k * 700.0, 2.0**k * 700.0 * 1.01, 640.0 + 3 * k, 190.0 - k) for k in range(-3, 4)]
    while len(out) < n:
        fx = float(rng.uniform(80, 6000))
        out.append(pinhole(fx, fx * float(rng.uniform(0.9, 1.1)), float(rng.uniform(100, 1000)), float(rng.uniform(50, 600))))
    return np.asarray(out[:n], dtype=np.float32)


GENERAL_MATRICES = np.asarray([
    [[748.7, 0.3, 632.5], [0.0, 748.8, 179.4], [0.0, 0.0, 1.0]],        # the skew of test_aux_kernels
    [[1260.9, 0.0, 812.7], [0.0, 1260.8, 489.3], [0.0, 0.0, 2.5]],      # K22 != 1
    [[4.0, -1.0, 0.5], [1.5, 3.0, -0.75], [-0.25, 1.0, 5.0]],           # dense, well conditioned (diagonally dominant)
], dtype=np.float32)


def inverse_residual(K, got):
    """(max |K got - I|, max(|K| |got|)) per matrix, in float64: the backward bound of a cofactor inverse compares the two."""
    K = np.asarray(K, dtype=np.float64).reshape(-1, 3, 3)
    got = np.asarray(got, dtype=np.float64).reshape(-1, 3, 3)
    res = np.abs(K @ got - np.eye(3)).reshape(len(K), -1).max(1)
    size = (np.abs(K) @ np.abs(got)).reshape(len(K), -1).max(1)
    return res, size


# ------------------------------------------------------------------------------------------------------------ range guard
SUB, LINE = 16, 32  # a watched launch owns 16 sub-maxima, one per 128-byte line: 32 floats apart


def build_amax(maxima, poison):
    """[n, 16] sub-maxima -> the flat f32 array the kernels read: entry (i, j) at float (i * 16 + j) * 32, `poison` in between."""
    maxima = np.asarray(maxima, dtype=np.float32).reshape(-1, SUB)
    flat = np.full(max(1, maxima.shape[0]) * SUB * LINE, poison, dtype=np.float32)
    flat[:maxima.size * LINE:LINE][:maxima.size] = maxima.reshape(-1)
    return flat


def launch_maxima(amax_flat, n):
    """f32 [n]: max over each launch's 16 sub-maxima, starting from 0 (what fmaxf(0, ...) over them gives for non-NaN entries)."""
    v = np.asarray(amax_flat, dtype=np.float32)[:n * SUB * LINE:LINE].reshape(n, SUB)
    return np.maximum(v.max(1), np.float32(0)) if n else np.zeros(0, np.float32)


def fold_ref(status, amax_flat, n, floor):
    m = launch_maxima(amax_flat, n)
    return np.array([0 if status is None else int(status), int(bool(((m > 0) & (m < np.float32(floor))).any()))], dtype=np.int32)


def pack_ref(det_count, status, amax_flat, n, flags, nrec, flag_stride):
    """The read-back record, word for word: (status, G, n, nrec), G counts, n maxima (bit patterns), 2 * nrec gathered flag words."""
    det_count = np.zeros(0, np.int32) if det_count is None else np.asarray(det_count, dtype=np.int32)
    head = np.array([0 if status is None else int(status), len(det_count), n, nrec], dtype=np.int32)
    gathered = np.zeros(0, np.int32)
    if nrec:
        f = np.asarray(flags, dtype=np.int32)
        gathered = np.stack([f[np.arange(nrec) * flag_stride], f[np.arange(nrec) * flag_stride + 1]], 1).reshape(-1)
    return np.concatenate([head, det_count, launch_maxima(amax_flat, n).view(np.int32), gathered])


def fold_cases(floor):
    """[(name, [n, 16] sub-maxima)]: launches whose maximum is >= floor except where the name says otherwise."""
    floor = np.float32(floor)
    below = np.nextafter(floor, np.float32(0))
    rng = np.random.default_rng(5)

    def healthy(n):
        m = rng.uniform(0.0, 0.9, size=(n, SUB)).astype(np.float32) * floor  # sub-maxima below the floor, some exactly zero ...
        m[rng.random((n, SUB)) < 0.3] = 0.0
        m[np.arange(n), rng.integers(0, SUB, n)] = rng.uniform(1.0, 1000.0, n).astype(np.float32) * floor  # ... and one at or above it
        return m

    def low_at(n, i, slot=None):
        m = healthy(n)
        m[i] = rng.uniform(0.0, 0.5, SUB).astype(np.float32) * floor
        m[i, rng.integers(0, SUB) if slot is None else slot] = 0.75 * floor
        return m

    cases = [("n0", np.zeros((0, SUB), np.float32))]
    for n in (1, 255, 256, 257, 700):
        cases.append((f"n{n}_healthy", healthy(n)))
        cases.append((f"n{n}_low_first", low_at(n, 0)))
        cases.append((f"n{n}_low_last", low_at(n, n - 1)))
        if n > 256:
            cases.append((f"n{n}_low_at_256", low_at(n, 256)))
    for slot in (0, 15):
        cases.append((f"low_in_slot{slot}", low_at(300, 123, slot)))
        m = np.zeros((300, SUB), np.float32)  # the only non-zero entry of the launch, at the floor's other side
        m[:] = healthy(300)
        m[200] = 0.0
        m[200, slot] = floor
        cases.append((f"exactly_floor_in_slot{slot}", m.copy()))
        m[200, slot] = below
        cases.append((f"just_below_floor_in_slot{slot}", m.copy()))
    z = healthy(300)
    z[7] = 0.0
    cases.append(("one_launch_all_zero", z))
    cases.append(("every_launch_all_zero", np.zeros((257, SUB), np.float32)))
    return cases
