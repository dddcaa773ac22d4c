"""Reference gradients of the dense-depth loss for the tests of its backward (csrc/dense_depth_loss_grads.hip): torch autograd through
the CPU oracle of the loss (tests/dense_depth_loss_oracle.py: the reference's aligned_bilinear, the focal-length division, the masked
smooth-L1 mean, weight and level divisor), in float64 (the truth) and in float32 (whose distance from the truth sets the bar), and the
fixture builder that keeps every valid pixel away from the jump of the derivative at |pred - gt| = beta.
"""
import numpy as np
import torch

from tests import dense_depth_loss_oracle as DO

KINK_MARGIN = 1e-3  # about 50x the f32 spacing of values near 50


def upsampled_maps(raw, strides, offset, intrinsics=None, focal_factor=None):
    """DO.upsampled_maps in the dtype of `raw` (that one casts to float32; tests/test_dense_depth_grads.py pins the two to the same bits
    in float32) and differentiable."""
    from oracle.dense_depth_oracle import aligned_bilinear
    maps = [aligned_bilinear(d, int(s), offset).squeeze(1) for d, s in zip(raw, strides)]
    if focal_factor is not None:
        inv_K = torch.as_tensor(intrinsics).to(raw[0].dtype).inverse()
        pixel_size = torch.norm(torch.stack([inv_K[:, 0, 0], inv_K[:, 1, 1]], dim=-1), dim=-1)
        scaled = (pixel_size * focal_factor).reshape(-1, 1, 1)
        maps = [m / scaled for m in maps]
    return maps


def losses(raw, gt, strides, offset, intrinsics, focal_factor, min_depth, max_depth, beta, weight):
    """The per-level loss values as a differentiable function of `raw` (per level (B, 1, h, w), any float dtype): x[M].mean() of the
    smooth-L1 terms, weight and divisor as in DO.level_value.  An empty selection gives NaN values with zero gradients, as torch does."""
    dtype = raw[0].dtype
    gt = torch.as_tensor(gt).detach().to("cpu", torch.float32)
    M = DO.valid_mask(gt, min_depth, max_depth)
    tgt = gt[M].to(dtype)
    out = []
    for l, m in enumerate(upsampled_maps(raw, strides, offset, intrinsics, focal_factor)):
        out.append(DO.level_value(DO.smooth_l1_terms(m[M], tgt, beta).mean(), weight, l))
    return out


def raw_grads(raw, gt, strides, offset, intrinsics, focal_factor, min_depth, max_depth, beta, weight, upstream=None, dtype=torch.float64):
    """d (sum_l upstream[l] * loss_l) / d raw[l] by autograd in `dtype`: (per-level (B, 1, h, w) gradients in `dtype`, loss values)."""
    leaf = [torch.as_tensor(r).detach().to(dtype).clone().requires_grad_(True) for r in raw]
    out = losses(leaf, gt, strides, offset, intrinsics, focal_factor, min_depth, max_depth, beta, weight)
    up = torch.ones(len(raw), dtype=dtype) if upstream is None else torch.as_tensor(upstream).to(dtype)
    total = sum(up[l] * v for l, v in enumerate(out))
    g = torch.autograd.grad(total, leaf, allow_unused=True)
    return [torch.zeros_like(r) if gi is None else gi for r, gi in zip(leaf, g)], [v.detach() for v in out]


def bar(g64, g32, keep=None):
    """(bar, d32, max|g64|) over the pixels `keep` (all of them when None): bar = 8 * max(d32, 2^-23 * max|g64|), the project's bar for
    gradients (tests/test_loss_grads_gpu.py): d32 is the float32 autograd's own distance from the float64 one."""
    a, b = g64.double(), g32.double()
    if keep is not None:
        a, b = a[keep], b[keep]
    if a.numel() == 0:
        return 0.0, 0.0, 0.0
    d32, gmax = float((a - b).abs().max()), float(a.abs().max())
    return 8.0 * max(d32, 2.0**-23 * gmax), d32, gmax


def derivative_terms(maps, gt, min_depth, max_depth, beta):
    """s'(v - gt) at the valid pixels of float maps, 0 elsewhere: per level a (B, Hp, Wp) tensor in the maps' dtype."""
    M = DO.valid_mask(gt, min_depth, max_depth)
    out = []
    for m in maps:
        d = m - gt.to(m.dtype)
        s = torch.sign(d) if beta < 1e-5 else torch.where(d.abs() < beta, d, torch.sign(d))
        out.append(torch.where(M, s, torch.zeros_like(s)))
    return out


def remove_kinks(gt, maps, min_depth, max_depth, beta, margin=KINK_MARGIN):
    """The ground truth with 0 (no return) wherever ANY level's | |v_l - gt| - beta | < margin (|v_l - gt| < margin for beta < 1e-5, where
    the derivative jumps at 0): there a float32 and a float64 evaluation may legitimately take different branches.  Returns (gt, the
    fraction of the valid pixels removed)."""
    gt = gt.clone()
    M = DO.valid_mask(gt, min_depth, max_depth)
    near = torch.zeros_like(M)
    for m in maps:
        n = (m.float() - gt).abs()
        near |= (n < margin) if beta < 1e-5 else ((n - beta).abs() < margin)
    near &= M
    gt[near] = 0.0
    return gt, float(near.sum()) / max(int(M.sum()), 1)


def quadratic_share(maps, gt, level, min_depth, max_depth, beta):
    """The share of the valid pixels on the quadratic branch at `level`."""
    M = DO.valid_mask(gt, min_depth, max_depth)
    return float(((maps[level][M] - gt[M]).abs() < beta).float().mean())


def focal_pixel_size(intrinsics, focal_factor):
    """pix_b of the gradient's formula, float64."""
    inv_K = torch.as_tensor(intrinsics).double().inverse()
    return torch.sqrt(inv_K[:, 0, 0]**2 + inv_K[:, 1, 1]**2) * focal_factor


def level_scale(weight, level, count):
    """weight / (divisor_l * N), float64."""
    return float(weight) / (float(np.sqrt(2)**level) * count)


# ------------------------------------------------------------------------------------------------ the cases both test files share
STRIDES = (8, 16, 32, 64, 128)
MIN_DEPTH, MAX_DEPTH, BETA, WEIGHT, FOCAL_FACTOR = 0.1, 80.0, 0.05, 1.0, 500.0
_CASES = {}


class Case:
    """One seam case: hand-made raw maps (tests/test_dense_depth_loss_gpu.raw_maps, seed 11), two focal lengths in a batch, the sparse
    ground truth of sparse_gt (seed 21) built around the up-sampled map of level `around` with the kinks removed, a random non-uniform
    upstream vector, and the float64 / float32 autograd gradients.  Computed once and shared; nobody writes into it."""
    def __init__(self, shape, half, focal, around=0, beta=BETA, raw=None):
        from tests.test_dense_depth_loss_gpu import intrinsics, raw_maps, sparse_gt
        B, Hp, Wp = shape
        self.shape, self.half, self.focal, self.beta, self.around = shape, half, focal, beta, around
        self.raw = raw_maps(B, Hp, Wp, seed=11) if raw is None else raw
        self.K = intrinsics(B)
        self.offset, self.factor = "half" if half else "none", FOCAL_FACTOR if focal else None
        self.maps = upsampled_maps(self.raw, STRIDES, self.offset, self.K, self.factor)
        gt = sparse_gt(B, Hp, Wp, self.maps[around], seed=21)
        self.valid_before = int(DO.valid_mask(gt, MIN_DEPTH, MAX_DEPTH).sum())
        self.gt, self.removed = remove_kinks(gt, self.maps, MIN_DEPTH, MAX_DEPTH, beta)
        self.count = int(DO.valid_mask(self.gt, MIN_DEPTH, MAX_DEPTH).sum())
        self.share = quadratic_share(self.maps, self.gt, around, MIN_DEPTH, MAX_DEPTH, beta)
        self.up = (0.25 + 1.5 * torch.rand(len(STRIDES), generator=torch.Generator().manual_seed(31))).float()
        self.g64, self.loss64 = self.grads(torch.float64)
        self.g32, _ = self.grads(torch.float32)

    def grads(self, dtype, gt=None, up=None, beta=None):
        return raw_grads(self.raw, self.gt if gt is None else gt, STRIDES, self.offset, self.K, self.factor, MIN_DEPTH, MAX_DEPTH,
                         self.beta if beta is None else beta, WEIGHT, self.up if up is None else up, dtype)


def case(shape, half, focal, around=0, beta=BETA):
    key = (tuple(shape), bool(half), bool(focal), around, beta)
    if key not in _CASES:
        _CASES[key] = Case(shape, half, focal, around, beta)
    return _CASES[key]
