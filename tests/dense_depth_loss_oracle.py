"""CPU ORACLE of the dense-depth training loss of DD3DDenseDepth (test infrastructure only).

Restates the training branch of tridet/modeling/dd3d/dense_depth.py:140-145,165-171 and DenseDepthL1Loss.forward
(dense_depth_loss.py:28-36) with tridet/layers/smooth_l1_loss.py in plain torch, taking the per-level up-sampled maps as input:

  1. the ground-truth maps padded to the canvas with 0.0 (ImageList.from_tensors, image_list.py:94-158);
  2. valid iff NOT gt < MIN_DEPTH and NOT gt > MAX_DEPTH, one mask for all levels;
  3. per pixel 0.5 n^2 below beta (not / beta), n - 0.5 beta otherwise, plain n for beta < 1e-5, in float32;
  4. the mean with float64 accumulation of those float32 terms (the reference sums them in float32);
  5. loss_l = f32(weight) * f32(mean), then / f32(np.sqrt(2) ** l), in float32; no valid pixel gives NaN.

Pinned by tests/golden/dense_depth_loss_*.npz, recorded from the reference's own classes.
"""
from collections import OrderedDict

import numpy as np
import torch


def pad_depth(depths, Hp, Wp):
    """(B, Hp, Wp) float32 canvas: every map in its top-left corner, 0.0 elsewhere."""
    canvas = torch.zeros((len(depths), Hp, Wp), dtype=torch.float32)
    for i, d in enumerate(depths):
        canvas[i, :d.shape[-2], :d.shape[-1]] = torch.as_tensor(d).detach().to("cpu", torch.float32)
    return canvas


def valid_mask(gt, min_depth, max_depth):
    """dense_depth_loss.py:29-33, with its two comparisons (a NaN passes both)."""
    m = (gt < min_depth).to(torch.float32) + (gt > max_depth).to(torch.float32)
    return m == 0.


def smooth_l1_terms(pred, target, beta):
    """tridet/layers/smooth_l1_loss.py:57-74, reduction 'none'."""
    n = torch.abs(pred - target)
    if beta < 1e-5:
        return n
    return torch.where(n < beta, 0.5 * n**2, n - 0.5 * beta)


def level_value(mean, weight, level):
    """Points 5: f32(weight) * mean, then / f32(np.sqrt(2) ** level); `mean` a 0-d float32 tensor."""
    return (weight * mean) / (np.sqrt(2)**level)


def dense_depth_loss(maps, gt, min_depth, max_depth, beta, weight):
    """maps: per level (B, Hp, Wp) float32; gt: (B, Hp, Wp) float32 canvas.  Returns (OrderedDict of 0-d float32 tensors in level order,
    valid-pixel count, per-level list of the float32 terms at the valid pixels)."""
    gt = gt.detach().to("cpu", torch.float32)
    M = valid_mask(gt, min_depth, max_depth)
    count = int(M.sum())
    out, terms = OrderedDict(), []
    for l, m in enumerate(maps):
        m = m.detach().to("cpu", torch.float32)
        t = smooth_l1_terms(m[M], gt[M], beta)
        terms.append(t)
        mean = (t.double().sum() / count).float() if count else torch.tensor(float("nan"))
        out[f"loss_dense_depth_lvl_{l}"] = level_value(mean, weight, l)
    return out, count, terms


def upsampled_maps(raw, strides, offset, intrinsics=None, focal_factor=None):
    """dense_depth.py:153-163 on the head's raw per-level maps (B, 1, h, w): aligned_bilinear by the stride, then the division by the
    focal-length pixel size when `focal_factor` is given (intrinsics: (B, 3, 3))."""
    from oracle.dense_depth_oracle import aligned_bilinear
    maps = [aligned_bilinear(torch.as_tensor(d).float(), int(s), offset).squeeze(1) for d, s in zip(raw, strides)]
    if focal_factor is not None:
        inv_K = torch.as_tensor(intrinsics).float().inverse()
        pixel_size = torch.norm(torch.stack([inv_K[:, 0, 0], inv_K[:, 1, 1]], dim=-1), dim=-1)
        scaled = (pixel_size * focal_factor).reshape(-1, 1, 1)
        maps = [m / scaled for m in maps]
    return maps
