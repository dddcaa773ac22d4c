"""Seeded inputs of the stem-backward tests (tests/test_stem_grads.py, tests/test_stem_grads_gpu.py): one stem convolution per case
(backbone_grad_cases.ConvCase at a stem shape), a three-layer stem with its parameters, and the call shapes of the measured sizes."""
import torch

from tests.backbone_grad_cases import ConvCase
from tests.stem_grad_oracle import SHAPES

# the padded canvases the timing script measures: 1 and 4 KITTI images, the 6-camera 896 x 1600 nuScenes sample (padded to 896 x 1664)
MEASURED = {"kitti_b1": (1, 384, 1280), "kitti_b4": (4, 384, 1280), "nusc_b6": (6, 896, 1664)}


def stem_case(layer, hw, B=1, seed=0, **kw):
    k, s, cin, cout = SHAPES[layer]
    return ConvCase(hw, B, cin, cout, k, s, seed=seed, **kw)


def call_shapes(B, Hp, Wp):
    """(B, H, W, Cin, Cout, ksize, stride) of the three stem calls on a B x Hp x Wp canvas, H x W the call's INPUT."""
    return [(B, Hp, Wp, cin, cout, k, s) for k, s, cin, cout in SHAPES.values()]


def stem_params(norm, seed=0):
    """{layer: p} of a seeded stem for stem_grad_oracle: norm "BN" (a norm with weight, bias and statistics, no conv bias) or "" (a conv bias, no norm).  The
    7 x 7 carries a zero filter for the image's fourth channel."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for name, (k, s, cin, cout) in SHAPES.items():
        w = torch.randn(cout, cin, k, k, generator=gen, dtype=torch.float64) / (k * k * min(cin, 3 if k == 7 else cin))**0.5
        if k == 7:
            w[:, 3] = 0.0
        p = {"w": w}
        if norm:
            p.update(gamma=0.5 + torch.rand(cout, generator=gen, dtype=torch.float64), beta=0.2 * torch.randn(cout, generator=gen, dtype=torch.float64),
                     mean=0.2 * torch.randn(cout, generator=gen, dtype=torch.float64), var=0.5 + torch.rand(cout, generator=gen, dtype=torch.float64))
        else:
            p["b"] = 0.2 * torch.randn(cout, generator=gen, dtype=torch.float64)
        out[name] = p
    return out
