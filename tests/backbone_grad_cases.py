"""Seeded inputs of the backbone-backward tests (tests/test_backbone_grads.py, tests/test_backbone_grads_gpu.py): one backbone convolution
(ConvCase), 2x2 pools with constructed ties (pool_input), a small DLA with every path of BackboneLowering._tree (mini_dla)."""
import torch

from tests import backbone_grad_oracle as BO
from tests.predictor_grad_cases import encode_bf16x3, encode_f16x2  # noqa: F401


class ConvCase:
    """One k x k, stride-s convolution: x (input), y (stored output; None for a project), g (gradient at the output), w, scale, NCHW
    float32; optionally `add` and the residual pair (`res_g`, `res_y`), all of the input's shape."""
    def __init__(self, hw, B, Cin, Cout, ksize, stride, seed=0, with_y=True, with_add=False, with_res=False, negative_y=False, zero_scale=False):
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen)
        self.hw, self.B, self.Cin, self.Cout, self.ksize, self.stride = tuple(hw), B, Cin, Cout, ksize, stride
        h, w = hw
        ho, wo = (h + stride - 1) // stride, (w + stride - 1) // stride
        self.out_hw = (ho, wo)
        self.x = rnd(B, Cin, h, w)
        self.w = rnd(Cout, Cin, ksize, ksize) * (0.5 / (ksize * ksize * Cin)**0.5)
        self.scale = torch.zeros(Cout) if zero_scale else 0.5 + torch.rand(Cout, generator=gen)
        self.g = rnd(B, Cout, ho, wo)
        self.y = (-rnd(B, Cout, ho, wo).abs() if negative_y else rnd(B, Cout, ho, wo)) if with_y else None
        self.add = rnd(B, Cin, h, w) if with_add else None
        self.res_g = rnd(B, Cin, h, w) if with_res else None
        self.res_y = rnd(B, Cin, h, w) if with_res else None

    def ref(self, dtype=torch.float64, x=None, y=None, res_y=None, add=True):
        x = self.x if x is None else x
        y = self.y if y is None else y
        res = (self.res_g, self.res_y if res_y is None else res_y) if self.res_g is not None else None
        return BO.layer_grads(x, y, self.g, self.w, self.scale, self.stride, dtype, add=self.add if add else None, res=res)


def pool_input(kind, B, C, hw, seed=0):
    """The stored input of a 2x2 pool.  "random": seeded normals; "equal": one value everywhere (every window a four-way tie); "two_max":
    every window holds its positive maximum twice, at (0,1) and (1,0), above two smaller entries; "relu": rectified normals (windows of
    zeros tie, as the stored activations do)."""
    gen = torch.Generator().manual_seed(seed)
    h, w = hw
    if kind == "equal":
        return torch.full((B, C, h, w), 0.75)
    x = torch.randn(B, C, h, w, generator=gen)
    if kind == "relu":
        return torch.relu(x)
    if kind == "two_max":
        x = -x.abs()
        top = 0.5 + torch.rand(B, C, h // 2, w // 2, generator=gen)
        x[:, :, 0::2, 1::2] = top
        x[:, :, 1::2, 0::2] = top
    return x


def randomize(dla, seed=17):
    """Seeded values for every parameter and norm statistic of a DLA (filters small enough that activations stay O(1))."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, conv in dla.named_modules():
            if getattr(getattr(conv, "weight", None), "dim", lambda: 0)() != 4:
                continue
            k = conv.weight.shape[-1]
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (1.0 / (k * k * conv.weight.shape[1])**0.5))
            if conv.bias is not None:
                conv.bias.copy_(torch.randn(conv.weight.shape[0], generator=gen) * 0.2)
            n = getattr(conv, "norm", None)
            if n is not None:
                n.weight.copy_(0.5 + torch.rand(conv.weight.shape[0], generator=gen))
                n.bias.copy_(torch.randn(conv.weight.shape[0], generator=gen) * 0.2)
                n.running_mean.copy_(torch.randn(conv.weight.shape[0], generator=gen) * 0.2)
                n.running_var.copy_(0.5 + torch.rand(conv.weight.shape[0], generator=gen))
    return dla


# channels of level0 .. level5: level2 a depth-1 tree with a project (32 -> 64), level3 a depth-2 level_root tree WITHOUT a project (64 ->
# 64: the pooled tensor is tree1's residual), level4 a depth-2 level_root tree with one (64 -> 96), level5 a depth-1 level_root tree (96 -> 128)
MINI_LEVELS, MINI_CHANNELS = [1, 1, 1, 2, 2, 1], [32, 32, 64, 64, 96, 128]


def mini_dla(norm="BN", seed=23, levels=None, channels=None):
    from dd3d_amd.modeling.dla import DLA
    dla = DLA(levels or MINI_LEVELS, channels or MINI_CHANNELS, out_features=["level3", "level4", "level5"], norm=norm)
    return randomize(dla, seed).eval()


def mini_inputs(dla, B=2, hw=(32, 64), seed=5, dtype=torch.float32):
    """A seeded, rectified level1 tensor and a gradient for the outputs of level3 .. level5."""
    gen = torch.Generator().manual_seed(seed)
    level1 = torch.relu(torch.randn(B, dla.channels[1], hw[0], hw[1], generator=gen)).to(dtype)
    outs = BO.forward(dla, BO.state(dla, dtype), level1)
    G = {k: torch.randn(outs[k].shape, generator=gen).to(dtype) for k in ("level3", "level4", "level5")}
    return level1, G


CONFIGS = {"kitti_dla34": ("dd3d_kitti_dla34", None), "nusc_dla34": ("dd3d_nusc_dla34", None)}
