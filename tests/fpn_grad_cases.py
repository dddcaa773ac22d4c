"""Seeded inputs of the FPN-backward tests (tests/test_fpn_grads.py, tests/test_fpn_grads_gpu.py): one convolution of the FPN family per
level (ConvCase), a small FPN module with every parameter kind (mini_model), the configurations the dry-run plans are built for."""
from collections import OrderedDict

import torch

from tests import fpn_grad_oracle as FO
from tests.predictor_grad_cases import encode_bf16x3, encode_f16x2  # noqa: F401


class ConvCase:
    """One k x k, stride-s convolution per level: x (input), g (gradient at the output), w, scale per level, NCHW float32; optionally
    `mask` (a stored tensor of the input's shape), `add` (same shape) and `pool` (levels after the first add the 2x2 sums of the level
    before: the levels must halve)."""
    def __init__(self, in_hw, B, Cin, Cout, ksize, stride, seed=0, with_mask=False, with_add=False, chain=False, in_relu=False, zero_scale_level=None,
                 negative_mask=False):
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen)
        self.in_hw, self.B, self.Cin, self.Cout, self.ksize, self.stride, self.L = list(in_hw), B, Cin, Cout, ksize, stride, len(in_hw)
        self.in_relu, self.chain = in_relu, chain
        out = lambda n: (n + stride - 1) // stride
        self.x = [rnd(B, Cin, h, w) for h, w in in_hw]
        self.w = [rnd(Cout, Cin, ksize, ksize) * (0.5 / (ksize * ksize * Cin)**0.5) for _ in in_hw]
        self.scale = [0.5 + torch.rand(Cout, generator=gen) for _ in in_hw]
        if zero_scale_level is not None:
            self.scale[zero_scale_level] = torch.zeros(Cout)
        self.g = [rnd(B, Cout, out(h), out(w)) for h, w in in_hw]
        self.mask = [(-rnd(B, Cin, h, w).abs() if negative_mask else rnd(B, Cin, h, w)) for h, w in in_hw] if with_mask else None
        self.add = [rnd(B, Cin, h, w) for h, w in in_hw] if with_add else None

    def ref(self, dtype=torch.float64, x=None, mask=None, add=True, pool=True):
        """Per-level oracle results; with `chain`, level l > 0 adds the 2x2 sums of level l - 1's da (of the same run)."""
        x, mask = x or self.x, mask or self.mask
        res = []
        for l in range(self.L):
            res.append(FO.layer_grads(x[l], self.g[l], self.w[l], self.scale[l], self.stride, dtype, in_relu=self.in_relu,
                                      mask=None if mask is None else mask[l], add=self.add[l] if (self.add is not None and add) else None,
                                      pool=res[l - 1]["da"] if (self.chain and pool and l > 0) else None))
        return res


class _BottomUp(torch.nn.Module):
    def __init__(self, shapes):
        super().__init__()
        self._shapes = shapes

    def output_shape(self):
        return self._shapes


class MiniModel(torch.nn.Module):
    """A bare FPN under the name `backbone`, seeded: what fpn_grad_oracle.chain_grads and engine.losses.fpn_backward take."""
    def __init__(self, in_channels=(32, 64, 96), out_channels=64, norm="BN", top="p6p7", seed=31):
        super().__init__()
        from dd3d_amd.modeling.dla import FPN, LastLevelP6, LastLevelP6P7
        from dd3d_amd.structures import ShapeSpec
        names = [f"c{i + 3}" for i in range(len(in_channels))]
        shapes = OrderedDict((n, ShapeSpec(channels=c, stride=2**(i + 3))) for i, (n, c) in enumerate(zip(names, in_channels)))
        tb = {"p6p7": LastLevelP6P7, "p6": LastLevelP6}[top](out_channels, out_channels, "p5") if top else None
        self.backbone = FPN(_BottomUp(shapes), names, out_channels, norm=norm, top_block=tb)
        randomize_fpn(self, seed)
        self.eval()


def randomize_fpn(model, seed=17):
    """Seeded values for every FPN parameter and norm statistic (filters small enough that activations stay O(1))."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, conv in model.backbone.named_modules():
            if name.startswith("bottom_up") or getattr(getattr(conv, "weight", None), "dim", lambda: 0)() != 4:
                continue
            k = conv.weight.shape[-1]
            conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (0.7 / (k * k * conv.weight.shape[1])**0.5))
            if conv.bias is not None:
                conv.bias.copy_(torch.randn(conv.weight.shape[0], generator=gen) * 0.2)
            n = getattr(conv, "norm", None)
            if n is not None:
                n.weight.copy_(0.5 + torch.rand(conv.weight.shape[0], generator=gen))
                n.bias.copy_(torch.randn(conv.weight.shape[0], generator=gen) * 0.2)
                n.running_mean.copy_(torch.randn(conv.weight.shape[0], generator=gen) * 0.2)
                n.running_var.copy_(0.5 + torch.rand(conv.weight.shape[0], generator=gen))
    return model


def mini_inputs(model, B, hw3, seed=5, dtype=torch.float32):
    """Seeded backbone features of a MiniModel on a finest level of hw3 (each next level half of it) and a gradient per FPN output."""
    gen = torch.Generator().manual_seed(seed)
    fpn = model.backbone
    shapes = fpn.bottom_up.output_shape()
    feats = OrderedDict()
    h, w = hw3
    for n in fpn.in_features:
        feats[n] = torch.randn(B, shapes[n].channels, h, w, generator=gen).to(dtype)
        h, w = h // 2, w // 2
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in model.state_dict().items()}
    outs = FO.forward(sd, feats, FO.spec(model))
    G = {k: torch.randn(v.shape, generator=gen).to(dtype) for k, v in outs.items()}
    return feats, G, sd


# the plans of tests/test_fpn_grads.py: experiment, overrides
CONFIGS = {
    "kitti_dla34": ("dd3d_kitti_dla34", None),
    "nusc_dla34": ("dd3d_nusc_dla34", None),
    "kitti_v99": ("dd3d_kitti_v99", None),
    "box2d_only": ("dd3d_kitti_dla34", {"MODEL": {"BOX3D_ON": False}}),
    "fpn_no_norm": ("dd3d_kitti_dla34", {"FE": {"FPN": {"NORM": ""}}}),
    "fpn_bn": ("dd3d_kitti_dla34", {"FE": {"FPN": {"NORM": "BN"}}}),
}
