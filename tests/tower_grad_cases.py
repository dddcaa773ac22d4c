"""Seeded inputs of the tower-backward tests (tests/test_tower_grads.py, tests/test_tower_grads_gpu.py): one tower layer on a list of
levels -- input, filter, per-level folded norm, the stored float32 output with its exact zeros, a dense incoming gradient -- and the
CPU models of the head configurations the plan tests build."""
import torch

from tests import tower_grad_oracle as TO
from tests.predictor_grad_cases import PYRAMID_64x128, REFERENCE_CANVAS, REFERENCE_CASES, SAMPLE_CAP, encode_bf16x3, encode_f16x2, tower_sample  # noqa: F401


class LayerCase:
    """x, y, g: per-level NCHW float32; w: (Cout, Cin, 3, 3); scale, shift: per-level (Cout)."""
    def __init__(self, level_hw, B, Cin, Cout=None, seed=0, zero_scale_level=None, all_masked=False, with_da_add=False):
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen)
        Cout = Cin if Cout is None else Cout
        L = len(level_hw)
        self.level_hw, self.B, self.Cin, self.Cout, self.L = list(level_hw), B, Cin, Cout, L
        self.x = [rnd(B, Cin, h, w) for h, w in level_hw]
        self.w = rnd(Cout, Cin, 3, 3) * (0.5 / (9 * Cin)**0.5)
        self.scale = [0.5 + torch.rand(Cout, generator=gen) for _ in range(L)]
        if zero_scale_level is not None:
            self.scale[zero_scale_level] = torch.zeros(Cout)
        self.shift = [rnd(Cout) * 0.2 + (0.3 if zero_scale_level == l else 0.0) for l in range(L)]
        self.y = TO.forward(self.x, self.w, self.scale, self.shift)  # stored float32 outputs: exact zeros where the ReLU clamps
        if all_masked:
            self.y = [torch.zeros_like(v) for v in self.y]
        self.g = [rnd(B, Cout, h, w) for h, w in level_hw]
        self.da_add = [rnd(B, Cin, h, w) for h, w in level_hw] if with_da_add else None

    def ref(self, dtype=torch.float64, x=None, y=None, da_add=True):
        return TO.layer_grads(self.x if x is None else x, self.y if y is None else y, self.g, self.w, self.scale, dtype,
                              da_add=self.da_add if da_add else None)


CONFIGS = {
    "kitti": ("dd3d_kitti_dla34", None),
    "nusc": ("dd3d_nusc_dla34", None),
    "box2d_only": ("dd3d_kitti_dla34", {"MODEL": {"BOX3D_ON": False}}),
    "frozen_2d": ("dd3d_kitti_dla34", {"DD3D": {"FCOS2D": {"NORM": "FrozenBN"}}}),
    "no_norm_3d": ("dd3d_kitti_dla34", {"DD3D": {"FCOS3D": {"NORM": ""}}}),
}


def randomize_towers(model, seed=17):
    """Seeded values for every tower parameter and norm statistic of a CPU model (filters small enough that activations stay O(1))."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for convs in TO.tower_modules(model).values():
            for conv in convs:
                conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen) * (0.7 / (9 * conv.in_channels)**0.5))
                if conv.bias is not None:
                    conv.bias.copy_(torch.randn(conv.out_channels, generator=gen) * 0.2)
                norms = list(conv.norm) if isinstance(conv.norm, torch.nn.ModuleList) else [conv.norm] if conv.norm is not None else []
                for n in norms:
                    n.weight.copy_(0.5 + torch.rand(conv.out_channels, generator=gen))
                    n.bias.copy_(torch.randn(conv.out_channels, generator=gen) * 0.2)
                    n.running_mean.copy_(torch.randn(conv.out_channels, generator=gen) * 0.2)
                    n.running_var.copy_(0.5 + torch.rand(conv.out_channels, generator=gen))
    return model
