"""Seeded inputs and oracle glue of the VoVNet-V2 stem_1 backward tests (tests/test_vovnet_stem_grads.py,
tests/test_vovnet_stem_grads_gpu.py, tests/test_vovnet_stem_whole_model_gpu.py): the seam cases of dd3d_vovnet_stem_wgrad as
backbone_grad_cases.ConvCase at (ksize, stride, Cin, Cout) = (3, 2, 4, 64) -- the float64 oracle is backbone_grad_oracle.layer_grads --
and the map from the oracle forward's ReLU calls to a LossPlan's stored tensors with stem_1's call mapped too (`stem.0`)."""
import functools

from tests import vovnet_grad_oracle as VG
from tests.backbone_grad_cases import ConvCase

KSIZE, STRIDE, CIN, COUT = SHAPE = (3, 2, 4, 64)
STEM1 = "backbone.bottom_up.stem.stem_1/"
MEASURED = {"kitti_b1": (1, 384, 1280), "kitti_b4": (4, 384, 1280), "nusc": (6, 896, 1600)}

# (input size, B, seed).  Units are up to 64 output pixels of an output row, a slice is 8 units, 64 slices a sub-sum:
#   a  only the centre tap lands inside the image           b  2 x 2: one output pixel, four taps inside
#   c  odd sizes: the last taps fall outside the image       d  even sizes: only the first row / column of taps falls outside
#   e  Wo = 131: three units a row, the last one three pixels long -- its only MFMA step is partial
#   f  Ho x Wo = 9 x 166, B = 2: 54 units = seven slices, the last of six units; a wave takes two units of a slice
#   g  64 x 320, B = 2: 640 units = 80 slices: two sub-sums of the reduce, the second of 16 slices
SEAM_CASES = {"a_1x1": ((1, 1), 1, 41), "b_2x2": ((2, 2), 1, 42), "c_5x9": ((5, 9), 1, 43), "d_6x8": ((6, 8), 1, 44), "e_4x262": ((4, 262), 1, 45),
              "f_18x331_b2": ((18, 331), 2, 46), "g_128x640_b2": ((128, 640), 2, 47)}
SLICES = {"a_1x1": 1, "b_2x2": 1, "c_5x9": 1, "d_6x8": 1, "e_4x262": 1, "f_18x331_b2": 7, "g_128x640_b2": 80}


@functools.lru_cache(maxsize=None)
def seam_case(name):
    """The ConvCase of a seam case: x with four live channels (the fourth channel's dw column is compared like the others)."""
    hw, B, seed = SEAM_CASES[name]
    return ConvCase(hw, B, CIN, COUT, KSIZE, STRIDE, seed=seed)


@functools.lru_cache(maxsize=None)
def seam_refs(name, storage="f32"):
    """(float64, float32) oracle results of a seam case under the masks its stored output decodes to in `storage`; computed once."""
    import torch
    from tests.predictor_grad_cases import encode_bf16x3, encode_f16x2
    case = seam_case(name)
    y = case.y if storage == "f32" else (encode_f16x2(case.y, 16.0) if storage == "f16x2" else encode_bf16x3(case.y))[1]
    strip = lambda r: {k: v for k, v in r.items() if k != "da"}  # (the image has no gradient)
    return strip(case.ref(torch.float64, y=y)), strip(case.ref(torch.float32, y=y))


_vovnet_relu_sites = VG.relu_sites  # (plan_masks below swaps the module's name for the call)


def relu_sites(plan):
    """vovnet_grad_oracle.relu_sites with stem_1's ReLU call mapped to its stored tensor `stem.0` as well: no call is left to the oracle's
    own sign."""
    sites = _vovnet_relu_sites(plan)
    assert sites[0] is None and all(s is not None for s in sites[1:])
    return [("stem.0", plan.bufs["stem.0"], 0, None, False)] + sites[1:]


def plan_masks(plan, pre64, report=None):
    """vovnet_grad_oracle.plan_masks over `relu_sites` above: one mask per ReLU call from the plan's decoded stored tensor, stem_1's
    included, each validated by value against the float64 forward."""
    saved, VG.relu_sites = VG.relu_sites, relu_sites
    try:
        return VG.plan_masks(plan, pre64, report)
    finally:
        VG.relu_sites = saved
