"""Gradient of the dense-depth loss, the parts that need no GPU: the autograd oracle checks itself (tests/dense_depth_grad_oracle.py),
the empty selection against torch itself, the closed form of a level's gradient sum, the bindings' layout and the input validation of
dd3d_amd.losses.FusedDenseDepthLoss.  The HIP path is tests/test_dense_depth_grads_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dense_depth_grad_oracle as GO
from tests import dense_depth_loss_oracle as DO

CASES = [((1, 128, 128), False, True), ((1, 128, 128), True, False), ((2, 128, 256), False, False), ((2, 128, 256), True, True)]
IDS = ["1x128x128-none-focal", "1x128x128-half-nofocal", "2x128x256-none-nofocal", "2x128x256-half-focal"]


def test_the_oracles_upsampling_is_the_loss_oracles_in_float32():
    from tests.test_dense_depth_loss_gpu import intrinsics, raw_maps
    raw, K = raw_maps(2, 128, 256, seed=11), intrinsics(2)
    for offset in ("none", "half"):
        for factor in (None, GO.FOCAL_FACTOR):
            a = DO.upsampled_maps(raw, GO.STRIDES, offset, K, factor)
            b = GO.upsampled_maps(raw, GO.STRIDES, offset, K, factor)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = GO.case((2, 128, 256), True, True)
    ref, count, _ = DO.dense_depth_loss(c.maps, c.gt, GO.MIN_DEPTH, GO.MAX_DEPTH, GO.BETA, GO.WEIGHT)
    assert count == c.count
    for v, w in zip(c.loss64, ref.values()):  # the differentiable statement of the loss is the loss oracle's
        assert abs(float(v) - float(w)) <= 2e-6 * abs(float(w))


@pytest.mark.parametrize("shape,half,focal", CASES, ids=IDS)
def test_float32_autograd_is_close_to_float64_and_the_fixture_keeps_its_promises(shape, half, focal):
    """The kink removal takes at most 2 % of the valid pixels, both branches occur at the level the ground truth was built around, and
    the float32 autograd lies within 1e-5 of the float64 one relative to max|g64| (measured: 2e-7 .. 6e-6)."""
    c = GO.case(shape, half, focal)
    print(f"{shape} half={half} focal={focal}: removed {100 * c.removed:.3f} % of {c.valid_before}, quadratic share {c.share:.3f}")
    assert c.removed <= 0.02 and 0.2 < c.share < 0.8 and c.count > 0
    for l, (a, b) in enumerate(zip(c.g64, c.g32)):
        bar, d32, gmax = GO.bar(a, b)
        print(f"  level {l}: max|g64| {gmax:.3e} d32 {d32:.3e} ({d32 / gmax:.2e} of max)")
        assert gmax > 0 and d32 <= 1e-5 * gmax


def test_ground_truth_around_a_coarse_level_runs_the_quadratic_branch_there():
    c = GO.case((2, 128, 256), True, True, around=3)
    assert c.removed <= 0.02 and 0.2 < c.share < 0.8


def test_empty_selection_gives_zero_gradients_like_torch_itself():
    x = torch.arange(6.0, requires_grad=True)
    m = x[torch.zeros(6, dtype=torch.bool)].mean()
    m.backward()
    assert bool(torch.isnan(m)) and torch.equal(x.grad, torch.zeros(6))  # torch's convention, which the kernel follows
    c = GO.case((1, 128, 128), False, True)
    g, out = c.grads(torch.float64, gt=torch.zeros_like(c.gt))
    assert all(bool(torch.isnan(v)) for v in out) and all(float(t.abs().max()) == 0.0 for t in g)


@pytest.mark.parametrize("shape,half,focal", CASES, ids=IDS)
def test_a_levels_gradient_sums_to_the_scaled_sum_of_the_derivative(shape, half, focal):
    """The tap weights of a pixel sum to 1, so sum_ij g_l(b, i, j) = up[l] * weight / (divisor_l * N * pix_b) * sum_p s'(v_l(p) - gt(p))
    over the valid pixels p of image b."""
    c = GO.case(shape, half, focal)
    maps64 = GO.upsampled_maps([r.double() for r in c.raw], GO.STRIDES, c.offset, c.K, c.factor)
    terms = GO.derivative_terms(maps64, c.gt, GO.MIN_DEPTH, GO.MAX_DEPTH, c.beta)
    pix = GO.focal_pixel_size(c.K, c.factor) if focal else torch.ones(shape[0], dtype=torch.float64)
    for l in range(len(GO.STRIDES)):
        for b in range(shape[0]):
            want = float(c.up[l]) * GO.level_scale(GO.WEIGHT, l, c.count) / float(pix[b]) * float(terms[l][b].sum())
            got = float(c.g64[l][b].sum())
            scale = float(c.up[l]) * GO.level_scale(GO.WEIGHT, l, c.count) / float(pix[b]) * float(terms[l][b].abs().sum())
            assert abs(got - want) <= 1e-10 * scale, (l, b, got, want)


def test_dense_depth_grad_args_layout_matches_header(hiplib):
    from dd3d_amd import hip
    out = (C.c_int64 * 8)()
    n = hiplib.dd3d_dense_depth_grad_layout(out, 8)
    names = ["d_raw", "upstream", "slab", "n_slab"]
    assert n == len(names) + 1 and [f[0] for f in hip.DenseDepthGradArgs._fields_] == names
    assert out[0] == C.sizeof(hip.DenseDepthGradArgs)
    assert [out[i + 1] for i in range(len(names))] == [getattr(hip.DenseDepthGradArgs, f).offset for f in names]
    assert hiplib.dd3d_dense_depth_grad_layout(out, 4) != 0 and "8 slots" in hiplib.dd3d_last_error().decode()


def _host_args(B, Hp, Wp, strides, half):
    """Loss args over host memory, for the host-only slab sizing (nothing is launched and no pointer is followed)."""
    from dd3d_amd import hip
    keep = [np.zeros(16, dtype=np.float32) for _ in range(4 + len(strides))]
    a = hip.DenseDepthLossArgs()
    for l, s in enumerate(strides):
        a.raw[l], a.h[l], a.w[l], a.stride[l], a.divisor[l] = keep[4 + l].ctypes.data, Hp // s, Wp // s, s, 1.0
    a.gt, a.partials, a.out, a.count = (k.ctypes.data // 16 * 16 + 16 for k in keep[:4])
    a.num_levels, a.B, a.Hp, a.Wp, a.pitch, a.offset_half, a.n_partials = len(strides), B, Hp, Wp, 4, int(half), 1
    return a, keep


def test_slab_rows_follow_the_cells_and_sub_tiles(hiplib):
    """One row per level, image, cell and sub-tile: whole cells up to 1024 / stride rows, ceil((stride [+ stride / 2]) / rows) sub-tiles."""
    from dd3d_amd import hip
    a, keep = _host_args(1, 128, 128, GO.STRIDES, False)
    assert hip.dense_depth_grad_rows(a) == 256 + 64 + 16 + 4 * 4 + 1 * 16  # rows per sub-tile 8, 16, 32, 16, 8
    a, keep = _host_args(2, 384, 1280, GO.STRIDES, True)
    assert hip.dense_depth_grad_rows(a) == 2 * (48 * 160 + 24 * 80 + 12 * 40 * 2 + 6 * 20 * 6 + 3 * 10 * 24)
    a, keep = _host_args(1, 3280, 3280, (328, ), False)  # fl(fl(1 / 328) * 328) < 1 in float32: pixel 328 would still belong to cell 0
    with pytest.raises(RuntimeError, match="power of two"):
        hip.dense_depth_grad_rows(a)
    a, keep = _host_args(1, 128, 128, (4, ), True)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        hip.dense_depth_grad_rows(a)


# ------------------------------------------------------------------------------------------------ FusedDenseDepthLoss: validation
class _Shape:
    def __init__(self, stride):
        self.stride = stride


class _Model:
    """What FusedDenseDepthLoss reads of a DD3DDenseDepth."""
    def __init__(self, focal=True):
        from dd3d_amd import get_cfg
        self.cfg = get_cfg("dd3d_kitti_dla34", {"MODEL": {"META_ARCHITECTURE": "DD3DDenseDepth"},
                                                "DD3D": {"FCOS3D": {"DEPTH_HEAD": {"LOSS_TYPE": "L1", "LOSS_WEIGHT": 1.0}}}})
        self.backbone_output_shape = [_Shape(s) for s in GO.STRIDES]
        self.feature_locations_offset = "none"
        self.scale_depth_by_focal_lengths, self.scale_depth_by_focal_lengths_factor = focal, 500.0


def test_fused_dense_depth_loss_validates_before_it_launches():
    from dd3d_amd import get_cfg
    from dd3d_amd.losses import FusedDenseDepthLoss, check_dense_depth_maps
    model = _Model()
    fused = FusedDenseDepthLoss(model)
    maps = [torch.zeros((2, 1, 128 // s, 256 // s)) for s in GO.STRIDES]
    K, depths = torch.eye(3).repeat(2, 1, 1), [torch.zeros((128, 256)), torch.zeros((100, 200))]
    with pytest.raises(ValueError, match=r"dense_depth_maps\[0\] is on cpu"):
        fused(maps, K, depths)
    with pytest.raises(ValueError, match="has 4 levels; the model has 5"):
        fused(maps[:4], K, depths)
    with pytest.raises(ValueError, match="per-level list"):
        fused(maps[0], K, depths)
    meta = [m.to("meta") for m in maps]  # device and dtype are checked in that order; "meta" is not the HIP device either
    with pytest.raises(ValueError, match=r"dense_depth_maps\[0\] is on meta"):
        fused(meta, K, depths)
    # the remaining rules do not depend on the device: checked on CPU tensors
    on_cpu = lambda ts: (ts, "cpu")
    assert check_dense_depth_maps(model, *on_cpu(maps)) == (2, 128, 256)
    with pytest.raises(ValueError, match=r"dense_depth_maps\[2\] is torch.float64"):
        check_dense_depth_maps(model, *on_cpu(maps[:2] + [maps[2].double()] + maps[3:]))
    with pytest.raises(ValueError, match=r"dense_depth_maps\[3\] has shape \(2, 1, 2, 5\) at stride 64: it does not tile the 2 x 128 x 256 canvas"):
        check_dense_depth_maps(model, *on_cpu(maps[:3] + [torch.zeros((2, 1, 2, 5))] + maps[4:]))
    with pytest.raises(ValueError, match=r"dense_depth_maps\[1\] must be a \(B, 1, h, w\) tensor"):
        check_dense_depth_maps(model, *on_cpu([maps[0], torch.zeros((2, 2, 8, 16))] + maps[2:]))
    with pytest.raises(ValueError, match="multiple of 4"):
        check_dense_depth_maps(_one_level(model, 2), *on_cpu([torch.zeros((1, 1, 8, 3))]))
    with pytest.raises(ValueError, match="DEPTH_HEAD"):  # the loss settings are read when the object is built
        bad = _Model()
        bad.cfg = get_cfg("dd3d_kitti_dla34", {"MODEL": {"META_ARCHITECTURE": "DD3DDenseDepth"}})
        FusedDenseDepthLoss(bad)


def _one_level(model, stride):
    m = _Model()
    m.backbone_output_shape = [_Shape(stride)]
    return m
