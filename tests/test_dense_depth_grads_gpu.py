"""Gradient of the dense-depth loss on the MI355X: dd3d_dense_depth_loss_backward at its seam against torch autograd through the CPU
oracle (tests/dense_depth_grad_oracle.py), DD3DDenseDepth.compute_losses(head_grads=True) and dd3d_amd.losses.FusedDenseDepthLoss end
to end.

The bar of a level in a case is 8 * max(d32, 2^-23 * max|g64|): d32 is the deviation of the oracle's float32 autograd from its float64
autograd over the pixels compared (dense_depth_grad_oracle.bar), the bar of tests/test_loss_grads_gpu.py.  The ground truth keeps 1e-3
away from the jump of the derivative at |pred - gt| = beta at every level (dense_depth_grad_oracle.remove_kinks).

A NaN ground-truth pixel: it counts in N; its difference compares false both ways, so the kernel adds 0 for it, while torch's autograd
puts NaN on its four taps at every level.  The test compares every raw pixel that is NOT one of its taps and asserts nothing about the
taps.  Measured on the MI355X: see DESIGN.md, "The dense-depth loss gradient"."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dense_depth_grad_oracle as GO
from tests import dense_depth_loss_oracle as DO
from tests.golden import make_dense_depth_loss_golden as G
from tests.test_dense_depth_loss_gpu import Seam, case_inputs, case_model, raw_maps

pytestmark = pytest.mark.gpu

STRIDES, MIN_DEPTH, MAX_DEPTH, BETA, WEIGHT, FOCAL_FACTOR = GO.STRIDES, GO.MIN_DEPTH, GO.MAX_DEPTH, GO.BETA, GO.WEIGHT, GO.FOCAL_FACTOR


class GradSeam(Seam):
    """The loss seam with gradient buffers: NHWC pitch 4, pre-filled with NaN before every call."""
    def backward(self, gt, half, focal, up, beta=BETA, null_level=None, slab_short=0):
        """dd3d_dense_depth_loss, then dd3d_dense_depth_loss_backward on the same args: (rc of the backward, per-level (B, 1, h, w) CPU
        gradients, the raw NHWC buffers, loss values, count)."""
        from dd3d_amd.engine.dense_depth_loss import dense_depth_grad_args, level_divisors
        hip = self.hip
        a = hip.DenseDepthLossArgs()
        for l in range(self.L):
            a.raw[l] = self.dev[l].data_ptr()
            a.h[l], a.w[l], a.stride[l] = self.hw[l][0], self.hw[l][1], STRIDES[l]
        for l, d in enumerate(level_divisors(self.L)):
            a.divisor[l] = d
        gt_dev = gt.to("cuda", torch.float32).contiguous()
        a.gt, a.inv_K = gt_dev.data_ptr(), self.inv_K.data_ptr()
        a.partials, a.n_partials = self.partials.data_ptr(), self.partials.shape[0]
        a.out, a.count = self.out.data_ptr(), self.count.data_ptr()
        a.num_levels, a.B, a.Hp, a.Wp, a.pitch = self.L, self.B, self.Hp, self.Wp, 4
        a.offset_half, a.focal_factor = int(half), FOCAL_FACTOR if focal else 0.0
        a.min_depth, a.max_depth, a.beta, a.loss_weight = MIN_DEPTH, MAX_DEPTH, beta, WEIGHT
        hip.check(self.lib.dd3d_dense_depth_loss(C.byref(a), hip.current_stream()), "dense_depth_loss")
        d_raw = [torch.full_like(t, float("nan")) for t in self.dev]
        up_dev = torch.as_tensor(up, dtype=torch.float32).cuda()
        rows = hip.dense_depth_grad_rows(a)
        slab = torch.full((rows, hip.DDG_ROW), float("nan"), dtype=torch.float32, device="cuda")
        g = dense_depth_grad_args(a, d_raw, up_dev, slab)
        g.n_slab = rows - slab_short
        if null_level is not None:
            g.d_raw[null_level] = None
        rc = self.lib.dd3d_dense_depth_loss_backward(C.byref(a), C.byref(g), hip.current_stream())
        torch.cuda.synchronize()
        self.last_args, self.last_grad_args = a, g
        return rc, [d[..., 0].unsqueeze(1).cpu() for d in d_raw], [d.cpu() for d in d_raw], self.out.cpu(), int(self.count.cpu())


def assert_within_bar(got, g64, g32, what, keep=None):
    """Every level within its bar of the float64 autograd over `keep` (per level a boolean mask, or None: every raw pixel)."""
    for l, (k, a, b) in enumerate(zip(got, g64, g32)):
        m = None if keep is None else keep[l]
        bar, d32, gmax = GO.bar(a, b, m)
        diff = (k.double() - a.double()).abs()
        dev = float((diff if m is None else diff[m]).max()) if diff.numel() and (m is None or bool(m.any())) else 0.0
        print(f"[dense_depth_grads] {what} level {l}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} "
              f"(dev/bar {dev / max(bar, 1e-300):.2f})")
        assert dev <= bar, (what, l, dev, bar, d32, gmax)


def assert_channel0_only(bufs, what):
    for l, d in enumerate(bufs):
        assert bool(torch.isfinite(d[..., 0]).all()), (what, l, "channel 0 not finite everywhere")
        assert bool(torch.isnan(d[..., 1:]).all()), (what, l, "a pad channel was written")


# ------------------------------------------------------------------------------------------------ 1. the seam against autograd
SHAPES = [(1, 128, 128), (2, 128, 256), (1, 256, 384)]


def run_case(hiplib, c, what):
    seam = GradSeam(hiplib, c.raw, c.K)
    rc, got, bufs, out, count = seam.backward(c.gt, c.half, c.focal, c.up, beta=c.beta)
    assert rc == 0 and count == c.count
    assert_within_bar(got, c.g64, c.g32, what)
    assert_channel0_only(bufs, what)
    rc2, got2, _, out2, _ = seam.backward(c.gt, c.half, c.focal, c.up, beta=c.beta)
    assert rc2 == 0 and torch.equal(out, out2) and all(torch.equal(x, y) for x, y in zip(got, got2))  # no float atomics: bit for bit
    return got


@pytest.mark.parametrize("focal", [True, False], ids=["focal", "nofocal"])
@pytest.mark.parametrize("half", [False, True], ids=["none", "half"])
@pytest.mark.parametrize("shape", SHAPES, ids=["1x128x128", "2x128x256", "1x256x384"])
def test_seam_matches_autograd(hiplib, shape, half, focal):
    """Strides 8 .. 128.  1 x 128 x 128: level 4 is 1 x 1 (every tap clamps), level 3 is 2 x 2; 2 x 128 x 256: two focal lengths in one
    batch; 1 x 256 x 384: level 4 is 2 x 3, interior and edge cells at every level.  No grid or slab of the kernel is capped."""
    c = GO.case(shape, half, focal)
    assert c.removed <= 0.02 and 0.2 < c.share < 0.8
    run_case(hiplib, c, f"seam {shape} half={half} focal={focal}")


def test_seam_with_the_quadratic_branch_at_a_coarse_level(hiplib):
    c = GO.case((2, 128, 256), True, True, around=3)
    assert c.removed <= 0.02 and 0.2 < c.share < 0.8  # both branches at level 3
    run_case(hiplib, c, "seam around level 3")


# ------------------------------------------------------------------------------------------------ 2. one valid pixel
def tap_mask(raw_l, stride, offset, b, y, x, zero_weight=False):
    """The raw pixels of one level that pixel (b, y, x) of the canvas reads with a weight that is not zero: where autograd through the
    oracle's up-sampling leaves a derivative.  (A tap of weight 0 gets an exact 0 from the kernel, as from autograd.)  `zero_weight`:
    the taps of weight 0 too -- a NaN sent back through the up-sampling stays NaN under a weight of 0."""
    from oracle.dense_depth_oracle import aligned_bilinear
    r = torch.zeros_like(raw_l, dtype=torch.float64).requires_grad_(True)
    aligned_bilinear(r, stride, offset)[b, 0, y, x].backward(torch.tensor(float("nan") if zero_weight else 1.0, dtype=torch.float64))
    return torch.isnan(r.grad) if zero_weight else r.grad != 0


@pytest.mark.parametrize("half", [False, True], ids=["none", "half"])
def test_single_valid_pixel_reaches_its_taps_only(hiplib, half):
    """The pixel list of the bit-exact loss test: the canvas corners, the last row and column, a pixel with x < stride / 2, interior
    pixels.  The raw pixels under the pixel's taps are within the bar; every other raw pixel is exactly zero."""
    B, Hp, Wp = 2, 128, 256
    c = GO.case((B, Hp, Wp), half, True)
    seam = GradSeam(hiplib, c.raw, c.K)
    pixels = [(0, 0, 0), (0, 0, Wp - 1), (0, Hp - 1, 0), (1, Hp - 1, Wp - 1), (1, Hp - 1, 77), (0, 53, Wp - 1), (1, 40, 2), (0, 3, 130), (1, 71, 149),
              (0, 64, 128)]
    for k, (b, y, x) in enumerate(pixels):
        dgt = (0.01 + 0.003 * k) if k % 2 else (0.3 + 0.01 * k)  # below and above beta at level 0, in turn
        gt = torch.zeros((B, Hp, Wp))
        gt[b, y, x] = float(c.maps[0][b, y, x]) + dgt
        gt, removed = GO.remove_kinks(gt, c.maps, MIN_DEPTH, MAX_DEPTH, BETA)
        assert removed == 0.0 and MIN_DEPTH < float(gt[b, y, x]) < MAX_DEPTH
        g64, _ = c.grads(torch.float64, gt=gt)
        g32, _ = c.grads(torch.float32, gt=gt)
        rc, got, bufs, _, count = seam.backward(gt, half, True, c.up)
        assert rc == 0 and count == 1
        taps = [tap_mask(r, s, c.offset, b, y, x) for r, s in zip(c.raw, STRIDES)]
        assert all(1 <= int(t.sum()) <= 4 for t in taps)
        assert_within_bar(got, g64, g32, f"one pixel {(b, y, x)} half={half}", keep=taps)
        for l, (t, gl) in enumerate(zip(taps, got)):
            assert float(gl[~t].abs().sum()) == 0.0, (l, (b, y, x))
            assert float(g64[l][t].abs().min()) > 0.0  # every tap found carries weight
        assert_channel0_only(bufs, f"one pixel {(b, y, x)}")


# ------------------------------------------------------------------------------------------------ 3. special values
def test_special_values_at_the_seam(hiplib):
    B, Hp, Wp = 1, 128, 128
    c = GO.case((B, Hp, Wp), False, True)
    seam = GradSeam(hiplib, c.raw, c.K)
    gt = torch.zeros((B, Hp, Wp))
    gt[0, 5, 7], gt[0, 90, 3] = -1.0, 200.0
    rc, got, bufs, out, count = seam.backward(gt, False, True, c.up)  # nothing valid: NaN losses, zero gradients
    assert rc == 0 and count == 0 and bool(torch.isnan(out).all()) and all(float(g.abs().max()) == 0.0 for g in got)
    assert_channel0_only(bufs, "N = 0")

    def compare(gt, what, beta=BETA, keep=None):
        gt, removed = GO.remove_kinks(gt, c.maps, MIN_DEPTH, MAX_DEPTH, beta)
        assert removed == 0.0
        g64, _ = c.grads(torch.float64, gt=gt, beta=beta)
        g32, _ = c.grads(torch.float32, gt=gt, beta=beta)
        rc, got, bufs, _, count = seam.backward(gt, False, True, c.up, beta=beta)
        assert rc == 0 and count == int(DO.valid_mask(gt, MIN_DEPTH, MAX_DEPTH).sum())
        assert_within_bar(got, g64, g32, what, keep=keep)
        return bufs

    gt[0, 10, 10], gt[0, 11, 100], gt[0, 100, 50] = 3.03, 4.0, 5.0  # (3.03: level 1 on the quadratic branch, no level within 1e-3 of beta)
    # exactly MIN_DEPTH and exactly MAX_DEPTH (as float32) are valid
    gt[0, 20, 20], gt[0, 21, 21] = float(np.float32(MIN_DEPTH)), float(np.float32(MAX_DEPTH))
    assert int(DO.valid_mask(gt, MIN_DEPTH, MAX_DEPTH).sum()) == 5
    assert_channel0_only(compare(gt, "range ends"), "range ends")
    compare(gt, "beta 0", beta=0.0)  # plain L1: sign everywhere
    # one NaN ground-truth pixel: every raw pixel that is not one of its taps is finite and within the bar
    gt[0, 64, 64] = float("nan")
    keep = [~tap_mask(r, s, "none", 0, 64, 64, zero_weight=True) for r, s in zip(c.raw, STRIDES)]
    assert all(bool(k.any()) for k in keep[:4])  # (level 4 is one pixel: it is the tap)
    bufs = compare(gt, "NaN ground truth", keep=keep)
    for l, (d, k) in enumerate(zip(bufs, keep)):
        assert bool(torch.isfinite(d[..., 0].unsqueeze(1)[k]).all()), l


def test_bad_arguments_are_rejected_before_any_launch(hiplib):
    from dd3d_amd import hip
    B, Hp, Wp = 1, 128, 128
    c = GO.case((B, Hp, Wp), False, True)
    seam = GradSeam(hiplib, c.raw, c.K)
    rc, _, bufs, _, _ = seam.backward(c.gt, False, True, c.up, null_level=2)
    assert rc != 0 and all(bool(torch.isnan(d).all()) for d in bufs)  # nothing ran: the buffers keep their NaN fill
    with pytest.raises(RuntimeError, match="level 2 has no gradient map"):
        hip.check(rc, "dense_depth_loss_backward")
    rc, _, bufs, _, _ = seam.backward(c.gt, False, True, c.up, slab_short=1)
    assert rc != 0 and all(bool(torch.isnan(d).all()) for d in bufs)
    with pytest.raises(RuntimeError, match="the slab holds"):
        hip.check(rc, "dense_depth_loss_backward")
    assert hiplib.dd3d_dense_depth_loss_backward(C.byref(seam.last_args), None, hip.current_stream()) != 0


# ------------------------------------------------------------------------------------------------ 4. through the model
def plan_raw_maps(plan):
    """The plan's own raw predictor maps of the last run, as the oracle takes them: per level (B, 1, h, w) on the CPU."""
    return [m.t[..., 0].unsqueeze(1).float().cpu() for m in plan.dd_raw]


@pytest.mark.parametrize("name", ["ragged_min0", "ragged"])
def test_compute_losses_with_head_grads(hiplib, name):
    """Losses bit-identical to head_grads=False; gradients within the bar of the oracle's autograd fed the plan's own raw maps (this
    isolates the backward from the convolutions' arithmetic); identical with use_graph=False and after an intervening full-size batch."""
    from dd3d_amd.synthetic import make_depth_maps, make_inputs
    cfg, model = case_model(name)
    g, inputs = case_inputs(name)
    c3 = cfg.DD3D.FCOS3D
    plain = model.compute_losses(inputs)
    losses, grads = model.compute_losses(inputs, head_grads=True)
    assert list(losses) == list(plain) and all(torch.equal(losses[k], plain[k]) for k in plain)
    plan = model.get_loss_plan(2, G.H, G.W, head_grads=True)
    assert plan is not model.get_loss_plan(2, G.H, G.W) and plan.graph is not None
    assert [op.name for op in model.get_loss_plan(2, G.H, G.W).ops if "dense_depth_loss" in op.name] == ["dense_depth_loss"]
    assert [op.name for op in plan.ops if "dense_depth_loss" in op.name] == ["dense_depth_loss", "dense_depth_loss_backward"]
    assert list(grads) == [f"dense_depth{l}" for l in range(5)]
    raw = plan_raw_maps(plan)
    assert all(tuple(grads[f"dense_depth{l}"].shape) == tuple(raw[l].shape) and grads[f"dense_depth{l}"].is_cuda for l in range(5))
    K = torch.stack([x["intrinsics"].float() for x in inputs])
    gt = DO.pad_depth([x["depth"] for x in inputs], G.H, G.W)
    factor = float(model.scale_depth_by_focal_lengths_factor) if model.scale_depth_by_focal_lengths else None
    args = (gt, STRIDES, model.feature_locations_offset, K, factor, float(c3.MIN_DEPTH), float(c3.MAX_DEPTH), float(c3.LOSS.SMOOTH_L1_BETA),
            float(c3.DEPTH_HEAD.LOSS_WEIGHT))
    assert [s.stride for s in model.backbone_output_shape] == list(STRIDES)
    g64, _ = GO.raw_grads(raw, *args, dtype=torch.float64)
    g32, _ = GO.raw_grads(raw, *args, dtype=torch.float32)
    first = [grads[f"dense_depth{l}"].cpu() for l in range(5)]
    assert_within_bar(first, g64, g32, f"compute_losses({name})")
    # a full-size batch in between, then the same batch again
    full = make_inputs(2, G.H, G.W)
    for x, d in zip(full, make_depth_maps(full, seed=5)):
        x["depth"] = d
    _, other = model.compute_losses(full, head_grads=True)
    assert not torch.equal(other["dense_depth0"].cpu(), first[0])
    _, after = model.compute_losses(inputs, head_grads=True)
    assert all(torch.equal(after[f"dense_depth{l}"].cpu(), first[l]) for l in range(5))
    _, eager = case_model(name, use_graph=False)
    _, launched = eager.compute_losses(inputs, head_grads=True)
    assert eager.get_loss_plan(2, G.H, G.W, head_grads=True).graph is None
    assert all(torch.equal(launched[f"dense_depth{l}"].cpu(), first[l]) for l in range(5))


# ------------------------------------------------------------------------------------------------ 5. FusedDenseDepthLoss in a torch graph
def test_fused_dense_depth_loss_in_a_torch_graph(hiplib):
    """maps_l = p_l * a_l + b_l with learnable scalars; backward of a weighted sum of the dict gives a_l.grad = sum(p_l * g_l) and
    b_l.grad = sum(g_l), g_l the gradient at the maps.  With the per-pixel bar of level l (8 * max(d32, 2^-23 max|g64|), both autograds
    taken at the maps), the bar propagated through that map is bar_l * sum|p_l| for a_l and bar_l * numel for b_l; torch's own float32
    sums on the device add at most 2^-23 * log2(numel) * sum|p_l g_l| on top (pairwise reduction), which is included."""
    from dd3d_amd.losses import FusedDenseDepthLoss
    cfg, model = case_model("ragged")
    B, Hp, Wp = 2, 128, 256
    p = raw_maps(B, Hp, Wp, seed=17)
    a0 = [1.0 + 0.02 * l for l in range(5)]
    b0 = [0.25 * l for l in range(5)]
    half = model.feature_locations_offset == "half"
    c = GO.Case((B, Hp, Wp), half, bool(model.scale_depth_by_focal_lengths), raw=[pl * a + b for pl, a, b in zip(p, a0, b0)])
    assert c.removed <= 0.02
    c3 = cfg.DD3D.FCOS3D
    assert (float(c3.MIN_DEPTH), float(c3.MAX_DEPTH), float(c3.LOSS.SMOOTH_L1_BETA), float(c3.DEPTH_HEAD.LOSS_WEIGHT)) == (MIN_DEPTH, MAX_DEPTH, BETA, WEIGHT)
    assert float(model.scale_depth_by_focal_lengths_factor) == FOCAL_FACTOR
    a = [torch.tensor(v, device="cuda", requires_grad=True) for v in a0]
    b = [torch.tensor(v, device="cuda", requires_grad=True) for v in b0]
    maps = [pl.cuda() * al + bl for pl, al, bl in zip(p, a, b)]
    depths = [c.gt[0], c.gt[1, :100, :200].clone()]  # per-image maps of the images' own sizes; the second is smaller than the canvas
    gt = DO.pad_depth(depths, Hp, Wp)
    out = FusedDenseDepthLoss(model)(maps, c.K, depths)
    assert list(out) == [f"loss_dense_depth_lvl_{l}" for l in range(5)] and all(v.dim() == 0 and v.requires_grad for v in out.values())
    sum(float(c.up[l]) * v for l, v in enumerate(out.values())).backward()
    g64, loss64 = c.grads(torch.float64, gt=gt)
    g32, _ = c.grads(torch.float32, gt=gt)
    for l, v in enumerate(out.values()):
        assert abs(float(v.detach()) - float(loss64[l])) <= 5e-6 * abs(float(loss64[l])), (l, float(v.detach()), float(loss64[l]))
    for l in range(5):
        bar, d32, gmax = GO.bar(g64[l], g32[l])
        pd = p[l].double()
        want_a, want_b = float((pd * g64[l]).sum()), float(g64[l].sum())
        n = pd.numel()
        slack = 2.0**-23 * max(np.log2(n), 1.0)
        bar_a = bar * float(pd.abs().sum()) + slack * float((pd * g64[l]).abs().sum())
        bar_b = bar * n + slack * float(g64[l].abs().sum())
        da, db = abs(float(a[l].grad) - want_a), abs(float(b[l].grad) - want_b)
        print(f"[dense_depth_grads] fused level {l}: a.grad {float(a[l].grad):.6e} (dev {da:.2e}, bar {bar_a:.2e}); "
              f"b.grad {float(b[l].grad):.6e} (dev {db:.2e}, bar {bar_b:.2e})")
        assert da <= bar_a and db <= bar_b, (l, da, bar_a, db, bar_b)
    with pytest.raises(ValueError, match="intrinsics has shape"):
        FusedDenseDepthLoss(model)(maps, c.K[:1], depths)
    with pytest.raises(ValueError, match="1 depth maps for dense_depth_maps of 2 images"):
        FusedDenseDepthLoss(model)(maps, c.K, depths[:1])
