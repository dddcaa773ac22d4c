"""Dense-depth loss of DD3DDenseDepth on the MI355X: dd3d_dense_depth_loss at its seam against the CPU oracle
(tests/dense_depth_loss_oracle.py) and, pixel by pixel, against the existing up-sampling kernel; DD3DDenseDepth.compute_losses end to end
against the oracle and the reference's goldens."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dense_depth_loss_oracle as DO
from tests.golden import make_dense_depth_loss_golden as G

pytestmark = pytest.mark.gpu

STRIDES = (8, 16, 32, 64, 128)
MIN_DEPTH, MAX_DEPTH, BETA, WEIGHT, FOCAL_FACTOR = 0.1, 80.0, 0.05, 1.0, 500.0


def raw_maps(B, Hp, Wp, seed):
    """Hand-made raw predictor maps (B, 1, h, w) per level, a different range per level, such that the focal-scaled values (/ ~9.5 and
    / ~7.6 for the two intrinsics below) and the unscaled ones both lie inside the depth range."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand((B, 1, Hp // s, Wp // s), generator=g) * (30.0 - 4.0 * l) + 20.0 + 3.0 * l) for l, s in enumerate(STRIDES)]


def intrinsics(B):
    from dd3d_amd.synthetic import KITTI_K
    K = torch.tensor(KITTI_K).float()
    return torch.stack([K * torch.tensor([[s], [s], [1.0]]) for s in ([0.1, 0.125] * B)[:B]])  # two different focal lengths in a batch


class Seam:
    """Device copies of one set of raw maps (NHWC, pitch 4, NaN in the channels nobody may read) and K^-1 as the plan computes it."""
    def __init__(self, lib, raw, K):
        from dd3d_amd import hip
        self.lib, self.hip = lib, hip
        self.B, self.L = raw[0].shape[0], len(raw)
        self.hw = [(int(r.shape[2]), int(r.shape[3])) for r in raw]
        self.Hp, self.Wp = self.hw[0][0] * STRIDES[0], self.hw[0][1] * STRIDES[0]
        self.dev = []
        for r in raw:
            t = torch.full((self.B, r.shape[2], r.shape[3], 4), float("nan"), dtype=torch.float32, device="cuda")
            t[..., 0] = r[:, 0].cuda()
            self.dev.append(t)
        self.K = K.reshape(self.B, 9).contiguous().cuda()
        self.inv_K = torch.zeros_like(self.K)
        hip.check(lib.dd3d_invert_intrinsics(self.K.data_ptr(), self.inv_K.data_ptr(), self.B, hip.current_stream()), "invert")
        nb = hip.dense_depth_loss_blocks(self.B, self.Hp, self.Wp)
        self.partials = torch.zeros((nb, hip.DDL_ROW), dtype=torch.float32, device="cuda")
        self.out = torch.zeros(self.L, dtype=torch.float32, device="cuda")
        self.count = torch.zeros(1, dtype=torch.int64, device="cuda")

    def loss(self, gt, half, focal, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, beta=BETA, weight=WEIGHT):
        """One dd3d_dense_depth_loss call: (per-level values as a CPU float32 tensor, valid count)."""
        from dd3d_amd.engine.dense_depth_loss import level_divisors
        hip = self.hip
        a = hip.DenseDepthLossArgs()
        for l in range(self.L):
            a.raw[l] = self.dev[l].data_ptr()
            a.h[l], a.w[l], a.stride[l] = self.hw[l][0], self.hw[l][1], STRIDES[l]
        for l, d in enumerate(level_divisors(self.L)):
            a.divisor[l] = d
        gt_dev = gt.to("cuda", torch.float32).contiguous()
        assert tuple(gt_dev.shape) == (self.B, self.Hp, self.Wp)
        a.gt, a.inv_K = gt_dev.data_ptr(), self.inv_K.data_ptr()
        a.partials, a.n_partials = self.partials.data_ptr(), self.partials.shape[0]
        a.out, a.count = self.out.data_ptr(), self.count.data_ptr()
        a.num_levels, a.B, a.Hp, a.Wp, a.pitch = self.L, self.B, self.Hp, self.Wp, 4
        a.offset_half, a.focal_factor = int(half), FOCAL_FACTOR if focal else 0.0
        a.min_depth, a.max_depth, a.beta, a.loss_weight = min_depth, max_depth, beta, weight
        self.out.fill_(-1.0)
        self.count.fill_(-1)
        hip.check(self.lib.dd3d_dense_depth_loss(C.byref(a), hip.current_stream()), "dense_depth_loss")
        torch.cuda.synchronize()
        return self.out.cpu(), int(self.count.cpu())

    def upsampled(self, half, focal):
        """The existing dd3d_aligned_bilinear_scale on the same raw maps: per level a (B, Hp, Wp) CPU tensor."""
        hip, maps = self.hip, []
        for l in range(self.L):
            o = torch.zeros((self.B, self.Hp, self.Wp), dtype=torch.float32, device="cuda")
            hip.check(self.lib.dd3d_aligned_bilinear_scale(self.dev[l].data_ptr(), o.data_ptr(), self.inv_K.data_ptr(), self.B, self.hw[l][0],
                                                           self.hw[l][1], 4, STRIDES[l], int(half), FOCAL_FACTOR if focal else 0.0,
                                                           hip.current_stream()), "aligned_bilinear")
            maps.append(o)
        torch.cuda.synchronize()
        return [m.cpu() for m in maps]


def oracle_maps(raw, K, half, focal):
    return DO.upsampled_maps(raw, STRIDES, "half" if half else "none", K, FOCAL_FACTOR if focal else None)


def sparse_gt(B, Hp, Wp, base, seed):
    """make_depth_maps around the oracle's level-0 map: zeros, values below / above the range, base +- d on both sides of beta."""
    from dd3d_amd.synthetic import make_depth_maps
    fake = [{"image": torch.empty((3, Hp, Wp), dtype=torch.uint8)} for _ in range(B)]
    return torch.stack(make_depth_maps(fake, seed=seed, valid_fraction=0.4, base=[base[i] for i in range(B)], min_depth=MIN_DEPTH,
                                       max_depth=MAX_DEPTH, beta=BETA))


def assert_close(out, count, ref, ref_count, what):
    """5e-6 relative on every level (the bar tests/test_losses_gpu.py uses for loss sums), the count exact."""
    assert count == ref_count, (what, count, ref_count)
    for l, v in enumerate(ref.values()):
        rel = abs(float(out[l]) - float(v)) / abs(float(v))
        print(f"{what} level {l}: hip {float(out[l]):.9g} oracle {float(v):.9g} rel {rel:.2e}")
        assert rel <= 5e-6, (what, l, float(out[l]), float(v))


# ------------------------------------------------------------------------------------------------ 1. the seam against the oracle
@pytest.mark.parametrize("focal", [True, False], ids=["focal", "nofocal"])
@pytest.mark.parametrize("half", [False, True], ids=["none", "half"])
@pytest.mark.parametrize("shape", [(2, 128, 256), (1, 128, 128)], ids=["2x128x256", "1x128x128"])
def test_seam_matches_oracle(hiplib, shape, half, focal):
    """Hand-made raw maps, strides 8 .. 128; on 1 x 128 x 128 the last level is 1 x 1 and every tap clamps."""
    B, Hp, Wp = shape
    raw, K = raw_maps(B, Hp, Wp, seed=11), intrinsics(B)
    maps = oracle_maps(raw, K, half, focal)
    gt = sparse_gt(B, Hp, Wp, maps[0], seed=21)
    ref, ref_count, terms = DO.dense_depth_loss(maps, gt, MIN_DEPTH, MAX_DEPTH, BETA, WEIGHT)
    assert 0.05 < ref_count / gt.numel() < 0.95 and 0.2 < float((terms[0] < 0.5 * BETA * BETA).float().mean()) < 0.8  # both branches at level 0
    seam = Seam(hiplib, raw, K)
    out, count = seam.loss(gt, half, focal)
    assert_close(out, count, ref, ref_count, f"seam {shape} half={half} focal={focal}")
    out2, count2 = seam.loss(gt, half, focal)
    assert torch.equal(out, out2) and count2 == count  # no float atomics: bit for bit


# ------------------------------------------------------------------------------------------------ 2. one valid pixel: bit-exact
def f32_level_values(v, gt, beta, weight, divisors):
    """Points 4-5 of the loss in float32, one operation at a time, for the single term of a one-pixel mean."""
    f = np.float32
    out = []
    for vl, d in zip(v, divisors):
        n = np.abs(f(vl) - f(gt))
        term = n if f(beta) < f(1e-5) else (f(0.5) * (n * n) if n < f(beta) else n - f(0.5) * f(beta))
        mean = term / f(1.0)
        out.append((f(weight) * mean) / f(d))
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize("half", [False, True], ids=["none", "half"])
def test_single_pixel_is_bit_identical_to_the_upsampling_kernel(hiplib, half):
    """The ground truth is valid at exactly one pixel, so the mean has one term and no summation order is involved: every level's value
    must EQUAL the float32 statement of the loss evaluated on what dd3d_aligned_bilinear_scale writes at that pixel for the same raw
    map.  This pins the fused interpolation to the existing kernel."""
    from dd3d_amd.engine.dense_depth_loss import level_divisors
    B, Hp, Wp = 2, 128, 256
    raw, K = raw_maps(B, Hp, Wp, seed=12), intrinsics(B)
    seam = Seam(hiplib, raw, K)
    div = level_divisors(5)
    # the canvas corners, the last row and column, a pixel with x < stride / 2 (clamped under "half" on every level), interior pixels
    pixels = [(0, 0, 0), (0, 0, Wp - 1), (0, Hp - 1, 0), (1, Hp - 1, Wp - 1), (1, Hp - 1, 77), (0, 53, Wp - 1), (1, 40, 2), (0, 3, 130), (1, 71, 149),
              (0, 64, 128)]
    for focal in (True, False):
        maps = seam.upsampled(half, focal)
        for k, (b, y, x) in enumerate(pixels):
            v = [float(m[b, y, x]) for m in maps]
            for dgt in (0.01 + 0.003 * k, 0.3 + 0.01 * k):  # below and above beta at level 0
                gt = torch.zeros((B, Hp, Wp))
                gt[b, y, x] = v[0] + dgt
                assert MIN_DEPTH < float(gt[b, y, x]) < MAX_DEPTH
                out, count = seam.loss(gt, half, focal)
                want = f32_level_values(v, float(gt[b, y, x]), BETA, WEIGHT, div)
                assert count == 1
                assert out.numpy().tobytes() == want.tobytes(), (half, focal, (b, y, x), out.tolist(), want.tolist())


# ------------------------------------------------------------------------------------------------ 3. special values
def test_special_values_at_the_seam(hiplib):
    B, Hp, Wp = 1, 128, 128
    raw, K = raw_maps(B, Hp, Wp, seed=13), intrinsics(B)
    seam = Seam(hiplib, raw, K)
    maps = oracle_maps(raw, K, False, True)
    gt = torch.zeros((B, Hp, Wp))
    gt[0, 5, 7], gt[0, 90, 3] = -1.0, 200.0
    out, count = seam.loss(gt, False, True)  # nothing valid: the mean of an empty selection at every level
    assert count == 0 and bool(torch.isnan(out).all())
    gt[0, 10, 10], gt[0, 11, 100], gt[0, 100, 50] = 3.0, 4.0, 5.0
    out, count = seam.loss(gt, False, True)
    ref, ref_count, _ = DO.dense_depth_loss(maps, gt, MIN_DEPTH, MAX_DEPTH, BETA, WEIGHT)
    assert_close(out, count, ref, 3, "three valid pixels")
    # exactly MIN_DEPTH and exactly MAX_DEPTH (as float32) are valid
    gt[0, 20, 20], gt[0, 21, 21] = float(np.float32(MIN_DEPTH)), float(np.float32(MAX_DEPTH))
    out, count = seam.loss(gt, False, True)
    ref, ref_count, _ = DO.dense_depth_loss(maps, gt, MIN_DEPTH, MAX_DEPTH, BETA, WEIGHT)
    assert ref_count == 5
    assert_close(out, count, ref, 5, "range ends")
    # beta = 0: plain L1
    out, count = seam.loss(gt, False, True, beta=0.0)
    ref, ref_count, _ = DO.dense_depth_loss(maps, gt, MIN_DEPTH, MAX_DEPTH, 0.0, WEIGHT)
    l1 = [float((m[0][DO.valid_mask(gt[0], MIN_DEPTH, MAX_DEPTH)] - gt[0][DO.valid_mask(gt[0], MIN_DEPTH, MAX_DEPTH)]).abs().double().mean()) for m in maps]
    assert all(abs(float(v) * float(np.sqrt(2)**l) - l1[l]) <= 1e-5 * l1[l] for l, v in enumerate(ref.values()))
    assert_close(out, count, ref, 5, "beta 0")
    # one NaN ground-truth pixel passes both comparisons and makes every level NaN
    gt[0, 64, 64] = float("nan")
    out, count = seam.loss(gt, False, True)
    assert count == 6 and bool(torch.isnan(out).all())


def test_bad_arguments_are_rejected(hiplib):
    from dd3d_amd import hip
    B, Hp, Wp = 1, 128, 128
    seam = Seam(hiplib, raw_maps(B, Hp, Wp, seed=14), intrinsics(B))
    a = hip.DenseDepthLossArgs()
    assert hiplib.dd3d_dense_depth_loss(C.byref(a), hip.current_stream()) != 0  # no levels, null pointers
    seam.hw[2] = (seam.hw[2][0], seam.hw[2][1] - 1)  # h * stride == Hp but w * stride != Wp
    with pytest.raises(RuntimeError, match="does not tile"):
        seam.loss(torch.zeros((B, Hp, Wp)), False, False)


# ------------------------------------------------------------------------------------------------ 4. the looping regime
def test_canvas_larger_than_one_sweep_of_the_capped_grid(hiplib):
    """1 x 768 x 1408 = 1 081 344 pixels; one sweep of the capped grid covers DDL_MAX_BLOCKS x 256 threads x 4 pixels = 1 048 576."""
    from dd3d_amd import hip
    B, Hp, Wp = 1, 768, 1408
    assert B * Hp * Wp > hip.DDL_MAX_BLOCKS * hip.DDL_QUADS_PER_BLOCK * 4 and hip.dense_depth_loss_blocks(B, Hp, Wp) == hip.DDL_MAX_BLOCKS
    raw, K = raw_maps(B, Hp, Wp, seed=15), intrinsics(B)
    maps = oracle_maps(raw, K, True, True)
    gt = sparse_gt(B, Hp, Wp, maps[0], seed=25)
    ref, ref_count, _ = DO.dense_depth_loss(maps, gt, MIN_DEPTH, MAX_DEPTH, BETA, WEIGHT)
    out, count = Seam(hiplib, raw, K).loss(gt, True, True)
    assert_close(out, count, ref, ref_count, "looping 1x768x1408")


# ------------------------------------------------------------------------------------------------ 5. end to end
_MODELS = {}


def case_model(name, math=None, use_graph=True):
    from dd3d_amd import get_cfg
    from tests.util import bundle, gpu_model
    key = (name, math, use_graph)
    if key not in _MODELS:
        cfg, sd = bundle(G.EXPERIMENT, G.CALIB, G.case_overrides(name))
        _MODELS[key] = (cfg, gpu_model(cfg, G.case_state_dict(name, sd), use_graph=use_graph, math=math))
    return _MODELS[key]


def case_inputs(name):
    g = np.load(G.fixture_path(name))
    inputs = G.case_inputs()
    for i, x in enumerate(inputs):
        x["depth"] = torch.from_numpy(g[f"gt{i}"])
    return g, inputs


def test_compute_losses_is_consistent_with_predict_dense_depth(hiplib):
    """The ragged 2 x 128 x 256 case: within 5e-6 relative of the oracle fed the maps the same model's predict_dense_depth returns,
    bit-identical on a second call, with use_graph = False, and after an intervening full-size batch (stale padding)."""
    from dd3d_amd.synthetic import make_depth_maps, make_inputs
    cfg, model = case_model("ragged_min0")  # MIN_DEPTH 0.0: the padding counts, so stale pixels there would show
    g, inputs = case_inputs("ragged_min0")
    c3 = cfg.DD3D.FCOS3D
    losses = model.compute_losses(inputs)
    assert list(losses) == [f"loss_dense_depth_lvl_{l}" for l in range(5)]
    assert all(v.dtype == torch.float32 and v.dim() == 0 and v.is_cuda for v in losses.values())
    plan = model.get_loss_plan(2, G.H, G.W)
    assert plan.graph is not None and not hasattr(plan, "depth_maps")  # one hipGraph, no full-resolution maps
    count = int(plan.valid_count.cpu())
    maps = [m.cpu() for m in model.predict_dense_depth(inputs)]
    gt = DO.pad_depth([x["depth"] for x in inputs], G.H, G.W)
    ref, ref_count, _ = DO.dense_depth_loss(maps, gt, float(c3.MIN_DEPTH), float(c3.MAX_DEPTH), float(c3.LOSS.SMOOTH_L1_BETA), float(c3.DEPTH_HEAD.LOSS_WEIGHT))
    first = torch.stack(list(losses.values())).cpu()
    assert_close(first, count, ref, ref_count, "compute_losses vs oracle on predict_dense_depth")
    assert count == int(g["valid_count"])
    again = torch.stack(list(model.compute_losses(inputs).values())).cpu()
    assert torch.equal(first, again)
    # a full-size batch in between: its ground truth must not survive in the second image's padding
    full = make_inputs(2, G.H, G.W)
    for x, d in zip(full, make_depth_maps(full, seed=5)):
        x["depth"] = d.cuda().double()  # (a device tensor of another float dtype)
    other = torch.stack(list(model.compute_losses(full).values())).cpu()
    assert not torch.equal(other, first)
    after = torch.stack(list(model.compute_losses(inputs).values())).cpu()
    assert torch.equal(first, after) and int(plan.valid_count.cpu()) == count
    _, eager = case_model("ragged_min0", use_graph=False)
    launched = torch.stack(list(eager.compute_losses(inputs).values())).cpu()
    assert eager.get_loss_plan(2, G.H, G.W).graph is None and torch.equal(first, launched)


@pytest.mark.parametrize("name,math", [(n, None) for n in G.CASES] + [("ragged", "bf16x3")], ids=lambda v: str(v))
def test_compute_losses_matches_the_reference_golden(hiplib, name, math):
    """The bar follows from the forward's: with delta = 1e-3 * max|reference map| (the per-pixel bar of tests/test_dense_depth.py) a level's
    loss may differ from the reference's by at most  w / sqrt(2)^l * (delta + 0.024 * n_cut / N),  n_cut = the valid pixels whose |x| lies
    within delta of beta (recorded by the generator), 0.024 = the jump of this smooth-L1 at beta = 0.05 (0.025 - 0.00125).  n_cut / N is
    at most 0.2 % on every fixture and level, and delta at most 0.02 (tests/test_dense_depth_loss.py asserts both).  Measured on the
    MI355X: |diff| at most 9.5e-7 on the default arithmetic and 2.9e-6 on bf16x3, against bars of 1.3e-4 .. 2.0e-2."""
    cfg, model = case_model(name, math=math)
    g, inputs = case_inputs(name)
    losses = model.compute_losses(inputs)
    plan = model.get_loss_plan(2, G.H, G.W)
    N = int(g["valid_count"])
    assert list(losses) == [f"loss_dense_depth_lvl_{l}" for l in range(5)] and int(plan.valid_count.cpu()) == N
    w = float(cfg.DD3D.FCOS3D.DEPTH_HEAD.LOSS_WEIGHT)
    for l, v in enumerate(losses.values()):
        bar = w / float(np.sqrt(2)**l) * (float(g["delta"][l]) + 0.024 * int(g["n_cut"][l]) / N)
        dev = abs(float(v) - float(g["losses"][l]))
        print(f"{name} math={math} level {l}: hip {float(v):.9g} reference {float(g['losses'][l]):.9g} |diff| {dev:.3e} bar {bar:.3e}")
        assert dev <= bar, (name, l, float(v), float(g["losses"][l]), bar)
