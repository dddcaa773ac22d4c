"""Dense-depth loss of DD3DDenseDepth on the CPU: the oracle (tests/dense_depth_loss_oracle.py) against the goldens recorded from the
reference's own classes (tests/golden/make_dense_depth_loss_golden.py), the bindings' layout, the host staging and the config errors.
The HIP path is tests/test_dense_depth_loss_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dense_depth_loss_oracle as DO
from tests.golden import make_dense_depth_loss_golden as G

STRIDES = (8, 16, 32, 64, 128)
_CACHE = {}


def load_case(name):
    """(cfg, fixture, inputs with 'depth', oracle result on the reference's maps), computed once per session."""
    if name not in _CACHE:
        from dd3d_amd import get_cfg
        cfg = get_cfg(G.EXPERIMENT, G.case_overrides(name))
        g = np.load(G.fixture_path(name))
        inputs = G.case_inputs()
        for i, x in enumerate(inputs):
            x["depth"] = torch.from_numpy(g[f"gt{i}"])
        c3 = cfg.DD3D.FCOS3D
        K = torch.stack([x["intrinsics"] for x in inputs])
        maps = DO.upsampled_maps([g[f"raw{l}"] for l in range(5)], STRIDES, cfg.DD3D.FEATURE_LOCATIONS_OFFSET, K,
                                 c3.SCALE_DEPTH_BY_FOCAL_LENGTHS_FACTOR if c3.SCALE_DEPTH_BY_FOCAL_LENGTHS else None)
        gt = DO.pad_depth([x["depth"] for x in inputs], G.H, G.W)
        res = DO.dense_depth_loss(maps, gt, float(c3.MIN_DEPTH), float(c3.MAX_DEPTH), float(c3.LOSS.SMOOTH_L1_BETA), float(c3.DEPTH_HEAD.LOSS_WEIGHT))
        _CACHE[name] = (cfg, g, inputs, maps, gt, res)
    return _CACHE[name]


@pytest.mark.parametrize("name", list(G.CASES))
def test_oracle_reproduces_the_reference_loss_dict(name):
    """Keys in level order, every value within 2e-6 relative of the reference's: an f32 mean (the reference) against a float64 sum of the
    same f32 terms (the oracle), i.e. the reference's own summation error.  Measured on the three fixtures (printed below): the largest
    gap is 1.5e-7 relative (half_noscale level 0; ragged 6.7e-8, ragged_min0 0 at every level), so the 2e-6 bar holds as stated."""
    cfg, g, inputs, maps, gt, (losses, count, terms) = load_case(name)
    assert list(losses) == [f"loss_dense_depth_lvl_{l}" for l in range(5)]
    assert count == int(g["valid_count"])
    for l, (k, v) in enumerate(losses.items()):
        assert v.dtype == torch.float32 and v.dim() == 0
        ref = float(g["losses"][l])
        rel = abs(float(v) - ref) / abs(ref)
        print(f"{name} level {l}: oracle {float(v):.9g} reference {ref:.9g} rel {rel:.2e}")
        assert rel <= 2e-6, (name, k, float(v), ref)


@pytest.mark.parametrize("name", list(G.CASES))
def test_fixture_is_not_vacuous(name):
    """On the oracle side: a valid share between 5 % and 95 %, at least 20 % of the valid pixels on each side of beta (at level 0, whose
    map the ground truth was built around), and at least one pixel each below MIN_DEPTH, above MAX_DEPTH and exactly zero."""
    cfg, g, inputs, maps, gt, (losses, count, terms) = load_case(name)
    c3 = cfg.DD3D.FCOS3D
    beta = float(c3.LOSS.SMOOTH_L1_BETA)
    assert 0.05 <= count / gt.numel() <= 0.95
    M = DO.valid_mask(gt, float(c3.MIN_DEPTH), float(c3.MAX_DEPTH))
    n = (maps[0][M] - gt[M]).abs()
    assert float((n < beta).float().mean()) >= 0.20 and float((n >= beta).float().mean()) >= 0.20
    assert int((gt < float(c3.MIN_DEPTH)).sum()) >= 1 and int((gt > float(c3.MAX_DEPTH)).sum()) >= 1 and int((gt == 0).sum()) >= 1
    assert inputs[1]["image"].shape[-2:] != inputs[0]["image"].shape[-2:]  # ragged: the second image leaves padding
    # the golden bar of tests/test_dense_depth_loss_gpu.py is only sharp where few pixels sit in the beta +- delta band: n_cut / N <= 1 %,
    # recounted here from the reference's maps rather than taken from the file
    for l, m in enumerate(maps):
        delta = 1e-3 * float(m.abs().max())
        n_cut = int((((m[M] - gt[M]).abs() - beta).abs() <= delta).sum())
        assert n_cut == int(g["n_cut"][l]) and abs(delta - float(g["delta"][l])) <= 1e-9 and n_cut <= 0.01 * count, (name, l, n_cut, count)
        assert delta < 0.5 * beta


def test_padding_counts_with_min_depth_zero():
    """MIN_DEPTH 0.0: the padded pixels (and every no-return pixel) are valid; with the released 0.1 they are not."""
    _, _, inputs, _, gt, (_, count0, _) = load_case("ragged_min0")
    _, _, _, _, _, (_, count, _) = load_case("ragged")
    h1, w1 = inputs[1]["image"].shape[-2:]
    pad = G.H * G.W - h1 * w1
    assert pad > 0 and count0 >= count + pad and bool((gt[1, h1:, :] == 0).all()) and bool((gt[1, :, w1:] == 0).all())


def test_oracle_special_values():
    """A self-check of the test oracle (no product code involved)."""
    maps = [torch.full((1, 4, 8), 2.0), torch.full((1, 4, 8), 3.0)]
    gt = torch.zeros(1, 4, 8)
    out, count, _ = DO.dense_depth_loss(maps, gt, 0.1, 80.0, 0.05, 1.0)
    assert count == 0 and all(torch.isnan(v) for v in out.values())
    gt[0, 1, 2] = 2.03  # |2 - 2.03| < beta: 0.5 n^2, not divided by beta
    out, count, _ = DO.dense_depth_loss(maps, gt, 0.1, 80.0, 0.05, 1.0)
    n = torch.tensor(2.0) - torch.tensor(2.03)
    assert count == 1 and float(out["loss_dense_depth_lvl_0"]) == float(0.5 * n.abs()**2)
    n1 = (torch.tensor(3.0) - torch.tensor(2.03)).abs()
    assert float(out["loss_dense_depth_lvl_1"]) == float((n1 - 0.5 * 0.05) / np.sqrt(2))
    gt[0, 0, 0] = float("nan")
    out, count, _ = DO.dense_depth_loss(maps, gt, 0.1, 80.0, 0.05, 1.0)
    assert count == 2 and all(torch.isnan(v) for v in out.values())


def test_dense_depth_loss_args_layout_matches_header(hiplib):
    from dd3d_amd import hip
    out = (C.c_int64 * 32)()
    n = hiplib.dd3d_dense_depth_loss_layout(out, 32)
    names = ["raw", "gt", "inv_K", "partials", "out", "count", "h", "w", "stride", "divisor", "num_levels", "B", "Hp", "Wp", "pitch",
             "offset_half", "n_partials", "focal_factor", "min_depth", "max_depth", "beta", "loss_weight"]
    assert n == len(names) + 1 and [f[0] for f in hip.DenseDepthLossArgs._fields_] == names
    assert out[0] == C.sizeof(hip.DenseDepthLossArgs)
    assert [out[i + 1] for i in range(len(names))] == [getattr(hip.DenseDepthLossArgs, f).offset for f in names]
    assert hip.dense_depth_loss_blocks(1, 128, 128) == 16 and hip.dense_depth_loss_blocks(4, 384, 1280) == hip.DDL_MAX_BLOCKS


def test_level_divisors_are_the_float64_powers_rounded_once():
    from dd3d_amd.engine.dense_depth_loss import level_divisors
    d = level_divisors(5)
    assert d == [float(np.float32(np.sqrt(2)**l)) for l in range(5)] and d[0] == 1.0 and d[2] == float(np.float32(2.0000000000000004))


def test_staging_leaves_zeros_in_the_padding_after_a_full_size_batch():
    from dd3d_amd.engine.dense_depth_loss import stage_depth_canvas
    canvas = torch.full((2, 16, 32), 7.0)
    full = [torch.full((16, 32), 3.0, dtype=torch.float64), torch.full((16, 32), 4.0, dtype=torch.float16)]
    stage_depth_canvas(canvas, full, [(16, 32), (16, 32)])
    assert canvas.dtype == torch.float32 and bool((canvas[0] == 3).all()) and bool((canvas[1] == 4).all())
    ragged = [torch.full((16, 32), 5.0), torch.full((11, 27), 6.0)]
    stage_depth_canvas(canvas, ragged, [(16, 32), (11, 27)])
    assert bool((canvas[0] == 5).all()) and bool((canvas[1, :11, :27] == 6).all())
    assert bool((canvas[1, 11:, :] == 0).all()) and bool((canvas[1, :, 27:] == 0).all())
    assert torch.equal(canvas, DO.pad_depth(ragged, 16, 32))


def test_staging_rejects_maps_that_are_not_the_images_size():
    from dd3d_amd.engine.dense_depth_loss import stage_depth_canvas
    canvas = torch.zeros((2, 16, 32))
    ok = torch.ones(16, 32)
    for bad in (torch.ones(1, 16, 32), torch.ones(16, 31), torch.ones(16, 32, dtype=torch.int32), np.ones((16, 32), dtype=np.float32)):
        with pytest.raises(ValueError, match="image 1"):
            stage_depth_canvas(canvas, [ok, bad], [(16, 32), (16, 32)])
    assert bool((canvas == 0).all())  # a rejected batch leaves the canvas as it was


def _cpu_model(overrides):
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import META_ARCH_REGISTRY, get_cfg
    return META_ARCH_REGISTRY.get("DD3DDenseDepth")(get_cfg(G.EXPERIMENT, overrides))


def _labelled_inputs():
    from dd3d_amd.synthetic import make_depth_maps
    inputs = G.case_inputs()
    for x, d in zip(inputs, make_depth_maps(inputs)):
        x["depth"] = d
    return inputs


def test_config_and_input_errors_are_named_value_errors():
    """Raised before any plan is built, so they show on a machine without a GPU too."""
    no_head = dict(G.BASE_OVERRIDES, DD3D={"IN_FEATURES": G.BASE_OVERRIDES["DD3D"]["IN_FEATURES"]})
    model = _cpu_model(no_head)  # constructing the model needs no DEPTH_HEAD
    with pytest.raises(ValueError, match="DD3D.FCOS3D.DEPTH_HEAD"):
        model.compute_losses(_labelled_inputs())
    with pytest.raises(ValueError, match="DD3D.FCOS3D.DEPTH_HEAD.LOSS_WEIGHT"):
        _cpu_model(G._merge(no_head, {"DD3D": {"FCOS3D": {"DEPTH_HEAD": {"LOSS_TYPE": "L1"}}}})).compute_losses(_labelled_inputs())
    with pytest.raises(ValueError, match="berHu"):
        _cpu_model(G._merge(G.BASE_OVERRIDES, {"DD3D": {"FCOS3D": {"DEPTH_HEAD": {"LOSS_TYPE": "berHu"}}}})).compute_losses(_labelled_inputs())
    model = _cpu_model(G.BASE_OVERRIDES)
    inputs = _labelled_inputs()
    del inputs[1]["depth"]
    with pytest.raises(ValueError, match="image 1.*'depth'"):
        model.compute_losses(inputs)
    inputs = _labelled_inputs()
    inputs[1]["depth"] = torch.zeros(G.H, G.W)  # the canvas' size, not the (smaller) image's
    with pytest.raises(ValueError, match="image 1"):
        model.compute_losses(inputs)
    with pytest.raises(NotImplementedError):
        model(_labelled_inputs())  # forward() keeps raising
    with pytest.raises(NotImplementedError):
        model.train()


def test_make_depth_maps_shares_and_beta_split():
    from dd3d_amd.synthetic import make_depth_maps
    inputs = G.case_inputs()
    a = make_depth_maps(inputs, seed=7, valid_fraction=0.3)
    b = make_depth_maps(inputs, seed=7, valid_fraction=0.3)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not torch.equal(a[0], make_depth_maps(inputs, seed=8, valid_fraction=0.3)[0])
    for x, d in zip(inputs, a):
        assert d.dtype == torch.float32 and d.shape == x["image"].shape[-2:]
        n = d.numel()
        inside = ((d >= 0.1) & (d <= 80.0)).sum() / n
        assert abs(float(inside) - 0.3) < 0.01 and float((d == 0).sum() / n) > 0.5
        assert abs(float((d > 80.0).sum() / n) - 0.10) < 0.01 and abs(float((d < 0.1).sum() / n) - float((d == 0).sum() / n) - 0.05) < 0.01
    base = [torch.rand(G.H, G.W) * 60 + 5 for _ in inputs]
    for x, d, bm in zip(inputs, make_depth_maps(inputs, seed=7, valid_fraction=0.3, base=base), base):
        h, w = x["image"].shape[-2:]
        v = (d >= 0.1) & (d <= 80.0)
        e = (d - bm[:h, :w]).abs()[v]
        assert abs(float((e < 0.05).float().mean()) - 0.5) < 0.05 and float(((e - 0.05).abs()).min()) >= 1e-3 and float(e.max()) < 0.21
