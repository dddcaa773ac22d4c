"""Tower backward on the MI355X (csrc/tower_grads.hip, engine.LossPlan(tower_grads=True)): dd3d_tower_wgrad and dd3d_tower_dgrad at
their C-ABI seam on seeded dense layers (tests/tower_grad_cases.py) against the float64 autograd of the CPU oracle
(tests/tower_grad_oracle.py), in the three activation storages and every input-gradient tile; sentinel-framed outputs, an all-masked
layer, a zero scale, da_add, the shared filter's sum, rejected arguments, determinism; DD3D.compute_losses(tower_grads=True) end to
end; and the reference-modules golden.

The bar of a family (weight, norm_weight, norm_bias / bias, da, feature) in a case is 8 * max(d32, 2^-23 * max|g64|): d32 is the
deviation of the oracle's float32 autograd from its float64 autograd, computed here on the CPU (loss_grad_oracle.bar).
"""
import pytest
import torch

from tests import loss_grad_cases as GC
from tests import predictor_grad_cases as PC
from tests import tower_grad_cases as TC
from tests import tower_grad_oracle as TO

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
POISON = 3.0e30  # pad words of the inputs: a kernel that read them would not stay finite


def nhwc(x, pitch, pad=POISON):
    B, C, H, W = x.shape
    t = torch.full((B, H, W, pitch), pad, dtype=torch.float32)
    t[..., :C] = x.permute(0, 2, 3, 1)
    return t.contiguous().cuda()


def _store(tensors, storage, plane_scale, pad):
    """Per-level NCHW float32 -> (device buffers, bindings (mode, address, pitch, plane scale), the float32 values the storage decodes to)."""
    from dd3d_amd import hip
    C_ = tensors[0].shape[1]
    if storage == "f32":
        bufs = [nhwc(a, C_ + pad) for a in tensors]
        return bufs, [(hip.PG_ACT_F32, b.data_ptr(), C_ + pad, 1.0) for b in bufs], list(tensors)
    enc = [TC.encode_f16x2(a, plane_scale) if storage == "f16x2" else TC.encode_bf16x3(a) for a in tensors]
    bufs = [p.cuda() for p, _ in enc]
    mode = hip.PG_ACT_F16X2 if storage == "f16x2" else hip.PG_ACT_BF16X3
    return bufs, [(mode, b.data_ptr(), 0, float(plane_scale)) for b in bufs], [d for _, d in enc]


def run_seam(case, storage="f32", plane_scale=1.0, y_storage=None, y_plane_scale=None, pad=0, dgrad_rows=0, fill=SENTINEL, da_add=True):
    """One weight-gradient and one input-gradient call on a LayerCase.  Returns (results shaped like TO.layer_grads, on the CPU; the
    TowerLayerGrads; the float32 x and y the storages decode to)."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import TowerLayerGrads
    xb, xbind, xdec = _store(case.x, storage, plane_scale, pad)
    yb, ybind, ydec = _store(case.y, y_storage or storage, y_plane_scale or plane_scale, pad)
    gpitch = case.Cout + 4  # (always padded with poison words: the gradient's layout does not depend on the storages of x and y)
    g = [nhwc(v, gpitch) for v in case.g]
    w = case.w.permute(0, 2, 3, 1).contiguous().cuda()
    scale = [s.contiguous().cuda() for s in case.scale]
    add = [nhwc(v, case.Cin) for v in case.da_add] if (case.da_add is not None and da_add) else None
    lay = TowerLayerGrads("cuda", case.B, case.level_hw, case.Cin, case.Cout, xbind, ybind, g, gpitch, w, scale, da_add=add, fill=fill, guard=64,
                          dgrad_rows=dgrad_rows)
    lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    lay.keep_alive = (xb, yb)
    return collect(lay), lay, xdec, ydec


def collect(lay):
    nchw_w = lambda t: t.view(lay.Cout, 3, 3, lay.Cin).permute(0, 3, 1, 2).cpu()
    return {"dw_level": [nchw_w(lay.dw_level[l]) for l in range(lay.L)], "dw": nchw_w(lay.dw), "q": [lay.q[l].cpu() for l in range(lay.L)],
            "r": [lay.r[l].cpu() for l in range(lay.L)], "da": [d.permute(0, 3, 1, 2).cpu() for d in lay.da]}


def check(got, ref64, ref32, what, families=TO.FAMILIES):
    a, b, k = TO.family_vectors(ref64), TO.family_vectors(ref32), TO.family_vectors(got)
    for fam in families:
        assert bool(torch.isfinite(k[fam]).all()), (what, fam)
        bar, d32, gmax = TO.bar(a[fam], b[fam], torch.ones(a[fam].shape[0], dtype=torch.bool))
        dev = float((k[fam].double() - a[fam]).abs().max())
        print(f"[tower_grads] {what} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} "
              f"(uses {8 * dev / bar if bar > 0 else 0.0:.2f} of the factor 8)")
        assert dev <= bar, (what, fam, dev, bar, d32, gmax)


def frame_ok(lay, fill=SENTINEL):
    """Guard words keep the sentinel; every output word is written (the scratch rows in use included)."""
    assert lay.guards_intact(fill)
    for t in [lay.part, lay.qpart, lay.dw_level, lay.dw, lay.q, lay.r] + lay.da:
        assert not bool((t == fill).any())


def same_bits(a, b):
    va, vb = TO.family_vectors(a), TO.family_vectors(b)
    return all(torch.equal(va[f], vb[f]) for f in va)


# level shapes: 1x1 (only the centre tap lands), 1x257 (a row longer than four units, the last one pixel long), 3x10 and 5x7 (odd, a
# multiple of no tile), 30x70 (several units per slice, several tiles per level), the pyramid of a 64x128 canvas, 100x64 x 3 at 256
# channels (300 units: the slab's byte budget decides the slice size); channels 32, 64, 256 and 64 -> 32; the input-gradient tiles of
# 2, 4 and 8 rows forced (the automatic choice takes the larger ones at sizes no seam case has: test_input_gradient_tiles_give_the_same_bits)
SEAM_CASES = {
    "1x1_c32_f32": (dict(level_hw=[(1, 1)], B=1, Cin=32, seed=1), dict(storage="f32")),
    "1x257_c64_f16s16": (dict(level_hw=[(1, 257)], B=1, Cin=64, seed=2), dict(storage="f16x2", plane_scale=16.0)),
    "3x10_5x7_c64to32_bf16x3": (dict(level_hw=[(3, 10), (5, 7)], B=2, Cin=64, Cout=32, seed=3), dict(storage="bf16x3", dgrad_rows=4)),
    "3x10_5x7_c32to64_f32_x_f16_y": (dict(level_hw=[(3, 10), (5, 7)], B=2, Cin=32, Cout=64, seed=8),
                                     dict(storage="f32", y_storage="f16x2", y_plane_scale=16.0, dgrad_rows=8)),
    "30x70_c32_f32": (dict(level_hw=[(30, 70)], B=1, Cin=32, seed=4), dict(storage="f32", dgrad_rows=8)),
    "pyramid_c256_f16s1": (dict(level_hw=PC.PYRAMID_64x128, B=2, Cin=256, seed=5), dict(storage="f16x2", plane_scale=1.0)),
    "pyramid_c256_f32_rows8": (dict(level_hw=PC.PYRAMID_64x128, B=2, Cin=256, seed=6, with_da_add=True), dict(storage="f32", dgrad_rows=8)),
    "pyramid_c64_bf16x3_rows4": (dict(level_hw=PC.PYRAMID_64x128, B=2, Cin=64, seed=7), dict(storage="bf16x3", dgrad_rows=4)),
    "100x64_b3_c256_f32_budget": (dict(level_hw=[(100, 64)], B=3, Cin=256, seed=9), dict(storage="f32")),
}


@pytest.mark.parametrize("name", list(SEAM_CASES))
def test_seam_against_oracle(hiplib, name):
    kw, run = SEAM_CASES[name]
    case = TC.LayerCase(**kw)
    run = dict(run, pad=4 if run["storage"] == "f32" and "y_storage" not in run else 0)
    got, lay, xdec, ydec = run_seam(case, **run)
    frame_ok(lay)
    check(got, case.ref(torch.float64, xdec, ydec), case.ref(torch.float32, xdec, ydec), name)
    again, _, _, _ = run_seam(case, **run)
    assert same_bits(again, got), name  # the same call twice: the same bits


def test_slab_budget_decides_the_slice_size(hiplib):
    import ctypes as C
    from dd3d_amd import hip
    assert hip.tower_grad_slices(1, [(1, 1)], 32, 32) == 1 and hip.tower_grad_slices(1, [(1, 257)], 64, 64) == 2
    assert hip.tower_grad_slices(1, [(30, 70)], 32, 32) == 15  # 60 units, four per slice
    assert hip.tower_grad_slices(2, PC.PYRAMID_64x128, 256, 256) == 4 + 2 + 1 + 1 + 1
    assert hip.tower_grad_slices(3, [(100, 64)], 256, 256) == 60  # 300 units against 71 slices of 2.36 MB: five per slice
    case = TC.LayerCase(level_hw=[(3, 10)], B=1, Cin=32, seed=51)
    _, lay, _, _ = run_seam(case)
    assert hiplib.dd3d_tower_grad_slices(C.byref(lay.args)) == lay.n_slices == 1
    bare = hip.TowerGradArgs()  # the count needs the geometry and the channel counts alone: no pointer is set
    bare.num_levels, bare.B, bare.Cin, bare.Cout, bare.H[0], bare.W[0] = 1, 3, 256, 256, 100, 64
    assert hiplib.dd3d_tower_grad_slices(C.byref(bare)) == 60
    bare.Cout = 48
    assert hiplib.dd3d_tower_grad_slices(C.byref(bare)) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_tower_grad_slices")


@pytest.mark.parametrize("storage,ps", [("f16x2", 16.0), ("f16x2", 1.0), ("bf16x3", 1.0)])
def test_plane_and_f32_paths_agree_on_the_same_values(hiplib, storage, ps):
    kw = dict(level_hw=[(5, 7), (3, 10)], B=2, Cin=64, seed=11)
    case = TC.LayerCase(**kw)
    got, _, xdec, ydec = run_seam(case, storage, ps)
    twin = TC.LayerCase(**kw)
    twin.x, twin.y = xdec, ydec  # the f32 loader on the values the planes decode to
    f32, _, _, _ = run_seam(twin, "f32")
    assert same_bits(got, f32)  # the loaders hand over the same float32 values
    check(got, case.ref(torch.float64, xdec, ydec), case.ref(torch.float32, xdec, ydec), f"{storage}@{ps}")


def test_input_gradient_tiles_give_the_same_bits(hiplib):
    """256 x 256 pixels at 32 channels: 512 tiles of 8 x 16, so the automatic choice takes the largest tile; 128 x 256: the 4-row tile.
    The forced tiles of 2, 4 and 8 rows and the automatic one write the same bits (a pixel's sum has one order), and the oracle's."""
    for hw in ((256, 256), (128, 256)):
        case = TC.LayerCase(level_hw=[hw], B=1, Cin=32, seed=61)
        auto, lay, _, _ = run_seam(case)
        frame_ok(lay)
        for rows in (2, 4, 8):
            forced, _, _, _ = run_seam(case, dgrad_rows=rows)
            assert all(torch.equal(a, b) for a, b in zip(forced["da"], auto["da"])), (hw, rows)
        check(auto, case.ref(torch.float64), case.ref(torch.float32), f"tiles:{hw[0]}x{hw[1]}", families=("da", ))


def test_all_masked_layer_gives_exact_zeros(hiplib):
    case = TC.LayerCase(level_hw=[(3, 10), (5, 7)], B=2, Cin=32, seed=21, all_masked=True)
    got, lay, _, _ = run_seam(case)
    frame_ok(lay)
    for fam, v in TO.family_vectors(got).items():
        assert float(v.abs().max()) == 0.0, fam


def test_zero_scale_level(hiplib):
    """s_l = 0 on one level: everything finite, dw gets nothing from that level, its r and q are the oracle's (no division by s_l), its
    da is an exact zero; an infinite scale on a masked entry would not matter either (exact zeros are staged, not products)."""
    kw = dict(level_hw=[(3, 10), (5, 7)], B=2, Cin=32, seed=23, zero_scale_level=1)
    case = TC.LayerCase(**kw)
    assert bool((case.y[1] > 0).any())  # the level still has live entries (its shift is positive): r and q are not trivially zero
    got, lay, _, _ = run_seam(case)
    frame_ok(lay)
    check(got, case.ref(torch.float64), case.ref(torch.float32), "zero-scale")
    assert float(got["da"][1].abs().max()) == 0.0 and float(got["r"][1].abs().max()) > 0.0 and float(got["q"][1].abs().max()) > 0.0
    assert torch.equal(got["dw"], case.scale[0][:, None, None, None] * got["dw_level"][0])  # fmaf(s_1 = 0, P_1, s_0 * P_0) = s_0 * P_0


def test_da_add_is_added_last(hiplib):
    case = TC.LayerCase(level_hw=[(3, 10), (5, 7)], B=2, Cin=64, Cout=32, seed=25, with_da_add=True)
    with_add, lay, _, _ = run_seam(case)
    frame_ok(lay)
    without, _, _, _ = run_seam(case, da_add=False)
    for l in range(case.L):
        assert torch.equal(with_add["da"][l], case.da_add[l] + without["da"][l])  # da = da_add + sum: one rounding
    other, lay2, _, _ = run_seam(case, fill=7.5)
    frame_ok(lay2, 7.5)
    assert same_bits(other, with_add)  # nothing of the buffers' previous contents enters
    check(with_add, case.ref(torch.float64), case.ref(torch.float32), "da_add")


def test_shared_filter_sum_equals_scaled_per_level_partials(hiplib):
    case = TC.LayerCase(level_hw=PC.PYRAMID_64x128, B=2, Cin=32, seed=41)
    got, _, _, _ = run_seam(case)
    total, mag = torch.zeros_like(got["dw"], dtype=torch.float64), torch.zeros_like(got["dw"], dtype=torch.float64)
    for l in range(case.L):
        s = case.scale[l][:, None, None, None].double()
        total, mag = total + s * got["dw_level"][l].double(), mag + (s * got["dw_level"][l].double()).abs()
    # the kernel's sum is one fmaf per level: at most one float32 rounding of a partial sum per level
    assert bool(((total - got["dw"].double()).abs() <= case.L * 2.0**-24 * mag).all())


def test_bad_arguments_are_rejected(hiplib):
    import ctypes as C
    from dd3d_amd import hip
    case = TC.LayerCase(level_hw=[(3, 10)], B=1, Cin=32, seed=51)
    _, lay, _, _ = run_seam(case, pad=4)
    lib, st = hip.lib(), hip.current_stream()
    a = lay.args
    both = (("dd3d_tower_wgrad", lib.dd3d_tower_wgrad), ("dd3d_tower_dgrad", lib.dd3d_tower_dgrad))
    for field, value, entries in (("Cin", 48, both), ("Cin", 288, both), ("Cout", 16, both), ("Cout", 320, both), ("g_pitch", 34, both), ("g_pitch", 28, both),
                                  ("x_pitch", 34, both[:1]), ("x_pitch", 28, both[:1]), ("y_pitch", 34, both), ("x_mode", 7, both[:1]), ("y_mode", 7, both),
                                  ("n_slices", 0, both[:1]), ("dgrad_rows", 3, both), ("num_levels", 0, both), ("B", 0, both)):
        old = getattr(a, field)
        setattr(a, field, value)
        for name, fn in entries:
            assert fn(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(name), (field, name)
        setattr(a, field, old)
    for field, entries in (("g", both), ("y", both), ("scale", both), ("x", both[:1]), ("da", both[1:])):
        arr = getattr(a, field)
        old = arr[0]
        arr[0] = None
        for name, fn in entries:
            assert fn(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(name), (field, name)
        arr[0] = old
    for field, entries in (("w", both), ("part", both[:1]), ("qpart", both[:1]), ("dw_level", both[:1]), ("dw", both[:1]), ("q", both[:1]), ("r", both[:1])):
        old = getattr(a, field)
        setattr(a, field, None)
        for name, fn in entries:
            assert fn(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(name), (field, name)
        setattr(a, field, old)
    a.y_mode, a.y_plane_scale = hip.PG_ACT_F16X2, 0.0
    assert lib.dd3d_tower_dgrad(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_tower_dgrad")
    a.y_mode, a.y_plane_scale = hip.PG_ACT_F32, 1.0
    assert lib.dd3d_tower_grad_slices(None) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_tower_grad_slices")
    assert lib.dd3d_tower_wgrad(C.byref(a), st) == 0 and lib.dd3d_tower_dgrad(C.byref(a), st) == 0  # the restored arguments still run
    torch.cuda.synchronize()
    frame_ok(lay)


# ---------------------------------------------------------------------------------------------------------------------- end to end
def _layer_inputs(plan, key):
    """A captured layer's inputs as the oracle takes them: the plan's own stored x and y (the values its storages decode to), the
    incoming gradient, filter and scales, NCHW on the CPU."""
    lay = plan.tower_layers[key]
    info = plan.tower_info[key]
    g, w, scale, da_add, _ = lay.keep
    case = TC.LayerCase.__new__(TC.LayerCase)
    case.x = [v.nchw().float().cpu().contiguous() for v in info["x"]]
    case.y = [v.nchw().float().cpu().contiguous() for v in info["y"]]
    case.g = [t[..., :lay.Cout].permute(0, 3, 1, 2).cpu().contiguous() for t in g]
    case.w, case.scale = w.permute(0, 3, 1, 2).cpu().contiguous(), [s.cpu() for s in scale]
    case.da_add = None if da_add is None else [t.permute(0, 3, 1, 2).cpu().contiguous() for t in da_add]
    return case, lay


def _check_named(got_p, got_f, ref64, ref32, what):
    p64, f64 = ref64
    p32, f32 = ref32
    fams = {}
    for k in sorted(got_p):
        fams.setdefault(TO.family_of(k), []).append(k)
    rows = [(fam, [d[k] for k in ks], [p64[k] for k in ks], [p32[k] for k in ks]) for fam, ks in fams.items() for d in (got_p, )]
    rows.append(("feature", [got_f[k] for k in sorted(got_f)], [f64[k] for k in sorted(got_f)], [f32[k] for k in sorted(got_f)]))
    for fam, c, a, b in rows:
        c, a, b = (torch.cat([v.reshape(-1).cpu() for v in vs]) for vs in (c, a, b))
        bar, d32, gmax = TO.bar(a.double(), b, torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((c.double() - a.double()).abs().max())
        print(f"[tower_grads] {what} named {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} "
              f"(uses {8 * dev / bar if bar > 0 else 0.0:.2f} of the factor 8)")
        assert dev <= bar and gmax > 0.0, (what, fam, dev, bar)


def _end_to_end(exp, weights, B, H, W, ds, math=None, act_scale=None):
    from dd3d_amd.synthetic import make_gt_instances, make_inputs
    from tests.test_loss_grads_gpu import _model
    model = _model(exp, weights)
    model.math, model.act_scale = math, act_scale
    nusc = hasattr(model, "attr_logits")
    inputs = make_inputs(B, H, W, dataset=ds)
    gt = make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES,
                           num_attributes=model.attr_logits.out_channels if nusc else None, empty_images=(1, ))
    for x, g in zip(inputs, gt):
        x["instances"] = g
    ref_losses, ref_grads, ref_params = model.compute_losses(inputs, predictor_grads=True)
    losses, grads, params = model.compute_losses(inputs, tower_grads=True)
    # the loss dict and everything the predictor backward returns are those of predictor_grads=True, bit for bit
    assert list(losses) == list(ref_losses) and all(torch.equal(losses[k], ref_losses[k]) for k in losses)
    assert all(torch.equal(grads[k], ref_grads[k]) for k in ref_grads) and all(torch.equal(params[k], ref_params[k]) for k in ref_params)
    plan = model.get_loss_plan(*model.canvas_size(inputs), tower_grads=True)
    # its own cache key: the two plans live side by side under keys that differ in the last entry only
    keys = {k[-1]: k for k in model._plans if k[0] == "losses"}
    assert keys["tower_grads"][:-1] == keys["pred_grads"][:-1] and model._plans[keys["tower_grads"]] is plan
    assert model._plans[keys["pred_grads"]] is not plan and model._plans[keys["pred_grads"]].tower_info is None
    L = len(plan.features)
    names = [op.name for op in plan.ops]
    assert names[-12:] == [f"tower_grads.{t}.{i}" for t in TO.TOWERS for i in (3, 2, 1, 0)] and names[-13] == "predictor_grads.box3d_map"
    assert sorted(set(grads) - set(ref_grads)) == [f"feature{l}" for l in range(L)]
    assert all(grads[f"feature{l}"].shape == (B, 256, plan.features[l].H, plan.features[l].W) and grads[f"feature{l}"].dtype == torch.float32 for l in range(L))
    cpu = GC.cpu_model(exp)
    tparams = {k: v for k, v in params.items() if k not in ref_params}
    assert sorted(tparams) == TO.tower_param_names(cpu)
    assert all(params[k].shape == p.shape and params[k].dtype == torch.float32 for k, p in cpu.named_parameters() if k in tparams)
    # every (tower, layer): the raw outputs against the layer oracle on the plan's own stored x, y and incoming g
    stored = {t: [None] * 4 for t in TO.TOWERS}
    for key in plan.tower_layers:
        case, lay = _layer_inputs(plan, key)
        stored[key[0]][key[1]] = (case.x, case.y)
        assert lay.guards_intact(0.0)
        check(collect(lay), case.ref(torch.float64), case.ref(torch.float32), f"e2e:{ds}:{key[0]}.{key[1]}")
    # the named parameters and the feature gradients against the chain oracle: float64, the bar from the chain's own float32 run
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    g_top = {t: [ref_grads[f"{t}_tower_out{l}"].cpu() for l in range(L)] for t in TO.TOWERS}
    p64, f64, _ = TO.chain_grads(cpu, stored, g_top, torch.float64)
    p32, f32, _ = TO.chain_grads(cpu, stored, g_top, torch.float32)
    _check_named(tparams, {k: grads[k] for k in f64}, (p64, f64), (p32, f32), f"e2e:{ds}")
    # a second call is bit-equal; the captured graph equals launch-by-launch execution
    _, g2, p2 = model.compute_losses(inputs, tower_grads=True)
    assert all(torch.equal(g2[k], grads[k]) for k in grads) and all(torch.equal(p2[k], params[k]) for k in params)
    model.use_graph = False
    model.invalidate_plans()
    l3, g3, p3 = model.compute_losses(inputs, tower_grads=True)
    assert all(torch.equal(l3[k], losses[k]) for k in losses)
    assert all(torch.equal(g3[k], grads[k]) for k in grads) and all(torch.equal(p3[k], params[k]) for k in params)
    return model, plan


@pytest.mark.parametrize("exp,weights,B,H,W,ds", [("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti"),
                                                   ("dd3d_nusc_dla34", "dla34_nusc", 6, 128, 224, "nusc")])
def test_compute_losses_tower_grads_end_to_end(hiplib, exp, weights, B, H, W, ds):
    from dd3d_amd import hip
    model, plan = _end_to_end(exp, weights, B, H, W, ds)
    a = plan.tower_layers[("cls", 3)].args
    assert a.x_mode == a.y_mode == hip.PG_ACT_F16X2 and a.y_plane_scale == 16.0


def test_compute_losses_tower_grads_bf16x3(hiplib):
    from dd3d_amd import hip
    _, plan = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti", math="bf16x3")
    assert plan.tower_layers[("box3d", 0)].args.y_mode == hip.PG_ACT_BF16X3


def test_compute_losses_tower_grads_plane_scale_1(hiplib):
    _, plan = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti", act_scale=1.0)
    assert plan.tower_layers[("box2d", 1)].args.y_plane_scale == 1.0


def test_reduced_modes_name_themselves(hiplib):
    from tests.test_loss_grads_gpu import _model
    model = _model("dd3d_kitti_dla34", "dla34_kitti")
    model.math = "bf16x2"
    with pytest.raises(NotImplementedError, match="bf16x2"):
        model.get_loss_plan(1, 128, 128, tower_grads=True)
    model.math = None
    with pytest.raises(RuntimeError):
        model.train()


# --------------------------------------------------------------------------------------------------- the reference-modules golden
@pytest.mark.parametrize("name", list(TC.REFERENCE_CASES))
def test_kernels_match_the_reference_modules_golden(hiplib, name):
    """The reference's own heads and loss modules under torch autograd (tests/golden/tower_grads_*.npz) against the kernels on the
    golden's chain: f32 storage, the CPU modules' tower activations, the tower-output gradients of the predictor oracle, every (tower,
    layer) run last layer first, assembled under the parameters' names by engine.losses.assemble_tower_grads.  Within 2 * bar of the
    golden (a float32 autograd, within one bar of the float64 gradient like the kernels) and within bar of float64."""
    import os
    import numpy as np
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import TowerLayerGrads, assemble_tower_grads
    from dd3d_amd.layers import fold_norm
    from tests import predictor_grad_oracle as PO
    from tests.test_tower_grads import ROOT, golden_families, reference_chain
    z = np.load(os.path.join(ROOT, "tests", "golden", f"tower_grads_{name}.npz"))
    model, stored, g_top64, g_top32 = reference_chain(name)
    B = stored["cls"][0][0][0].shape[0]
    layers, feature_da = {}, None
    for t, convs in TO.tower_modules(model).items():
        g = [nhwc(v.float(), 256) for v in g_top32[t]]
        for i in reversed(range(len(convs))):
            x, y = stored[t][i]
            conv = convs[i]
            xb, xbind, _ = _store(x, "f32", 1.0, 0)
            yb, ybind, _ = _store(y, "f32", 1.0, 0)
            scale = [fold_norm(conv, TO.level_norm(conv, l))[0].cuda() for l in range(len(x))]
            lay = TowerLayerGrads("cuda", B, PC.PYRAMID_64x128, 256, 256, xbind, ybind, g, 256, conv.weight.detach().permute(0, 2, 3, 1).contiguous().cuda(),
                                  scale, da_add=feature_da if i == 0 else None, fill=SENTINEL, guard=64)
            lay.launch(hip.lib(), hip.current_stream())
            torch.cuda.synchronize()
            frame_ok(lay)
            lay.conv, lay.norms, lay.keep_alive = conv, [TO.level_norm(conv, l) for l in range(len(x))], (xb, yb)
            layers[(t, i)] = lay
            g = lay.da
        feature_da = g
    feats, params = assemble_tower_grads(model, layers, feature_da)
    params, feats = {k: v.cpu() for k, v in params.items()}, {k: v.cpu() for k, v in feats.items()}
    p64, f64, _ = TO.chain_grads(model, stored, g_top64, torch.float64)
    p32, f32, _ = TO.chain_grads(model, stored, g_top32, torch.float32)
    a64, a32, got = golden_families(z, p64, f64), golden_families(z, p32, f32), golden_families(z, params, feats)
    for fam, (gold, a) in a64.items():
        bar, d32, gmax = TO.bar(a.double(), a32[fam][1], torch.ones(a.shape[0], dtype=torch.bool))
        dev, dev64 = float((got[fam][1].double() - gold.double()).abs().max()), float((got[fam][1].double() - a.double()).abs().max())
        print(f"[tower_grads] ref:{name} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernels against the golden {dev:.3e} (bar {2 * bar:.3e}), "
              f"against float64 {dev64:.3e} (bar {bar:.3e})")
        assert dev <= 2 * bar and dev64 <= bar, (name, fam, dev, dev64, bar)
