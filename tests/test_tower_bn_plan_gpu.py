"""DD3D.compute_losses(batch_stats=True) on the MI355X: the head towers whose norm is a trainable BatchNorm2d on the batch's statistics,
forward and backward, end to end from the uint8 images (engine.LossPlan(batch_stats=True), csrc/tower_bn.hip).

Per case (kitti_dla34 and nusc_dla34 at B = 2 on 64 x 128 images -- a 128 x 128 canvas after the padding to the FPN's size divisibility,
where P7 is 1 x 1 and has two values per channel -- and kitti_dla34 at B = 1 on 128 x 256):
the tower parameters' and the FPN outputs' gradients against the float64 oracle chain (tests/tower_bn_oracle.py) at the plan's stored
x and y and the gradient the predictor backward delivered, every family -- weight, norm_weight, norm_bias, da, feature -- within
loss_grad_oracle.bar = 8 * max(d32, 2^-23 * max|g64|); the stored raw c against the oracle's convolution; the loss dict against the
oracle forward with batch statistics on the plan's own features (the tolerance of tests/test_whole_model_grads_gpu.py);
tower_batch_stats() against the oracle; equal bits over two runs, between graph replay and launch by launch, and on a second batch
between the same plan and a fresh one; the plan without the flag unchanged by a plan with it.  One case goes on through the FPN, one
through the range guard's retry."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from tests import loss_grad_cases as GC
from tests import loss_oracle as LO
from tests import tower_bn_oracle as BO
from tests import tower_grad_oracle as TO

pytestmark = pytest.mark.gpu

LOSS_REL = {"kitti": 1e-4, "nusc": 2e-4}  # tests/test_whole_model_grads_gpu.py
RAW_TOL = 1e-5  # the stored raw c against the oracle's float64 convolution of the stored x, relative to max|c|: filters are 22-bit pairs
WORST = {}


@pytest.fixture(autouse=True)
def _default_arithmetic(monkeypatch):
    monkeypatch.delenv("DD3D_MATH", raising=False)
    monkeypatch.delenv("DD3D_F16_ACT_SCALE", raising=False)


def _batch(model, B, H, W, ds, seed=0, gt_seed=None, empty=()):
    from dd3d_amd.synthetic import make_gt_instances, make_inputs
    nusc = hasattr(model, "attr_logits")
    inputs = make_inputs(B, H, W, dataset=ds, seed=seed) if seed else make_inputs(B, H, W, dataset=ds)
    kw = {} if gt_seed is None else {"seed": gt_seed}
    gt = make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, n_per_image=8,
                           num_attributes=model.attr_logits.out_channels if nusc else None, empty_images=empty, **kw)
    for x, g in zip(inputs, gt):
        x["instances"] = g
    return inputs


def _same(a, b):
    return all(set(x) == set(y) and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


def _bar(got, ref64, ref32, what):
    cat = lambda vs: torch.cat([v.reshape(-1).cpu() for v in vs])
    c, a, b = cat(got), cat(ref64).double(), cat(ref32)
    bar, d32, gmax = BO.bar(a, b, torch.ones(a.shape[0], dtype=torch.bool))
    dev = float((c.double() - a).abs().max())
    use = 8 * dev / bar if bar > 0 else 0.0
    fam = what.split(":")[-1]
    WORST[fam] = max(WORST.get(fam, 0.0), use)
    print(f"[tower_bn] {what}: max|ref64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
    assert bool(torch.isfinite(c).all()) and dev <= bar and gmax > 0.0, (what, dev, bar, d32, gmax)


def _stored(plan):
    """{tower: [(x levels, y levels)]} and {(tower, layer): raw c levels} as the plan's storages decode them, NCHW on the CPU."""
    nchw = lambda v: v.nchw().float().cpu().contiguous()
    stored, raw = {t: [None] * 4 for t in TO.TOWERS}, {}
    for (t, i), info in plan.tower_info.items():
        stored[t][i] = ([nchw(v) for v in info["x"]], [nchw(v) for v in info["y"]])
        if info["raw"] is not None:
            raw[(t, i)] = [nchw(v) for v in info["raw"]]
    return stored, raw


def _end_to_end(exp, weights, B, H, W, ds, math=None):
    from tests.test_loss_grads_gpu import _model
    from tests.test_losses_gpu import _close
    model = _model(exp, weights)
    model.math = math
    inputs = _batch(model, B, H, W, ds)
    base = model.compute_losses(inputs, tower_grads=True)  # running statistics, before any batch-statistics plan exists
    pred = model.compute_losses(inputs, predictor_grads=True, batch_stats=True)
    losses, grads, params = model.compute_losses(inputs, tower_grads=True, batch_stats=True)
    plan = model.get_loss_plan(*model.canvas_size(inputs), tower_grads=True, batch_stats=True)
    assert plan.batch_stats and len(plan.tower_bn) == 8 and model.get_loss_plan(*model.canvas_size(inputs), tower_grads=True) is not plan
    # the same forward in both batch-statistics plans; keys and shapes as without the flag, other values
    assert _same((losses, ), (pred[0], )) and all(torch.equal(grads[k], pred[1][k]) for k in pred[1]) and all(torch.equal(params[k], pred[2][k]) for k in pred[2])
    assert list(losses) == list(base[0]) and set(grads) == set(base[1]) and set(params) == set(base[2])
    assert all(grads[k].shape == base[1][k].shape for k in grads) and all(params[k].shape == base[2][k].shape for k in params)
    assert not torch.equal(grads["feature0"], base[1]["feature0"]) and not torch.equal(losses["loss_cls"], base[0]["loss_cls"])
    cpu = GC.cpu_model(exp)
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    L = len(plan.features)
    stored, raw = _stored(plan)
    # the stored raw c is the convolution of the stored x; every guard word of the backward's outputs is intact
    for (t, i), cs in raw.items():
        conv = TO.tower_modules(cpu)[t][i]
        for l, c in enumerate(cs):
            ref = F.conv2d(stored[t][i][0][l].double(), conv.weight.detach().double(), padding=1)
            assert float((c.double() - ref).abs().max()) <= RAW_TOL * float(ref.abs().max()), (t, i, l)
    assert all(lay.guards_intact(0.0) and (lay.bn is None or lay.bn.guards_intact(0.0)) for lay in plan.tower_layers.values())
    # gradients: the chain oracle at the stored activations, from the gradient the predictor backward delivered
    g_top = {t: [pred[1][f"{t}_tower_out{l}"].cpu() for l in range(L)] for t in TO.TOWERS}
    p64, f64, d64 = BO.chain_grads(cpu, stored, g_top, torch.float64)
    p32, f32, d32 = BO.chain_grads(cpu, stored, g_top, torch.float32)
    tparams = {k: v for k, v in params.items() if k not in pred[2]}
    assert sorted(tparams) == TO.tower_param_names(cpu)
    for fam in ("weight", "norm_weight", "norm_bias"):
        ks = [k for k in sorted(tparams) if TO.family_of(k) == fam]
        _bar([tparams[k] for k in ks], [p64[k] for k in ks], [p32[k] for k in ks], f"{ds}{B}:{fam}")
    keys = sorted(plan.tower_layers)
    _bar([d.permute(0, 3, 1, 2) for k in keys for d in plan.tower_layers[k].da if k[1] > 0], [v for k in keys for v in d64[k] if k[1] > 0],
         [v for k in keys for v in d32[k] if k[1] > 0], f"{ds}{B}:da")
    _bar([grads[k] for k in sorted(f64)], [f64[k] for k in sorted(f64)], [f32[k] for k in sorted(f64)], f"{ds}{B}:feature")
    # the loss dict: the oracle's heads with batch statistics on the plan's own FPN outputs, then the loss oracle
    feats = [v.nchw().float().cpu().contiguous() for v in plan.features]
    level_hw = [(f.H, f.W) for f in plan.features]
    with torch.no_grad():
        maps = BO.head_maps(cpu, feats, torch.float32)
    targets = GC.oracle_targets(cpu, level_hw, [x["instances"] for x in inputs])
    ref_losses = LO.losses(maps, targets, plan.inv_K.view(-1, 3, 3).cpu(), dict(LO.settings(cpu), num_levels=L))
    for k in losses:
        print(f"[tower_bn] {ds}{B} {k}: {float(losses[k]):.7g} oracle {float(ref_losses[k]):.7g} running statistics {float(base[0][k]):.7g}")
    _close({k: v.cpu() for k, v in losses.items()}, ref_losses, LOSS_REL[ds])
    # the statistics: batch mean / variance and the running values after the step, against the oracle on the stored x
    stats = plan.tower_batch_stats()
    assert sorted(stats) == BO.batch_stats_names(cpu)
    bufs = {id(b): k for k, b in cpu.named_buffers()}
    rows = {k: ([], [], []) for k in ("batch_mean", "batch_var", "running_mean", "running_var")}
    for (t, i) in raw:
        conv = TO.tower_modules(cpu)[t][i]
        for l in range(L):
            norm = TO.level_norm(conv, l)
            stem = bufs[id(norm.running_mean)][:-len("running_mean")]
            x = stored[t][i][0][l]
            n = x.shape[0] * x.shape[2] * x.shape[3]
            for dtype, slot in ((torch.float64, 1), (torch.float32, 2)):
                mu, v = BO.stats(F.conv2d(x.to(dtype), conv.weight.detach().to(dtype), padding=1), dtype)
                rm, rv = BO.running_update(norm.running_mean.to(dtype), norm.running_var.to(dtype), mu, v, n)
                for k, val in (("batch_mean", mu), ("batch_var", v), ("running_mean", rm), ("running_var", rv)):
                    rows[k][slot].append(val)
            for k in rows:
                rows[k][0].append(stats[stem + k])
    for k, (got, r64, r32) in rows.items():
        _bar(got, r64, r32, f"{ds}{B}:{k}")
    assert all(torch.equal(b.cpu(), cpu.state_dict()[k]) for k, b in model.named_buffers() if "running" in k)  # the model's buffers are never written
    # a second call is bit-equal; so is a plan without the flag built after this one; the captured graph equals launch by launch
    again = model.compute_losses(inputs, tower_grads=True, batch_stats=True)
    assert _same(again, (losses, grads, params)) and _same((plan.tower_batch_stats(), ), (stats, ))
    model._plans.clear()
    assert _same(model.compute_losses(inputs, tower_grads=True), base)
    model.use_graph = False
    model.invalidate_plans()
    assert _same(model.compute_losses(inputs, tower_grads=True, batch_stats=True), (losses, grads, params))
    return model, plan, inputs


@pytest.mark.parametrize("exp,weights,B,H,W,ds", [("dd3d_kitti_dla34", "dla34_kitti", 2, 64, 128, "kitti"), ("dd3d_nusc_dla34", "dla34_nusc", 2, 64, 128, "nusc"),
                                                   ("dd3d_kitti_dla34", "dla34_kitti", 1, 128, 256, "kitti")])
def test_compute_losses_batch_stats_end_to_end(hiplib, exp, weights, B, H, W, ds):
    from dd3d_amd import hip
    model, plan, inputs = _end_to_end(exp, weights, B, H, W, ds)
    assert plan.tower_layers[("cls", 3)].bn.args.y_mode == hip.PG_ACT_F16X2 and plan.tower_bn[("cls", 0)]["args"].math_mode == hip.MATH_F16X2
    if B == 1:
        with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
            model.compute_losses(_batch(model, 1, 64, 128, ds), batch_stats=True)


def test_compute_losses_batch_stats_bf16x3(hiplib):
    from dd3d_amd import hip
    _, plan, _ = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 64, 128, "kitti", math="bf16x3")
    assert plan.tower_layers[("box2d", 0)].bn.args.y_mode == hip.PG_ACT_BF16X3 and plan.tower_bn[("cls", 0)]["args"].math_mode == hip.MATH_BF16X3


def test_one_plan_on_a_second_batch_equals_a_fresh_plan(hiplib):
    """As tests/test_loss_plan_history_gpu.py: the captured plan replayed on other images and other GT against a fresh model on that batch."""
    from tests.test_loss_grads_gpu import _model
    model = _model("dd3d_kitti_dla34", "dla34_kitti")
    a, b = _batch(model, 2, 64, 128, "kitti"), _batch(model, 2, 64, 128, "kitti", seed=5, gt_seed=31, empty=(0, ))
    first = model.compute_losses(a, tower_grads=True, batch_stats=True)
    second = model.compute_losses(b, tower_grads=True, batch_stats=True)
    plan = model.get_loss_plan(*model.canvas_size(b), tower_grads=True, batch_stats=True)
    stats = plan.tower_batch_stats()
    assert len([k for k in model._plans if k[0] == "losses"]) == 1 and not _same(first, second)
    fresh = _model("dd3d_kitti_dla34", "dla34_kitti")
    want = fresh.compute_losses(b, tower_grads=True, batch_stats=True)
    assert _same(second, want) and _same((stats, ), (fresh.get_loss_plan(*fresh.canvas_size(b), tower_grads=True, batch_stats=True).tower_batch_stats(), ))
    assert _same(model.compute_losses(a, tower_grads=True, batch_stats=True), first)


def test_fpn_grads_consume_the_batch_statistics_feature_gradients(hiplib):
    """fpn_grads=True with batch_stats=True: everything tower_grads returns, bit for bit, and the FPN's outputs against the FPN oracle
    fed with this plan's feature<l> (the chain and the bar of tests/test_fpn_grads_gpu.py)."""
    from tests import fpn_grad_oracle as FO
    from tests.test_fpn_grads_gpu import _plan_tensors, check_named
    from tests.test_loss_grads_gpu import _model
    exp = "dd3d_kitti_dla34"
    model = _model(exp, "dla34_kitti")
    inputs = _batch(model, 2, 64, 128, "kitti")
    ref = model.compute_losses(inputs, tower_grads=True, batch_stats=True)
    losses, grads, params = model.compute_losses(inputs, fpn_grads=True, batch_stats=True)
    assert _same((losses, ), (ref[0], )) and all(torch.equal(grads[k], ref[1][k]) for k in ref[1]) and all(torch.equal(params[k], ref[2][k]) for k in ref[2])
    plan = model.get_loss_plan(*model.canvas_size(inputs), fpn_grads=True, batch_stats=True)
    fpn = model.backbone
    cpu = GC.cpu_model(exp)
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    new_g, new_p = {k: v.cpu() for k, v in grads.items() if k not in ref[1]}, {k: v.cpu() for k, v in params.items() if k not in ref[2]}
    assert sorted(new_g) == sorted(f"backbone_{n}" for n in fpn.in_features) and sorted(new_p) == FO.fpn_param_names(cpu)
    feats, stored = _plan_tensors(model, plan)
    sel = list(model.in_features)
    G = {n: grads[f"feature{sel.index(n)}"].cpu() for n in fpn._out_features if n in sel}
    check_named(new_p, new_g, FO.chain_grads(cpu, stored, feats, G, torch.float64), FO.chain_grads(cpu, stored, feats, G, torch.float32), "batch_stats")


def test_range_guard_retry_with_batch_stats(hiplib):
    """The first cls-tower layer's norm weights and biases scaled so that its output passes 4094 (the half range at plane scale 16) and
    stays below 16376: dd3d_bn_apply_relu_split sets the status bit, an explicit f16x2 model raises, a model on the default arithmetic
    lowers its plane scale to 4 inside compute_losses and returns the bits of a fresh model built at plane scale 4.  (The next layer's
    batch statistics absorb the scale: the function itself hardly changes.)"""
    from tests.test_loss_grads_gpu import _model
    base = _model("dd3d_kitti_dla34", "dla34_kitti")
    inputs = _batch(base, 2, 64, 128, "kitti")
    base.compute_losses(inputs, tower_grads=True, batch_stats=True)
    plan = base.get_loss_plan(*base.canvas_size(inputs), tower_grads=True, batch_stats=True)
    a0 = max(float(v.nchw().float().abs().max()) for v in plan.tower_info[("cls", 0)]["y"])
    sd = {k: v.clone() for k, v in base.state_dict().items()}
    for l in range(5):
        for k in ("weight", "bias"):
            sd[f"fcos2d_head.cls_tower.0.norm.{l}.{k}"] *= 6000.0 / a0

    def build(math=None, act_scale=None):
        m = GC.cpu_model("dd3d_kitti_dla34")
        m.load_state_dict({k: v.cpu() for k, v in sd.items()})
        m = m.to("cuda").eval()
        m.math, m.act_scale = math, act_scale
        return m

    with pytest.raises(FloatingPointError, match="half range"):
        build(math="f16x2").compute_losses(inputs, tower_grads=True, batch_stats=True)
    model = build()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = model.compute_losses(inputs, tower_grads=True, batch_stats=True)
    msgs = [str(x.message) for x in w if "dd3d_amd" in str(x.message)]
    assert (model.math, model.act_scale) == (None, 4.0) and any("plane scale lowered 16 -> 4" in m for m in msgs), (model.math, model.act_scale, msgs)
    p4 = model.get_loss_plan(*model.canvas_size(inputs), tower_grads=True, batch_stats=True)
    assert p4.tower_bn[("cls", 0)]["args"].plane_scale == 4.0 and p4.tower_layers[("cls", 0)].bn.args.plane_scale == 4.0
    assert abs(max(float(v.nchw().float().abs().max()) for v in p4.tower_info[("cls", 0)]["y"]) - 6000.0) < 60.0
    there = build(act_scale=4.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        want = there.compute_losses(inputs, tower_grads=True, batch_stats=True)
    assert not [x for x in w if "lowered" in str(x.message) or "switching" in str(x.message)]
    assert _same(got, want) and all(bool(torch.isfinite(v).all()) for d in got for v in d.values())


def test_worst_use_of_the_bar_is_reported(hiplib):
    """(Runs last in this file.)  The largest share of the factor 8 any family above used: what profiles/tower_bn_errors.txt records."""
    for k, v in sorted(WORST.items()):
        print(f"[tower_bn] plan level, worst use of the factor 8, {k}: {v:.2f}")
    assert all(v <= 8.0 for v in WORST.values())
