"""compute_losses(fpn_batch_stats=True) on the MI355X: the FPN's lateral and output norms (FE.FPN.NORM: BN) on the batch's statistics,
forward and backward, end to end from the uint8 images (engine.LossPlan(fpn_batch_stats=True), csrc/fpn_bn.hip).

Images of 64 x 128 at B = 2 give a 128 x 128 canvas after the padding to the FPN's size divisibility, where P7 is 1 x 1 with two values
per channel (as in tests/test_tower_bn_plan_gpu.py).  The FPN's parameter gradients by family (weight, norm_weight, norm_bias, the top
block's bias) and the gradients at the backbone's output features against the float64 chain oracle (tests/fpn_bn_oracle.py) at the
plan's stored activations and the feature<l> gradients the towers delivered, each within loss_grad_oracle.bar = 8 * max(d32, 2^-23 *
max|g64|); the stored raw convolution outputs, the statistics read-out and the loss dict against the oracle; equal bits over runs,
between graph replay and launch by launch, on other batches, through the range guard's retry, and for the unflagged plan of the same
model; one case against ONE autograd pass of the whole model with the towers' norms on batch statistics as well."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from tests import fpn_bn_oracle as NO
from tests import fpn_grad_oracle as FO
from tests import loss_grad_cases as GC
from tests import loss_oracle as LO
from tests.test_tower_bn_plan_gpu import _batch, _same

pytestmark = pytest.mark.gpu

FPN_BN = {"FE": {"FPN": {"NORM": "BN"}}}
LOSS_REL = {"kitti": 1e-4, "nusc": 2e-4}  # tests/test_whole_model_grads_gpu.py
RAW_TOL = 1e-5  # tests/test_tower_bn_plan_gpu.py: a stored raw c against the float64 convolution of the stored x, relative to max|c|
SENTINEL = -12345.0
WORST = {}


@pytest.fixture(autouse=True)
def _default_arithmetic(monkeypatch):
    monkeypatch.delenv("DD3D_MATH", raising=False)
    monkeypatch.delenv("DD3D_F16_ACT_SCALE", raising=False)


def _bar(got, ref64, ref32, what):
    cat = lambda vs: torch.cat([v.reshape(-1).cpu() for v in vs])
    c, a, b = cat(got), cat(ref64).double(), cat(ref32)
    bar, d32, gmax = NO.bar(a, b, torch.ones(a.shape[0], dtype=torch.bool))
    dev = float((c.double() - a).abs().max())
    use = 8 * dev / bar if bar > 0 else 0.0
    fam = what.split(":")[-1]
    WORST[fam] = max(WORST.get(fam, 0.0), use)
    print(f"[fpn_bn] {what}: n {a.numel()} max|ref64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
    assert bool(torch.isfinite(c).all()) and dev <= bar and gmax > 0.0, (what, dev, bar, d32, gmax)


def _cpu_twin(model, exp, overrides=FPN_BN):
    cpu = GC.cpu_model(exp, overrides)
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    return cpu


def _check_chain(tag, cpu, plan, grads, params, shallower):
    """The FPN's new keys of (grads, params) against the chain oracle at the plan's stored activations; `shallower`: the (grads, params) of
    the call one flag up, whose keys are not the FPN's."""
    from tests.test_fpn_grads_gpu import _plan_tensors
    fpn = cpu.backbone
    new_g = {k: v.cpu() for k, v in grads.items() if k not in shallower[0]}
    new_p = {k: v.cpu() for k, v in params.items() if k not in shallower[1]}
    assert sorted(new_g) == sorted(f"backbone_{n}" for n in fpn.in_features) and sorted(new_p) == FO.fpn_param_names(cpu)
    named = dict(cpu.named_parameters())
    assert all(v.shape == named[k].shape and v.dtype == torch.float32 for k, v in new_p.items())
    feats, stored = _plan_tensors(plan.model, plan)
    sel = list(plan.model.in_features)
    G = {n: grads[f"feature{sel.index(n)}"].cpu() for n in fpn._out_features if n in sel}
    (p64, f64), (p32, f32) = NO.chain_grads(cpu, stored, feats, G, torch.float64), NO.chain_grads(cpu, stored, feats, G, torch.float32)
    fams = {}
    for k in sorted(new_p):
        fams.setdefault(NO.family_of(k), []).append(k)
    assert {"weight", "norm_weight", "norm_bias"} <= set(fams)
    for fam, ks in sorted(fams.items()):
        _bar([new_p[k] for k in ks], [p64[k] for k in ks], [p32[k] for k in ks], f"{tag}:{fam}")
    for k in sorted(new_g):
        _bar([new_g[k]], [f64[k]], [f32[k]], f"{tag}:{k}")
    return feats, stored


def _check_raws_and_stats(tag, cpu, plan, feats, stored):
    fpn = cpu.backbone
    nchw = lambda v: v.nchw().float().cpu().contiguous()
    for kind, xs, pad in (("fpn_lateral", {s: feats[n] for s, n in zip(fpn.stages, fpn.in_features)}, 0), ("fpn_output", stored["t"], 1)):
        for s in fpn.stages:
            conv = getattr(fpn, f"{kind}{s}")
            ref = F.conv2d(xs[s].double(), conv.weight.detach().double(), padding=pad)
            c = nchw(plan.bufs[f"{kind}{s}.raw"].view())
            assert float((c.double() - ref).abs().max()) <= RAW_TOL * float(ref.abs().max()), (tag, kind, s)
    stats = plan.fpn_batch_stats()
    assert sorted(stats) == NO.batch_stats_names(cpu)
    w64, w32 = NO.expected_stats(cpu, stored, feats, torch.float64), NO.expected_stats(cpu, stored, feats, torch.float32)
    for kind in ("batch_mean", "batch_var", "running_mean", "running_var"):
        ks = [k for k in sorted(stats) if k.endswith(kind)]
        _bar([stats[k] for k in ks], [w64[k] for k in ks], [w32[k] for k in ks], f"{tag}:{kind}")
    return stats


def _check_losses(tag, cpu, plan, inputs, losses, ds, tower_batch_stats=False):
    """The loss dict against the float32 oracle forward on the plan's own backbone features: FPN with batch statistics, heads, losses."""
    from tests.test_fpn_grads_gpu import _plan_tensors
    from tests.test_losses_gpu import _close
    feats, _ = _plan_tensors(plan.model, plan)
    sd = {k: (v.detach().float() if v.is_floating_point() else v.detach()) for k, v in cpu.state_dict().items()}
    with torch.no_grad():
        outs = NO.forward(sd, feats, FO.spec(cpu))
        maps = NO.head_maps(cpu, [outs[n] for n in cpu.in_features], torch.float32, tower_batch_stats=tower_batch_stats)
    level_hw = [(f.H, f.W) for f in plan.features]
    targets = GC.oracle_targets(cpu, level_hw, [x["instances"] for x in inputs])
    ref = LO.losses(maps, targets, plan.inv_K.view(-1, 3, 3).cpu(), dict(LO.settings(cpu), num_levels=len(level_hw)))
    for k in losses:
        print(f"[fpn_bn] {tag} {k}: {float(losses[k]):.7g} oracle {float(ref[k]):.7g}")
    _close({k: v.cpu() for k, v in losses.items()}, ref, LOSS_REL[ds])


def _guards(plan):
    return all(lay.guards_intact(0.0) for lay in list(plan.fpn_layers.values()) + list(plan.fpn_bn_layers.values()))


def _end_to_end(exp, weights, math=None, B=2, H=64, W=128, ds="kitti"):
    from tests.test_loss_grads_gpu import _model
    model = _model(exp, weights, FPN_BN)
    model.math = math
    inputs = _batch(model, B, H, W, ds)
    flagged = dict(fpn_grads=True, fpn_batch_stats=True)
    base = model.compute_losses(inputs, fpn_grads=True)  # running statistics, before any flagged plan exists
    tow = model.compute_losses(inputs, tower_grads=True, fpn_batch_stats=True)
    losses, grads, params = model.compute_losses(inputs, **flagged)
    canvas = model.canvas_size(inputs)
    plan = model.get_loss_plan(*canvas, **flagged)
    assert plan.with_fpn_batch_stats and model.get_loss_plan(*canvas, fpn_grads=True) is not plan and plan.graph is not None
    # everything the shallower flag returns: the same bits; keys and shapes as without the flag, other values
    assert _same((losses, ), (tow[0], )) and all(torch.equal(grads[k], tow[1][k]) for k in tow[1]) and all(torch.equal(params[k], tow[2][k]) for k in tow[2])
    assert list(losses) == list(base[0]) and set(grads) == set(base[1]) and set(params) == set(base[2])
    assert all(grads[k].shape == base[1][k].shape for k in grads) and all(params[k].shape == base[2][k].shape for k in params)
    n0 = f"backbone_{model.backbone.in_features[0]}"
    assert not torch.equal(grads[n0], base[1][n0]) and not torch.equal(losses["loss_cls"], base[0]["loss_cls"])
    cpu = _cpu_twin(model, exp)
    tag = f"{exp[5:]}{'' if math is None else ':' + math}"
    feats, stored = _check_chain(tag, cpu, plan, grads, params, tow[1:])
    stats = _check_raws_and_stats(tag, cpu, plan, feats, stored)
    _check_losses(tag, cpu, plan, inputs, losses, ds)
    assert _guards(plan)
    assert all(torch.equal(b.cpu(), cpu.state_dict()[k]) for k, b in model.named_buffers() if "running" in k)  # the model's buffers are never written
    # a second call is bit-equal; the unflagged plan returns what it returned before; the captured graph equals launch by launch
    assert _same(model.compute_losses(inputs, **flagged), (losses, grads, params)) and _same((plan.fpn_batch_stats(), ), (stats, ))
    assert _same(model.compute_losses(inputs, fpn_grads=True), base)
    model._plans.clear()
    assert _same(model.compute_losses(inputs, fpn_grads=True), base)
    model.use_graph = False
    model.invalidate_plans()
    assert _same(model.compute_losses(inputs, **flagged), (losses, grads, params))
    return model, plan, inputs


def test_compute_losses_fpn_batch_stats_kitti_dla34(hiplib):
    from dd3d_amd import hip
    _, plan, _ = _end_to_end("dd3d_kitti_dla34", "dla34_kitti")
    lat = plan.fpn_bn["laterals"]["args"]
    assert lat.bn.math_mode == hip.MATH_F16X2 and lat.bn.plane_scale == 16.0 and [lat.up[i] for i in range(3)] == [1, 2, -1]
    assert [lat.bn.N[i] for i in range(3)] == [2 * 16 * 16, 2 * 8 * 8, 2 * 4 * 4] and (plan.features[-1].H, plan.features[-1].W) == (1, 1)


def test_compute_losses_fpn_batch_stats_bf16x3(hiplib):
    from dd3d_amd import hip
    _, plan, _ = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", math="bf16x3")
    assert plan.fpn_bn["outputs"]["args"].bn.math_mode == hip.MATH_BF16X3 and plan.fpn_layers["outputs"].args.x_mode == hip.PG_ACT_BF16X3


def test_compute_losses_fpn_batch_stats_kitti_v99(hiplib):
    """LastLevelP6, four linked stages, the Cin 1024 lateral; backbone_stage2..5 within the bar."""
    _, plan, _ = _end_to_end("dd3d_kitti_v99", "v99_kitti")
    lat = plan.fpn_bn["laterals"]["args"]
    assert [lat.up[i] for i in range(4)] == [1, 2, 3, -1] and plan.fpn_layers["lateral5"].Cin == 1024
    assert sorted(plan.backbone_feature_grads) == ["stage2", "stage3", "stage4", "stage5"]


def test_whole_model_gradient_with_tower_and_fpn_batch_stats(hiplib):
    """batch_stats=True, fpn_batch_stats=True, stem_grads=True against ONE autograd pass of the whole model per precision under the stored
    signs of all ReLUs (tests/whole_model_grad_oracle.py, the stem's three included: tests/stem_grad_oracle.py), the towers' and the FPN's
    norms on batch statistics in the oracle (fpn_bn_oracle.norms_on).  The GT seed is pinned to a batch without a positive on a non-smooth
    point of the loss on the float64 forward (asserted below, as whole_model_grad_oracle.CASES documents).  The batch is that of the
    whole-model cases, two 128 x 384 images: the oracle accepts a plan's stored ReLU output as the source of a mask only within 1e-4 of
    its own float64 tensor, and on a 128 x 128 canvas the towers' norms at P7 (two values per channel: xhat = +-1 up to eps) amplify the
    forward's rounding past that (4e-4 measured at cls_tower.1 on P7) -- a property of the towers' N = 2 statistics, which
    tests/test_tower_bn_plan_gpu.py covers with the chain oracle, not of the FPN's."""
    from tests import loss_grad_oracle as GO
    from tests import stem_grad_oracle as SO
    from tests import whole_model_grad_oracle as WO
    from tests.test_loss_grads_gpu import _model
    from tests.test_losses_gpu import _close
    exp = "dd3d_kitti_dla34"
    model = _model(exp, "dla34_kitti", FPN_BN)
    cpu = _cpu_twin(model, exp)
    inputs, gt = WO.case_inputs(dict(WO.CASES["kitti_dla34"], gt_seed=WHOLE_MODEL_GT_SEED), cpu)
    for x, g in zip(inputs, gt):
        x["instances"] = g
    flags = dict(stem_grads=True, batch_stats=True, fpn_batch_stats=True)
    shallow = model.compute_losses(inputs, backbone_grads=True, batch_stats=True, fpn_batch_stats=True)
    losses, grads, params = model.compute_losses(inputs, **flags)
    assert _same((shallow[0], ), (losses, )) and all(torch.equal(grads[k], v) for k, v in shallow[1].items()) and all(torch.equal(params[k], v) for k, v in shallow[2].items())
    plan = model.get_loss_plan(*model.canvas_size(inputs), **flags)
    named = dict(cpu.named_parameters())
    assert sorted(params) == sorted(named) and all(params[k].shape == named[k].shape for k in params)
    inv_K = plan.inv_K.view(-1, 3, 3).cpu()
    F64, F32 = torch.float64, torch.float32
    with NO.norms_on(cpu) as chosen:
        assert len(chosen) == 8 * 5 + 6
        nat = {}
        pre64 = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, inv_K=inv_K, extras=nat, backward=False, batch_stats=True)[2]
        assert nat["targets"]["pos_inds"].numel() == 127 and int(GO.near_kink(nat["maps"], nat["targets"], inv_K, nat["p"]).sum()) == 0
        report = []
        masks = SO.stem_plan_masks(plan, pre64, report)
        total, bad, far = sum(v.numel() for v in pre64), sum(r[2] for r in report), sum(r[3] for r in report)
        print(f"[fpn_bn] whole model signs: {bad} of {total} ReLU elements differ ({bad / total:.1e}; cap 1e-4), {far} beyond 2^-16 (cap 0)")
        assert far == 0 and bad <= WO.SIGN_CAP * total, (bad, far, total)
        e32 = {}
        p64, a64, _ = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, masks=masks, inv_K=inv_K, batch_stats=True)
        p32, a32, _ = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F32, masks=masks, inv_K=inv_K, batch_stats=True, extras=e32)
    fams = {}
    for k in sorted(params):
        sf = WO.stage_and_family(k) or ("stem", "filter" if k.endswith(".weight") and ".norm." not in k else "norm")
        fams.setdefault(sf if sf[0] != "fpn" else ("fpn", NO.family_of(k)), []).append(k)
    assert {("fpn", f) for f in ("weight", "norm_weight", "norm_bias")} <= set(fams) and ("stem", "filter") in fams
    for (stage, fam), ks in sorted(fams.items()):
        _bar([params[k] for k in ks], [p64[k] for k in ks], [p32[k] for k in ks], f"whole:{stage} {fam}")
    tf = {}
    for k in a64:
        tf.setdefault(WO.tensor_family_of(k), []).append(k)
    for fam, ks in sorted(tf.items()):
        _bar([grads[k] for k in ks], [a64[k] for k in ks], [a32[k] for k in ks], f"whole:at {fam}")
    _close({k: v.cpu() for k, v in losses.items()}, {k: e32["losses"][k] for k in losses}, LOSS_REL["kitti"])


# whole_model_grad_oracle.case_inputs' GT seeds 2000 .. 2009 scanned on the CPU on the float64 forward with both norm groups on batch
# statistics: 2003, 2005, 2006 and 2009 leave no positive inside loss_grad_oracle.KINK_MARGIN of a non-smooth point of the loss (the others
# one or two); 2009 has the most positives (127) of those.
WHOLE_MODEL_GT_SEED = 2009


def test_dense_depth_fpn_batch_stats(hiplib):
    """DD3DDenseDepth on DLA-34 with FE.FPN.NORM: BN: fpn_grads under the flag against the chain oracle at the plan's stored activations
    and the feature<l> gradients its box3d tower delivered; the bits of the shallower flag; graph replay against launch by launch."""
    from dd3d_amd.synthetic import make_depth_maps
    from tests import dense_depth_param_grad_oracle as PO
    from tests.util import gpu_model
    case = dict(PO.CASES["dla34_frozenbn_none"])
    case["overrides"] = PO._merge(case["overrides"], FPN_BN)
    cpu = PO.cpu_model(case)
    model = gpu_model(cpu.cfg, {k: v.clone() for k, v in cpu.state_dict().items()}, use_graph=True)
    inputs = PO.case_images(case)
    for x, d in zip(inputs, make_depth_maps(inputs)):
        x["depth"] = d
    base = model.compute_losses(inputs, fpn_grads=True)
    tow = model.compute_losses(inputs, tower_grads=True, fpn_batch_stats=True)
    losses, grads, params = model.compute_losses(inputs, fpn_grads=True, fpn_batch_stats=True)
    assert _same((losses, ), (tow[0], )) and all(torch.equal(grads[k], v) for k, v in tow[1].items()) and all(torch.equal(params[k], v) for k, v in tow[2].items())
    assert set(grads) == set(base[1]) and set(params) == set(base[2]) and not torch.equal(grads["backbone_level3"], base[1]["backbone_level3"])
    plan = model.get_loss_plan(len(inputs), case["H"], case["W"], fpn_grads=True, fpn_batch_stats=True)
    feats, stored = _check_chain("dense_depth", cpu, plan, grads, params, tow[1:])
    _check_raws_and_stats("dense_depth", cpu, plan, feats, stored)
    assert _guards(plan) and all(bool(torch.isfinite(v).all()) for v in losses.values())
    assert _same(model.compute_losses(inputs, fpn_grads=True), base)
    eager = gpu_model(cpu.cfg, {k: v.clone() for k, v in cpu.state_dict().items()}, use_graph=False)
    assert _same(eager.compute_losses(inputs, fpn_grads=True, fpn_batch_stats=True), (losses, grads, params))


def test_one_flagged_plan_on_differing_batches_equals_fresh_models(hiplib):
    """As tests/test_loss_plan_history_gpu.py: one captured plan replayed on batch A, on other pixels and GT, then on a batch without GT,
    with a sentinel written over every tensor the backward's calls and the norms' statistics write in between, against a fresh model on
    each batch."""
    from tests.test_loss_grads_gpu import _model
    from tests.test_loss_plan_history_gpu import _grad_calls_in_the_ops
    flags = dict(fpn_grads=True, fpn_batch_stats=True)
    model = _model("dd3d_kitti_dla34", "dla34_kitti", FPN_BN)
    batches = [_batch(model, 2, 64, 128, "kitti"), _batch(model, 2, 64, 128, "kitti", seed=5, gt_seed=31, empty=(0, )),
               _batch(model, 2, 64, 128, "kitti", seed=7, gt_seed=32, empty=(0, 1))]
    got = []
    for b in batches:
        res = model.compute_losses(b, **flags)
        plan = model.get_loss_plan(*model.canvas_size(b), **flags)
        got.append((res, plan.fpn_batch_stats()))
        calls = _grad_calls_in_the_ops(plan)
        assert {"FpnBnGrads", "FpnConvGrads"} <= {type(c).__name__ for c in calls}
        poisoned = [t for c in calls for t, _ in c._raw] + [st for rec in plan.fpn_bn.values() for st in rec["stats"]] + [plan.fpn_bn_part] + list(plan.tower_slab)
        torch.cuda.synchronize()
        for t in poisoned:
            t.fill_(SENTINEL)
    assert len([k for k in model._plans if k[0] == "losses"]) == 1 and not _same(got[0][0], got[1][0]) and not _same(got[1][0], got[2][0])
    for b, (res, stats) in zip(batches, got):
        fresh = _model("dd3d_kitti_dla34", "dla34_kitti", FPN_BN)
        want = fresh.compute_losses(b, **flags)
        assert _same(res, want) and _same((stats, ), (fresh.get_loss_plan(*fresh.canvas_size(b), **flags).fpn_batch_stats(), ))
        assert not any(bool((v == SENTINEL).any()) for d in res for v in d.values()) and all(bool(torch.isfinite(v).all()) for d in res for v in d.values())
    assert _same(model.compute_losses(batches[0], **flags), got[0][0])


def test_range_guard_retry_with_fpn_batch_stats(hiplib):
    """fpn_output3's norm weight and bias scaled so that p3 passes 4094 (the half range at plane scale 16) and stays below 16376:
    dd3d_bn_apply_topdown_split sets the status bit, an explicit f16x2 model raises, a model on the default arithmetic lowers its plane
    scale to 4 inside compute_losses and returns the bits of a fresh model built at plane scale 4."""
    from tests.test_loss_grads_gpu import _model
    flags = dict(fpn_grads=True, fpn_batch_stats=True)
    base = _model("dd3d_kitti_dla34", "dla34_kitti", FPN_BN)
    inputs = _batch(base, 2, 64, 128, "kitti")
    base.compute_losses(inputs, **flags)
    plan = base.get_loss_plan(*base.canvas_size(inputs), **flags)
    a0 = float(plan.bufs["p3"].view().nchw().float().abs().max())
    sd = {k: v.clone() for k, v in base.state_dict().items()}
    for k in ("weight", "bias"):
        sd[f"backbone.fpn_output3.norm.{k}"] *= 6000.0 / a0

    def build(math=None, act_scale=None):
        m = GC.cpu_model("dd3d_kitti_dla34", FPN_BN)
        m.load_state_dict({k: v.cpu() for k, v in sd.items()})
        m = m.to("cuda").eval()
        m.math, m.act_scale = math, act_scale
        return m

    with pytest.raises(FloatingPointError, match="half range"):
        build(math="f16x2").compute_losses(inputs, **flags)
    model = build()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = model.compute_losses(inputs, **flags)
    msgs = [str(x.message) for x in w if "dd3d_amd" in str(x.message)]
    assert (model.math, model.act_scale) == (None, 4.0) and any("plane scale lowered 16 -> 4" in m for m in msgs), (model.math, model.act_scale, msgs)
    p4 = model.get_loss_plan(*model.canvas_size(inputs), **flags)
    assert p4.fpn_bn["outputs"]["args"].bn.plane_scale == 4.0 and p4.fpn_layers["outputs"].args.x_plane_scale == 4.0
    assert abs(float(p4.bufs["p3"].view().nchw().float().abs().max()) - 6000.0) < 60.0
    there = build(act_scale=4.0)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        want = there.compute_losses(inputs, **flags)
    assert not [x for x in w if "lowered" in str(x.message) or "switching" in str(x.message)]
    assert _same(got, want) and all(bool(torch.isfinite(v).all()) for d in got for v in d.values())


def test_worst_use_of_the_bar_is_reported(hiplib):
    """(Runs last in this file.)  The largest share of the factor 8 any family above used: what profiles/fpn_bn_errors.txt records."""
    for k, v in sorted(WORST.items()):
        print(f"[fpn_bn] plan level, worst use of the factor 8, {k}: {v:.2f}")
    assert all(v <= 8.0 for v in WORST.values())
