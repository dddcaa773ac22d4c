"""compute_losses(backbone_batch_stats=True) on the MI355X: the DLA-34 bottom-up network's norms (FE.BACKBONE.NORM: BN) on the batch's
statistics, forward and backward, end to end from the uint8 images (engine.LossPlan(backbone_batch_stats=True), csrc/backbone_bn.hip).

dd3d_kitti_dla34 on the whole-model cases' batch, two 128 x 384 images (the smallest canvas tests/whole_model_grad_oracle.py uses): the flag
alone under stem_grads, and together with batch_stats and fpn_batch_stats under FE.FPN.NORM: BN -- BN everywhere, the reference's train()
step -- each against ONE autograd pass of the whole model per precision under the stored signs of all ReLUs, the chosen norms through
F.batch_norm(training=True) (tests/backbone_bn_oracle.norms_on).  Every parameter and tensor gradient by family within loss_grad_oracle.bar
= 8 * max(d32, 2^-23 * max|g64|); every name of named_parameters() present; backbone_batch_stats() against expected_stats on the plan's
stored raw convolution outputs; the model's buffers unchanged; a second replay on another batch bit-equal to a fresh plan on that batch.
The composed call on DD3DDenseDepth against the chain oracle of the bottom-up network.  The GT seeds are pinned to batches without a
positive on a non-smooth point of the loss on the float64 forward (asserted)."""
import pytest
import torch

from tests import backbone_bn_oracle as BN
from tests import loss_grad_cases as GC
from tests.test_tower_bn_plan_gpu import _batch, _same

pytestmark = pytest.mark.gpu

BB_BN = {"FE": {"BACKBONE": {"NORM": "BN"}}}
EVERYWHERE = {"FE": {"BACKBONE": {"NORM": "BN"}, "FPN": {"NORM": "BN"}}}
LOSS_REL = 1e-4  # tests/test_whole_model_grads_gpu.py (KITTI)
WORST = {}
# whole_model_grad_oracle.case_inputs' GT seeds 2000 .. 2011 scanned on the CPU on the float64 forward with the case's norms on batch
# statistics: alone, 2002, 2003, 2008 and 2011 leave no positive inside loss_grad_oracle.KINK_MARGIN of a non-smooth point of the loss (the
# others one or two), 2011 with the most positives (130); with BN everywhere 2005, 2006, 2008 and 2009 do, 2009 with the most (127).
GT_SEED = {"alone": 2011, "everywhere": 2009}
POSITIVES = {"alone": 130, "everywhere": 127}


@pytest.fixture(autouse=True)
def _default_arithmetic(monkeypatch):
    monkeypatch.delenv("DD3D_MATH", raising=False)
    monkeypatch.delenv("DD3D_F16_ACT_SCALE", raising=False)


def _bar(got, ref64, ref32, what):
    cat = lambda vs: torch.cat([v.reshape(-1).cpu() for v in vs])
    c, a, b = cat(got), cat(ref64).double(), cat(ref32)
    bar, d32, gmax = BN.bar(a, b, torch.ones(a.shape[0], dtype=torch.bool))
    dev = float((c.double() - a).abs().max())
    use = 8 * dev / bar if bar > 0 else 0.0
    fam = what.split(":", 1)[-1]
    WORST[fam] = max(WORST.get(fam, 0.0), use)
    print(f"[backbone_bn] {what}: n {a.numel()} max|ref64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
    assert bool(torch.isfinite(c).all()) and dev <= bar and gmax > 0.0, (what, dev, bar, d32, gmax)


def _cpu_twin(model, exp, overrides):
    cpu = GC.cpu_model(exp, overrides)
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    return cpu


def _stored_raws(model, plan):
    """{norm prefix: the plan's stored raw convolution output, NCHW float32 on the CPU}."""
    names = {id(b): k for k, b in model.named_buffers()}
    return {names[id(rec["norm"].running_mean)][:-len(".running_mean")]: rec["raw"].nchw().float().cpu().contiguous() for rec in plan.backbone_bn.values()}


def _check_stats(tag, cpu, model, plan):
    stats = plan.backbone_batch_stats()
    assert sorted(stats) == BN.batch_stats_names(cpu) and len(stats) == 4 * 37
    stored = dict(raw=_stored_raws(model, plan))
    w64, w32 = BN.expected_stats(cpu, stored, torch.float64), BN.expected_stats(cpu, stored, torch.float32)
    for kind in ("batch_mean", "batch_var", "running_mean", "running_var"):
        ks = [k for k in sorted(stats) if k.endswith(kind)]
        _bar([stats[k] for k in ks], [w64[k] for k in ks], [w32[k] for k in ks], f"{tag}:{kind}")
    return stats


def _masks_off_the_plan(tag, plan, pre64, pre32, report):
    """whole_model_grad_oracle.plan_masks / stem_grad_oracle.stem_plan_masks -- one boolean mask per ReLU call, the sign of the plan's
    decoded stored tensor, the mapping from call to buffer checked by value -- with the condition for taking a mask stated against the
    reference's own error: the stored tensor is within max(STORED_TOL * max(1, max|ref64|), 8 * d32) of the float64 ReLU output, d32 the
    distance of torch's float32 forward from the float64 one at that call.  With BN everywhere torch's float32 forward itself is up to
    4.6e-4 from float64 at the towers' P7 layers (six values per channel behind the bottom-up network's level5 norms, 96 values per
    channel: measured on the CPU, 1.5 times the 1e-4 condition at three calls, within it at the other 96), so no float32 forward can meet
    the fixed condition there; everywhere else the first term decides, as in plan_masks.  The sign report's margin follows the same
    rule: a stored sign may differ from the float64 one where |pre| <= max(SIGN_NEAR * max|pre|, 8 * d32) of its call."""
    from tests import stem_grad_oracle as SO
    from tests import whole_model_grad_oracle as WO
    from tests.util import decode
    sites = WO.relu_sites(plan)
    for k, name in enumerate(SO.STEM_BUFFERS):
        sites[k] = (name, plan.bufs[name], 0, None, False)
    assert len(sites) == len(pre64) == len(pre32) and all(s is not None for s in sites)
    masks, worst = [], (0.0, None)
    for k, ((label, buf, c0, n, stored_is_pre), pre, p32) in enumerate(zip(sites, pre64, pre32)):
        got = decode(buf, c0, n).double()
        ref = pre.double() if stored_is_pre else pre.double().clamp(min=0)
        r32 = p32.double() if stored_is_pre else p32.double().clamp(min=0)
        assert tuple(got.shape) == tuple(ref.shape), (k, label)
        err, d32, fixed = float((got - ref).abs().max()), float((r32 - ref).abs().max()), WO.STORED_TOL * max(1.0, float(ref.abs().max()))
        tol = max(fixed, 8 * d32)
        if err / tol > worst[0]:
            worst = (err / tol, f"{label}: stored {err:.3e} from float64, torch float32 {d32:.3e}, fixed condition {fixed:.3e}, condition {tol:.3e}")
        if err > fixed:
            print(f"[backbone_bn] {tag} ReLU call {k} ({label}): stored {err:.3e} from float64 (fixed condition {fixed:.3e}); torch float32 is {d32:.3e} from it")
        assert err <= tol, (k, label, err, d32, fixed)
        mask = got > 0
        masks.append(mask)
        bad = mask != (pre > 0)
        near = max(WO.SIGN_NEAR * float(pre.abs().max()), 8 * d32)  # (a pre-activation inside the reference's own float32 error of zero has no sign to keep)
        report.append((label, pre.numel(), int(bad.sum()), int((bad & (pre.abs() > near)).sum())))
    print(f"[backbone_bn] {tag} stored activations, closest to the condition: {worst[1]}")
    return masks


def _whole_model(tag, overrides, norms, towers, fpn):
    from tests import loss_grad_oracle as GO
    from tests import whole_model_grad_oracle as WO
    from tests.test_loss_grads_gpu import _model
    from tests.test_losses_gpu import _close
    exp = "dd3d_kitti_dla34"
    model = _model(exp, "dla34_kitti", overrides)
    cpu = _cpu_twin(model, exp, overrides)
    inputs, gt = WO.case_inputs(dict(WO.CASES["kitti_dla34"], gt_seed=GT_SEED[tag]), cpu)
    for x, g in zip(inputs, gt):
        x["instances"] = g
    flags = dict(norms, stem_grads=True)
    shallow = model.compute_losses(inputs, backbone_grads=True, **norms)
    losses, grads, params = model.compute_losses(inputs, **flags)
    assert _same((shallow[0], ), (losses, )) and all(torch.equal(grads[k], v) for k, v in shallow[1].items()) and all(torch.equal(params[k], v) for k, v in shallow[2].items())
    canvas = model.canvas_size(inputs)
    plan = model.get_loss_plan(*canvas, **flags)
    assert plan.with_backbone_batch_stats and not plan.fused_stem and plan.graph is not None and model.get_loss_plan(*canvas, stem_grads=True) is not plan
    named = dict(cpu.named_parameters())
    assert sorted(params) == sorted(named) and all(params[k].shape == named[k].shape and params[k].dtype == torch.float32 for k in params)
    inv_K = plan.inv_K.view(-1, 3, 3).cpu()
    F64, F32 = torch.float64, torch.float32
    with BN.norms_on(cpu, towers=towers, fpn=fpn) as chosen:
        assert len(chosen) == 37 + (8 * 5 if towers else 0) + (6 if fpn else 0)
        nat = {}
        pre64 = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, inv_K=inv_K, extras=nat, backward=False, batch_stats=True)[2]
        assert nat["targets"]["pos_inds"].numel() == POSITIVES[tag] and int(GO.near_kink(nat["maps"], nat["targets"], inv_K, nat["p"]).sum()) == 0
        pre32 = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F32, inv_K=inv_K, backward=False, batch_stats=True)[2]
        report = []
        masks = _masks_off_the_plan(tag, plan, pre64, pre32, report)
        total, bad, far = sum(v.numel() for v in pre64), sum(r[2] for r in report), sum(r[3] for r in report)
        print(f"[backbone_bn] {tag} signs: {bad} of {total} ReLU elements differ ({bad / total:.1e}; cap 1e-4), {far} beyond max(2^-16 max|pre|, 8 d32) (cap 0)")
        assert far == 0 and bad <= WO.SIGN_CAP * total, (bad, far, total)
        e32 = {}
        p64, a64, _ = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, masks=masks, inv_K=inv_K, batch_stats=True)
        p32, a32, _ = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F32, masks=masks, inv_K=inv_K, batch_stats=True, extras=e32)
    fams = {}
    for k in sorted(params):
        sf = WO.stage_and_family(k)
        if sf is None:
            sf = ("stem", BN.family_of(k))
        elif sf[0].startswith("backbone") or sf[0] == "fpn":
            sf = (sf[0], BN.family_of(k))
        fams.setdefault(sf, []).append(k)
    assert {("stem", f) for f in ("weight", "norm_weight", "norm_bias")} <= set(fams) and ("backbone level5", "norm_weight") in fams
    for (stage, fam), ks in sorted(fams.items()):
        _bar([params[k] for k in ks], [p64[k] for k in ks], [p32[k] for k in ks], f"{tag}:{stage} {fam}")
    tf = {}
    for k in a64:
        tf.setdefault(WO.tensor_family_of(k), []).append(k)
    for fam, ks in sorted(tf.items()):
        _bar([grads[k] for k in ks], [a64[k] for k in ks], [a32[k] for k in ks], f"{tag}:at {fam}")
    _close({k: v.cpu() for k, v in losses.items()}, {k: e32["losses"][k] for k in losses}, LOSS_REL)
    stats = _check_stats(tag, cpu, model, plan)
    assert all(lay.guards_intact(0.0) for lay in list(plan.backbone_layers.values()) + list(plan.stem_layers.values()))
    assert all(lay.bn.guards_intact(0.0) for lay in list(plan.backbone_layers.values()) + list(plan.stem_layers.values()) if getattr(lay, "bn", None) is not None)
    assert all(torch.equal(b.cpu(), cpu.state_dict()[k]) for k, b in model.named_buffers())  # the model's buffers are never written
    # the same call again: the same bits; then another batch on the same captured plan against a fresh model's plan on that batch
    assert _same(model.compute_losses(inputs, **flags), (losses, grads, params)) and _same((plan.backbone_batch_stats(), ), (stats, ))
    other = _batch(model, 2, 128, 384, "kitti", seed=5, gt_seed=31)
    got = model.compute_losses(other, **flags)
    assert model.get_loss_plan(*model.canvas_size(other), **flags) is plan and not _same((got[2], ), (params, ))
    got_stats = plan.backbone_batch_stats()
    fresh = _model(exp, "dla34_kitti", overrides)
    want = fresh.compute_losses(other, **flags)
    assert _same(got, want) and _same((got_stats, ), (fresh.get_loss_plan(*fresh.canvas_size(other), **flags).backbone_batch_stats(), ))
    assert all(bool(torch.isfinite(v).all()) for d in got for v in d.values())
    return model, plan


def test_backbone_batch_stats_alone_against_the_whole_model(hiplib):
    """compute_losses(stem_grads=True, backbone_batch_stats=True): the bottom-up norms on batch statistics, the FPN norm-less, the towers
    on their running statistics."""
    from dd3d_amd import hip
    _, plan = _whole_model("alone", BB_BN, dict(backbone_batch_stats=True), False, False)
    assert len(plan.backbone_bn) == 37 and not hasattr(plan, "fpn_bn") and not plan.tower_bn
    rec = plan.backbone_bn["level5.tree1.conv2"]
    assert rec["args"].bn.C == 512 and rec["args"].bn.N[0] == 2 * 4 * 12 and rec["args"].act == hip.BBN_RESIDUAL and rec["args"].bn.math_mode == hip.MATH_F16X2
    assert plan.backbone_bn["base_layer"]["args"].bn.C == 16 and plan.backbone_bn["base_layer"]["args"].bn.math_mode == hip.MATH_F32


def test_bn_everywhere_against_the_whole_model(hiplib):
    """batch_stats=True, fpn_batch_stats=True, backbone_batch_stats=True under FE.FPN.NORM: BN: every norm of the model on the batch's
    statistics -- the loss dict, the running statistics and all parameter gradients of the reference's train() step from one plan."""
    _, plan = _whole_model("everywhere", EVERYWHERE, dict(batch_stats=True, fpn_batch_stats=True, backbone_batch_stats=True), True, True)
    assert len(plan.backbone_bn) == 37 and len(plan.tower_bn) == 8 and sorted(plan.fpn_bn) == ["laterals", "outputs"]
    assert len(plan.tower_batch_stats()) == 4 * 40 and len(plan.fpn_batch_stats()) == 4 * 6


def _bottom_up_masks(plan):
    """One boolean mask per ReLU call of the bottom-up network (the oracle's call order), from the plan's stored tensors."""
    from tests import stem_grad_oracle as SO
    from tests import whole_model_grad_oracle as WO
    from tests.util import decode
    dla = plan.model.backbone.bottom_up
    masks = [decode(plan.bufs[n]) > 0 for n in SO.STEM_BUFFERS]
    for lvl in range(2, 6):
        masks += [decode(plan.bufs[n], c0, c) > 0 for n, c0, c in WO._tree_sites(getattr(dla, f"level{lvl}"), f"level{lvl}")]
    return [m.cpu() for m in masks]


def test_dense_depth_bn_everywhere(hiplib):
    """DD3DDenseDepth on DLA-34 with BN in the bottom-up network, the FPN and the box3d tower, all three norm flags under stem_grads: the
    bits of the shallower flag; every name of named_parameters(); the bottom-up network's parameter gradients and the gradients at the
    stem's tensors against the chain oracle (autograd through the batch-statistics forward on the plan's normalised canvas, under the
    plan's stored signs, fed the backbone_level<n> gradients the FPN delivered); the statistics read-out; graph replay against launch
    by launch."""
    from dd3d_amd.synthetic import make_depth_maps
    from tests import dense_depth_param_grad_oracle as PO
    from tests.util import gpu_model
    case = dict(PO.CASES["dla34_bn_none"])
    case["overrides"] = PO._merge(case["overrides"], EVERYWHERE)
    cpu = PO.cpu_model(case)
    model = gpu_model(cpu.cfg, {k: v.clone() for k, v in cpu.state_dict().items()}, use_graph=True)
    inputs = PO.case_images(case)
    for x, d in zip(inputs, make_depth_maps(inputs)):
        x["depth"] = d
    norms = dict(batch_stats=True, fpn_batch_stats=True, backbone_batch_stats=True)
    shallow = model.compute_losses(inputs, fpn_grads=True, **norms)
    losses, grads, params = model.compute_losses(inputs, stem_grads=True, **norms)
    assert _same((losses, ), (shallow[0], )) and all(torch.equal(grads[k], v) for k, v in shallow[1].items()) and all(torch.equal(params[k], v) for k, v in shallow[2].items())
    assert sorted(params) == sorted(k for k, _ in cpu.named_parameters()) and all(bool(torch.isfinite(v).all()) for v in losses.values())
    plan = model.get_loss_plan(len(inputs), case["H"], case["W"], stem_grads=True, **norms)
    img = plan.normalized_image().float().cpu().contiguous()
    masks = _bottom_up_masks(plan)
    G = {n: grads[f"backbone_{n}"].cpu() for n in ("level3", "level4", "level5")}
    (p64, a64), (p32, a32) = BN.chain_grads(cpu, masks, img, G, torch.float64), BN.chain_grads(cpu, masks, img, G, torch.float32)
    fams = {}
    for k in sorted(p64):
        fams.setdefault(BN.family_of(k), []).append(k)
    for fam, ks in sorted(fams.items()):
        _bar([params[k] for k in ks], [p64[k] for k in ks], [p32[k] for k in ks], f"dense_depth:bottom_up {fam}")
    # (the level1 gradient the plan returns is the tree's part alone, as the chain oracle's: the bottom-up outputs are its only consumers)
    for k in sorted(a64):
        _bar([grads[k]], [a64[k]], [a32[k]], f"dense_depth:at {k}")
    _check_stats("dense_depth", cpu, model, plan)
    assert all(torch.equal(b.cpu(), cpu.state_dict()[k]) for k, b in model.named_buffers())
    eager = gpu_model(cpu.cfg, {k: v.clone() for k, v in cpu.state_dict().items()}, use_graph=False)
    assert _same(eager.compute_losses(inputs, stem_grads=True, **norms), (losses, grads, params))


def test_worst_use_of_the_bar_is_reported(hiplib):
    """(Runs last in this file.)  The largest share of the factor 8 any family above used: what profiles/backbone_bn_errors.txt records."""
    for k, v in sorted(WORST.items()):
        print(f"[backbone_bn] plan level, worst use of the factor 8, {k}: {v:.2f}")
    assert all(v <= 8.0 for v in WORST.values())
