"""The composed training backward on the MI355X against ONE autograd pass of the whole model (tests/whole_model_grad_oracle.py):
param_grads and grads of DD3D.compute_losses(inputs, backbone_grads=True) (V2-99: fpn_grads=True; one case with batch_stats=True, the
oracle's tower norms then on the batch's statistics as well) are the gradient of the sum of the loss
dict with respect to the model's parameters, the stem's output, the backbone's output features, the FPN outputs and the head maps.

The five stage tests feed each stage's oracle the gradient the previous stage's kernels produced; nothing here comes from the kernels but
the signs of the plan's stored ReLU outputs (whole_model_grad_oracle.plan_masks: the kernels mask by the stored output, and a float64
forward puts a handful of pre-activations of ~1e-7 relative size on the other side of 0 -- rounding, which moves a gradient
discontinuously).  Those signs are themselves held to two conditions: a mask differs from the float64 sign only where |pre64| is at most
2^-16 of its tensor's largest magnitude, and on at most 1e-4 of all ReLU elements.  The GT seeds are pinned to batches without a positive
on a non-smooth point of the loss (tests/test_whole_model_grads.py).

The bar of a stage's family is the project's, 8 * max(d32, 2^-23 * max|g64|): d32 is the deviation of the oracle's float32 pass from its
float64 pass under the same masks (loss_grad_oracle.bar)."""
import pytest
import torch

from tests import loss_grad_cases as GC
from tests import loss_grad_oracle as GO
from tests import whole_model_grad_oracle as WO

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
LOSS_REL = {"kitti": 1e-4, "nusc": 2e-4}  # tests/test_losses_gpu.py, the loss dict end to end from the uint8 images against a reference forward
_NATURAL = {}


def _natural_forward(case, cpu, inputs, gt, inv_K):
    """The unforced float64 oracle forward of a case's reference (pre-activations, head maps, targets), once per reference."""
    key = case["ref"]
    if key not in _NATURAL:
        ex = {}
        pre = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, inv_K=inv_K, extras=ex, backward=False, batch_stats=bool(case.get("batch_stats")))[2]
        _NATURAL[key] = (pre, ex, inv_K.clone())
    pre, ex, k0 = _NATURAL[key]
    assert torch.equal(k0, inv_K)
    return pre, ex


def _compare(what, rows):
    """rows: (stage, family, kernel tensors, float64 tensors, float32 tensors); one line and one assertion per row."""
    worst = 0.0
    for stage, fam, c, a, b in rows:
        c, a, b = (torch.cat([v.reshape(-1).cpu() for v in vs]) for vs in (c, a, b))
        assert bool(torch.isfinite(c).all()), (what, stage, fam)
        bar, d32, gmax = GO.bar(a.double(), b, torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((c.double() - a.double()).abs().max())
        use = 8 * dev / bar if bar > 0 else 0.0
        worst = max(worst, use)
        print(f"[whole_model_grads] {what} {stage} {fam}: n {a.numel()} max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
        assert gmax > 0.0, (what, stage, fam)
        assert dev <= bar, (what, stage, fam, dev, bar, d32, gmax)
    print(f"[whole_model_grads] {what}: the worst family uses {worst:.2f} of the factor 8")
    return worst


def compare_with_whole_model_oracle(name, case, model, cpu, inputs, gt):
    """The body of the comparison, shared with tests/test_loss_plan_history_gpu.py (plane scale 4, reached through the range guard):
    `model` on the GPU and `cpu` carry the same state dict, `inputs` carry `gt` as their instances; `case`: an entry like those of
    WO.CASES (`ref` keys the cached natural float64 forward; `math` / `act_scale`: what the plan's stored activations must show).
    Returns (the worst use of the factor 8, losses, grads, param_grads of the call)."""
    from tests.test_losses_gpu import _close
    through = {case["grads"]: True}  # backbone_grads, or fpn_grads for V2-99, whose backward stops at the backbone's output features
    bs = bool(case.get("batch_stats"))  # the towers' BatchNorm on the batch's statistics, in the plan and in the oracle alike
    if bs:
        through["batch_stats"] = True
    losses, grads, params = model.compute_losses(inputs, **through)
    plan = model.get_loss_plan(*model.canvas_size(inputs), **through)
    if case["math"] == "bf16x3":  # the case's arithmetic and plane scale reached the stored activations
        assert plan.bufs["level5.cat"].np == 3 and not plan.bufs["level5.cat"].f16
    elif case["act_scale"] is not None:
        assert plan.bufs["level5.cat"].f16 and plan.bufs["level5.cat"].plane_scale == case["act_scale"]
    inv_K = plan.inv_K.view(-1, 3, 3).cpu()
    pre64, nat = _natural_forward(case, cpu, inputs, gt, inv_K)
    assert nat["targets"]["pos_inds"].numel() == case["positives"] and int(GO.near_kink(nat["maps"], nat["targets"], inv_K, nat["p"]).sum()) == 0

    # the signs the kernels used, and the two conditions on them
    report = []
    masks = WO.plan_masks(plan, pre64, report)
    total = sum(v.numel() for v in pre64)
    bad, far = sum(r[2] for r in report), sum(r[3] for r in report)
    for label, n, b, f in report:
        if b:
            print(f"[whole_model_grads] {name} signs {label}: {b} of {n} differ from the float64 forward's, {f} of them beyond 2^-16 of the tensor's maximum")
    print(f"[whole_model_grads] {name} signs: {bad} of {total} ReLU elements differ ({bad / total:.1e}; cap 1e-4), {far} beyond 2^-16 of their tensor's maximum (cap 0)")
    assert far == 0 and bad <= WO.SIGN_CAP * total, (name, bad, far, total)

    e32 = {}
    p64, a64, _ = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, masks=masks, inv_K=inv_K, batch_stats=bs)
    p32, a32, _ = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F32, masks=masks, inv_K=inv_K, extras=e32, batch_stats=bs)

    # every returned parameter, by stage and family; the key sets match
    stage_of = lambda k: WO.stage_and_family(k, backbone_grads=case["grads"] == "backbone_grads")
    compared = sorted(k for k in p64 if stage_of(k) is not None)
    assert sorted(params) == compared
    named = dict(cpu.named_parameters())
    assert all(params[k].shape == named[k].shape and params[k].dtype == F32 for k in params)
    fams = {}
    for k in compared:
        fams.setdefault(stage_of(k), []).append(k)
    rows = [(st, fam, [params[k] for k in ks], [p64[k] for k in ks], [p32[k] for k in ks]) for (st, fam), ks in sorted(fams.items())]
    assert {st for st, *_ in rows} == {"predictors", "towers", "fpn"} | ({f"backbone level{n}" for n in (2, 3, 4, 5)} if case["grads"] == "backbone_grads" else set())
    # the gradients at tensors: level1, the backbone features (the FPN's part), the FPN outputs (the heads' part), the head maps
    assert all(k in grads for k in a64)
    tf = {}
    for k in a64:
        tf.setdefault(WO.tensor_family_of(k), []).append(k)
    rows += [("tensors", fam, [grads[k] for k in ks], [a64[k] for k in ks], [a32[k] for k in ks]) for fam, ks in sorted(tf.items())]
    worst = _compare(name, rows)

    # the loss dict against the float32 oracle's own forward
    ref_losses = {k: e32["losses"][k] for k in losses}
    for k in losses:
        print(f"[whole_model_grads] {name} {k}: {float(losses[k]):.7g} oracle {float(ref_losses[k]):.7g}")
    _close({k: v.cpu() for k, v in losses.items()}, ref_losses, LOSS_REL[case["ds"]])
    return worst, losses, grads, params


@pytest.mark.parametrize("name", list(WO.CASES))
def test_composed_backward_is_the_whole_model_gradient(hiplib, name):
    from tests.test_loss_grads_gpu import _model
    case = WO.CASES[name]
    model = _model(case["exp"], case["weights"], case["overrides"])
    model.math, model.act_scale = case["math"], case["act_scale"]
    cpu = GC.cpu_model(case["exp"], case["overrides"])
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    inputs, gt = WO.case_inputs(case, cpu)
    for x, g in zip(inputs, gt):
        x["instances"] = g
    through = dict({case["grads"]: True}, **({"batch_stats": True} if case.get("batch_stats") else {}))
    _, losses, grads, params = compare_with_whole_model_oracle(name, case, model, cpu, inputs, gt)

    # a second call is bit-equal; the captured graph equals launch-by-launch execution
    l2, g2, p2 = model.compute_losses(inputs, **through)
    assert all(torch.equal(l2[k], losses[k]) for k in losses) and all(torch.equal(g2[k], grads[k]) for k in grads) and all(torch.equal(p2[k], params[k]) for k in params)
    model.use_graph = False
    model.invalidate_plans()
    l3, g3, p3 = model.compute_losses(inputs, **through)
    assert all(torch.equal(l3[k], losses[k]) for k in losses) and all(torch.equal(g3[k], grads[k]) for k in grads) and all(torch.equal(p3[k], params[k]) for k in params)
