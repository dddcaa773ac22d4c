"""DD3D.compute_losses(vovnet_grads=True) on the MI355X against ONE autograd pass of the whole V2-99 model (the kitti_v99 case of
tests/whole_model_grad_oracle.py: its model, weights, 1 x 128 x 256 canvas and GT seed): param_grads and grads are the gradient of the sum
of the loss dict with respect to every parameter but stem_1's filter, stem_1's output, the backbone's output features (the FPN's part),
the FPN outputs and the head maps.

Nothing comes from the kernels but the signs of the plan's stored ReLU outputs (vovnet_grad_oracle.plan_masks: every VoVNet ReLU but
stem_1's is mapped to its stored tensor and validated by value), held to whole_model_grad_oracle's SIGN_NEAR / SIGN_CAP.  Two more
non-smooth points are asserted away rather than forced: no eSE gate's z within 1e-3 of the hard sigmoid's clamp edges +-3 (the kernels'
and the float64 forward's), and no 3x3 pool window whose arg-max differs between the decoded stored input and the float64 forward.  The
forward depends on the seeded image and weights alone; should a change to either violate a condition, pick another input seed.

The bar of a stage's family is the project's, 8 * max(d32, 2^-23 * max|g64|) (loss_grad_oracle.bar).  The float64 and float32 oracle
passes run once, in a module-scoped fixture."""
import os

import pytest
import torch

from tests import loss_grad_cases as GC
from tests import loss_grad_oracle as GO
from tests import vovnet_grad_oracle as VG
from tests import whole_model_grad_oracle as WO
from tests.util import decode

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
ERRORS = os.environ.get("DD3D_VOVNET_ERRORS_FILE")  # tests/gpu_vovnet_grad_time.py sets it: the measured ratios go to profiles/


@pytest.fixture(scope="module")
def run(hiplib):
    from tests.test_loss_grads_gpu import _model
    case = WO.CASES["kitti_v99"]
    model = _model(case["exp"], case["weights"], case["overrides"])
    cpu = GC.cpu_model(case["exp"], case["overrides"])
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    inputs, gt = WO.case_inputs(case, cpu)
    for x, g in zip(inputs, gt):
        x["instances"] = g
    ref = model.compute_losses(inputs, fpn_grads=True)
    ref = tuple({k: v.clone() for k, v in d.items()} for d in ref)
    losses, grads, params = model.compute_losses(inputs, vovnet_grads=True)
    plan = model.get_loss_plan(*model.canvas_size(inputs), vovnet_grads=True)
    inv_K = plan.inv_K.view(-1, 3, 3).cpu()
    nat = {}
    pre64 = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, inv_K=inv_K, extras=nat, backward=False)[2]
    report = []
    masks = VG.plan_masks(plan, pre64, report)
    e32 = {}
    p64, a64, _ = VG.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, masks=masks, inv_K=inv_K)
    p32, a32, _ = VG.whole_model_grads(cpu, cpu.cfg, inputs, gt, F32, masks=masks, inv_K=inv_K, extras=e32)
    return dict(case=case, model=model, cpu=cpu, inputs=inputs, gt=gt, ref=ref, losses=losses, grads=grads, params=params, plan=plan, inv_K=inv_K, nat=nat,
                pre64=pre64, report=report, p64=p64, a64=a64, p32=p32, a32=a32, e32=e32)


def test_the_case_is_away_from_every_non_smooth_point(run):
    case, nat, plan, cpu = run["case"], run["nat"], run["plan"], run["cpu"]
    assert len(run["pre64"]) == case["relus"] and nat["targets"]["pos_inds"].numel() == case["positives"]
    assert int(GO.near_kink(nat["maps"], nat["targets"], run["inv_K"], nat["p"]).sum()) == 0
    # ReLU signs: the conditions of tests/test_whole_model_grads_gpu.py, now over the VoVNet's stored tensors too
    total = sum(v.numel() for v in run["pre64"])
    bad, far = sum(r[2] for r in run["report"]), sum(r[3] for r in run["report"])
    assert len(run["report"]) == case["relus"] - 1  # every ReLU call but stem_1's reads a stored tensor
    print(f"[vovnet_whole_model] signs: {bad} of {total} ReLU elements differ ({bad / total:.1e}; cap 1e-4), {far} beyond 2^-16 of their tensor's maximum (cap 0)")
    assert far == 0 and bad <= WO.SIGN_CAP * total, (bad, far, total)
    # eSE gates: none within 1e-3 of a clamp edge, in the kernels' z and in the float64 forward's, and both on the same side
    z64 = VG.ese_gates64(cpu, nat["relu_out"])
    margin = 1e9
    for key, z in z64.items():
        zk = plan.vovnet_layers[key + ".ese"].z.cpu().double()
        margin = min(margin, float((z.abs() - 3).abs().min()), float((zk.abs() - 3).abs().min()))
        assert torch.equal(zk > -3, z > -3) and torch.equal(zk < 3, z < 3), key
    print(f"[vovnet_whole_model] eSE gates: the closest z is {margin:.3e} from a clamp edge (bar 1e-3)")
    assert margin > 1e-3
    # pools: the arg-max of every window agrees between the decoded stored input and the float64 forward
    for sname in ("stage2", "stage3", "stage4"):
        by, bx = VG.pool3_argmax(decode(plan.bufs[sname + ".out"]))
        ry, rx = VG.pool3_argmax(nat["bottom_up"][sname].double())
        differ = int(((by != ry) | (bx != rx)).sum())
        print(f"[vovnet_whole_model] pool after {sname}: {differ} of {by.numel()} windows pick another arg-max than the float64 forward")
        assert differ == 0, sname


def test_everything_fpn_grads_returns_is_bit_equal(run):
    ref_losses, ref_grads, ref_params = run["ref"]
    losses, grads, params = run["losses"], run["grads"], run["params"]
    assert list(losses) == list(ref_losses) and all(torch.equal(losses[k], ref_losses[k]) for k in losses)
    assert all(torch.equal(grads[k], ref_grads[k]) for k in ref_grads) and all(torch.equal(params[k], ref_params[k]) for k in ref_params)
    assert [k for k in grads if k not in ref_grads] == ["backbone_stem_1"]
    assert sorted(k for k in params if k not in ref_params) == VG.vovnet_param_names(run["cpu"])
    plan = run["plan"]
    assert grads["backbone_stem_1"].shape == (1, 64, plan.Hp // 2, plan.Wp // 2) and grads["backbone_stem_1"].dtype == F32
    assert all(lay.guards_intact(0.0) for lay in plan.vovnet_layers.values())
    with pytest.raises(NotImplementedError, match="V2-99"):
        run["model"].get_loss_plan(1, 128, 256, backbone_grads=True)


def test_composed_backward_is_the_whole_model_gradient(run):
    params, grads, p64, p32, a64, a32, cpu = (run[k] for k in ("params", "grads", "p64", "p32", "a64", "a32", "cpu"))

    def stage_of(k):
        if k.startswith("backbone.bottom_up."):
            if ".stem.stem_1/" in k:
                return None
            return "vovnet " + k.split(".")[2], VG.family_of(k)
        return WO.stage_and_family(k, backbone_grads=False)

    compared = sorted(k for k in p64 if stage_of(k) is not None)
    assert sorted(params) == compared
    named = dict(cpu.named_parameters())
    assert all(params[k].shape == named[k].shape and params[k].dtype == F32 for k in params)
    fams = {}
    for k in compared:
        fams.setdefault(stage_of(k), []).append(k)
    rows = [(st, fam, [params[k] for k in ks], [p64[k] for k in ks], [p32[k] for k in ks]) for (st, fam), ks in sorted(fams.items())]
    assert {st for st, *_ in rows} == {"predictors", "towers", "fpn", "vovnet stem"} | {f"vovnet stage{n}" for n in (2, 3, 4, 5)}
    assert all(k in grads for k in a64) and "backbone_stem_1" in a64
    tf = {}
    for k in a64:
        tf.setdefault(WO.tensor_family_of(k), []).append(k)
    rows += [("tensors", fam, [grads[k] for k in ks], [a64[k] for k in ks], [a32[k] for k in ks]) for fam, ks in sorted(tf.items())]
    lines, failed = [], []
    for stage, fam, c, a, b in rows:
        c, a, b = (torch.cat([v.reshape(-1).cpu() for v in vs]) for vs in (c, a, b))
        assert bool(torch.isfinite(c).all()), (stage, fam)
        bar, d32, gmax = GO.bar(a.double(), b, torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((c.double() - a.double()).abs().max())
        use = 8 * dev / bar if bar > 0 else 0.0
        lines.append(f"{stage} {fam}: n {a.numel()} max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
        print("[vovnet_whole_model]", lines[-1])
        if not (gmax > 0.0 and dev <= bar):
            failed.append((stage, fam, dev, bar, d32, gmax))
    if ERRORS:
        with open(ERRORS, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert not failed, failed
    # the loss dict against the float32 oracle's own forward
    from tests.test_losses_gpu import _close
    _close({k: v.cpu() for k, v in run["losses"].items()}, {k: run["e32"]["losses"][k] for k in run["losses"]}, 1e-4)


def test_a_second_run_and_launch_by_launch_execution_give_the_same_bits(run):
    model, inputs = run["model"], run["inputs"]
    l2, g2, p2 = model.compute_losses(inputs, vovnet_grads=True)
    assert all(torch.equal(l2[k], run["losses"][k]) for k in l2) and all(torch.equal(g2[k], run["grads"][k]) for k in g2)
    assert all(torch.equal(p2[k], run["params"][k]) for k in p2)
    model.use_graph = False
    model.invalidate_plans()
    try:
        l3, g3, p3 = model.compute_losses(inputs, vovnet_grads=True)
    finally:
        model.use_graph = True
        model.invalidate_plans()
    assert all(torch.equal(l3[k], run["losses"][k]) for k in l3) and all(torch.equal(g3[k], run["grads"][k]) for k in g3)
    assert all(torch.equal(p3[k], run["params"][k]) for k in p3)
