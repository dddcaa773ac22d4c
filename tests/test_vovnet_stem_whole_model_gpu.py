"""DD3D.compute_losses(vovnet_stem_grads=True) on the MI355X against ONE autograd pass of the whole V2-99 model (the kitti_v99 case of
tests/whole_model_grad_oracle.py, as tests/test_vovnet_whole_model_gpu.py runs it): everything vovnet_grads returns bit for bit, param_grads'
keys are named_parameters(), and stem_1's filter -- with a BN backbone its norm weight and bias too -- is the gradient of the sum of the
loss dict.

Nothing comes from the kernels but the signs of the plan's stored ReLU outputs: EVERY ReLU call is mapped to its stored tensor and
validated by value, stem_1's (`stem.0`) included (vovnet_stem_grad_cases.plan_masks), held to whole_model_grad_oracle's SIGN_NEAR /
SIGN_CAP; tests/test_vovnet_stem_grads.py shows on the CPU that the reference alone meets that condition in stem_1.  The other
non-smooth points are asserted away as in tests/test_vovnet_whole_model_gpu.py: no kink positive, no eSE gate within 1e-3 of a clamp edge,
no pool window with another arg-max.

The bar is the project's, 8 * max(d32, 2^-23 * max|g64|) (loss_grad_oracle.bar).  The oracle passes run once per backbone norm, in
module-scoped fixtures."""
import os

import pytest
import torch

from tests import loss_grad_cases as GC
from tests import loss_grad_oracle as GO
from tests import loss_plan_history_cases as HC
from tests import vovnet_grad_oracle as VG
from tests import vovnet_stem_grad_cases as VS
from tests import whole_model_grad_oracle as WO
from tests.util import decode

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
ERRORS = os.environ.get("DD3D_VOVNET_STEM_ERRORS_FILE")  # tests/gpu_vovnet_stem_grad_time.py sets it: the measured ratios go to profiles/
BN_BACKBONE = {"FE": {"BACKBONE": {"NORM": "BN"}}}
W1, NW1, NB1 = VS.STEM1 + "conv.weight", VS.STEM1 + "norm.weight", VS.STEM1 + "norm.bias"


def _clone(res):
    return tuple({k: v.clone() for k, v in d.items()} for d in res)


def _run(norm):
    from tests.test_loss_grads_gpu import _model
    case = dict(WO.CASES["kitti_v99"], overrides=BN_BACKBONE if norm == "BN" else None)
    model = _model(case["exp"], case["weights"], case["overrides"])
    cpu = GC.cpu_model(case["exp"], case["overrides"])
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    inputs, gt = WO.case_inputs(case, cpu)
    for x, g in zip(inputs, gt):
        x["instances"] = g
    ref = _clone(model.compute_losses(inputs, vovnet_grads=True))
    losses, grads, params = model.compute_losses(inputs, vovnet_stem_grads=True)
    plan = model.get_loss_plan(*model.canvas_size(inputs), vovnet_stem_grads=True)
    inv_K = plan.inv_K.view(-1, 3, 3).cpu()
    nat = {}
    pre64 = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, inv_K=inv_K, extras=nat, backward=False)[2]
    report = []
    masks = VS.plan_masks(plan, pre64, report)
    p64, a64, _ = VG.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, masks=masks, inv_K=inv_K)
    p32, a32, _ = VG.whole_model_grads(cpu, cpu.cfg, inputs, gt, F32, masks=masks, inv_K=inv_K)
    return dict(case=case, model=model, cpu=cpu, inputs=inputs, gt=gt, ref=ref, losses=losses, grads=grads, params=params, plan=plan, inv_K=inv_K, nat=nat,
                pre64=pre64, report=report, p64=p64, a64=a64, p32=p32, a32=a32)


@pytest.fixture(scope="module")
def run(hiplib):
    return _run("FrozenBN")


@pytest.fixture(scope="module")
def run_bn(hiplib):
    return _run("BN")


def _rows(r, rows, what):
    lines, failed = [], []
    for stage, fam, keys in rows:
        c, a, b = (torch.cat([d[k].reshape(-1).cpu() for k in keys]) for d in (r["params"], r["p64"], r["p32"]))
        assert bool(torch.isfinite(c).all()), (stage, fam)
        bar, d32, gmax = GO.bar(a.double(), b, torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((c.double() - a.double()).abs().max())
        use = 8 * dev / bar if bar > 0 else 0.0
        lines.append(f"{what} {stage} {fam}: n {a.numel()} max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
        print("[vovnet_stem_whole_model]", lines[-1])
        if not (gmax > 0.0 and dev <= bar):
            failed.append((stage, fam, dev, bar, d32, gmax))
    if ERRORS:
        with open(ERRORS, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not failed, failed


def test_the_case_is_away_from_every_non_smooth_point_with_stem_1_mapped(run):
    r = run
    case, nat, plan, cpu = r["case"], r["nat"], r["plan"], r["cpu"]
    assert len(r["pre64"]) == case["relus"] and nat["targets"]["pos_inds"].numel() == case["positives"]
    assert int(GO.near_kink(nat["maps"], nat["targets"], r["inv_K"], nat["p"]).sum()) == 0
    # every ReLU call reads a stored tensor, stem_1's too: `stem.0`, validated by value like the others
    assert len(r["report"]) == case["relus"] and r["report"][0][0] == "stem.0" and r["report"][0][1] == r["pre64"][0].numel() == 64 * 64 * 128
    total = sum(v.numel() for v in r["pre64"])
    bad, far = sum(x[2] for x in r["report"]), sum(x[3] for x in r["report"])
    print(f"[vovnet_stem_whole_model] signs stem.0: {r['report'][0][2]} of {r['report'][0][1]} differ from the float64 forward's, {r['report'][0][3]} beyond 2^-16")
    print(f"[vovnet_stem_whole_model] signs: {bad} of {total} ReLU elements differ ({bad / total:.1e}; cap 1e-4), {far} beyond 2^-16 of their tensor's "
          "maximum (cap 0)")
    assert far == 0 and bad <= WO.SIGN_CAP * total, (bad, far, total)
    z64 = VG.ese_gates64(cpu, nat["relu_out"])
    margin = 1e9
    for key, z in z64.items():
        zk = plan.vovnet_layers[key + ".ese"].z.cpu().double()
        margin = min(margin, float((z.abs() - 3).abs().min()), float((zk.abs() - 3).abs().min()))
        assert torch.equal(zk > -3, z > -3) and torch.equal(zk < 3, z < 3), key
    assert margin > 1e-3
    for sname in ("stage2", "stage3", "stage4"):
        by, bx = VG.pool3_argmax(decode(plan.bufs[sname + ".out"]))
        ry, rx = VG.pool3_argmax(nat["bottom_up"][sname].double())
        assert int(((by != ry) | (bx != rx)).sum()) == 0, sname


def test_everything_vovnet_grads_returns_is_bit_equal_and_the_keys_are_named_parameters(run):
    r = run
    ref_losses, ref_grads, ref_params = r["ref"]
    losses, grads, params = r["losses"], r["grads"], r["params"]
    assert list(losses) == list(ref_losses) and all(torch.equal(losses[k], ref_losses[k]) for k in losses)
    assert list(grads) == list(ref_grads) and all(torch.equal(grads[k], ref_grads[k]) for k in grads) and "backbone_stem_1" in grads
    assert all(torch.equal(params[k], ref_params[k]) for k in ref_params)
    assert [k for k in params if k not in ref_params] == [W1]
    named = dict(r["cpu"].named_parameters())
    assert sorted(params) == sorted(named) and all(params[k].shape == named[k].shape and params[k].dtype == F32 for k in params)
    plan = r["plan"]
    lay = plan.vovnet_stem_layers["stem_1"]
    assert lay.guards_intact(0.0) and all(l.guards_intact(0.0) for l in plan.vovnet_layers.values())
    # backbone_stem_1 is still the gradient BEFORE stem_1's own ReLU mask: it is nonzero where the stored output is zero
    off = decode(plan.bufs["stem.0"]) <= 0
    assert bool(off.any()) and float(grads["backbone_stem_1"].cpu()[off].abs().max()) > 0.0
    assert torch.equal(params[W1], lay.dw.view(64, 3, 3, 4)[..., :3].permute(0, 3, 1, 2).contiguous())
    assert bool((lay.dw.view(64, 3, 3, 4)[..., 3] == 0).all())  # the image's fourth channel holds zeros


def test_stem_1_filter_is_the_whole_model_gradient(run):
    r = run
    stem_filters = sorted(k for k in r["params"] if k.startswith("backbone.bottom_up.stem.") and k.endswith("conv.weight"))
    assert W1 in stem_filters and len(stem_filters) == 3 and r["params"][W1].shape == (64, 3, 3, 3)
    _rows(r, [("vovnet stem", "stem_1 filter", [W1]), ("vovnet stem", "filter", stem_filters)], "kitti_v99")
    # the call itself against the layer oracle, fed what it read
    from tests import backbone_grad_oracle as BO
    plan = r["plan"]
    lay = plan.vovnet_stem_layers["stem_1"]
    x, g = lay.keep[0].permute(0, 3, 1, 2).cpu(), lay.keep[1].permute(0, 3, 1, 2).cpu()
    w, sc, y = lay.keep[2].permute(0, 3, 1, 2).cpu(), lay.scale.cpu(), decode(plan.bufs["stem.0"])
    assert torch.equal(x[:, :3], plan.bufs["img4"].nchw(0, 3).cpu()) and bool((x[:, 3] == 0).all()) and torch.equal(g, r["grads"]["backbone_stem_1"].cpu())
    got = {"dw_level": lay.dw_level.view(64, 3, 3, 4).permute(0, 3, 1, 2).cpu(), "dw": lay.dw.view(64, 3, 3, 4).permute(0, 3, 1, 2).cpu(), "q": lay.q.cpu(),
           "r": lay.r.cpu()}
    r64, r32 = (BO.layer_grads(x, y, g, w, sc, 2, dt) for dt in (F64, F32))
    a, b, k = BO.family_vectors(r64), BO.family_vectors(r32), BO.family_vectors(got)
    for fam in ("filter", "bias", "norm_weight"):
        bar, d32, gmax = GO.bar(a[fam], b[fam], torch.ones(a[fam].shape[0], dtype=torch.bool))
        dev = float((k[fam].double() - a[fam]).abs().max())
        print(f"[vovnet_stem_whole_model] kitti_v99 call stem_1 {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e}")
        assert gmax > 0.0 and dev <= bar, (fam, dev, bar, d32, gmax)


def test_bn_backbone_adds_stem_1_norm_weight_and_bias(run_bn):
    r = run_bn
    params, named = r["params"], dict(r["cpu"].named_parameters())
    assert sorted(params) == sorted(named) and NW1 in named and NB1 in named
    ref_params = r["ref"][2]
    assert sorted(k for k in params if k not in ref_params) == sorted([W1, NW1, NB1]) and all(torch.equal(params[k], ref_params[k]) for k in ref_params)
    assert len(r["report"]) == r["case"]["relus"] and sum(x[3] for x in r["report"]) == 0
    assert sum(x[2] for x in r["report"]) <= WO.SIGN_CAP * sum(v.numel() for v in r["pre64"])
    _rows(r, [("vovnet stem", "stem_1 filter", [W1]), ("vovnet stem", "stem_1 norm_weight", [NW1]), ("vovnet stem", "stem_1 norm_bias", [NB1])], "kitti_v99 BN")


def test_a_second_run_and_launch_by_launch_execution_give_the_same_bits(run):
    r = run
    model, inputs = r["model"], r["inputs"]
    same = lambda res: all(torch.equal(res[0][k], r["losses"][k]) for k in r["losses"]) and all(torch.equal(res[1][k], r["grads"][k]) for k in r["grads"]) and \
        all(torch.equal(res[2][k], r["params"][k]) for k in r["params"])
    assert same(model.compute_losses(inputs, vovnet_stem_grads=True))
    model.use_graph = False
    model.invalidate_plans()
    try:
        assert same(model.compute_losses(inputs, vovnet_stem_grads=True))
    finally:
        model.use_graph = True
        model.invalidate_plans()


def test_one_plan_on_a_second_batch_equals_a_fresh_model(run):
    """History: the plan that ran the case's batch runs a second batch on the same canvas -- other pixels, other GT -- and every result
    equals, bit for bit, a fresh model's on that batch alone: nothing the first batch left in a plan buffer is read."""
    from dd3d_amd.synthetic import make_inputs
    from tests.test_loss_grads_gpu import _model
    r = run
    case, model = r["case"], r["model"]
    inputs = make_inputs(case["B"], case["H"], case["W"], dataset=case["ds"], seed=1100)
    for x, g in zip(inputs, HC._gt(r["cpu"], inputs, 2011, 24, ())):
        x["instances"] = g
    assert not torch.equal(inputs[0]["image"], r["inputs"][0]["image"])
    model.compute_losses(r["inputs"], vovnet_stem_grads=True)  # the plan's buffers hold the case's batch
    plan = model.get_loss_plan(*model.canvas_size(inputs), vovnet_stem_grads=True)
    second = _clone(model.compute_losses(inputs, vovnet_stem_grads=True))
    assert model.get_loss_plan(*model.canvas_size(inputs), vovnet_stem_grads=True) is plan
    assert int(plan.det_count.cpu()) > 0 and not torch.equal(second[2][W1], r["params"][W1])
    fresh = _model(case["exp"], case["weights"], case["overrides"])
    alone = fresh.compute_losses(inputs, vovnet_stem_grads=True)
    for a, b in zip(second, alone):
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)
