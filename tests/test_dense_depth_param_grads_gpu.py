"""DD3DDenseDepth's backward chain on the MI355X: the predictor group's entry points at the shape the detector never gave them (n = 1 at
pitch 4, a filter per level), and param_grads / grads of DD3DDenseDepth.compute_losses(stem_grads=True) -- V2-99: vovnet_stem_grads=True
-- against ONE autograd pass of the whole model (tests/dense_depth_param_grad_oracle.py), with the tower on running and on batch
statistics; then the bits: every depth of the chain against the shallower one, graph replay against launch by launch, a second run, and
one plan replayed over differing batches against fresh models.

Nothing comes from the kernels but the signs of the plan's stored ReLU outputs (held to whole_model_grad_oracle's SIGN_NEAR / SIGN_CAP)
and the distance of the plan's up-sampled maps from the oracle's, which widens the fixture's kink margin.  The bar of a (stage, family) is
the project's, 8 * max(d32, 2^-23 * max|g64|): d32 is the float32 pass's own distance from the float64 one under the same masks
(dense_depth_grad_oracle.bar).  The measured ratios are in profiles/dense_depth_param_grads_errors.txt (tests/gpu_dense_depth_param_grad_time.py
writes the file)."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import dense_depth_grad_oracle as GO
from tests import dense_depth_param_grad_oracle as PO
from tests import predictor_grad_cases as PC
from tests import whole_model_grad_oracle as WO

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
ERRORS = os.environ.get("DD3D_DENSE_DEPTH_ERRORS_FILE")  # tests/gpu_dense_depth_param_grad_time.py sets it: the measured ratios go to profiles/
LOSS_REL = 1e-4  # the loss dict end to end from the uint8 images against the float32 oracle's own forward (tests/test_whole_model_grads_gpu.py, KITTI)
SENTINEL = -12345.0
PYRAMID = [(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)]  # the five levels of a 128 x 256 canvas at strides 8 .. 128


@pytest.fixture(autouse=True)
def _default_arithmetic(monkeypatch):
    monkeypatch.delenv("DD3D_MATH", raising=False)
    monkeypatch.delenv("DD3D_F16_ACT_SCALE", raising=False)


# ------------------------------------------------------------------------------------------------ 1. the seam at n = 1
def depth_group(B, seed):
    """The dense-depth head's predictor group as a GroupCase: one channel, a filter and a bias per level, no clamp, the channel in slot 0
    with a Scale and an Offset per level: maps = (conv + b) * s + o."""
    from tests import predictor_grad_oracle as PGO
    case = PC.GroupCase(level_hw=PYRAMID, B=B, n=1, Cin=256, seed=seed, per_level=True, clamp=False)
    gen = torch.Generator().manual_seed(seed + 100)
    case.slot = torch.zeros(1, dtype=torch.int32)
    case.scale = [0.5 + torch.rand(1, generator=gen) for _ in PYRAMID]
    case.offset = [torch.randn(1, generator=gen) for _ in PYRAMID]
    case.maps = PGO.forward(case.act, case.w, case.bias, case.scale, case.offset, case.lo)
    return case


@pytest.mark.parametrize("storage,ps", [("f16x2", 16.0), ("f32", 1.0)], ids=["f16x2", "f32"])
@pytest.mark.parametrize("B", [1, 2])
def test_predictor_group_seam_at_one_channel(hiplib, B, storage, ps):
    """dd3d_predictor_wgrad / dd3d_predictor_dgrad with n = 1, g_pitch = 4, five levels down to 1 x 2, per-level filters, Scale + Offset
    in slot 0, against the float64 autograd of (conv + b) * s + o.  Channels 1 .. 3 of the pitch are poisoned (3e30 in g and in the
    maps): every output stays finite and within the bar, so nothing reads them."""
    from tests import predictor_grad_oracle as PGO
    from tests.test_predictor_grads_gpu import check, frame_ok, run_seam
    case = depth_group(B, seed=60 + B)
    got, grp, dec = run_seam(case, storage, ps, act_pad=4 if storage == "f32" else 0)
    a = grp.args
    assert (a.n, a.g_pitch, a.num_levels) == (1, 4, 5) and grp.owners == [0, 1, 2, 3, 4] and (a.H[4], a.W[4]) == (1, 2)
    frame_ok(grp)
    ref64, ref32 = case.ref(F64, dec), case.ref(F32, dec)
    check(got, ref64, ref32, f"n1 B{B} {storage}")
    assert all(float(v.abs().max()) > 0 for v in PGO.family_vectors(ref64).values())
    # only slot 0 of dscale / doffset belongs to the group: the other slots hold exact zeros
    assert float(got["dscale"][:, 1:].abs().max()) == 0.0 and float(got["doffset"][:, 1:].abs().max()) == 0.0
    again, _, _ = run_seam(case, storage, ps, act_pad=4 if storage == "f32" else 0)
    for fam, v in PGO.family_vectors(again).items():
        assert torch.equal(v, PGO.family_vectors(got)[fam]), fam


# ------------------------------------------------------------------------------------------------ the whole model
def _gpu_model(case, cpu, use_graph=True):
    from tests.util import gpu_model
    return gpu_model(cpu.cfg, {k: v.clone() for k, v in cpu.state_dict().items()}, use_graph=use_graph)


def _flags(case):
    return dict({case["flag"]: True}, **({"batch_stats": True} if case["batch_stats"] else {}))


def _clone(res):
    return tuple({k: v.clone() for k, v in d.items()} for d in res)


def _same(a, b):
    return all(list(x) == list(y) and all(torch.equal(x[k], y[k]) for k in x) for x, y in zip(a, b))


_RUNS = {}


def _run(name):
    """One case end to end, once per session: the float64 forward, the fixture (the plan's own distance from the oracle's maps widens the
    kink margin), the call, the masks off the plan's stored tensors and the two oracle passes."""
    if name in _RUNS:
        return _RUNS[name]
    case = PO.CASES[name]
    cpu = PO.cpu_model(case)
    model = _gpu_model(case, cpu)
    inputs, s, bs = PO.case_images(case), PO.loss_settings(cpu), case["batch_stats"]
    nat = {}
    pre64 = PO.param_grads(cpu, inputs, [torch.zeros(h, w) for h, w in case["sizes"]], F64, extras=nat, backward=False, batch_stats=bs)[2]
    depths = PO.ground_truth(inputs, nat["maps"], s, case["gt_seed"])
    flags = _flags(case)
    for x, d in zip(inputs, depths):
        x["depth"] = d
    model.compute_losses(inputs, **flags)  # the forward does not read the ground truth: the plan's maps of this batch
    plan = model.get_loss_plan(len(inputs), case["H"], case["W"], **{PLAN_FLAG[k]: v for k, v in flags.items()})
    extra = max(float((a.double() - b).abs().max()) for a, b in zip(PO.plan_maps(plan, s, inputs), nat["maps"]))
    depths, removed, quad = PO.remove_kinks(depths, nat["maps"], s, case["H"], case["W"], extra)
    print(f"[dense_depth_param_grads] {name}: max|plan map - float64 map| {extra:.3e}; kink margin {PO.KINK_MARGIN + extra:.3e} removes "
          f"{100 * removed:.3f} % of the valid pixels (cap 2 %); quadratic share of the kept ones {quad}")
    assert extra <= PO.CPU_SCAN_EXTRA and removed <= PO.KINK_CAP and quad == 0.0, (extra, removed, quad)
    for x, d in zip(inputs, depths):
        x["depth"] = d
    losses, grads, params = model.compute_losses(inputs, **flags)
    assert model.get_loss_plan(len(inputs), case["H"], case["W"], **{PLAN_FLAG[k]: v for k, v in flags.items()}) is plan and plan.graph is not None
    report = []
    masks = PO.plan_masks(plan, pre64, report)
    p64, a64, _ = PO.param_grads(cpu, inputs, depths, F64, masks=masks, batch_stats=bs)
    e32 = {}
    p32, a32, _ = PO.param_grads(cpu, inputs, depths, F32, masks=masks, batch_stats=bs, extras=e32)
    _RUNS[name] = dict(case=case, cpu=cpu, model=model, inputs=inputs, plan=plan, losses=losses, grads=grads, params=params, pre64=pre64, report=report,
                       p64=p64, a64=a64, p32=p32, a32=a32, e32=e32, flags=flags)
    return _RUNS[name]


PLAN_FLAG = {"stem_grads": "stem_grads", "vovnet_stem_grads": "vovnet_stem_grads", "batch_stats": "batch_stats", "head_grads": "head_grads",
             "predictor_grads": "pred_grads", "tower_grads": "tower_grads", "fpn_grads": "fpn_grads", "backbone_grads": "backbone_grads"}


def _compare(what, rows):
    """rows: (stage, family, kernel tensors, float64 tensors, float32 tensors); one line and one verdict per row, all rows printed before
    the first assertion."""
    lines, failed, worst = [], [], 0.0
    for stage, fam, c, a, b in rows:
        c, a, b = (torch.cat([v.reshape(-1).cpu() for v in vs]) for vs in (c, a, b))
        bar, d32, gmax = GO.bar(a.double(), b, torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((c.double() - a.double()).abs().max())
        use = 8 * dev / bar if bar > 0 else 0.0
        worst = max(worst, use)
        lines.append(f"{what} {stage} {fam}: n {a.numel()} max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
        print("[dense_depth_param_grads]", lines[-1])
        if not (bool(torch.isfinite(c).all()) and gmax > 0.0 and dev <= bar):
            failed.append((stage, fam, dev, bar, d32, gmax))
    print(f"[dense_depth_param_grads] {what}: the worst family uses {worst:.2f} of the factor 8")
    if ERRORS:
        with open(ERRORS, "a") as f:
            f.write("\n".join(lines) + "\n")
    assert not failed, failed


def _whole_model(name):
    r = _run(name)
    cpu, plan, params, grads, losses = r["cpu"], r["plan"], r["params"], r["grads"], r["losses"]
    # the signs the kernels used, every ReLU call mapped to its stored tensor, and the two conditions on them
    total = sum(v.numel() for v in r["pre64"])
    bad, far = sum(x[2] for x in r["report"]), sum(x[3] for x in r["report"])
    assert len(r["report"]) == len(r["pre64"])
    print(f"[dense_depth_param_grads] {name} signs: {bad} of {total} ReLU elements differ ({bad / total:.1e}; cap 1e-4), {far} beyond 2^-16 of their "
          "tensor's maximum (cap 0)")
    assert far == 0 and bad <= WO.SIGN_CAP * total, (name, bad, far, total)
    # every entry of param_grads, by stage and family: the keys are named_parameters()
    named = dict(cpu.named_parameters())
    assert sorted(params) == sorted(named) == sorted(r["p64"]) and all(params[k].shape == named[k].shape and params[k].dtype == F32 for k in named)
    fams = {}
    for k in sorted(params):
        fams.setdefault(PO.stage_and_family(k), []).append(k)
    rows = [(st, fam, [params[k] for k in ks], [r["p64"][k] for k in ks], [r["p32"][k] for k in ks]) for (st, fam), ks in sorted(fams.items())]
    # every entry of grads, by family
    assert sorted(grads) == sorted(r["a64"]) and all(grads[k].shape == r["a64"][k].shape for k in grads)
    tf = {}
    for k in r["a64"]:
        tf.setdefault(WO.tensor_family_of(k), []).append(k)
    rows += [("tensors", fam, [grads[k] for k in ks], [r["a64"][k] for k in ks], [r["a32"][k] for k in ks]) for fam, ks in sorted(tf.items())]
    _compare(name, rows)
    assert all(lay.guards_intact(0.0) for lay in list(plan.pred_groups.values()) + list(plan.tower_layers.values()) + list(plan.fpn_layers.values()))
    # the loss dict against the float32 oracle's own forward
    assert list(losses) == [f"loss_dense_depth_lvl_{l}" for l in range(5)]
    for l, (k, v) in enumerate(losses.items()):
        ref = float(r["e32"]["losses"][l])
        print(f"[dense_depth_param_grads] {name} {k}: {float(v):.7g} oracle {ref:.7g}")
        assert abs(float(v) - ref) <= LOSS_REL * abs(ref), (k, float(v), ref)
    return r


@pytest.mark.parametrize("name", ["dla34_frozenbn_none", "dla34_frozenbn_half", "dla34_bn_none", "dla34_bn_half"])
def test_dla34_param_grads_are_the_whole_model_gradient(hiplib, name):
    """FCOS3D.NORM FrozenBN and BN (running statistics), focal scaling on, offset "none" and "half"; 2 x 128 x 256, the second image 100 x 200."""
    r = _whole_model(name)
    assert r["plan"].fused_stem and not r["plan"].tower_bn
    assert ("fcos3d_head.box3d_tower.0.norm.4.weight" in r["params"]) == ("_bn_" in name)


def test_dla34_batch_stats_param_grads_are_the_whole_model_gradient(hiplib):
    """NORM: BN with batch_stats=True: the oracle's tower norms on the batch's statistics too; tower_batch_stats() against nn.BatchNorm2d in
    train() on the convolution of the plan's stored layer input (float64; the float32 module sets the bar); the model's buffers untouched."""
    r = _whole_model("dla34_bn_batch_stats")
    cpu, plan, model = r["cpu"], r["plan"], r["model"]
    assert sorted(plan.tower_bn) == [("box3d", i) for i in range(4)] and plan.batch_stats
    assert all(lay.bn is not None and lay.bn.guards_intact(0.0) for lay in plan.tower_layers.values())
    stats = plan.tower_batch_stats()
    rows = {k: ([], [], []) for k in ("batch_mean", "batch_var", "running_mean", "running_var")}
    for i, conv in enumerate(cpu.fcos3d_head.box3d_tower):
        for l in range(5):
            x = plan.tower_info[("box3d", i)]["x"][l].nchw().float().cpu().contiguous()
            stem = f"fcos3d_head.box3d_tower.{i}.norm.{l}."
            for dtype, slot in ((F64, 1), (F32, 2)):
                bn = torch.nn.BatchNorm2d(256, eps=conv.norm[l].eps, momentum=0.1).to(dtype).train()
                bn.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in conv.norm[l].state_dict().items()}, strict=False)
                c = F.conv2d(x.to(dtype), conv.weight.detach().to(dtype), padding=1)
                with torch.no_grad():
                    bn(c)
                vals = dict(batch_mean=c.mean((0, 2, 3)), batch_var=c.var((0, 2, 3), unbiased=False), running_mean=bn.running_mean, running_var=bn.running_var)
                for k in rows:
                    rows[k][slot].append(vals[k].detach())
            for k in rows:
                rows[k][0].append(stats[stem + k])
    assert len(stats) == 4 * 5 * 4
    _compare("dla34_bn_batch_stats", [("tower statistics", k, got, r64, r32) for k, (got, r64, r32) in rows.items()])
    sd = cpu.state_dict()
    assert all(torch.equal(b.cpu(), sd[k]) for k, b in model.named_buffers())  # the model's buffers are never written
    # the plan without a backward shares one raw buffer per level among the layers: the same forward, the same loss bits
    shallow = model.compute_losses(r["inputs"], batch_stats=True)
    assert list(shallow) == list(r["losses"]) and all(torch.equal(shallow[k], r["losses"][k]) for k in shallow)
    assert [n for n in model.get_loss_plan(2, 128, 256, batch_stats=True).bufs if n.startswith("ddraw")] == [f"ddraw.{l}" for l in range(5)]
    # the running-statistics plan of the same model is another plan with other values
    base = model.compute_losses(r["inputs"], stem_grads=True)
    assert not torch.equal(base[1]["feature0"], r["grads"]["feature0"]) and set(base[2]) == set(r["params"])


def test_v99_param_grads_are_the_whole_model_gradient(hiplib):
    """V2-99 under vovnet_stem_grads on the smallest two-image canvas of tests/loss_plan_history_cases.py, 2 x 128 x 256: strides 4 .. 64."""
    r = _whole_model("v99")
    assert r["plan"].strides == [4, 8, 16, 32, 64] and "backbone_stem_1" in r["grads"]
    assert r["params"]["backbone.bottom_up.stem.stem_1/conv.weight"].shape == (64, 3, 3, 3)
    # a second run and launch-by-launch execution: the same bits
    model, inputs = r["model"], r["inputs"]
    first = (r["losses"], r["grads"], r["params"])
    assert _same(model.compute_losses(inputs, vovnet_stem_grads=True), first)
    eager = _gpu_model(r["case"], r["cpu"], use_graph=False)
    assert _same(eager.compute_losses(inputs, vovnet_stem_grads=True), first)
    assert eager.get_loss_plan(2, 128, 256, vovnet_stem_grads=True).graph is None


# ------------------------------------------------------------------------------------------------ 5. bits
LADDER = ["head_grads", "predictor_grads", "tower_grads", "fpn_grads", "backbone_grads", "stem_grads"]


def _split(res):
    if isinstance(res, dict):
        return res, {}, {}
    return (res[0], res[1], {}) if len(res) == 2 else tuple(res)


def test_every_depth_returns_the_shallower_depths_bits(hiplib):
    r = _run("dla34_frozenbn_none")
    model, inputs = r["model"], r["inputs"]
    eager = _gpu_model(r["case"], r["cpu"], use_graph=False)
    prev = _clone(_split(model.compute_losses(inputs)))
    assert list(prev[0]) == list(r["losses"])
    for flag in LADDER:
        res = _split(model.compute_losses(inputs, **{flag: True}))
        assert (len(res[2]) > 0) == (flag != "head_grads")
        for a, b in zip(prev, res):  # the loss dict and every tensor the shallower call returned
            assert all(k in b and torch.equal(a[k], b[k]) for k in a), flag
        assert len(res[1]) > len(prev[1]) and (flag == "head_grads" or len(res[2]) > len(prev[2])), flag  # each depth adds keys
        res = _clone(res)
        assert _same(_split(model.compute_losses(inputs, **{flag: True})), res), flag  # a second run
        launched = _split(eager.compute_losses(inputs, **{flag: True}))
        assert eager.get_loss_plan(2, 128, 256, **{PLAN_FLAG[flag]: True}).graph is None and _same(launched, res), flag  # launch by launch
        prev = res
    assert _same(prev, (r["losses"], r["grads"], r["params"]))
    assert len([k for k in model._plans if str(k[0]).startswith("dense_depth_loss")]) >= len(LADDER)


# ------------------------------------------------------------------------------------------------ 6. history
def _backward_outputs(plan):
    """{name: tensor} of every floating-point tensor an op of the plan writes behind the forward."""
    out = {}
    for gname in ("pred_groups", "tower_layers", "fpn_layers", "backbone_layers", "stem_layers"):
        for key, lay in getattr(plan, gname).items():
            for j, (t, _) in enumerate(lay._raw):
                out[f"{gname}.{key}.raw{j}"] = t
    out["tower_slab.part"], out["tower_slab.qpart"] = plan.tower_slab
    for l, t in enumerate(plan.d_raw):
        out[f"d_raw[{l}]"] = t[..., 0]  # (the kernel writes channel 0; the pad channels stay the zeros they were allocated as)
    out["grad_slab"], out["partials"], out["loss_out"] = plan.grad_slab, plan.partials, plan.loss_out
    assert all(t.is_floating_point() for t in out.values())
    return out


def _history_batch(case, cpu, label):
    """A: the case's batch; B: other pixels, the second image ragged at another size, other ground truth; Z: no valid depth pixel."""
    r = _run("dla34_frozenbn_none")
    if label == "A":
        return r["inputs"]
    from dd3d_amd.synthetic import make_depth_maps
    spec = dict(case, sizes=[(128, 256), (90, 180)] if label == "B" else case["sizes"])
    inputs = PO.case_images(spec, seed=1100 if label == "B" else 1200)
    depths = make_depth_maps(inputs, seed=3200) if label == "B" else [torch.zeros(h, w) for h, w in spec["sizes"]]
    if label == "Z":
        depths[0][5, 7], depths[1][40, 3] = -1.0, 200.0  # outside the valid depths
    for x, d in zip(inputs, depths):
        x["depth"] = d
    return inputs


def test_one_plan_replayed_over_differing_batches_equals_fresh_models(hiplib):
    r = _run("dla34_frozenbn_none")
    case, cpu, model = r["case"], r["cpu"], r["model"]
    plan = model.get_loss_plan(2, 128, 256, stem_grads=True)
    assert plan is r["plan"]
    want = {}
    for label in "ABZ":
        want[label] = _clone(_gpu_model(case, cpu).compute_losses(_history_batch(case, cpu, label), stem_grads=True))
    assert _same(want["A"], (r["losses"], r["grads"], r["params"])) and not torch.equal(want["B"][2]["fcos3d_head.box3d_tower.0.weight"], r["params"]["fcos3d_head.box3d_tower.0.weight"])
    # no valid pixel: NaN losses, as without the backward, and every gradient exactly zero
    assert all(bool(torch.isnan(v)) for v in want["Z"][0].values())
    assert all(float(v.abs().max()) == 0.0 for d in want["Z"][1:] for v in d.values())
    for step, label in enumerate(["A", "B", "A", "Z", "A"]):
        if step == 2:  # every backward output holds a sentinel before this run
            for t in _backward_outputs(plan).values():
                t.fill_(SENTINEL)
        got = model.compute_losses(_history_batch(case, cpu, label), stem_grads=True)
        assert model.get_loss_plan(2, 128, 256, stem_grads=True) is plan
        for a, b in zip(got, want[label]):
            assert list(a) == list(b), (step, label)
            for k in a:
                assert torch.equal(a[k], b[k]) or (label == "Z" and bool(torch.isnan(a[k]).all()) and bool(torch.isnan(b[k]).all())), (step, label, k)
        assert not any(bool((v == SENTINEL).any()) for d in got for v in d.values()), (step, label)
