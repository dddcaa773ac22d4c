"""Batch-statistics BN in the FPN, the parts that need no GPU: the oracle (tests/fpn_bn_oracle.py) against torch.nn.BatchNorm2d in
train() inserted by hand and its chain statement against autograd through its forward; the op list, buffers, read-out keys and cache
keys of the dry-run plans under fpn_batch_stats; the unchanged plan without the flag; every refusal; the ctypes layout of
dd3d_fpn_bn_args against the header."""
import ctypes as C
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import fpn_bn_oracle as NO
from tests import fpn_grad_cases as FC
from tests import fpn_grad_oracle as FO
from tests import loss_grad_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FPN_BN = {"FE": {"FPN": {"NORM": "BN"}}}


# ---------------------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("top", ["p6p7", "p6"])
def test_oracle_forward_is_batchnorm2d_in_train_mode(top):
    """fpn_bn_oracle.forward and its norm-by-norm statement against the FPN written out by hand with torch.nn.BatchNorm2d modules in
    train(): float64, 1e-12 of each output's largest entry; the modules' running statistics after that one step are the read-out's."""
    model = FC.MiniModel(norm="BN", top=top)
    feats, _, sd = FC.mini_inputs(model, 2, (12, 20), dtype=torch.float64)
    sp = FO.spec(model)
    out = NO.forward(sd, feats, sp)
    stored = NO.stored_activations(sd, feats, sp)
    fpn, prev, by_hand, norms = model.backbone, None, {}, {}
    for s, n in reversed(list(zip(fpn.stages, fpn.in_features))):
        for kind in ("fpn_lateral", "fpn_output"):
            bn = torch.nn.BatchNorm2d(64, eps=1e-5).double().train()
            bn.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in getattr(fpn, f"{kind}{s}").norm.state_dict().items()}, strict=False)
            norms[f"{kind}{s}"] = bn
        with torch.no_grad():
            lat = norms[f"fpn_lateral{s}"](F.conv2d(feats[n], sd[f"backbone.fpn_lateral{s}.weight"]))
            if prev is not None:
                lat = lat + F.interpolate(prev, scale_factor=2.0, mode="nearest")
            prev = lat
            by_hand[f"p{s}"] = norms[f"fpn_output{s}"](F.conv2d(lat, sd[f"backbone.fpn_output{s}.weight"], padding=1))
    for k, ref in by_hand.items():
        assert float((out[k] - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), k
        assert float((stored["p"][int(k[1:])] - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), k
    eval_out = FO.forward(sd, feats, sp)  # the running-statistics forward is another function
    assert float((eval_out["p3"] - out["p3"]).abs().max()) > 1e-2 * float(out["p3"].abs().max())
    s5 = fpn.stages[-1]
    assert float((out[f"p{s5 + 1}"] - stored["p"][s5 + 1]).abs().max()) <= 1e-12 * float(out[f"p{s5 + 1}"].abs().max())
    want = NO.expected_stats(model, stored, feats, torch.float64)
    assert sorted(want) == NO.batch_stats_names(model)
    for name, bn in norms.items():
        assert float((want[f"backbone.{name}.norm.running_mean"] - bn.running_mean).abs().max()) <= 1e-12
        assert float((want[f"backbone.{name}.norm.running_var"] - bn.running_var).abs().max()) <= 1e-12
        mu, v = stored["stats"][f"backbone.{name}.norm"]
        assert torch.equal(mu, want[f"backbone.{name}.norm.batch_mean"]) and torch.equal(v, want[f"backbone.{name}.norm.batch_var"])


@pytest.mark.parametrize("top", ["p6p7", "p6"])
def test_chain_oracle_is_autograd_through_the_forward(top):
    """chain_grads at the forward's own activations against autograd through the whole FPN forward: float64, 1e-10 of each gradient."""
    model = FC.MiniModel(norm="BN", top=top)
    feats, G, sd = FC.mini_inputs(model, 2, (12, 20), dtype=torch.float64)
    sp = FO.spec(model)
    stored = NO.stored_activations(sd, feats, sp)
    params, fg = NO.chain_grads(model, stored, feats, G, torch.float64)
    assert sorted(params) == FO.fpn_param_names(model)
    ref_p, ref_f = NO.autograd_grads(sd, feats, sp, G, torch.float64, sorted(params))
    for got, ref in ((params, ref_p), (fg, ref_f)):
        for k in ref:
            assert float((got[k] - ref[k]).abs().max()) <= 1e-10 * float(ref[k].abs().max()), k
    assert {NO.family_of(k) for k in params} == {"weight", "norm_weight", "norm_bias", "bias"}
    # the running-statistics chain differs by far more
    other = FO.chain_grads(model, FO.stored_activations(sd, feats, sp), feats, G, torch.float64)[1]
    assert float((other["backbone_c3"] - fg["backbone_c3"]).abs().max()) > 1e-2 * float(fg["backbone_c3"].abs().max())


# ---------------------------------------------------------------------------------------------------------------------- dry plans
def _plan(model, B=2, H=64, W=128, **kw):
    from dd3d_amd.engine.losses import LossPlan
    return LossPlan(model, B, H, W, device="cpu", dry_run=True, **kw)


def _trunk_ops(plan):
    return [op.name for op in plan.ops if op.name.startswith(("fpn_", "top_block."))]


def _table(plan):
    return [op.name for op in plan.ops], {k: (b.B, b.H, b.W, b.pitch, b.has_f32, b.np) for k, b in plan.bufs.items()}


@pytest.mark.parametrize("exp,stages", [("dd3d_kitti_dla34", (3, 4, 5)), ("dd3d_kitti_v99", (2, 3, 4, 5))])
def test_dry_plans_under_the_flag(hiplib, exp, stages):
    from dd3d_amd import hip
    model = GC.cpu_model(exp, FPN_BN)
    before = _table(_plan(model, fpn_grads=True))  # built before any flagged plan
    plain, grads = _plan(model, fpn_batch_stats=True), _plan(model, fpn_grads=True, fpn_batch_stats=True)
    top = ["top_block.p6", "top_block.p7"] if exp == "dd3d_kitti_dla34" else ["top_block.p6"]
    forward_ops = [f"fpn_lateral{s}.raw" for s in reversed(stages)] + ["fpn_laterals.bn_stats", "fpn_laterals.bn_apply", "fpn_outputs.raw", "fpn_outputs.bn_stats",
                                                                       "fpn_outputs.bn_apply"] + top
    assert _trunk_ops(plain) == forward_ops
    back = [f"fpn_grads.{t}" for t in reversed(top)] + ["fpn_bn_grads.outputs", "fpn_grads.outputs", "fpn_bn_grads.laterals"] + [f"fpn_grads.lateral{s}"
                                                                                                                                   for s in reversed(stages)]
    assert _trunk_ops(grads) == forward_ops + back
    names = [op.name for op in grads.ops]
    assert "fpn_outputs" not in names and not any(n in names for n in [f"fpn_lateral{s}" for s in stages])
    ops = {op.name: op for op in grads.ops}
    n = len(stages)
    for s in stages:  # the lateral raws: f32 only, scale ones, bias zeros, no ReLU, no residual
        raw = ops[f"fpn_lateral{s}.raw"]
        assert not raw.desc["relu"] and raw.out_forms == [(True, False)] and raw.res_forms == [None]
        sg = raw.desc["segs"][0]
        assert sg["out"].buf.name == f"fpn_lateral{s}.raw" and bool((sg["scale"] == 1).all()) and not bool(sg["bias"].any())
    raw = ops["fpn_outputs.raw"]
    assert raw.info["nsegs"] == n and raw.out_forms == [(True, False)] * n and not raw.desc["relu"] and raw.res_forms == [None] * n
    assert [sg["in"].buf.name for sg in raw.desc["segs"]] == [f"fpn_lateral{s}" for s in reversed(stages)]
    assert [sg["out"].buf.name for sg in raw.desc["segs"]] == [f"fpn_output{s}.raw" for s in reversed(stages)]
    lat, out = grads.fpn_bn["laterals"]["args"], grads.fpn_bn["outputs"]["args"]
    assert [lat.up[i] for i in range(n)] == list(range(1, n)) + [-1] and [out.up[i] for i in range(n)] == [-1] * n
    for f, kind in ((lat, "fpn_lateral"), (out, "fpn_output")):
        a = f.bn
        assert a.num_segs == n and a.C == 256 and a.c_pitch == 256 and a.math_mode == hip.MATH_F16X2 and a.plane_scale == 16.0 and abs(a.eps - 1e-5) < 1e-12
        assert [a.N[i] for i in range(n)] == [f.B[i] * f.H[i] * f.W[i] for i in range(n)] == [2 * (64 >> s) * (128 >> s) for s in stages]
        assert a.n_slices >= hip.bn_slices([a.N[i] for i in range(n)]) and a.status == grads.status.data_ptr()
    assert [d["out"].buf.name for d in ops["fpn_laterals.bn_apply"].desc["segs"]] == [f"fpn_lateral{s}" for s in stages]
    assert [d["out"].buf.name for d in ops["fpn_outputs.bn_apply"].desc["segs"]] == [f"p{s}" for s in stages]
    assert all(op.branch == 0 for op in grads.ops if op.name.startswith(("fpn_l", "fpn_o", "fpn_bn", "fpn_grads")))
    # memory: both raws of every stage with the backward (pinned by the reads check), one per stage without
    raws = sorted([f"fpn_lateral{s}.raw" for s in stages] + [f"fpn_output{s}.raw" for s in stages])
    assert sorted(k for k in grads.bufs if "raw" in k and k.startswith("fpn")) == raws and sorted(grads.fpn_bn_reads) == raws
    assert sorted(k for k in plain.bufs if "raw" in k and k.startswith("fpn")) == [f"fpn_raw{s}" for s in stages]
    assert all(b.has_f32 and not b.np and b.pitch == 256 for k, b in list(grads.bufs.items()) + list(plain.bufs.items()) if "raw" in k and k.startswith("fpn"))
    assert all(grads.bufs[f"fpn_lateral{s}"].np and not grads.bufs[f"fpn_lateral{s}"].has_f32 for s in stages)
    assert "fpn_laterals.bn_apply" not in grads.amax_names and "fpn_lateral3.raw" not in grads.amax_names  # not watched by the range guard
    # the backward: the norms' calls feed the convolution calls their G_c; scale ones; the t<s> the outputs read are the apply's
    L = grads.fpn_layers
    bo, bl = grads.fpn_bn_layers["outputs"], grads.fpn_bn_layers["laterals"]
    assert [L["outputs"].args.g[i] for i in range(n)] == [g.data_ptr() for g in bo.gc] and L["outputs"].bn is bo
    assert [bl.args.g[i] for i in range(n)] == [d.data_ptr() for d in L["outputs"].da]
    assert all(L[f"lateral{s}"].args.g[0] == bl.gc[i].data_ptr() and L[f"lateral{s}"].bn is bl and L[f"lateral{s}"].bn_index == [i] for i, s in enumerate(stages))
    assert all(bool((sc == 1).all()) for key in ["outputs"] + [f"lateral{s}" for s in stages] for sc in L[key].keep[2])
    assert all(getattr(L[t], "bn", None) is None for t in top)
    assert bo.args.part == bl.args.part == lat.bn.part == out.bn.part and bo.args.part != grads.tower_slab[0].data_ptr()
    assert all(lay.part is grads.tower_slab[0] for lay in L.values())  # the convolution calls share the one slab as before
    # keys: param_grads and grads as without the flag; the statistics under the norms' state-dict names
    base = _plan(model, fpn_grads=True)
    assert sorted(grads.fpn_grads()[1]) == sorted(base.fpn_grads()[1]) == FO.fpn_param_names(model)
    assert sorted(grads.fpn_grads()[0]) == sorted(base.fpn_grads()[0])
    stats = grads.fpn_batch_stats()
    assert sorted(stats) == NO.batch_stats_names(model) and len(stats) == 8 * n and all(v.shape == (256, ) and v.dtype == torch.float32 for v in stats.values())
    assert sorted(k for k in stats if "running" in k) == sorted(k for k, _ in model.named_buffers() if k.startswith("backbone.fpn_") and "running" in k)
    with pytest.raises(RuntimeError, match="fpn_batch_stats=True"):
        base.fpn_batch_stats()
    # the plan without the flag: the ops and buffers it had before any flagged plan was built
    assert _table(base) == before and not hasattr(base, "fpn_bn") and base.with_fpn_batch_stats is False
    assert "fpn_outputs" in before[0] and all(f"fpn_lateral{s}" in before[0] for s in stages) and not any("raw" in k for k in before[1])


def test_flag_composes_with_tower_batch_stats_and_deeper_flags(hiplib):
    model = GC.cpu_model("dd3d_kitti_dla34", FPN_BN)
    both = _plan(model, batch_stats=True, fpn_batch_stats=True, stem_grads=True)
    names = [op.name for op in both.ops]
    assert "towers.0.bn_stats" in names and "fpn_laterals.bn_apply" in names and "tower_bn_grads.cls.0" in names and "fpn_bn_grads.laterals" in names
    assert names.index("fpn_grads.lateral3") < min(i for i, n in enumerate(names) if n.startswith("backbone_grads."))  # the deeper stages follow
    assert len(both.tower_bn) == 8 and both.fpn_bn_part is not both.bn_part
    # keys of every read-out together: those of named_parameters()
    params = {}
    for read in (both.predictor_grads, both.tower_grads, both.fpn_grads, both.backbone_grads, both.stem_grads):
        params.update(read()[1])
    assert sorted(params) == sorted(k for k, _ in model.named_parameters())
    v99 = GC.cpu_model("dd3d_kitti_v99", FPN_BN)
    deep = _plan(v99, B=1, H=128, W=256, fpn_batch_stats=True, vovnet_stem_grads=True)
    assert [deep.fpn_bn["laterals"]["args"].up[i] for i in range(4)] == [1, 2, 3, -1]


def test_dense_depth_plan_takes_the_flag(hiplib):
    from dd3d_amd.engine import DenseDepthLossPlan
    from tests.test_dense_depth_param_grads import _dla
    model = _dla(FE=FPN_BN["FE"])
    plan = DenseDepthLossPlan(model, 2, 128, 256, device="cpu", dry_run=True, fpn_grads=True, fpn_batch_stats=True)
    names = [op.name for op in plan.ops]
    assert "fpn_laterals.bn_apply" in names and "fpn_bn_grads.outputs" in names and "fpn_outputs" not in names
    assert sorted(plan.fpn_batch_stats()) == NO.batch_stats_names(model)
    with pytest.raises(NotImplementedError, match="FE.FPN.NORM"):
        DenseDepthLossPlan(model, 2, 128, 256, device="cpu", dry_run=True, batch_stats=True)


def test_cache_keys_are_distinct(hiplib, monkeypatch):
    """get_loss_plan: one cache key more per flag set; the unflagged key is the one from before the flag existed."""
    import dd3d_amd.engine.losses as EL
    from dd3d_amd.modeling.dd3d import DD3D
    model = GC.cpu_model("dd3d_kitti_dla34", FPN_BN)
    made = []

    class Fake:
        def __init__(self, model, B, Hp, Wp, **kw):
            made.append(kw)

        def capture(self):
            pass

    monkeypatch.setattr(EL, "LossPlan", Fake)
    model.use_graph = False
    a = DD3D.get_loss_plan(model, 2, 128, 128, fpn_grads=True)
    b = DD3D.get_loss_plan(model, 2, 128, 128, fpn_grads=True, fpn_batch_stats=True)
    c = DD3D.get_loss_plan(model, 2, 128, 128, fpn_grads=True, fpn_batch_stats=True, batch_stats=True)
    d = DD3D.get_loss_plan(model, 2, 128, 128, fpn_grads=True, batch_stats=True)
    assert len({id(x) for x in (a, b, c, d)}) == 4 and DD3D.get_loss_plan(model, 2, 128, 128, fpn_grads=True, fpn_batch_stats=True) is b
    keys = [k for k in model._plans if k[0] == "losses"]
    assert len(keys) == 4 and sum("fpn_batch_stats" in k for k in keys) == 2 and sum("batch_stats" in k for k in keys) == 2
    plain = next(k for k in keys if "fpn_batch_stats" not in k and "batch_stats" not in k)
    assert plain == ("losses", 2, 128, 128, model.math, model.act_scale, getattr(model, "tile_policy", None), "fpn_grads")
    assert made == [dict(fpn_grads=True), dict(fpn_grads=True, fpn_batch_stats=True), dict(fpn_grads=True, batch_stats=True, fpn_batch_stats=True),
                    dict(fpn_grads=True, batch_stats=True)]


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(hiplib, monkeypatch):
    import inspect
    from dd3d_amd.engine import DenseDepthLossPlan
    from dd3d_amd.engine.losses import LossPlan
    from dd3d_amd.modeling.dd3d import DD3D
    built = []
    orig = LossPlan._trunk
    monkeypatch.setattr(LossPlan, "_trunk", lambda self, *a, **k: (built.append(1), orig(self, *a, **k))[1])
    model = GC.cpu_model("dd3d_kitti_dla34", FPN_BN)
    # batch_stats alone keeps its refusal, in its words
    with pytest.raises(NotImplementedError, match="batch_stats covers the head towers; FE.FPN.NORM = 'BN'"):
        _plan(model, batch_stats=True)
    for over, err, match in (({"FE": {"FPN": {"NORM": "FrozenBN"}}}, ValueError, "FE.FPN.NORM"), ({"FE": {"FPN": {"NORM": ""}}}, ValueError, "FE.FPN.NORM"),
                             (None, ValueError, "FE.FPN.NORM"), (WOBN, NotImplementedError, "FE.BACKBONE.NORM"),
                             (dict(FE=dict(FPN=dict(NORM="BN", FUSE_TYPE="avg"))), NotImplementedError, "FUSE_TYPE"),
                             (dict(FE=dict(FPN=dict(NORM="BN", OUT_CHANNELS=288))), NotImplementedError, "OUT_CHANNELS"),
                             (dict(FE=dict(FPN=dict(NORM="BN", OUT_CHANNELS=48))), NotImplementedError, "OUT_CHANNELS")):
        bad = GC.cpu_model("dd3d_kitti_dla34", over)
        for kw in (dict(), dict(batch_stats=True), dict(fpn_grads=True)):
            with pytest.raises(err, match=match):
                _plan(bad, fpn_batch_stats=True, **kw)
    # one value per channel: P5 of one 16 x 16 image is 1 x 1 -- in torch's words; two such images pass this check
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        _plan(model, B=1, H=32, W=32, fpn_batch_stats=True)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        _plan(model, B=1, H=64, W=128, batch_stats=True, fpn_batch_stats=True)  # (the towers' P7)
    # the lowerings without the fused split-plane FPN, and the reduced modes
    for math, env, match in (("f32", {}, "DD3D_MATH=f32"), ("bf16x3", {"DD3D_PLANES": "0"}, "DD3D_PLANES=0"), (None, {"DD3D_PLANES_ONLY": "0"}, "DD3D_PLANES_ONLY=0"),
                             ("bf16x2", {}, "bf16x2"), ("bf16", {}, "bf16")):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            model.math = math
            with pytest.raises(NotImplementedError, match=match):
                _plan(model, fpn_batch_stats=True)
            if math not in ("bf16x2", "bf16"):
                _plan(model)  # (the unflagged plan still builds there)
    model.math = None
    assert built == [1, 1, 1]  # every refusal came before anything was built: only the three unflagged plans reached the trunk
    for math in ("bf16x3", None):
        model.math = math
        assert _trunk_ops(_plan(model, fpn_batch_stats=True))[3:5] == ["fpn_laterals.bn_stats", "fpn_laterals.bn_apply"]
    model.math = None
    for fn in (DD3D.compute_losses, DD3D.get_loss_plan, LossPlan.__init__, DenseDepthLossPlan.__init__):
        assert inspect.signature(fn).parameters["fpn_batch_stats"].default is False
    with pytest.raises(TypeError, match="unexpected keyword argument 'fpn_batchstats'"):
        DD3D.compute_losses(model, [], fpn_batchstats=True)


WOBN = {"FE": {"BACKBONE": {"NORM": "BN"}, "FPN": {"NORM": "BN"}}}


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_fpn_bn_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    cls, cname = hip.FpnBnArgs, "dd3d_fpn_bn_args"
    assert [f[0] for f in cls._fields_] == ["bn", "y32", "up", "B", "H", "W", "y32_pitch", "reserved"] and cls._fields_[0][1] is hip.TowerBnArgs
    out = (C.c_int64 * 32)()
    n = hiplib.dd3d_fpn_bn_layout(out, 32)
    assert n == len(cls._fields_) + 1 and out[n] == -1 and out[0] == C.sizeof(cls)
    assert [out[1 + j] for j in range(len(cls._fields_))] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert hiplib.dd3d_fpn_bn_layout(out, 8) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_fpn_bn_layout")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {', f'  printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));' for f in cls._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(cls) and C.sizeof(cls) <= 4096  # (travels to the kernel by value)
    for f in cls._fields_:
        assert int(got[f"{cname}.{f[0]}"]) == getattr(cls, f[0]).offset, f[0]
    assert all(e in hip.EXPORTS for e in ("dd3d_bn_apply_topdown_split", "dd3d_bn_backward_reduce_linear", "dd3d_bn_backward_apply_linear", "dd3d_fpn_bn_layout"))
    assert all(hasattr(hiplib, e) for e in hip.EXPORTS)
    assert hip.ABI_VERSION == 7 and hiplib.dd3d_abi_version() == 7
    # host-side rejections need no device: null arguments, a bad link, a size that is no exact halving
    st = None
    f = cls()
    assert hiplib.dd3d_bn_apply_topdown_split(None, st) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_bn_apply_topdown_split")
    assert hiplib.dd3d_bn_apply_topdown_split(C.byref(f), st) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_bn_apply_topdown_split")
    for fn, name in ((hiplib.dd3d_bn_backward_reduce_linear, "dd3d_bn_backward_reduce_linear"), (hiplib.dd3d_bn_backward_apply_linear, "dd3d_bn_backward_apply_linear")):
        assert fn(None, st) == -1 and hiplib.dd3d_last_error().decode().startswith(name)
        assert fn(C.byref(f.bn), st) == -1 and hiplib.dd3d_last_error().decode().startswith(name)
    keep = [(C.c_float * 4)() for _ in range(8)]  # dummy non-null addresses: every case below is refused before any launch
    a = f.bn
    a.num_segs, a.C, a.c_pitch, a.math_mode, a.plane_scale = 2, 32, 32, hip.MATH_F16X2, 16.0
    for s, (h, w) in enumerate(((4, 6), (2, 3))):
        a.c[s], a.stats[s], a.y[s], a.beta[s] = (C.addressof(k) for k in keep[4 * s:4 * s + 4])
        a.N[s], f.B[s], f.H[s], f.W[s], f.up[s] = h * w, 1, h, w, (1 if s == 0 else -1)
    for arr, idx, bad, what in ((f.H, 1, 3, "N ="), (f.up, 0, 2, "links to"), (f.up, 1, 0, "links to")):
        old = arr[idx]
        arr[idx] = bad
        assert hiplib.dd3d_bn_apply_topdown_split(C.byref(f), st) == -1
        err = hiplib.dd3d_last_error().decode()
        assert err.startswith("dd3d_bn_apply_topdown_split") and what in err, err
        arr[idx] = old
    f.H[1], f.W[1], a.N[1] = 3, 2, 6  # consistent with N, but no exact halving of (4, 6)
    assert hiplib.dd3d_bn_apply_topdown_split(C.byref(f), st) == -1 and "is not twice its coarser segment" in hiplib.dd3d_last_error().decode()
