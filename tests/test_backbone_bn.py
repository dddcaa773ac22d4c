"""Batch-statistics BN in the DLA-34 bottom-up network, the parts that need no GPU: the oracle (tests/backbone_bn_oracle.py) against the
bottom-up network written out by hand over dd3d_amd.modeling.dla's own module tree with torch.nn.BatchNorm2d modules in train(), forward,
running statistics and gradients; the op list, buffers, bindings, read-out keys and cache keys of the dry-run plans under
backbone_batch_stats; the unchanged plan without the flag; every refusal; the ctypes layout of dd3d_backbone_bn_args against the header."""
import ctypes as C
import inspect
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import backbone_bn_oracle as BN
from tests import loss_grad_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BB_BN = {"FE": {"BACKBONE": {"NORM": "BN"}}}
EVERYWHERE = {"FE": {"BACKBONE": {"NORM": "BN"}, "FPN": {"NORM": "BN"}}}


def _model(overrides=BB_BN, seed=3):
    """A CPU model whose bottom-up norms carry non-trivial weights, biases and running statistics."""
    model = GC.cpu_model("dd3d_kitti_dla34", overrides)
    g = torch.Generator().manual_seed(seed)
    sd = model.state_dict()
    for p in BN.norm_prefixes(model):
        n = sd[p + ".weight"].numel()
        sd[p + ".weight"] = 0.5 + torch.rand(n, generator=g)
        sd[p + ".bias"] = 0.2 * torch.randn(n, generator=g)
        sd[p + ".running_mean"] = 0.1 * torch.randn(n, generator=g)
        sd[p + ".running_var"] = 0.5 + torch.rand(n, generator=g)
    model.load_state_dict(sd)
    return model


# ---------------------------------------------------------------------------------------------------------------------- the oracle
_ByHand = BN.ModuleWalk


def _image(B=2, H=64, W=64, seed=11):
    return torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def test_oracle_forward_and_running_statistics_are_batchnorm2d_in_train_mode():
    """The oracle's forward on a 2 x 3 x 64 x 64 input against the hand-written module walk with nn.BatchNorm2d in train(): float64, 1e-12 of
    each output's largest entry; the modules' running statistics after that one step are expected_stats', the batch's own its stats."""
    model = _model()
    img = _image()
    before = {k: v.clone() for k, v in model.state_dict().items()}
    sd = BN.state(model, torch.float64)
    out = BN.forward(sd, img, out_features=("level2", "level3", "level4", "level5"))
    stored = BN.stored_activations(sd, img)
    hand = _ByHand(model.backbone.bottom_up)
    with torch.no_grad():
        ref = hand(img)
    for k, v in ref.items():
        assert float((out[k] - v).abs().max()) <= 1e-12 * float(v.abs().max()), k
    assert len(stored["relu_out"]) == len(hand.relus) == 3 + 5 * 6 and len(stored["raw"]) == len(hand.norms) == 37
    for a, b in zip(stored["relu_out"], hand.relus):  # the same call order: what the masks of chain_grads index
        assert a.shape == b.shape and float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    from oracle import dd3d_oracle as O
    with torch.no_grad():  # (the running-statistics forward is another function: it differs by far more)
        other = O.dla34_forward(sd, img)
    assert float((other["level5"] - out["level5"]).abs().max()) > 1e-2 * float(out["level5"].abs().max())
    want = BN.expected_stats(model, stored, torch.float64)
    assert sorted(want) == BN.batch_stats_names(model) and len(want) == 4 * 37
    mods = {id(m): n for n, m in model.named_modules()}
    for mid, bn in hand.norms.items():
        p = mods[mid] + ".norm"
        assert float((want[p + ".running_mean"] - bn.running_mean).abs().max()) <= 1e-12
        assert float((want[p + ".running_var"] - bn.running_var).abs().max()) <= 1e-12 * float(bn.running_var.abs().max())
        mu, v = stored["stats"][p]
        assert torch.equal(mu, want[p + ".batch_mean"]) and torch.equal(v, want[p + ".batch_var"])
    # nothing of the model was written
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_chain_oracle_is_autograd_through_the_module_walk():
    """chain_grads (natural signs, and the same signs handed over as masks) against autograd through the hand-written walk: float64,
    1e-9 of each gradient's largest entry."""
    model = _model()
    img = _image(H=64, W=64, seed=12)
    gen = torch.Generator().manual_seed(5)
    hand = _ByHand(model.backbone.bottom_up)
    ref_out = hand(img)
    G = {k: torch.randn(ref_out[k].shape, generator=gen, dtype=torch.float64) for k in ("level3", "level4", "level5")}
    for y in hand.relus[:3]:
        y.retain_grad()
    sum((ref_out[k] * G[k]).sum() for k in G).backward()
    mods = {id(m): n for n, m in model.named_modules()}
    ref = {}
    for mid, w in hand.leaves.items():
        ref[mods[mid] + ".weight"] = w.grad
        ref[mods[mid] + ".norm.weight"], ref[mods[mid] + ".norm.bias"] = hand.norms[mid].weight.grad, hand.norms[mid].bias.grad
    sd = BN.state(model, torch.float64)
    masks = [v > 0 for v in BN.stored_activations(sd, img)["relu_pre"]]
    for m in (None, masks):
        params, at = BN.chain_grads(model, m, img, G, torch.float64)
        assert sorted(params) == sorted(ref) == sorted(k for k, _ in model.named_parameters() if k.startswith(BN.PREFIX + "."))
        for k in ref:
            assert float((params[k] - ref[k]).abs().max()) <= 1e-9 * float(ref[k].abs().max()), k
        for k, y in zip(("backbone_base_layer", "backbone_level0", "backbone_level1"), hand.relus[:3]):
            assert float((at[k] - y.grad).abs().max()) <= 1e-9 * float(y.grad.abs().max()), k
    assert {BN.family_of(k) for k in ref} == {"weight", "norm_weight", "norm_bias"}


def test_closed_forms_are_autograd():
    """apply_closed / backward_closed (what the seam test holds the kernels to) against autograd through F.batch_norm(training=True)."""
    g = torch.Generator().manual_seed(9)
    N, Cc = 30, 16
    c, r, G = (torch.randn(N, Cc, generator=g, dtype=torch.float64) for _ in range(3))
    gamma, beta = 0.5 + torch.rand(Cc, generator=g, dtype=torch.float64), torch.randn(Cc, generator=g, dtype=torch.float64)
    for act in (BN.RELU, BN.LINEAR, BN.RESIDUAL):
        cl, ga, be = c.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        n = F.batch_norm(cl.t().reshape(1, Cc, N, 1), None, None, ga, be, training=True, eps=BN.EPS).reshape(Cc, N).t()
        y = n if act == BN.LINEAR else (n + r if act == BN.RESIDUAL else n).clamp(min=0)
        got, _, _ = BN.apply_closed(c, gamma, beta, act, r)
        assert float((got - y.detach()).abs().max()) <= 1e-12
        (y * G).sum().backward()
        q, p, gc = BN.backward_closed(c, None if act == BN.LINEAR else y.detach() > 0, G, gamma)
        for a, b in ((q, be.grad), (p, ga.grad), (gc, cl.grad)):
            assert float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))


# ---------------------------------------------------------------------------------------------------------------------- dry plans
def _plan(model, B=2, H=64, W=128, **kw):
    from dd3d_amd.engine.losses import LossPlan
    return LossPlan(model, B, H, W, device="cpu", dry_run=True, **kw)


def _table(plan):
    return [op.name for op in plan.ops], {k: (b.B, b.H, b.W, b.pitch, b.has_f32, b.np) for k, b in plan.bufs.items()}


def _layer_keys(dla):
    keys = ["base_layer", "level0.0", "level1.0"]
    for name, m in dla.named_modules():
        if name.split(".")[0] in ("level2", "level3", "level4", "level5") and hasattr(m, "norm") and hasattr(m, "weight"):
            keys.append(name[:-len(".conv")] if name.endswith(".root.conv") else name)
    return keys


def test_dry_plans_under_the_flag(hiplib, monkeypatch):
    from dd3d_amd import hip
    model = GC.cpu_model("dd3d_kitti_dla34", BB_BN)
    dla = model.backbone.bottom_up
    before = _table(_plan(model, stem_grads=True))  # built before any flagged plan
    plain, grads = _plan(model, backbone_batch_stats=True), _plan(model, stem_grads=True, backbone_batch_stats=True)
    keys = _layer_keys(dla)
    assert len(keys) == 37 and sorted(grads.backbone_bn) == sorted(keys) == sorted(plain.backbone_bn)
    names = [op.name for op in grads.ops]
    assert "stem" not in names and not grads.fused_stem and "stem" in before[0]  # the launch-by-launch stem under the flag, the fused one without
    ops = {op.name: op for op in grads.ops}
    for k in keys:  # raw convolution (f32 only, scale ones, bias zeros, no ReLU, no residual), statistics, apply -- in that order
        i = names.index(k + ".raw")
        assert names[i + 1:i + 3] == [k + ".bn_stats", k + ".bn_apply"] and k not in names
        rec, f = grads.backbone_bn[k], grads.backbone_bn[k]["args"]
        raw = grads.bufs[k + ".raw"]
        assert raw.has_f32 and not raw.np and raw.pitch == rec["conv"].out_channels and rec["raw"].buf is raw
        a = f.bn
        assert a.num_segs == 1 and a.C == raw.pitch == a.c_pitch and a.N[0] == raw.B * raw.H * raw.W and abs(a.eps - 1e-5) < 1e-12
        assert a.n_slices >= hip.bn_slices([a.N[0]]) and a.status == grads.status.data_ptr() and a.part == grads.backbone_bn_part.data_ptr()
        want = hip.BBN_LINEAR if k.endswith(".project") else hip.BBN_RESIDUAL if k.endswith(".conv2") else hip.BBN_RELU
        assert f.act == rec["act"] == want
        out = rec["out"]
        assert a.math_mode == (hip.MATH_F16X2 if out.np else hip.MATH_F32)
        if hasattr(ops[k + ".raw"], "desc") and "segs" in ops[k + ".raw"].desc:
            sg = ops[k + ".raw"].desc["segs"][0]
            assert not ops[k + ".raw"].desc["relu"] and bool((sg["scale"] == 1).all()) and not bool(sg["bias"].any()) and sg.get("res") is None
        assert k + ".raw" not in grads.amax_names and k + ".bn_apply" not in grads.amax_names
    # outputs land where the running-statistics lowering puts them: the same buffers, storages and channel slices
    flagged_bufs = {k: v for k, v in _table(grads)[1].items() if not k.endswith(".raw")}
    with monkeypatch.context() as mp:  # (the launch-by-launch stem is what the flagged plan takes)
        mp.setenv("DD3D_FUSED_STEM", "0")
        unfused = _table(_plan(model, stem_grads=True))[1]
    assert flagged_bufs == unfused
    l3 = grads.backbone_bn
    assert (l3["level3.tree1.tree2.conv2"]["out"].buf.name, l3["level3.tree1.tree2.conv2"]["out"].c0) == ("level3.tree1.cat", 0)
    assert (l3["level3.tree1.tree1.conv2"]["out"].buf.name, l3["level3.tree1.tree1.conv2"]["out"].c0) == ("level3.tree1.cat", 128)
    assert l3["level3.tree1.root"]["out"].buf.name == "level3.cat" and l3["level3.tree1.root"]["out"].c0 == 2 * 128 + 64
    assert l3["level2.tree1.conv2"]["args"].res_mode == hip.PG_ACT_F16X2 and l3["level2.tree1.conv2"]["args"].res_plane_scale == 16.0
    # the backward: a norm call in front of every convolution call, which reads its G_c unmasked with scale ones
    for k in keys:
        stage = "stem" if k in ("base_layer", "level0.0", "level1.0") else "backbone"
        i = names.index(f"{stage}_bn_grads.{k}")
        assert names[i + 1] == f"{stage}_grads.{k}"
        lay = (grads.stem_layers if stage == "stem" else grads.backbone_layers)[k]
        assert lay.bn is not None and lay.args.g == lay.bn.gc[0].data_ptr() and bool((lay.scale == 1).all()) and lay.bn.args.C == lay.Cout
        assert lay.bn.args.c[0] == grads.backbone_bn[k]["raw"].ptr and lay.bn.args.part == grads.backbone_bn_part.data_ptr() and lay.bn.masked
        if stage == "backbone":
            assert not lay.masked and lay.args.y is None
        else:
            assert lay.args.y == grads.stem_ones.data_ptr() and lay.args.y_mode == hip.PG_ACT_F32
    # a project's norm backward masks by the block's stored output x1 (the residual's share crossed that ReLU), not by its own output
    proj, c2 = grads.backbone_layers["level2.project"].bn, grads.backbone_layers["level2.tree1.conv2"].bn
    assert proj.args.y[0] == c2.args.y[0] and proj.args.y[0] != grads.backbone_bn["level2.project"]["out"].pptr
    assert sorted(grads.backbone_bn_reads) == sorted(k + ".raw" for k in keys)
    # keys: param_grads as without the flag; the statistics under the norms' state-dict names
    params = {}
    for read in (grads.predictor_grads, grads.tower_grads, grads.fpn_grads, grads.backbone_grads, grads.stem_grads):
        params.update(read()[1])
    assert sorted(params) == sorted(k for k, _ in model.named_parameters())
    stats = grads.backbone_batch_stats()
    assert sorted(stats) == BN.batch_stats_names(model) and len(stats) == 4 * 37 and all(v.dtype == torch.float32 for v in stats.values())
    assert sorted(k for k in stats if "running" in k) == sorted(k for k, _ in model.named_buffers() if k.startswith("backbone.bottom_up.") and "running" in k)
    base = _plan(model, stem_grads=True)
    with pytest.raises(RuntimeError, match="backbone_batch_stats=True"):
        base.backbone_batch_stats()
    # the plan without the flag: the ops and buffers it had before any flagged plan was built
    assert _table(base) == before and not hasattr(base, "backbone_bn") and base.with_backbone_batch_stats is False
    assert all(getattr(lay, "bn", None) is None for lay in list(base.backbone_layers.values()) + list(base.stem_layers.values()))


def test_flag_composes_with_the_other_norm_flags(hiplib):
    from dd3d_amd.engine import DenseDepthLossPlan
    from tests.test_dense_depth_param_grads import _dla
    model = GC.cpu_model("dd3d_kitti_dla34", EVERYWHERE)
    plan = _plan(model, B=2, H=128, W=128, stem_grads=True, batch_stats=True, fpn_batch_stats=True, backbone_batch_stats=True)
    names = [op.name for op in plan.ops]
    assert all(n in names for n in ("towers.0.bn_stats", "fpn_laterals.bn_apply", "level5.root.bn_apply", "tower_bn_grads.cls.0", "fpn_bn_grads.laterals",
                                    "backbone_bn_grads.level5.root", "stem_bn_grads.base_layer"))
    assert names.index("fpn_grads.lateral3") < names.index("backbone_bn_grads.level5.root") < names.index("stem_bn_grads.level1.0")
    assert plan.backbone_bn_part is not plan.fpn_bn_part and plan.backbone_bn_part is not plan.bn_part
    dd = _dla(FE=EVERYWHERE["FE"])
    dplan = DenseDepthLossPlan(dd, 2, 128, 256, device="cpu", dry_run=True, stem_grads=True, fpn_batch_stats=True, backbone_batch_stats=True)
    dn = [op.name for op in dplan.ops]
    assert "base_layer.bn_apply" in dn and "stem_bn_grads.base_layer" in dn and sorted(dplan.backbone_batch_stats()) == BN.batch_stats_names(dd)


def test_cache_keys_are_distinct(hiplib, monkeypatch):
    import dd3d_amd.engine.losses as EL
    from dd3d_amd.modeling.dd3d import DD3D
    model = GC.cpu_model("dd3d_kitti_dla34", EVERYWHERE)
    made = []

    class Fake:
        def __init__(self, model, B, Hp, Wp, **kw):
            made.append(kw)

        def capture(self):
            pass

    monkeypatch.setattr(EL, "LossPlan", Fake)
    model.use_graph = False
    a = DD3D.get_loss_plan(model, 2, 128, 128, stem_grads=True)
    b = DD3D.get_loss_plan(model, 2, 128, 128, stem_grads=True, backbone_batch_stats=True)
    c = DD3D.get_loss_plan(model, 2, 128, 128, stem_grads=True, backbone_batch_stats=True, fpn_batch_stats=True, batch_stats=True)
    assert len({id(x) for x in (a, b, c)}) == 3 and DD3D.get_loss_plan(model, 2, 128, 128, stem_grads=True, backbone_batch_stats=True) is b
    keys = [k for k in model._plans if k[0] == "losses"]
    assert len(keys) == 3 and sum("backbone_batch_stats" in k for k in keys) == 2
    plain = next(k for k in keys if "backbone_batch_stats" not in k)
    assert plain == ("losses", 2, 128, 128, model.math, model.act_scale, getattr(model, "tile_policy", None), "stem_grads")
    assert made == [dict(stem_grads=True), dict(stem_grads=True, backbone_batch_stats=True),
                    dict(stem_grads=True, batch_stats=True, fpn_batch_stats=True, backbone_batch_stats=True)]


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(hiplib, monkeypatch):
    from dd3d_amd.engine import DenseDepthLossPlan
    from dd3d_amd.engine.losses import LossPlan
    from dd3d_amd.modeling.dd3d import DD3D
    from dd3d_amd.modeling.dense_depth import DD3DDenseDepth
    built = []
    orig = LossPlan._trunk
    monkeypatch.setattr(LossPlan, "_trunk", lambda self, *a, **k: (built.append(1), orig(self, *a, **k))[1])
    model = GC.cpu_model("dd3d_kitti_dla34", EVERYWHERE)
    # without the new flag the two other flags keep their refusals, in their words
    with pytest.raises(NotImplementedError, match="batch_stats covers the head towers; FE.BACKBONE.NORM = 'BN'"):
        _plan(GC.cpu_model("dd3d_kitti_dla34", BB_BN), batch_stats=True)
    with pytest.raises(NotImplementedError, match="fpn_batch_stats covers the FPN; FE.BACKBONE.NORM = 'BN' would need batch statistics in the bottom-up network"):
        _plan(model, fpn_batch_stats=True)
    # with it, the backbone counts as covered -- the FPN's norm still needs its own flag
    with pytest.raises(NotImplementedError, match="batch_stats covers the head towers; FE.FPN.NORM = 'BN'"):
        _plan(model, B=2, H=128, W=128, batch_stats=True, backbone_batch_stats=True)
    # the flag is never a silent no-op
    for over in (None, {"FE": {"BACKBONE": {"NORM": "FrozenBN"}}}, {"FE": {"BACKBONE": {"NORM": ""}}}):
        for kw in (dict(), dict(batch_stats=True), dict(stem_grads=True)):
            with pytest.raises(ValueError, match="FE.BACKBONE.NORM"):
                _plan(GC.cpu_model("dd3d_kitti_dla34", over), backbone_batch_stats=True, **kw)
    with pytest.raises(NotImplementedError, match="VoVNet"):
        _plan(GC.cpu_model("dd3d_kitti_v99", BB_BN), B=1, H=128, W=256, backbone_batch_stats=True)
    with pytest.raises(NotImplementedError, match="Bottleneck"):
        _plan(GC.cpu_model("dd3d_kitti_dla34", {"FE": {"BACKBONE": {"NORM": "BN", "NAME": "DLA-60"}}}), backbone_batch_stats=True)
    generic = GC.cpu_model("dd3d_kitti_dla34", BB_BN)
    generic.force_generic_dla = True
    with pytest.raises(NotImplementedError, match="force_generic_dla"):
        _plan(generic, backbone_batch_stats=True)
    bb = GC.cpu_model("dd3d_kitti_dla34", BB_BN)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        _plan(bb, B=1, H=32, W=32, backbone_batch_stats=True)  # level5 of one 32 x 32 image is 1 x 1
    with pytest.raises(NotImplementedError, match="even canvas"):
        _plan(bb, B=2, H=64, W=127, stem_grads=True, backbone_batch_stats=True)
    for math, env, match in (("f32", {}, "DD3D_MATH=f32"), ("bf16x3", {"DD3D_PLANES": "0"}, "DD3D_PLANES=0"), (None, {"DD3D_PLANES_ONLY": "0"}, "DD3D_PLANES_ONLY=0"),
                             ("bf16x2", {}, "bf16x2"), ("bf16", {}, "bf16")):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            bb.math = math
            with pytest.raises(NotImplementedError, match=match):
                _plan(bb, backbone_batch_stats=True)
    bb.math = None
    assert built == []  # every refusal came before anything was built
    for math in ("bf16x3", None):
        bb.math = math
        assert "level5.root.bn_apply" in [op.name for op in _plan(bb, backbone_batch_stats=True).ops]
    bb.math = None
    for fn in (DD3D.compute_losses, DD3D.get_loss_plan, LossPlan.__init__, DenseDepthLossPlan.__init__):
        assert inspect.signature(fn).parameters["backbone_batch_stats"].default is False
    assert "backbone_batch_stats" not in inspect.signature(DD3DDenseDepth.compute_losses).parameters  # (taken from **branch, as its siblings)
    with pytest.raises(TypeError, match="unexpected keyword argument 'backbone_batchstats'"):
        DD3D.compute_losses(bb, [], backbone_batchstats=True)


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_backbone_bn_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    cls, cname = hip.BackboneBnArgs, "dd3d_backbone_bn_args"
    assert [f[0] for f in cls._fields_] == ["bn", "y32", "res", "act", "res_mode", "res_pitch", "y32_pitch", "res_plane_scale", "reserved"]
    assert cls._fields_[0][1] is hip.TowerBnArgs
    out = (C.c_int64 * 32)()
    n = hiplib.dd3d_backbone_bn_layout(out, 32)
    assert n == len(cls._fields_) + 1 and out[n] == -1 and out[0] == C.sizeof(cls)
    assert [out[1 + j] for j in range(len(cls._fields_))] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert hiplib.dd3d_backbone_bn_layout(out, 8) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_backbone_bn_layout")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {', f'  printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'  printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));' for f in cls._fields_]
    lines += ['  printf("min %d max %d acts %d %d %d\\n", DD3D_BBN_MIN_C, DD3D_BBN_MAX_C, DD3D_BBN_RELU, DD3D_BBN_LINEAR, DD3D_BBN_RESIDUAL);', '  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    text = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    got = dict(l.split(" ", 1) for l in text[:-1])
    assert int(got[cname]) == C.sizeof(cls) and C.sizeof(cls) <= 4096  # (travels to the kernel by value)
    for f in cls._fields_:
        assert int(got[f"{cname}.{f[0]}"]) == getattr(cls, f[0]).offset, f[0]
    assert text[-1] == f"min {hip.BBN_MIN_C} max {hip.BBN_MAX_C} acts {hip.BBN_RELU} {hip.BBN_LINEAR} {hip.BBN_RESIDUAL}"
    new = ("dd3d_backbone_bn_batch_stats", "dd3d_backbone_bn_apply", "dd3d_backbone_bn_backward_reduce", "dd3d_backbone_bn_backward_apply",
           "dd3d_backbone_bn_backward_reduce_linear", "dd3d_backbone_bn_backward_apply_linear", "dd3d_backbone_bn_slices", "dd3d_backbone_bn_layout")
    assert all(e in hip.EXPORTS and hasattr(hiplib, e) for e in new)
    assert [c for c in range(0, 600, 8) if hip.backbone_bn_width_ok(c)] == [16] + list(range(32, 257, 32)) + [512]
    # host-side rejections need no device: every case below is refused before any launch
    st, f = None, cls()
    assert hiplib.dd3d_backbone_bn_apply(None, st) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_backbone_bn_apply")
    for name in new[:1] + new[2:6]:
        fn = getattr(hiplib, name)
        assert fn(None, st) == -1 and hiplib.dd3d_last_error().decode().startswith(name + ":"), name
        assert fn(C.byref(f.bn), st) == -1 and hiplib.dd3d_last_error().decode().startswith(name + ":"), name
    keep = [(C.c_float * 4)() for _ in range(6)]  # dummy non-null addresses
    a = f.bn
    a.num_segs, a.c_pitch, a.math_mode, a.plane_scale, a.N[0] = 1, 512, hip.MATH_F16X2, 16.0, 30
    a.c[0], a.stats[0], a.y[0], a.beta[0] = (C.addressof(k) for k in keep[:4])
    for width in (8, 24, 48, 288, 384, 768, 1024):
        a.C = width
        assert hiplib.dd3d_backbone_bn_apply(C.byref(f), st) == -1 and f"C = {width}" in hiplib.dd3d_last_error().decode()
        assert hiplib.dd3d_backbone_bn_slices(C.byref(a)) == -1
    a.C = 512
    assert hiplib.dd3d_backbone_bn_slices(C.byref(a)) == 1
    a.N[0] = 130
    assert hiplib.dd3d_backbone_bn_slices(C.byref(a)) == 3 == hip.bn_slices([130])

    def refused(what):
        assert hiplib.dd3d_backbone_bn_apply(C.byref(f), st) == -1
        err = hiplib.dd3d_last_error().decode()
        assert err.startswith("dd3d_backbone_bn_apply:") and what in err, err

    f.act = 3
    refused("act = 3")
    f.act, f.res_pitch = hip.BBN_RESIDUAL, 512
    refused("no residual")
    f.res[0], f.res_mode = C.addressof(keep[4]), 7
    refused("res_mode = 7")
    f.res_mode, f.res_pitch = hip.PG_ACT_F32, 510
    refused("res_pitch = 510")
    f.res_mode, f.res_plane_scale = hip.PG_ACT_F16X2, 0.0
    refused("res_plane_scale")
    f.act, a.math_mode = hip.BBN_RELU, hip.MATH_BF16
    refused("math mode")
    a.math_mode, a.y[0] = hip.MATH_F16X2, None
    refused("neither split planes nor an f32 output")
    f.y32[0], f.y32_pitch = C.addressof(keep[5]), 100
    refused("y32_pitch = 100")
    a.C, a.c_pitch, a.y[0], f.y32[0] = 16, 16, C.addressof(keep[2]), None
    refused("split planes need C % 32 == 0")
    a.N[0] = 1
    refused("N = 1")
    # the towers' and the FPN's entry points keep their own limits
    a.N[0], a.C = 30, 16
    assert hiplib.dd3d_bn_slices(C.byref(a)) == -1 and "C = 16" in hiplib.dd3d_last_error().decode()
    a.C = 512
    assert hiplib.dd3d_bn_slices(C.byref(a)) == -1 and "C = 512" in hiplib.dd3d_last_error().decode()
    assert hip.ABI_VERSION == 7 and hiplib.dd3d_abi_version() == 7  # (new entry points beside the old ones: the number stays)
