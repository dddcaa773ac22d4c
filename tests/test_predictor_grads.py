"""Predictor-layer backward, the parts that need no GPU: the CPU oracle (tests/predictor_grad_oracle.py) against a float64 central finite
difference of the real forward (clamp included) and against the model's own modules applied one by one; an exactly-zero Scale gradient;
the key set of the parameter gradients for every head configuration; the op list of the plan; the ctypes layout of
dd3d_pred_grad_args against the header."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from tests import loss_grad_cases as GC
from tests import predictor_grad_cases as PC
from tests import predictor_grad_oracle as PO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fd_case():
    case = PC.GroupCase(level_hw=[(3, 4)], B=2, n=6, Cin=3, seed=5)
    case.act, case.w, case.bias = [a.double() for a in case.act], [case.w[0].double()], [case.bias[0].double()]
    case.scale, case.offset = [case.scale[0].double()], [case.offset[0].double()]
    case.maps = PO.forward(case.act, case.w, case.bias, case.scale, case.offset, case.lo)
    return case


@pytest.mark.parametrize("family", ["weight", "bias", "scale", "offset", "act"])
def test_oracle_matches_finite_difference(family):
    """d / d theta of sum G * clamp_lo((conv + b) * s + o), the real forward, by a float64 central difference (no entry of the 1-level
    3x4 case lies within the step of its clamp)."""
    case = _fd_case()
    clamped = torch.isfinite(case.lo)
    assert float(case.maps[0][:, clamped][case.maps[0][:, clamped] > 0].min()) > 1e-3 and bool((case.maps[0][:, clamped] == 0).any())
    ref = case.ref(torch.float64)
    leaves = {"weight": case.w[0], "bias": case.bias[0], "scale": case.scale[0], "offset": case.offset[0], "act": case.act[0]}
    want = {"weight": ref["dw"][0], "bias": ref["db"][0], "scale": ref["r"][0], "offset": ref["q"][0], "act": ref["da"][0]}[family]
    x = leaves[family]
    f = lambda: float((PO.forward(case.act, case.w, case.bias, case.scale, case.offset, case.lo)[0] * case.g[0].double()).sum())
    gen = torch.Generator().manual_seed(9)
    h = 1e-6
    for i in torch.randperm(x.numel(), generator=gen)[:24].tolist():
        old = float(x.view(-1)[i])
        x.view(-1)[i] = old + h
        up = f()
        x.view(-1)[i] = old - h
        dn = f()
        x.view(-1)[i] = old
        fd = (up - dn) / (2 * h)
        assert abs(fd - float(want.reshape(-1)[i])) <= 1e-7 * max(1.0, abs(fd)), (family, i, fd, float(want.reshape(-1)[i]))
    # the slot sums are the sums of the per-channel Scale / Offset gradients
    for j in (0, 1):
        sel = case.slot == j
        assert float(ref["dscale"][0, j]) == float(ref["r"][0][sel].sum()) and float(ref["doffset"][0, j]) == float(ref["q"][0][sel].sum())


def test_scale_with_all_channels_clamped_away_is_exactly_zero():
    case = PC.GroupCase(level_hw=[(3, 4), (2, 2)], B=1, n=8, Cin=4, seed=3)
    clamped = torch.isfinite(case.lo)
    for m in case.maps:
        m[:, clamped] = 0.0
    case.slot = torch.where(clamped, torch.tensor(2, dtype=torch.int32), case.slot)
    for dtype in (torch.float64, torch.float32):
        ref = case.ref(dtype)
        assert float(ref["dscale"][:, 2].abs().max()) == 0.0 and float(ref["doffset"][:, 2].abs().max()) == 0.0
        assert float(ref["dw"][0][clamped].abs().max()) == 0.0 and float(ref["dscale"][:, :2].abs().min()) > 0.0


CONFIGS = {
    "kitti": ("dd3d_kitti_dla34", None),
    "nusc": ("dd3d_nusc_dla34", None),
    "no_scale": ("dd3d_kitti_dla34", {"DD3D": {"FCOS2D": {"USE_SCALE": False}, "FCOS3D": {"USE_SCALE": False}}}),
    "per_level": ("dd3d_kitti_dla34", {"DD3D": {"FCOS3D": {"PER_LEVEL_PREDICTORS": True}}}),
    "class_agnostic": ("dd3d_kitti_dla34", {"DD3D": {"FCOS3D": {"CLASS_AGNOSTIC_BOX3D": True}}}),
    "box2d_only": ("dd3d_kitti_dla34", {"MODEL": {"BOX3D_ON": False}}),
}


def _dry_plan(model, B=1, H=64, W=128):
    from dd3d_amd.engine.losses import LossPlan
    return LossPlan(model, B, H, W, device="cpu", dry_run=True, pred_grads=True)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_param_grad_keys_follow_the_configuration(name):
    exp, over = CONFIGS[name]
    model = GC.cpu_model(exp, over)
    plan = _dry_plan(model)
    towers, params = plan.predictor_grads()
    named = dict(model.named_parameters())
    want = PO.predictor_param_names(model)
    assert sorted(params) == want and all(params[k].shape == named[k].shape and params[k].dtype == torch.float32 for k in want)
    L = len(plan.features)
    nt = ("cls", "box2d") + (() if model.only_box2d else ("box3d", ))
    assert sorted(towers) == sorted(f"{t}_tower_out{l}" for t in nt for l in range(L))
    assert all(towers[f"cls_tower_out{l}"].shape == (1, 256, plan.features[l].H, plan.features[l].W) for l in range(L))
    # what the configuration decides
    has = lambda k: k in params
    assert has("fcos2d_head.cls_logits.weight") and has("fcos2d_head.centerness.bias")
    assert has("fcos2d_head.scales_box2d_reg.2.scale") == (name != "no_scale")
    assert has("fcos3d_head.box3d_depth.0.weight") == (name != "box2d_only")
    assert has("fcos3d_head.offsets_depth.4.bias") == (name not in ("no_scale", "box2d_only"))
    assert has("fcos3d_head.box3d_depth.0.bias") == (name == "no_scale")  # box3d_depth has a bias only without Scale / Offset
    assert has("fcos3d_head.box3d_quat.4.weight") == (name == "per_level") and has("attr_logits.bias") == has("speed.weight") == (name == "nusc")
    if name == "class_agnostic":
        assert params["fcos3d_head.box3d_quat.0.weight"].shape == (4, 256, 3, 3)
    # every predictor channel belongs to exactly one named module
    for grp in plan.pred_groups.values():
        assert sum(c[0].out_channels for c in grp.convs) == grp.n and grp.owners == ([0] if name != "per_level" or grp.tower != "box3d" else list(range(L)))


def test_plan_ops_and_flags():
    from dd3d_amd.engine.losses import LossPlan
    model = GC.cpu_model("dd3d_nusc_dla34")
    with_g = LossPlan(model, 2, 128, 224, device="cpu", dry_run=True, grads=True)
    with_p = LossPlan(model, 2, 128, 224, device="cpu", dry_run=True, pred_grads=True)
    names = [op.name for op in with_g.ops]
    assert with_p.grads and with_p.pred_grads and not with_g.pred_grads
    assert [op.name for op in with_p.ops] == names + ["predictor_grads.cls_map", "predictor_grads.box2d_map", "predictor_grads.box3d_map"]
    assert all(op.branch == 0 for op in with_p.ops[-3:])  # no side streams
    with pytest.raises(RuntimeError, match="pred_grads"):
        with_g.predictor_grads()
    grp = with_p.pred_groups["cls_map"]
    assert grp.n == model.num_classes + model.attr_logits.out_channels + 1 and grp.tower == "cls"
    assert [tuple(d.shape) for d in grp.da] == [(2, f.H, f.W, 256) for f in with_p.features]


@pytest.mark.parametrize("name", ["kitti", "nusc", "per_level", "no_scale"])
def test_group_oracle_matches_the_models_own_modules(name):
    """The fused groups as ForwardPlan._heads folds them (concatenated filters, per-level scale vectors, the clamp vector, the depth
    Offset) differentiate to the same parameter gradients as the model's modules applied one by one."""
    exp, over = CONFIGS[name]
    model = GC.cpu_model(exp, over)
    gen = torch.Generator().manual_seed(17)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if PO.PREDICTOR_PARAM.match(k):
                p.copy_(torch.randn(p.shape, generator=gen) * (0.05 if k.endswith("weight") else 0.5) + (1.0 if k.endswith("scale") else 0.0))
    plan = _dry_plan(model, 2, 64, 128)
    L = len(plan.features)
    level_hw = [(f.H, f.W) for f in plan.features]
    assert level_hw == PC.PYRAMID_64x128
    tnames = ("cls", "box2d", "box3d")
    towers = {t: [torch.randn(2, 256, h, w, generator=gen).double() for h, w in level_hw] for t in tnames}
    keys = {"cls_map": ["logits"] + (["attr", "speed"] if name == "nusc" else []), "box2d_map": ["box2d_reg", "centerness"],
            "box3d_map": ["quat", "ctr", "depth", "size", "conf"]}
    G, maps, per_group = {}, {}, {}
    for gname, grp in plan.pred_groups.items():
        info = plan.pred_info[gname]
        ident, w, bias = {}, [], []  # one tensor object per distinct module set: the oracle tells shared from per-level filters by identity
        for l in range(L):
            mods = [c[l if len(c) > 1 else 0] for c in grp.convs]
            key = tuple(id(m) for m in mods)
            if key not in ident:
                ident[key] = (torch.cat([m.weight.detach() for m in mods]).double(),
                              torch.cat([m.bias.detach() if m.bias is not None else torch.zeros(m.out_channels) for m in mods]).double())
            w.append(ident[key][0])
            bias.append(ident[key][1])
        scale = [s.double() for s in info["scales"]]
        lo = info["lo"]
        slot = torch.full((grp.n, ), -1, dtype=torch.int32)
        for c0, cn, j, _, _ in grp.slots:
            slot[c0:c0 + cn] = j
        act = towers[grp.tower]
        m = PO.forward(act, w, bias, scale, [torch.zeros(grp.n, dtype=torch.float64)] * L, lo)
        g = [torch.randn(x.shape, generator=gen).double() for x in m]
        per_group[gname] = PO.group_grads(act, g, m, w, bias, scale, lo, slot, torch.float64)
        c0 = 0
        for key, conv in zip(keys[gname], grp.convs):
            oc = conv[0].out_channels
            for l in range(L):
                G[f"{key}{l}"], maps[f"{key}{l}"] = g[l][:, c0:c0 + oc], m[l][:, c0:c0 + oc]
            c0 += oc
    p64, t64 = PO.model_grads(model, towers, G, maps, torch.float64)
    assert sorted(p64) == PO.predictor_param_names(model)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-11 * max(1.0, float(b.abs().max()))
    for gname, grp in plan.pred_groups.items():
        res = per_group[gname]
        for l in range(L):
            assert close(res["da"][l], t64[f"{grp.tower}_tower_out{l}"]), (gname, l)
        names = {id(p): k for k, p in model.named_parameters()}
        c0 = 0
        for conv in grp.convs:
            oc = conv[0].out_channels
            for l in (range(L) if len(conv) > 1 else [0]):
                mod = conv[l]
                dw = res["dw"][l][c0:c0 + oc] if len(conv) > 1 else sum(res["dw"][o][c0:c0 + oc] for o in res["dw"])
                assert close(dw, p64[names[id(mod.weight)]]), names[id(mod.weight)]
                if mod.bias is not None:
                    db = res["db"][l][c0:c0 + oc] if len(conv) > 1 else sum(res["db"][o][c0:c0 + oc] for o in res["db"])
                    assert close(db, p64[names[id(mod.bias)]]), names[id(mod.bias)]
            c0 += oc
        for _, _, j, scales, offsets in grp.slots:
            for l in range(L):
                assert close(res["dscale"][l, j:j + 1], p64[names[id(scales[l].scale)]]), (gname, j, l)
                if offsets is not None:
                    assert close(res["doffset"][l, j:j + 1], p64[names[id(offsets[l].bias)]]), (gname, j, l)


def test_plane_encodings_decode_to_float32_values():
    x = torch.randn(2, 64, 3, 5, generator=torch.Generator().manual_seed(2))
    for ps in (16.0, 1.0):
        planes, dec = PC.encode_f16x2(x, ps)
        assert planes.shape == (2, 30, 2, 32) and planes.dtype == torch.int16
        assert float((dec - x).abs().max()) <= 2.0**-21 * float(x.abs().max())  # two half terms carry 22 bits
    planes, dec = PC.encode_bf16x3(x)
    assert planes.shape == (2, 30, 3, 32) and torch.equal(dec, x)  # the three-term split is exact
    # the layout is Buf's: channel chunk, pixel, plane, channel
    from dd3d_amd.engine.packing import Buf
    b = Buf(2, 3, 5, 64, "cpu", planes=3)
    b.t = None
    b.p = planes
    assert torch.equal(b.nchw(), x)


def test_slice_count_mirror():
    from dd3d_amd import hip
    assert hip.pred_grad_slices(1, [(1, 1)]) == 1 and hip.pred_grad_slices(1, [(1, 257)]) == 5
    assert hip.pred_grad_slices(1, [(30, 70)]) == 30  # 60 units, two per slice
    assert hip.pred_grad_slices(2, PC.PYRAMID_64x128) == 32


def test_pred_grad_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    cls = hip.PredGradArgs
    names = [f[0] for f in cls._fields_]
    assert names == ["act", "g", "map", "w", "bias", "scale", "da", "lo", "slot", "part", "qpart", "dw_level", "dw", "db", "q", "r", "dscale", "doffset",
                     "H", "W", "num_levels", "B", "Cin", "n", "g_pitch", "act_mode", "act_pitch", "n_slices", "plane_scale"]
    out = (C.c_int64 * 32)()
    n = hiplib.dd3d_pred_grad_layout(out, 32)
    assert n == len(names) + 1 and out[0] == C.sizeof(cls)
    assert [out[i + 1] for i in range(len(names))] == [getattr(cls, f).offset for f in names] and out[n] == -1
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(dd3d_pred_grad_args));', '  printf("slots %d\\n", DD3D_PG_MAX_SLOTS);',
             '  printf("maxn %d\\n", DD3D_PG_MAX_N);', '  printf("unit %d\\n", DD3D_PG_UNIT);',
             '  printf("modes %d%d%d\\n", DD3D_PG_ACT_F32, DD3D_PG_ACT_F16X2, DD3D_PG_ACT_BF16X3);']
    lines += [f'  printf("{f} %zu\\n", offsetof(dd3d_pred_grad_args, {f}));' for f in names] + ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) and int(got["slots"]) == hip.PG_MAX_SLOTS and int(got["maxn"]) == hip.PG_MAX_N
    assert int(got["unit"]) == hip.PG_UNIT and got["modes"] == f"{hip.PG_ACT_F32}{hip.PG_ACT_F16X2}{hip.PG_ACT_BF16X3}"
    for f in names:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert all(e in hip.EXPORTS for e in ("dd3d_predictor_wgrad", "dd3d_predictor_dgrad", "dd3d_predictor_grad_slices", "dd3d_pred_grad_layout"))


def golden_families(z, params, towers):
    """(golden, ours) flat vectors per family -- weight, bias, scale, offset and each tower's da -- at the golden's stored positions."""
    fam_of = lambda k: "weight" if k.endswith(".weight") else "scale" if k.endswith(".scale") else "offset" if "offsets_" in k else "bias"
    out = {}
    for fam in ("weight", "bias", "scale", "offset"):
        ks = [k for k in sorted(params) if fam_of(k) == fam]
        out[fam] = (torch.cat([torch.from_numpy(z["param:" + k]).reshape(-1) for k in ks]),
                    torch.cat([params[k].reshape(-1)[PC.tower_sample(params[k].shape)] for k in ks]))
    for t in ("cls", "box2d", "box3d"):
        ks = [k for k in sorted(towers) if k.startswith(t + "_tower_out")]
        out[t + "_da"] = (torch.cat([torch.from_numpy(z[f"tower:{t}{k[-1]}"]) for k in ks]),
                          torch.cat([towers[k].reshape(-1)[PC.tower_sample(towers[k].shape)] for k in ks]))
    return out


@pytest.mark.parametrize("name", list(PC.REFERENCE_CASES))
def test_oracle_matches_the_reference_modules_golden(name):
    """The reference's own FCOS2DHead / FCOS3DHead (+ nuScenes predictors) and loss modules under torch autograd
    (tests/golden/make_predictor_grad_golden.py) against this project's statements of the same chain: oracle towers and predictors, the
    loss oracle's head-map gradients, the predictor oracle.  Both sides are within one bar of the float64 gradient: 2 * bar."""
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", f"predictor_grads_{name}.npz"))
    model, towers, maps, case = PC.reference_chain(name)
    assert sorted(k[6:] for k in z.files if k.startswith("param:")) == PO.predictor_param_names(model)
    assert np.array_equal(z["pos_inds"], case.targets["pos_inds"].numpy()) and case.num_pos > 20
    p64, t64 = PO.model_grads(model, towers, case.ref(torch.float64), maps, torch.float64)
    p32, t32 = PO.model_grads(model, towers, case.ref(torch.float32), maps, torch.float32)
    f64, f32 = golden_families(z, p64, t64), golden_families(z, p32, t32)
    for fam, (gold, a) in f64.items():
        bar, d32, gmax = PO.bar(a, f32[fam][1], torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((gold.double() - a).abs().max())
        print(f"[predictor_grads] ref:{name} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} golden-dev {dev:.3e} bar {2 * bar:.3e}")
        assert gmax > 0.0 and dev <= 2 * bar, (name, fam, dev, bar)
