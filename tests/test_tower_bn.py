"""Batch-statistics BN in the head towers, the parts that need no GPU: the closed formulas of include/dd3d_hip.h against float64
autograd through F.batch_norm(training=True); the running-statistics update against nn.BatchNorm2d; the op list, buffers, bindings and
read-out keys of the dry-run plans with and without the backward; the unchanged plan without the flag; the ctypes layout of
dd3d_tower_bn_args against the header; every refusal; the chain oracle (tests/tower_bn_oracle.py) against the reference-modules golden
(tests/golden/make_tower_bn_golden.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_grad_cases as GC
from tests import predictor_grad_cases as PC
from tests import predictor_grad_oracle as PO
from tests import tower_bn_oracle as BO
from tests import tower_grad_cases as TC
from tests import tower_grad_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layer(seed=3, B=2, Cn=6, h=3, w=5, constant_channel=None):
    gen = torch.Generator().manual_seed(seed)
    c = torch.randn(B, Cn, h, w, generator=gen, dtype=torch.float64) * 1.7 + 0.3
    if constant_channel is not None:
        c[:, constant_channel] = 0.5
    gamma, beta = 0.5 + torch.rand(Cn, generator=gen, dtype=torch.float64), torch.randn(Cn, generator=gen, dtype=torch.float64) * 0.3
    G = torch.randn(B, Cn, h, w, generator=gen, dtype=torch.float64)
    return c, gamma, beta, G


def test_closed_formulas_equal_float64_autograd():
    """q, p, G_c (d beta, d gamma, the gradient at c) and the forward's mu, v, y: the header's formulas against autograd through
    F.batch_norm(training=True) under the stored mask, float64, 1e-12 relative to each tensor's largest entry.  (N = 2 is left to the
    kernel tests: there xhat = +-1 up to eps and G_c cancels to about 1e-5 of its terms, so a bound relative to the RESULT measures the
    cancellation, in autograd as much as in the formula.)"""
    for B, h, w in ((3, 2, 2), (2, 3, 5), (1, 8, 8)):
        c, gamma, beta, G = _layer(B=B, h=h, w=w)
        mu, v, s, t, y = BO.forward_closed(c, gamma, beta, 1e-5)
        ref_y = F.relu(F.batch_norm(c, None, None, gamma, beta, training=True, eps=1e-5))
        assert float((y - ref_y).abs().max()) <= 1e-12 * float(ref_y.abs().max())
        assert bool((y == 0).any()) and bool((y > 0).any())
        q, p, Gc = BO.backward_closed(c, y, G, gamma, 1e-5)
        dbeta, dgamma, dc = BO.backward_autograd(c, y, G, gamma, beta, 1e-5)
        for got, ref in ((q, dbeta), (p, dgamma), (Gc, dc)):
            assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
        assert float(Gc.sum(dim=(0, 2, 3)).abs().max()) <= 1e-12 * float(Gc.abs().max()) * B * h * w  # the mean term: sum G_c = 0


def test_constant_channel_and_all_masked_layer():
    c, gamma, beta, G = _layer(constant_channel=2)
    mu, v, s, t, y = BO.forward_closed(c, gamma, beta, 1e-5)
    assert float(v[2]) == 0.0 and bool(torch.isfinite(y).all()) and torch.equal(y[:, 2], F.relu(beta[2]).expand_as(y[:, 2]))
    q, p, Gc = BO.backward_closed(c, torch.zeros_like(y), G, gamma, 1e-5)
    assert not bool(q.any()) and not bool(p.any()) and not bool(Gc.any())


def test_running_update_equals_nn_batchnorm():
    """One training forward of nn.BatchNorm2d against running_update on the closed formulas' mu and v, both in float32.  Bound: the two
    evaluate the same expression with their sums in different orders; 16 * 2^-23 of the largest value covers N <= 240 terms."""
    gen = torch.Generator().manual_seed(11)
    for B, h, w in ((2, 1, 1), (2, 3, 5), (3, 8, 10)):
        bn = torch.nn.BatchNorm2d(7).train()
        with torch.no_grad():
            bn.running_mean.copy_(torch.randn(7, generator=gen) * 0.2), bn.running_var.copy_(0.5 + torch.rand(7, generator=gen))
        rm, rv = bn.running_mean.clone(), bn.running_var.clone()
        x = torch.randn(B, 7, h, w, generator=gen) * 1.3 + 0.4
        bn(x)
        mu, v = BO.stats(x, torch.float32)
        new_m, new_v = BO.running_update(rm, rv, mu, v, B * h * w)
        assert new_m.dtype == torch.float32 and BO.MOMENTUM == bn.momentum
        for got, ref in ((new_m, bn.running_mean), (new_v, bn.running_var)):
            assert float((got - ref).abs().max()) <= 16 * 2.0**-23 * float(ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------------- dry plans
def _plan(model, B=2, H=64, W=128, **kw):
    from dd3d_amd.engine.losses import LossPlan
    return LossPlan(model, B, H, W, device="cpu", dry_run=True, **kw)


def _model(key):
    exp, over = TC.CONFIGS[key]
    return GC.cpu_model(exp, over)


def _tower_ops(plan):
    return [op.name for op in plan.ops if op.name.startswith(("towers.", "tower_grads.", "tower_bn_grads."))]


@pytest.mark.parametrize("key", ["kitti", "nusc"])
def test_dry_plans_with_batch_stats(hiplib, key):
    from dd3d_amd import hip
    model = _model(key)
    L = 5
    plain, grads = _plan(model, batch_stats=True), _plan(model, batch_stats=True, tower_grads=True)
    forward_ops = [n for i in range(4) for n in (f"towers.{i}", f"towers.{i}.raw", f"towers.{i}.bn_stats", f"towers.{i}.bn_apply")]
    assert _tower_ops(plain) == forward_ops
    back = [n for t in ("cls", "box2d") for i in (3, 2, 1, 0) for n in (f"tower_bn_grads.{t}.{i}", f"tower_grads.{t}.{i}")]
    assert _tower_ops(grads) == forward_ops + back + [f"tower_grads.box3d.{i}" for i in (3, 2, 1, 0)]
    ops = {op.name: op for op in grads.ops}
    for i in range(4):
        # the FrozenBN box3d tower keeps the fused launch; cls and box2d moved to .raw, level-major inside a tower
        assert ops[f"towers.{i}"].info["nsegs"] == L and ops[f"towers.{i}.raw"].info["nsegs"] == 2 * L
        assert all(sg["out"].buf.name == f"towerL{i}.{l}" and sg["out"].c0 == 512 for l, sg in enumerate(ops[f"towers.{i}"].desc["segs"]))
        raw = ops[f"towers.{i}.raw"]
        assert not raw.desc["relu"] and raw.out_forms == [(True, False)] * (2 * L)
        assert [(sg["out"].buf.name, sg["out"].c0) for sg in raw.desc["segs"]] == [(f"towerraw{i}.{l}", 256 * t) for t in range(2) for l in range(L)]
        assert all(bool((sg["scale"] == 1).all()) and not bool(sg["bias"].any()) for sg in raw.desc["segs"])
        st = ops[f"towers.{i}.bn_stats"].desc
        assert st["kind"] == "bn_batch_stats" and [(s["tower"], s["level"]) for s in st["segs"]] == [(t, l) for t in ("cls", "box2d") for l in range(L)]
        assert all(s["out"].buf.name == f"towerL{i}.{s['level']}" and s["out"].c0 == (0 if s["tower"] == "cls" else 256) for s in st["segs"])
        assert ops[f"towers.{i}.bn_apply"].desc["kind"] == "bn_apply_relu_split" and ops[f"towers.{i}.bn_apply"].desc["planes"]
    # raw buffers: one per (layer, level) with the backward, one per level without; f32 only, two towers wide
    assert sorted(k for k in grads.bufs if "raw" in k) == sorted(f"towerraw{i}.{l}" for i in range(4) for l in range(L))
    assert sorted(k for k in plain.bufs if "raw" in k) == [f"towerraw.{l}" for l in range(L)]
    assert all(b.has_f32 and not b.np and b.pitch == 512 for k, b in grads.bufs.items() if "raw" in k)
    assert grads.tower_bn_reads == [f"towerraw{i}.{l}" for i in (3, 2, 1, 0) for l in range(L)] or sorted(grads.tower_bn_reads) == sorted(
        f"towerraw{i}.{l}" for i in range(4) for l in range(L))
    # the GEMM calls of a BN layer: g := G_c, scale ones, y := the plan's tensor of ones (f32), shared by every layer
    ones = [t.data_ptr() for t in grads.tower_ones]
    for (t, i), lay in grads.tower_layers.items():
        a = lay.args
        if t == "box3d":
            assert lay.bn is None and a.y_mode == hip.PG_ACT_F16X2
            continue
        assert a.y_mode == hip.PG_ACT_F32 and a.y_pitch == 256 and [a.y[l] for l in range(L)] == ones and a.g_pitch == 256
        assert [a.g[l] for l in range(L)] == [g.data_ptr() for g in lay.bn.gc] and all(bool((s == 1).all()) for s in lay.keep[2])
        b = lay.bn.args
        assert b.y_mode == hip.PG_ACT_F16X2 and b.num_segs == L and b.c_pitch == 512 and [b.N[l] for l in range(L)] == [2 * h * w for h, w in PC.PYRAMID_64x128]
        assert b.n_slices >= hip.bn_slices([b.N[l] for l in range(L)])
    assert all(bool((t == 1).all()) for t in grads.tower_ones)
    # keys: param_grads as without the flag; the statistics under the towers' running_* names and their batch_* twins
    base = _plan(model, tower_grads=True)
    assert sorted(grads.tower_grads()[1]) == sorted(base.tower_grads()[1]) == TO.tower_param_names(model)
    stats = grads.tower_batch_stats()
    assert sorted(stats) == BO.batch_stats_names(model) and len(stats) == 4 * 8 * L
    running = sorted(k for k, _ in model.named_buffers() if k.startswith(("fcos2d_head.cls_tower", "fcos2d_head.box2d_tower")) and "running" in k)
    assert sorted(k for k in stats if "running" in k) == running
    assert all(v.shape == (256, ) and v.dtype == torch.float32 for v in stats.values())
    with pytest.raises(RuntimeError, match="batch_stats=True"):
        base.tower_batch_stats()


def test_frozen_and_normless_towers_keep_the_fused_launch(hiplib):
    frozen = _plan(_model("frozen_2d"), batch_stats=True, tower_grads=True)
    assert _tower_ops(frozen) == _tower_ops(_plan(_model("frozen_2d"), tower_grads=True)) and not frozen.tower_bn and frozen.tower_batch_stats() == {}
    mixed = _plan(_model("no_norm_3d"), batch_stats=True)
    assert all(op.info["nsegs"] == 5 for op in mixed.ops if op.name in [f"towers.{i}" for i in range(4)]) and len(mixed.tower_bn) == 8
    # FCOS3D.NORM = BN: the third tower joins, nothing is left for the fused launch
    all_bn = _plan(GC.cpu_model("dd3d_kitti_dla34", {"DD3D": {"FCOS3D": {"NORM": "BN"}}}), batch_stats=True)
    assert "towers.0" not in [op.name for op in all_bn.ops] and len(all_bn.tower_bn) == 12
    assert next(op for op in all_bn.ops if op.name == "towers.0.raw").info["nsegs"] == 15 and all_bn.bufs["towerraw.0"].pitch == 768


def test_plan_without_the_flag_is_the_parents(hiplib):
    """Op names, buffers and the tower calls' bindings of a plan built without batch_stats: what the parent commit built."""
    from dd3d_amd import hip
    model = _model("kitti")
    plan = _plan(model, tower_grads=True)
    names = [op.name for op in plan.ops]
    tail = ["towers.0", "towers.1", "towers.2", "towers.3", "predictors.narrow", "predictors", "loss_assign", "loss_terms", "loss_backward",
            "predictor_grads.cls_map", "predictor_grads.box2d_map", "predictor_grads.box3d_map"] + [f"tower_grads.{t}.{i}" for t in TO.TOWERS for i in (3, 2, 1, 0)]
    assert names[-len(tail):] == tail and not any("bn" in n or "raw" in n for n in names)
    assert not any("raw" in k for k in plan.bufs) and not plan.tower_bn and plan.tower_ones is None and plan.batch_stats is False
    assert all(op.info["nsegs"] == 15 for op in plan.ops if op.name.startswith("towers."))
    assert all(lay.args.y_mode == hip.PG_ACT_F16X2 and lay.bn is None for lay in plan.tower_layers.values())
    assert hip.ABI_VERSION == 7 and hiplib.dd3d_abi_version() == 7


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals(hiplib, monkeypatch):
    import inspect
    from dd3d_amd.engine.losses import LossPlan
    from dd3d_amd.modeling.dd3d import DD3D
    from dd3d_amd.modeling.dense_depth import DD3DDenseDepth
    model = _model("kitti")
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        _plan(model, B=1, H=64, W=128, batch_stats=True)  # P7 is 1 x 1
    assert len(_plan(model, B=2, H=64, W=128, batch_stats=True).tower_bn) == 8 and len(_plan(model, B=1, H=128, W=256, batch_stats=True).tower_bn) == 8
    _plan(model, B=1, H=64, W=128)  # (the running-statistics plan has no such limit)
    for key, over in (("FE.BACKBONE.NORM", {"FE": {"BACKBONE": {"NORM": "BN"}}}), ("FE.FPN.NORM", {"FE": {"FPN": {"NORM": "BN"}}})):
        bn = GC.cpu_model("dd3d_kitti_dla34", over)
        with pytest.raises(NotImplementedError, match=key):
            _plan(bn, batch_stats=True)
        _plan(bn)
    for math in ("bf16x2", "bf16"):  # the reduced modes raise where tower_grads raises for them, and nowhere else
        model.math = math
        with pytest.raises(NotImplementedError, match=math):
            _plan(model, batch_stats=True, tower_grads=True)
        assert len(_plan(model, batch_stats=True).tower_bn) == 8
    model.math = None
    for fn in (DD3D.compute_losses, DD3D.get_loss_plan, LossPlan.__init__):
        assert inspect.signature(fn).parameters["batch_stats"].default is False
    assert "batch_stats" not in inspect.signature(DD3DDenseDepth.compute_losses).parameters
    assert "batch_stats" not in inspect.signature(DD3DDenseDepth.get_loss_plan).parameters


def test_planes_off_plans_write_f32(hiplib, monkeypatch):
    """DD3D_PLANES=0 (three-term arithmetic, f32 NHWC everywhere): tower_grads builds there, so batch_stats does; the apply writes f32."""
    from dd3d_amd import hip
    monkeypatch.setenv("DD3D_PLANES", "0")
    model = _model("kitti")
    model.math = "bf16x3"
    plan = _plan(model, batch_stats=True, tower_grads=True)
    a = plan.tower_bn[("cls", 0)]["args"]
    assert a.math_mode == hip.MATH_F32 and a.y_pitch == 768 and plan.tower_layers[("cls", 0)].bn.args.y_mode == hip.PG_ACT_F32


# ---------------------------------------------------------------------------------------------------------------------- the ABI
def test_tower_bn_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    cls, cname = hip.TowerBnArgs, "dd3d_tower_bn_args"
    assert [f[0] for f in cls._fields_] == ["c", "gamma", "beta", "run_mean", "run_var", "stats", "y", "g", "qp", "gc", "part", "status", "N", "num_segs", "C",
                                            "c_pitch", "g_pitch", "math_mode", "y_mode", "y_pitch", "n_slices", "eps", "momentum", "plane_scale", "reserved"]
    out = (C.c_int64 * 64)()
    n = hiplib.dd3d_tower_bn_layout(out, 64)
    assert n == len(cls._fields_) + 1 and out[n] == -1 and out[0] == C.sizeof(cls)
    assert [out[1 + j] for j in range(len(cls._fields_))] == [getattr(cls, f[0]).offset for f in cls._fields_]
    assert hiplib.dd3d_tower_bn_layout(out, 8) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_tower_bn_layout")
    consts = ("DD3D_BN_MAX_SEGS", "DD3D_BN_MAX_C", "DD3D_BN_SLICE", "DD3D_BN_STAT_ROWS", "DD3D_BN_ROW_MU", "DD3D_BN_ROW_VAR", "DD3D_BN_ROW_S", "DD3D_BN_ROW_T",
              "DD3D_BN_ROW_RSTD", "DD3D_BN_ROW_RUN_MEAN", "DD3D_BN_ROW_RUN_VAR")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {']
    lines += [f'  printf("{k} %d\\n", {k});' for k in consts]
    lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
    lines += [f'  printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));' for f in cls._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert [int(got[k]) for k in consts] == [hip.BN_MAX_SEGS, hip.BN_MAX_C, hip.BN_SLICE, hip.BN_STAT_ROWS, hip.BN_ROW_MU, hip.BN_ROW_VAR, hip.BN_ROW_S,
                                             hip.BN_ROW_T, hip.BN_ROW_RSTD, hip.BN_ROW_RUN_MEAN, hip.BN_ROW_RUN_VAR]
    assert int(got[cname]) == C.sizeof(cls)
    for f in cls._fields_:
        assert int(got[f"{cname}.{f[0]}"]) == getattr(cls, f[0]).offset, f[0]
    assert all(e in hip.EXPORTS for e in ("dd3d_bn_batch_stats", "dd3d_bn_apply_relu_split", "dd3d_bn_backward_reduce", "dd3d_bn_backward_apply",
                                          "dd3d_bn_slices", "dd3d_tower_bn_layout"))
    # the slice rule of the bindings is the library's; shapes it refuses
    a = cls()
    for pixels, Cn in (([2], 32), ([30, 256, 257], 64), ([1920, 2 * 48 * 160, 512], 256)):
        a.num_segs, a.C = len(pixels), Cn
        for s, npx in enumerate(pixels):
            a.N[s] = npx
        assert hiplib.dd3d_bn_slices(C.byref(a)) == hip.bn_slices(pixels)
    for field, bad in (("C", 48), ("C", 288), ("num_segs", 0), ("num_segs", hip.BN_MAX_SEGS + 1)):
        old = getattr(a, field)
        setattr(a, field, bad)
        assert hiplib.dd3d_bn_slices(C.byref(a)) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_bn_slices"), (field, bad)
        setattr(a, field, old)
    a.N[1] = 1
    assert hiplib.dd3d_bn_slices(C.byref(a)) == -1 and "N = 1" in hiplib.dd3d_last_error().decode()
    assert hiplib.dd3d_bn_slices(None) == -1


# --------------------------------------------------------------------------------------------------- the reference-modules golden
_CHAINS = {}


def reference_chain(name):
    """predictor_grad_cases.reference_chain and tower_grad_oracle's stored chain under batch statistics: the golden's seeded features
    through the CPU towers (float32; BN layers on the batch's statistics), the head maps and the loss oracle's case on them, and the
    gradients at the towers' outputs from the predictor oracle in float64 and float32.  Computed once per case."""
    if name not in _CHAINS:
        model = GC.cpu_model(PC.REFERENCE_CASES[name][0])
        with BO.batch_statistics(BO.bn_prefixes(model)):
            model, towers, maps, case = PC.reference_chain(name)
        _, feats, _, _ = PC.reference_inputs(name)
        stored, stats = {}, {}
        for t, convs in TO.tower_modules(model).items():
            x, stored[t] = list(feats), []
            for i, conv in enumerate(convs):
                _, y, st = BO.layer_forward(conv, x, torch.float32)
                stored[t].append((x, y))
                stats[(t, i)] = st
                x = y
        for t in stored:  # the chain's last outputs are the tower outputs the predictor oracle linearises at
            assert all(float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) for a, b in zip(stored[t][-1][1], towers[t]))
            stored[t][-1] = (stored[t][-1][0], towers[t])
        tops = []
        for dtype in (torch.float64, torch.float32):
            _, tw = PO.model_grads(model, towers, case.ref(dtype), maps, dtype)
            tops.append({t: [tw[f"{t}_tower_out{l}"] for l in range(len(feats))] for t in stored})
        _CHAINS[name] = (model, stored, tops[0], tops[1], stats, maps, case)
    return _CHAINS[name]


@pytest.mark.parametrize("name", list(PC.REFERENCE_CASES))
def test_chain_oracle_matches_the_reference_modules_golden(name):
    """The reference's own heads with fcos2d_head.train() under torch autograd (tests/golden/make_tower_bn_golden.py) against this
    project's statements of the same chain: gradients within 2 * bar (both sides are within one bar of the float64 gradient), the loss
    values within 1e-5 relative (two float32 forwards), the running statistics after the step within 16 * 2^-23 of their largest value."""
    from tests.test_tower_grads import golden_families
    z = np.load(os.path.join(ROOT, "tests", "golden", f"tower_bn_grads_{name}.npz"))
    model, stored, g64, g32, stats, maps, case = reference_chain(name)
    assert sorted(k[6:] for k in z.files if k.startswith("param:")) == TO.tower_param_names(model)
    p64, f64, _ = BO.chain_grads(model, stored, g64, torch.float64)
    p32, f32, _ = BO.chain_grads(model, stored, g32, torch.float32)
    a64, a32 = golden_families(z, p64, f64), golden_families(z, p32, f32)
    for fam, (gold, a) in a64.items():
        bar, d32, gmax = BO.bar(a.double(), a32[fam][1], torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((gold.double() - a.double()).abs().max())
        print(f"[tower_bn] ref:{name} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} golden against float64 {dev:.3e} (bar {2 * bar:.3e})")
        assert dev <= 2 * bar and gmax > 0, (name, fam, dev, bar)
    # the eval-mode golden is another function: the two differ by far more than the bar (the test would not pass on running statistics)
    z0 = np.load(os.path.join(ROOT, "tests", "golden", f"tower_grads_{name}.npz"))
    assert float(np.abs(z0["feature:0"] - z["feature:0"]).max()) > 1e-3 * float(np.abs(z["feature:0"]).max())
    ref_losses, ours = dict(zip([str(k) for k in z["loss_keys"]], z["loss_values"])), case.losses()
    assert set(ours) == set(ref_losses)
    for k, v in ours.items():
        assert abs(float(v) - ref_losses[k]) <= 1e-5 * abs(ref_losses[k]), (k, float(v), ref_losses[k])
    names = {id(b): k for k, b in model.named_buffers()}
    n_stat = 0
    for (tname, i), st in stats.items():
        conv = TO.tower_modules(model)[tname][i]
        for l, s in enumerate(st):
            if s is None:
                continue
            norm = TO.level_norm(conv, l)
            N = stored[tname][i][0][l].shape[0] * stored[tname][i][0][l].shape[2] * stored[tname][i][0][l].shape[3]
            new_m, new_v = BO.running_update(norm.running_mean, norm.running_var, s[0], s[1], N)
            for got, key in ((new_m, names[id(norm.running_mean)]), (new_v, names[id(norm.running_var)])):
                ref = torch.from_numpy(z["stat:" + key])
                assert float((got - ref).abs().max()) <= 16 * 2.0**-23 * float(ref.abs().max()), key
                n_stat += 1
    assert n_stat == 2 * 8 * 5 == sum(k.startswith("stat:") for k in z.files)
