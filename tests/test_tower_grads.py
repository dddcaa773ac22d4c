"""Tower backward, the parts that need no GPU: the layer oracle (tests/tower_grad_oracle.py) against a float64 central finite difference
of the real forward (ReLU included); the chain oracle against plain autograd through the module chain; the read-out formulas of
LossPlan.tower_grads against autograd through fold_norm's own expression; the op list, buffers and parameter names of the dry-run plan
for every head configuration; the ctypes layout of dd3d_tower_grad_args against the header; the chain oracle against the
reference-modules golden."""
import ctypes as C
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import loss_grad_cases as GC
from tests import predictor_grad_cases as PC
from tests import predictor_grad_oracle as PO
from tests import tower_grad_cases as TC
from tests import tower_grad_oracle as TO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fd_case():
    case = TC.LayerCase(level_hw=[(3, 4), (2, 3)], B=2, Cin=3, Cout=5, seed=5, with_da_add=True)
    case.x, case.w = [a.double() for a in case.x], case.w.double() * 3.0
    case.scale, case.shift = [s.double() for s in case.scale], [s.double() for s in case.shift]
    case.y = TO.forward(case.x, case.w, case.scale, case.shift)
    return case


@pytest.mark.parametrize("family", ["weight", "norm_weight", "norm_bias", "da"])
def test_layer_oracle_matches_finite_difference(family):
    """d / d theta of sum G * relu(s * conv + t), the real forward, by a float64 central difference (no entry of the case lies within
    the step of the kink; both sides of it occur)."""
    case = _fd_case()
    pos = torch.cat([v.reshape(-1) for v in case.y])
    assert float(pos[pos > 0].min()) > 1e-3 and bool((pos == 0).any()) and bool((pos > 0).any())
    pre = torch.cat([(F.conv2d(a, case.w, padding=1) * case.scale[l][None, :, None, None] + case.shift[l][None, :, None, None]).reshape(-1)
                     for l, a in enumerate(case.x)])
    assert float(pre.abs().min()) > 1e-3
    ref = case.ref(torch.float64, da_add=False)
    for l in range(case.L):
        leaves = {"weight": case.w, "norm_weight": case.scale[l], "norm_bias": case.shift[l], "da": case.x[l]}
        want = {"weight": ref["dw"], "norm_weight": ref["r"][l], "norm_bias": ref["q"][l], "da": ref["da"][l]}[family]
        x = leaves[family]
        f = lambda: float(sum((v * case.g[i].double()).sum() for i, v in enumerate(TO.forward(case.x, case.w, case.scale, case.shift))))
        gen = torch.Generator().manual_seed(9)
        h = 1e-6
        for i in torch.randperm(x.numel(), generator=gen)[:16].tolist():
            old = float(x.view(-1)[i])
            x.view(-1)[i] = old + h
            up = f()
            x.view(-1)[i] = old - h
            dn = f()
            x.view(-1)[i] = old
            fd = (up - dn) / (2 * h)
            assert abs(fd - float(want.reshape(-1)[i])) <= 1e-7 * max(1.0, abs(fd)), (family, l, i, fd, float(want.reshape(-1)[i]))
    # the shared filter's gradient is the scaled sum of the per-level partials; da_add is added on top
    total = sum(case.scale[l][:, None, None, None] * ref["dw_level"][l] for l in range(case.L))
    assert float((total - ref["dw"]).abs().max()) <= 1e-12 * float(ref["dw"].abs().max())
    added = case.ref(torch.float64)
    assert all(torch.equal(added["da"][l], case.da_add[l].double() + ref["da"][l]) for l in range(case.L))


@pytest.mark.parametrize("name", ["kitti", "frozen_2d", "no_norm_3d", "box2d_only"])
def test_chain_oracle_equals_autograd_through_the_module_chain(name):
    """With the chain's own stored activations the layer-by-layer backward is plain autograd through the towers (float64)."""
    exp, over = TC.CONFIGS[name]
    model = TC.randomize_towers(GC.cpu_model(exp, over))
    gen = torch.Generator().manual_seed(3)
    level_hw = [(5, 6), (2, 3)]
    feats = [torch.randn(2, 256, h, w, generator=gen, dtype=torch.float64) for h, w in level_hw]
    stored = TO.chain_forward(model, feats)
    g_top = {t: [torch.randn(v.shape, generator=gen, dtype=torch.float64) for v in stored[t][-1][1]] for t in stored}
    params, fgrads, _ = TO.chain_grads(model, stored, g_top, torch.float64)
    assert sorted(params) == [k for k in TO.tower_param_names(model) if ".norm." not in k or int(k.split(".")[-2]) < len(level_hw)]  # (two levels here)
    # plain autograd: parameters and features as leaves, the towers applied as fold_norm folds them
    names = dict(model.named_parameters())
    P = {k: names[k].detach().double().requires_grad_(True) for k in params}
    X = [f.clone().requires_grad_(True) for f in feats]
    total = 0
    for t, convs in TO.tower_modules(model).items():
        x = list(X)
        for i, conv in enumerate(convs):
            pre = TO.TOWER_PREFIX[t] + f".{i}"
            for l in range(len(x)):
                norm = TO.level_norm(conv, l)
                c = F.conv2d(x[l], P[pre + ".weight"], P.get(pre + ".bias"), padding=1)
                if norm is not None:
                    nw, nb = (P[pre + f".norm.{l}.weight"], P[pre + f".norm.{l}.bias"]) if pre + f".norm.{l}.weight" in P else \
                        (norm.weight.double(), norm.bias.double())
                    s = nw * torch.rsqrt(norm.running_var.float() + norm.eps).double()
                    c = (c - norm.running_mean.double()[None, :, None, None]) * s[None, :, None, None] + nb[None, :, None, None]
                x[l] = F.relu(c)
        total = total + sum((x[l] * g_top[t][l]).sum() for l in range(len(x)))
    total.backward()
    close = lambda a, b: float((a - b).abs().max()) <= 1e-10 * max(1.0, float(b.abs().max()))
    for k in params:
        assert close(params[k], P[k].grad), k
    for l in range(len(X)):
        assert close(fgrads[f"feature{l}"], X[l].grad), l


@pytest.mark.parametrize("name", ["kitti", "frozen_2d", "no_norm_3d"])
def test_read_out_formulas_match_autograd_through_fold_norm(name):
    """norm_param_grads turns the kernels' per-level sums q = sum g and r = sum g * conv into the gradients of a BN norm's weight and
    bias, of a norm-less tower's conv bias, and of nothing for a FrozenBN norm -- as autograd through fold_norm's expression gives them."""
    from dd3d_amd.engine.losses import norm_param_grads
    from dd3d_amd.layers import fold_norm
    exp, over = TC.CONFIGS[name]
    model = TC.randomize_towers(GC.cpu_model(exp, over))
    gen = torch.Generator().manual_seed(4)
    names = {id(p): k for k, p in model.named_parameters()}
    for t, convs in TO.tower_modules(model).items():
        conv = convs[1]
        if name == "kitti":
            conv.bias = torch.nn.Parameter(torch.randn(conv.out_channels, generator=gen) * 0.3, requires_grad=False)  # a conv bias under a norm
        x = [torch.randn(2, 256, 3, 4, generator=gen, dtype=torch.float64), torch.randn(2, 256, 2, 2, generator=gen, dtype=torch.float64)]
        sc, sh = zip(*[fold_norm(conv, TO.level_norm(conv, l)) for l in range(2)])
        y = TO.forward(x, conv.weight.double(), [s.double() for s in sc], [s.double() for s in sh])
        g = [torch.randn(v.shape, generator=gen, dtype=torch.float64) for v in y]
        want, _ = TO.module_layer_grads(conv, x, y, g, torch.float64)
        res = TO.layer_grads(x, y, g, conv.weight, [s.double() for s in sc], torch.float64)
        got = {}
        for l in range(2):
            norm = TO.level_norm(conv, l)
            out = norm_param_grads(conv, norm, sc[l].double(), res["q"][l], res["r"][l])
            for key, p in (("norm.weight", getattr(norm, "weight", None)), ("norm.bias", getattr(norm, "bias", None)), ("bias", conv.bias)):
                if key in out:
                    got[id(p)] = got.get(id(p), 0) + out[key]
        got = {k: v for k, v in got.items() if k in want}
        assert set(got) == set(want) - {id(conv.weight)}, (name, t)
        trainable = isinstance(getattr(TO.level_norm(conv, 0), "weight", None), torch.nn.Parameter)
        assert len(got) == (4 + (1 if conv.bias is not None else 0) if trainable else (1 if conv.bias is not None else 0)), (name, t)
        for k, v in got.items():
            assert float((v - want[k]).abs().max()) <= 1e-6 * max(1.0, float(want[k].abs().max())), (name, t, names.get(k))


def _dry_plan(model, B=1, H=64, W=128, **kw):
    from dd3d_amd.engine.losses import LossPlan
    return LossPlan(model, B, H, W, device="cpu", dry_run=True, **kw)


@pytest.mark.parametrize("name", list(TC.CONFIGS))
def test_dry_run_plan_ops_buffers_and_parameter_names(name):
    exp, over = TC.CONFIGS[name]
    model = GC.cpu_model(exp, over)
    with_p, plan = _dry_plan(model, pred_grads=True), _dry_plan(model, tower_grads=True)
    towers = [t for t in TO.TOWERS if t != "box3d" or not model.only_box2d]
    assert plan.pred_grads and plan.grads and plan.keep_tower_outputs and not with_p.keep_tower_outputs
    tail = [f"tower_grads.{t}.{i}" for t in towers for i in (3, 2, 1, 0)]
    base = [op.name for op in with_p.ops]
    assert [op.name for op in plan.ops] == base + tail and base[-1].startswith("predictor_grads.")
    assert all(op.branch == 0 for op in plan.ops[-len(tail):])  # no side streams: one graph on the main stream
    L = len(plan.features)
    # every layer has its own output buffers; the default plan keeps its two
    tb = sorted(b for b in plan.bufs if b.startswith("tower"))
    assert tb == sorted(f"towerL{i}.{l}" for i in range(4) for l in range(L))
    assert sorted(b for b in with_p.bufs if b.startswith("tower")) == sorted(f"tower{s}.{l}" for s in "AB" for l in range(L))
    ys = {plan.tower_info[(t, i)]["y"][l].buf.name for t in towers for i in range(4) for l in range(L)}
    assert len(ys) == 4 * L
    for t in towers:
        for i in range(4):
            lay = plan.tower_layers[(t, i)]
            nxt = plan.tower_layers[(t, i + 1)].da if i < 3 else {g.tower: g for g in plan.pred_groups.values()}[t].da
            assert all(a.data_ptr() == b.data_ptr() for a, b in zip(lay.keep[0], nxt))  # layer i reads layer i + 1's input gradient
            assert lay.part.data_ptr() == plan.tower_slab[0].data_ptr()  # one slab for every call
            if i < 3:
                assert [v.buf.name for v in plan.tower_info[(t, i + 1)]["x"]] == [v.buf.name for v in plan.tower_info[(t, i)]["y"]]
    # the first layers chain through da_add in tower order, up to the gradient at plan.features
    assert plan.tower_layers[("cls", 0)].keep[3] is None
    for a, b in zip(towers[:-1], towers[1:]):
        assert all(x.data_ptr() == y.data_ptr() for x, y in zip(plan.tower_layers[(b, 0)].keep[3], plan.tower_layers[(a, 0)].da))
    assert all(x.data_ptr() == y.data_ptr() for x, y in zip(plan.feature_grads, plan.tower_layers[(towers[-1], 0)].da))
    feats, params = plan.tower_grads()
    named = dict(model.named_parameters())
    want = TO.tower_param_names(model)
    assert sorted(params) == want and all(params[k].shape == named[k].shape and params[k].dtype == torch.float32 for k in want)
    assert list(feats) == [f"feature{l}" for l in range(L)]
    assert all(feats[f"feature{l}"].shape == (1, 256, plan.features[l].H, plan.features[l].W) for l in range(L))
    has = lambda k: k in params
    assert has("fcos2d_head.cls_tower.0.weight") and has("fcos2d_head.box2d_tower.3.weight")
    assert has("fcos2d_head.cls_tower.2.norm.4.weight") == has("fcos2d_head.box2d_tower.0.norm.0.bias") == (name != "frozen_2d")
    assert has("fcos3d_head.box3d_tower.1.weight") == (name != "box2d_only")
    assert has("fcos3d_head.box3d_tower.1.bias") == (name == "no_norm_3d")
    assert not has("fcos3d_head.box3d_tower.1.norm.0.weight")  # the released FCOS3D.NORM is FrozenBN: no parameters
    assert not any(k in params for k in with_p.predictor_grads()[1])
    with pytest.raises(RuntimeError, match="tower_grads"):
        with_p.tower_grads()


def test_default_plan_is_unchanged_and_nusc_rides_the_cls_tower():
    model = GC.cpu_model("dd3d_nusc_dla34")
    plain, with_t = _dry_plan(model, 2, 128, 224), _dry_plan(model, 2, 128, 224, tower_grads=True)
    names = [op.name for op in plain.ops]
    assert [n for n in names if n.startswith("towers.")] == [f"towers.{i}" for i in range(4)] and not any("grads" in n for n in names)
    assert [b for b in plain.bufs if b.startswith("tower")] == [f"tower{s}.{l}" for s in "AB" for l in range(len(plain.features))]
    assert [op.name for op in with_t.ops][:len(names)] == names  # the forward and the losses are the same ops
    assert plain.tower_info is None and sorted(with_t.tower_info) == sorted((t, i) for t in TO.TOWERS for i in range(4))
    assert with_t.pred_groups["cls_map"].n == model.num_classes + model.attr_logits.out_channels + 1
    assert with_t.tower_layers[("cls", 3)].keep[0][0].data_ptr() == with_t.pred_groups["cls_map"].da[0].data_ptr()


def test_slice_count_mirror():
    from dd3d_amd import hip
    assert hip.tower_grad_slices(1, [(1, 1)], 32, 32) == 1 and hip.tower_grad_slices(1, [(30, 70)], 32, 32) == 15
    assert hip.tower_grad_slices(3, [(100, 64)], 256, 256) == 60 and hip.tower_grad_slices(3, [(100, 64)], 64, 32) == 75
    kitti = [(48, 160), (24, 80), (12, 40), (6, 20), (3, 10)]
    a, b = hip.tower_grad_slices(1, kitti, 256, 256), hip.tower_grad_slices(4, kitti, 256, 256)
    assert a == 36 + 12 + 3 + 2 + 1 and a < b <= hip.TG_SLAB_BYTES // (256 * 9 * 256 * 4) + len(kitti)  # grows with the pixels, under the budget


def test_tower_grad_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    cls = hip.TowerGradArgs
    names = [f[0] for f in cls._fields_]
    assert names == ["x", "y", "g", "scale", "da_add", "da", "w", "part", "qpart", "dw_level", "dw", "q", "r", "H", "W", "num_levels", "B", "Cin", "Cout",
                     "g_pitch", "x_mode", "x_pitch", "y_mode", "y_pitch", "n_slices", "dgrad_rows", "x_plane_scale", "y_plane_scale"]
    out = (C.c_int64 * 32)()
    n = hiplib.dd3d_tower_grad_layout(out, 32)
    assert n == len(names) + 1 and out[0] == C.sizeof(cls)
    assert [out[i + 1] for i in range(len(names))] == [getattr(cls, f).offset for f in names] and out[n] == -1
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(dd3d_tower_grad_args));', '  printf("maxc %d\\n", DD3D_TG_MAX_C);',
             '  printf("unit %d\\n", DD3D_TG_UNIT);', '  printf("minunits %d\\n", DD3D_TG_MIN_UNITS_PER_SLICE);',
             '  printf("slab %lld\\n", (long long)DD3D_TG_SLAB_BYTES);', '  printf("tiles %d\\n", DD3D_TG_MIN_TILES);']
    lines += [f'  printf("{f} %zu\\n", offsetof(dd3d_tower_grad_args, {f}));' for f in names] + ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) and int(got["maxc"]) == hip.TG_MAX_C and int(got["unit"]) == hip.TG_UNIT
    assert int(got["minunits"]) == hip.TG_MIN_UNITS_PER_SLICE and int(got["slab"]) == hip.TG_SLAB_BYTES and int(got["tiles"]) == hip.TG_MIN_TILES
    for f in names:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert all(e in hip.EXPORTS for e in ("dd3d_tower_wgrad", "dd3d_tower_dgrad", "dd3d_tower_grad_slices", "dd3d_tower_grad_layout"))


# --------------------------------------------------------------------------------------------------- the reference-modules golden
_CHAINS = {}


def reference_chain(name):
    """The golden's seeded features through the CPU towers (float32, every layer's stored input and output), and the gradients at the
    towers' outputs from the predictor oracle on the loss oracle's head-map gradients, in float64 and float32.  Computed once per case."""
    if name not in _CHAINS:
        model, towers, maps, case = PC.reference_chain(name)
        _, feats, _, _ = PC.reference_inputs(name)
        stored = TO.chain_forward(model, feats)
        for t in stored:  # the chain's last outputs are the tower outputs the predictor oracle linearises at
            assert all(float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) for a, b in zip(stored[t][-1][1], towers[t]))
            stored[t][-1] = (stored[t][-1][0], towers[t])
        tops = []
        for dtype in (torch.float64, torch.float32):
            _, tw = PO.model_grads(model, towers, case.ref(dtype), maps, dtype)
            tops.append({t: [tw[f"{t}_tower_out{l}"] for l in range(len(feats))] for t in stored})
        _CHAINS[name] = (model, stored, tops[0], tops[1])
    return _CHAINS[name]


def golden_families(z, params, feats):
    """(golden, ours) flat vectors per family -- weight, norm_weight, norm_bias and feature -- at the golden's stored positions."""
    out = {}
    for fam in ("weight", "norm_weight", "norm_bias"):
        ks = [k for k in sorted(params) if TO.family_of(k) == fam]
        out[fam] = (torch.cat([torch.from_numpy(z["param:" + k]).reshape(-1) for k in ks]),
                    torch.cat([params[k].reshape(-1)[PC.tower_sample(params[k].shape)] for k in ks]))
    ks = sorted(feats)
    out["feature"] = (torch.cat([torch.from_numpy(z[f"feature:{k[-1]}"]) for k in ks]),
                      torch.cat([feats[k].reshape(-1)[PC.tower_sample(feats[k].shape)] for k in ks]))
    return out


@pytest.mark.parametrize("name", list(TC.REFERENCE_CASES))
def test_chain_oracle_matches_the_reference_modules_golden(name):
    """The reference's own FCOS2DHead / FCOS3DHead (+ nuScenes predictors) and loss modules under torch autograd with the features as
    leaves (tests/golden/make_tower_grad_golden.py) against this project's statements of the same chain.  Both sides are within one
    bar of the float64 gradient: 2 * bar."""
    import numpy as np
    z = np.load(os.path.join(ROOT, "tests", "golden", f"tower_grads_{name}.npz"))
    model, stored, g64, g32 = reference_chain(name)
    assert sorted(k[6:] for k in z.files if k.startswith("param:")) == TO.tower_param_names(model)
    p64, f64, _ = TO.chain_grads(model, stored, g64, torch.float64)
    p32, f32, _ = TO.chain_grads(model, stored, g32, torch.float32)
    a64, a32 = golden_families(z, p64, f64), golden_families(z, p32, f32)
    for fam, (gold, a) in a64.items():
        bar, d32, gmax = TO.bar(a, a32[fam][1], torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((gold.double() - a).abs().max())
        print(f"[tower_grads] ref:{name} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} golden-dev {dev:.3e} bar {2 * bar:.3e}")
        assert gmax > 0.0 and dev <= 2 * bar, (name, fam, dev, bar)
