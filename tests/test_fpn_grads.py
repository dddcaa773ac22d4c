"""FPN backward, the parts that need no GPU: the oracle's restatement (stored p6 mask, own top-down path) against
oracle.dd3d_oracle.fpn_forward; its autograd against float64 central differences for every family; the layer-by-layer chain oracle
against that autograd; the read-out formulas against autograd through fold_norm's expression for FrozenBN, "" and BN; the dry-run plans
(op names and order, the hand-overs of G, D and T, the buffers read, the key sets); the other plans unchanged; the ctypes layout of
dd3d_fpn_grad_args against the header.  There is no new golden: the FPN is detectron2's, the pin to the reference goes through the
forward goldens and fpn_forward."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from oracle import dd3d_oracle as O
from tests import fpn_grad_cases as FC
from tests import fpn_grad_oracle as FO
from tests import loss_grad_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MINI = {"bn_p6p7": dict(norm="BN", top="p6p7"), "none_p6": dict(norm="", top="p6", in_channels=(32, 64, 96, 128)), "frozen_p6p7": dict(norm="FrozenBN", top="p6p7")}


def _mini(name, hw=(8, 12), B=2):
    model = FC.MiniModel(**MINI[name])
    if name == "none_p6":
        hw = (16, 24)
    feats, G, sd = FC.mini_inputs(model, B, hw, dtype=torch.float64)
    return model, feats, G, sd, FO.spec(model)


@pytest.mark.parametrize("name", list(MINI))
def test_restatement_equals_fpn_forward(name):
    """The oracle's forward with the P7 mask from a stored p6, and its own statement of the top-down path, are fpn_forward (float64)."""
    model, feats, G, sd, sp = _mini(name)
    ref = O.fpn_forward(sd, feats, sp[0], sp[1], top_block=sp[2])
    ours, stored = FO.forward(sd, feats, sp), FO.stored_activations(sd, feats, sp)
    assert list(ours) == list(ref)
    st = FO.stages_of(sp)
    for k in ref:
        tol = 1e-13 * max(1.0, float(ref[k].abs().max()))
        assert float((ours[k] - ref[k]).abs().max()) <= tol and float((stored["p"][int(k[1:])] - ref[k]).abs().max()) <= tol, k
    if sp[2] == "p6p7":  # a stored p6 of other signs changes p7 and nothing else
        flipped = FO.forward(sd, feats, sp, p6_stored=-ref[f"p{st[-1] + 1}"])
        assert float((flipped[f"p{st[-1] + 2}"] - ref[f"p{st[-1] + 2}"]).abs().max()) > 1e-3
        assert all(torch.equal(flipped[k], ours[k]) for k in ref if k != f"p{st[-1] + 2}")


@pytest.mark.parametrize("name", list(MINI))
def test_oracle_matches_finite_differences(name):
    """d / d theta of sum_k <G_k, p_k> by float64 central differences of fpn_forward, for every parameter family and the backbone
    features; no p6 entry lies within the step of the kink, both signs occur."""
    model, feats, G, sd, sp = _mini(name)
    leaves = FO.fpn_param_names(model)
    ref = O.fpn_forward(sd, feats, sp[0], sp[1], top_block=sp[2])
    if sp[2] == "p6p7":
        p6 = ref[f"p{FO.stages_of(sp)[-1] + 1}"]
        assert float(p6.abs().min()) > 1e-4 and bool((p6 > 0).any()) and bool((p6 < 0).any())
    pg, fg = FO.autograd_grads(sd, feats, sp, G, torch.float64, leaves)
    f = lambda: float(sum((v * G[k]).sum() for k, v in O.fpn_forward(sd, feats, sp[0], sp[1], top_block=sp[2]).items()))
    gen = torch.Generator().manual_seed(9)
    h = 1e-6
    seen = set()
    targets = [(k, sd[k], pg[k]) for k in leaves] + [(f"backbone_{n}", feats[n], fg[f"backbone_{n}"]) for n in feats]
    for k, x, want in targets:
        seen.add("input" if k.startswith("backbone_") else FO.family_of(k))
        for i in torch.randperm(x.numel(), generator=gen)[:3].tolist():
            old = float(x.view(-1)[i])
            x.view(-1)[i] = old + h
            up = f()
            x.view(-1)[i] = old - h
            dn = f()
            x.view(-1)[i] = old
            fd = (up - dn) / (2 * h)
            assert abs(fd - float(want.reshape(-1)[i])) <= 2e-6 * max(1.0, abs(fd)), (k, i, fd, float(want.reshape(-1)[i]))
    assert seen == {"bn_p6p7": {"filter", "bias", "norm_weight", "input"}, "none_p6": {"filter", "bias", "input"},
                    "frozen_p6p7": {"filter", "bias", "input"}}[name]


@pytest.mark.parametrize("name", list(MINI))
def test_chain_oracle_equals_autograd(name):
    """The table of include/dd3d_hip.h, layer by layer on the forward's own stored activations, is autograd through fpn_forward."""
    model, feats, G, sd, sp = _mini(name)
    stored = FO.stored_activations(sd, feats, sp)
    pa, fa = FO.autograd_grads(sd, feats, sp, G, torch.float64, FO.fpn_param_names(model))
    pc, fc, raw = FO.chain_grads(model, stored, feats, G, torch.float64)
    assert sorted(pc) == sorted(pa) == FO.fpn_param_names(model) and sorted(fc) == sorted(fa)
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert all(close(pc[k], pa[k]) for k in pa) and all(close(fc[k], fa[k]) for k in fa)
    # an output the heads do not select has a zero gradient: leaving it out of G is the same as passing zeros
    st = FO.stages_of(sp)
    G0 = {k: (torch.zeros_like(v) if k == f"p{st[0]}" else v) for k, v in G.items()}
    p0, f0, _ = FO.chain_grads(model, stored, feats, G0, torch.float64)
    p1, f1, _ = FO.chain_grads(model, stored, feats, {k: v for k, v in G.items() if k != f"p{st[0]}"}, torch.float64)
    assert all(torch.equal(p0[k], p1[k]) for k in p0) and all(torch.equal(f0[k], f1[k]) for k in f0)


@pytest.mark.parametrize("name", list(MINI))
def test_read_out_formulas_match_autograd_through_fold_norm(name):
    """engine.losses.norm_param_grads on q = sum g and r = sum g * conv gives the gradients of a BN norm's weight and bias, of a norm-less
    convolution's bias, and nothing for FrozenBN -- as autograd through fold_norm's own expression y = (conv + b - mean) * w * rstd + beta."""
    from dd3d_amd.engine.losses import norm_param_grads
    from dd3d_amd.layers import fold_norm
    import torch.nn.functional as F
    model = FC.MiniModel(**MINI[name])
    gen = torch.Generator().manual_seed(4)
    for key in ("fpn_lateral4", "fpn_output3"):
        conv = getattr(model.backbone, key)
        if name == "bn_p6p7":
            conv.bias = torch.nn.Parameter(torch.randn(conv.weight.shape[0], generator=gen) * 0.3)  # a conv bias under a norm
        k = conv.weight.shape[-1]
        x = torch.randn(2, conv.weight.shape[1], 5, 6, generator=gen, dtype=torch.float64)
        g = torch.randn(2, conv.weight.shape[0], 5, 6, generator=gen, dtype=torch.float64)
        norm = conv.norm
        leaves = {}
        if conv.bias is not None:
            leaves["bias"] = conv.bias.detach().double().requires_grad_(True)
        if norm is not None and isinstance(norm.weight, torch.nn.Parameter):
            leaves["norm.weight"], leaves["norm.bias"] = norm.weight.detach().double().requires_grad_(True), norm.bias.detach().double().requires_grad_(True)
        c = F.conv2d(x, conv.weight.detach().double(), leaves.get("bias"), padding=(k - 1) // 2)
        if norm is not None:
            nw = leaves.get("norm.weight", norm.weight.detach().double())
            nb = leaves.get("norm.bias", norm.bias.detach().double())
            c = (c - norm.running_mean.double()[None, :, None, None]) * (nw * torch.rsqrt(norm.running_var.double() + norm.eps))[None, :, None, None] + \
                nb[None, :, None, None]
        if leaves:
            (c * g).sum().backward()
        scale = fold_norm(conv, None)[0]
        res = FO.layer_grads(x, g, conv.weight.detach(), scale, 1, torch.float64)
        got = norm_param_grads(conv, norm, scale.double(), res["q"], res["r"])
        assert set(got) == set(leaves) == {"bn_p6p7": {"bias", "norm.weight", "norm.bias"}, "none_p6": {"bias"}, "frozen_p6p7": set()}[name]
        for kk, v in got.items():
            assert float((v - leaves[kk].grad).abs().max()) <= 1e-6 * max(1.0, float(leaves[kk].grad.abs().max())), (name, key, kk)


def _dry_plan(model, B=1, H=128, W=256, **kw):
    from dd3d_amd.engine.losses import LossPlan
    return LossPlan(model, B, H, W, device="cpu", dry_run=True, **kw)


@pytest.mark.parametrize("name", list(FC.CONFIGS))
def test_dry_run_plan_ops_handovers_and_keys(name):
    exp, over = FC.CONFIGS[name]
    model = GC.cpu_model(exp, over)
    fpn = model.backbone
    with_t, plan = _dry_plan(model, tower_grads=True), _dry_plan(model, fpn_grads=True)
    assert plan.with_fpn_grads and plan.keep_tower_outputs and plan.pred_grads and plan.grads and not with_t.with_fpn_grads
    stages, two = list(fpn.stages), fpn.top_block.num_levels == 2
    tail = (["top_block.p7"] if two else []) + ["top_block.p6", "outputs"] + [f"lateral{s}" for s in reversed(stages)]
    base = [op.name for op in with_t.ops]
    assert [op.name for op in plan.ops] == base + ["fpn_grads." + t for t in tail] and base[-1].startswith("tower_grads.")
    assert list(plan.fpn_layers) == tail and all(op.branch == 0 for op in plan.ops[-len(tail):])  # one graph on the main stream
    assert sorted(plan.bufs) == sorted(with_t.bufs)  # the forward keeps its buffers; nothing had to be pinned
    assert plan.fpn_pinned == []
    s5 = stages[-1]
    want_reads = [plan.bottom_up[n].buf.name for n in fpn.in_features] + [f"fpn_lateral{s}" for s in stages] + [f"p{s5}"] + ([f"p{s5 + 1}"] if two else [])
    assert plan.fpn_reads == want_reads and len(set(want_reads)) == len(want_reads) and all(n in plan.bufs for n in want_reads)
    L = plan.fpn_layers
    same = lambda a, b: a.data_ptr() == b.data_ptr()
    sel = list(model.in_features)
    G = lambda n: plan.feature_grads[sel.index(n)]
    # G -> D: the top-block chain ends in D of the coarsest stage; D -> T: the output convolutions; T -> dF: the laterals
    if two:
        assert same(L["top_block.p7"].keep[0][0], G(f"p{s5 + 2}")) and same(L["top_block.p7"].keep[3][0], G(f"p{s5 + 1}"))
        assert same(L["top_block.p6"].keep[0][0], L["top_block.p7"].da[0])
        a7 = L["top_block.p7"].args
        assert a7.in_relu == 1 and a7.stride == 2 and a7.ksize == 3 and a7.mask[0] == a7.x[0]  # the mask is the STORED p6 the filter gradient reads
    else:
        assert same(L["top_block.p6"].keep[0][0], G(f"p{s5 + 1}"))
    assert same(L["top_block.p6"].keep[3][0], G(f"p{s5}")) and L["top_block.p6"].args.in_relu == 0 and L["top_block.p6"].keep[4] is None
    out = L["outputs"]
    assert out.L == len(stages) and same(out.keep[0][-1], L["top_block.p6"].da[0]) and all(same(out.keep[0][i], G(f"p{s}")) for i, s in enumerate(stages[:-1]))
    assert out.keep[4] == [None] + ["prev"] * (len(stages) - 1) and out.args.pool[0] is None
    assert all(out.args.pool[i] == out.da[i - 1].data_ptr() and (out.args.pool_H[i], out.args.pool_W[i]) == (2 * out.args.H[i], 2 * out.args.W[i])
               for i in range(1, len(stages)))
    assert len({out.args.w[i] for i in range(len(stages))}) == len(stages)  # a filter per stage
    for i, s in enumerate(stages):
        lat = L[f"lateral{s}"]
        assert same(lat.keep[0][0], out.da[i]) and lat.ksize == 1 and lat.Cin == plan.bottom_up[fpn.in_features[i]].C
    assert all(same(lay.part, plan.tower_slab[0]) for lay in L.values()) and all(same(lay.part, plan.tower_slab[0]) for lay in plan.tower_layers.values())
    assert all(lay.part.numel() >= lay.n_slices * lay.Cout * lay.ksize**2 * lay.Cin for lay in L.values())
    feats, params = plan.fpn_grads()
    named = dict(model.named_parameters())
    shapes = fpn.bottom_up.output_shape()
    assert list(feats) == [f"backbone_{n}" for n in reversed(fpn.in_features)]
    assert all(feats[f"backbone_{n}"].shape == (1, shapes[n].channels, plan.bottom_up[n].H, plan.bottom_up[n].W) for n in fpn.in_features)
    assert sorted(params) == FO.fpn_param_names(model) and all(params[k].shape == named[k].shape and params[k].dtype == torch.float32 for k in params)
    has = lambda k: k in params
    assert has(f"backbone.fpn_lateral{s5}.weight") and has(f"backbone.fpn_output{stages[0]}.weight") and has("backbone.top_block.p6.bias")
    assert has("backbone.top_block.p7.weight") == two
    assert has("backbone.fpn_lateral4.bias") == has("backbone.fpn_output4.bias") == (name == "fpn_no_norm")
    assert has("backbone.fpn_lateral4.norm.weight") == has("backbone.fpn_output4.norm.bias") == (name == "fpn_bn")
    assert not any(k in params for k in with_t.tower_grads()[1]) and not any(k in params for k in with_t.predictor_grads()[1])
    with pytest.raises(RuntimeError, match="fpn_grads"):
        with_t.fpn_grads()


def test_unselected_fpn_outputs_get_a_zero_gradient():
    model = GC.cpu_model("dd3d_kitti_dla34", {"DD3D": {"IN_FEATURES": ["p3", "p4", "p5", "p6"], "SIZES_OF_INTEREST": [64, 128, 256]}})
    plan = _dry_plan(model, fpn_grads=True)
    g7 = plan.fpn_layers["top_block.p7"].keep[0][0]
    assert float(g7.abs().max()) == 0.0 and all(g7.data_ptr() != t.data_ptr() for t in plan.feature_grads)
    assert plan.fpn_layers["top_block.p7"].keep[3][0].data_ptr() == plan.feature_grads[3].data_ptr()


def test_other_plans_are_unchanged():
    """A default plan and a tower_grads plan: the op list and the buffers of before (the tower tests pin them in detail)."""
    model = GC.cpu_model("dd3d_kitti_dla34")
    plain, with_t, with_f = _dry_plan(model), _dry_plan(model, tower_grads=True), _dry_plan(model, fpn_grads=True)
    names = [op.name for op in plain.ops]
    assert not any("grads" in n for n in names) and not hasattr(plain, "fpn_layers") and not hasattr(with_t, "fpn_layers")
    tn = [op.name for op in with_t.ops]
    assert tn[:len(names)] == names and not any(n.startswith("fpn_grads") for n in tn) and tn[-1] == "tower_grads.box3d.0"
    assert [op.name for op in with_f.ops][:len(tn)] == tn
    from dd3d_amd import hip
    level_hw = [(f.H, f.W) for f in with_t.features]
    assert with_t.tower_slab[0].numel() == hip.tower_grad_slices(1, level_hw, 256, 256) * 256 * 9 * 256  # the towers' own size
    assert with_f.tower_slab[0].numel() >= with_t.tower_slab[0].numel()


def test_slice_count_mirror():
    from dd3d_amd import hip
    assert hip.fpn_grad_slices(1, [(1, 1)], 32, 32, 3, 2) == 1 and hip.fpn_grad_slices(1, [(30, 70)], 128, 256, 1, 1) == 15
    assert hip.fpn_grad_slices(2, [(12, 40)], 64, 64, 3, 2) == 3 and hip.fpn_grad_slices(3, [(100, 64)], 256, 256, 3, 1) == 60
    assert hip.fpn_grad_slices(1, [(48, 160), (24, 80), (12, 40)], 256, 256, 3, 1) == 36  # the largest level's count
    big = hip.fpn_grad_slices(6, [(112, 200)], 128, 256, 1, 1)
    assert big == 672 and big * 256 * 128 * 4 <= hip.FG_SLAB_BYTES


def test_fpn_grad_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    cls = hip.FpnGradArgs
    names = [f[0] for f in cls._fields_]
    assert names == ["x", "g", "w", "scale", "mask", "add", "pool", "da", "part", "qpart", "dw_level", "dw", "q", "r", "H", "W", "pool_H", "pool_W",
                     "num_levels", "B", "Cin", "Cout", "g_pitch", "ksize", "stride", "in_relu", "x_mode", "x_pitch", "mask_mode", "mask_pitch", "n_slices",
                     "dgrad_rows", "x_plane_scale", "mask_plane_scale"]
    out = (C.c_int64 * 40)()
    n = hiplib.dd3d_fpn_grad_layout(out, 40)
    assert n == len(names) + 1 and out[0] == C.sizeof(cls)
    assert [out[i + 1] for i in range(len(names))] == [getattr(cls, f).offset for f in names] and out[n] == -1
    assert hiplib.dd3d_fpn_grad_layout(out, 8) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_fpn_grad_layout")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(dd3d_fpn_grad_args));', '  printf("maxcin %d\\n", DD3D_FG_MAX_CIN);', '  printf("maxcout %d\\n", DD3D_FG_MAX_COUT);',
             '  printf("unit %d\\n", DD3D_FG_UNIT);', '  printf("minunits %d\\n", DD3D_FG_MIN_UNITS_PER_SLICE);',
             '  printf("slab %lld\\n", (long long)DD3D_FG_SLAB_BYTES);', '  printf("tiles %d\\n", DD3D_FG_MIN_TILES);']
    lines += [f'  printf("{f} %zu\\n", offsetof(dd3d_fpn_grad_args, {f}));' for f in names] + ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) and int(got["maxcin"]) == hip.FG_MAX_CIN and int(got["maxcout"]) == hip.FG_MAX_COUT
    assert int(got["unit"]) == hip.FG_UNIT and int(got["minunits"]) == hip.FG_MIN_UNITS_PER_SLICE
    assert int(got["slab"]) == hip.FG_SLAB_BYTES and int(got["tiles"]) == hip.FG_MIN_TILES
    for f in names:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert all(e in hip.EXPORTS for e in ("dd3d_fpn_wgrad", "dd3d_fpn_dgrad", "dd3d_fpn_grad_slices", "dd3d_fpn_grad_layout"))
