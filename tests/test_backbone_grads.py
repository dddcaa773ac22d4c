"""DLA-34 backbone backward without a GPU: the oracle's two statements against each other and against central differences, the pool
oracle against torch autograd with constructed ties, the norm read-out, the dry-run plans (op order, hand-overs, key sets, reads, slab),
the other plans unchanged, the struct layouts against the header compiled as C, the unsupported models."""
import ctypes as C
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import backbone_grad_cases as BC
from tests import backbone_grad_oracle as BO
from tests import loss_grad_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PFX = "backbone.bottom_up."


@pytest.mark.parametrize("norm", ["BN", "FrozenBN", ""])
def test_chain_on_own_activations_equals_autograd(norm):
    """The table of include/dd3d_hip.h, call by call on the float64 forward's own stored activations, is torch autograd through the
    oracle's tree functions to float64 rounding: every parameter of level2 .. level5 and the gradient at level1."""
    dla = BC.mini_dla(norm)
    level1, G = BC.mini_inputs(dla, 2, (16, 32), dtype=torch.float64)
    S = BO.stored_activations(dla, level1)
    outs = BO.forward(dla, BO.state(dla, torch.float64), level1)
    for k, key in (("level2", "level2.out"), ("level3", "level3.tree2.out"), ("level4", "level4.tree2.out"), ("level5", "level5.out")):
        assert float((outs[k] - S[key]).abs().max()) <= 1e-12  # the restated forward is the oracle's
    pa, ga = BO.autograd_grads(dla, level1, G, torch.float64)
    pc, gc, raw = BO.chain_grads(dla, S, G, torch.float64)
    assert sorted(pc) == BO.param_names(dla)
    assert float((ga - gc).abs().max()) <= 1e-12 * max(1.0, float(ga.abs().max())) and float(ga.abs().max()) > 0.0
    for k in pc:
        ref = pa[k[len(PFX):]]
        assert pc[k].shape == ref.shape and float((pc[k] - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), k
    kinds = {BO.family_of(k) for k in pc}
    assert kinds == {"BN": {"filter", "norm_weight", "bias"}, "FrozenBN": {"filter"}, "": {"filter", "bias"}}[norm]
    assert [k for k in raw if k.endswith(".pool")] == ["level5.pool", "level4.tree1.pool", "level3.tree1.pool", "level2.pool"]


def test_dla34_chain_equals_autograd():
    """The same on the real DLA-34 shape (channels 16 .. 512, the 448- and 896-channel roots, the 1280-channel level5 root)."""
    from dd3d_amd.modeling.dla import DLA
    dla = BC.randomize(DLA([1, 1, 1, 2, 2, 1], [16, 32, 64, 128, 256, 512], out_features=["level3", "level4", "level5"], norm="BN"), 3).eval()
    level1, G = BC.mini_inputs(dla, 1, (16, 16), dtype=torch.float64)
    S = BO.stored_activations(dla, level1)
    assert S["level3.cat"].shape[1] == 448 and S["level4.cat"].shape[1] == 896 and S["level5.cat"].shape[1] == 1280
    pa, ga = BO.autograd_grads(dla, level1, G, torch.float64)
    pc, gc, _ = BO.chain_grads(dla, S, G, torch.float64)
    assert float((ga - gc).abs().max()) <= 1e-12 * max(1.0, float(ga.abs().max()))
    assert all(float((pc[k] - pa[k[len(PFX):]]).abs().max()) <= 1e-12 * max(1.0, float(pa[k[len(PFX):]].abs().max())) for k in pc)


@pytest.mark.parametrize("norm", ["BN", ""])
def test_central_differences_per_family(norm):
    """d sum <G, outputs> / d theta by central differences in float64, a few entries per family: filter, bias, norm weight, input."""
    dla = BC.mini_dla(norm)
    level1, G = BC.mini_inputs(dla, 1, (16, 16), dtype=torch.float64)
    level1 = level1 + 0.05  # away from the clamp: the difference quotient must not cross a ReLU kink of level1 itself
    S = BO.stored_activations(dla, level1)
    pc, gc, _ = BO.chain_grads(dla, S, G, torch.float64)

    def total(sd, x):
        outs = BO.forward(dla, sd, x)
        return float(sum((outs[k] * G[k]).sum() for k in G))

    sd = BO.state(dla, torch.float64)
    gen = torch.Generator().manual_seed(8)
    picks = {"filter": ["level2.tree1.conv1.weight", "level4.tree1.project.weight", "level5.root.conv.weight",
                        "level3.tree2.root.conv.weight", "level3.tree1.tree2.conv2.weight"]}
    if norm == "BN":
        picks["norm_weight"] = ["level2.project.norm.weight", "level4.tree2.tree1.conv1.norm.weight"]
        picks["bias"] = ["level3.tree1.root.conv.norm.bias", "level5.tree2.conv2.norm.bias"]
    else:
        picks["bias"] = ["level2.project.bias", "level4.tree2.tree1.conv1.bias", "level5.root.conv.bias"]
    h = 1e-6
    for fam, names in picks.items():
        for name in names:
            flat = sd[name].view(-1)
            for i in torch.randint(0, flat.numel(), (3, ), generator=gen).tolist():
                old = float(flat[i])
                flat[i] = old + h
                up = total(sd, level1)
                flat[i] = old - h
                dn = total(sd, level1)
                flat[i] = old
                got, fd = float(pc[PFX + name].reshape(-1)[i]), (up - dn) / (2 * h)
                assert abs(got - fd) <= 1e-5 * max(1.0, abs(fd)), (fam, name, i, got, fd)
    flat = level1.view(-1)
    for i in torch.randint(0, flat.numel(), (4, ), generator=gen).tolist():
        old = float(flat[i])
        flat[i] = old + h
        up = total(sd, level1)
        flat[i] = old - h
        dn = total(sd, level1)
        flat[i] = old
        got, fd = float(gc.reshape(-1)[i]), (up - dn) / (2 * h)
        assert abs(got - fd) <= 1e-5 * max(1.0, abs(fd)), ("input", i, got, fd)


@pytest.mark.parametrize("kind", ["random", "equal", "two_max", "relu"])
def test_pool_oracle_is_torch_autograd_with_ties(kind):
    """torch's CPU max_pool2d backward sends a window's gradient to its FIRST maximum in the order (0,0), (0,1), (1,0), (1,1): confirmed
    here on constructed ties, in float32 and float64, and that is the oracle's (and the kernel's) rule."""
    for dtype in (torch.float32, torch.float64):
        x = BC.pool_input(kind, 2, 32, (4, 6), seed=3).to(dtype).requires_grad_(True)
        g = torch.randn(2, 32, 2, 3, generator=torch.Generator().manual_seed(4)).to(dtype)
        (F.max_pool2d(x, 2, 2) * g).sum().backward()
        assert torch.equal(BO.pool_backward(x.detach(), g, dtype), x.grad), (kind, dtype)
    x = BC.pool_input("equal", 1, 32, (2, 2))
    got = BO.pool_backward(x, torch.ones(1, 32, 1, 1), torch.float32)
    assert bool((got[:, :, 0, 0] == 1).all()) and float(got.sum()) == 32.0
    x = BC.pool_input("two_max", 1, 32, (2, 2))
    got = BO.pool_backward(x, torch.ones(1, 32, 1, 1), torch.float32)
    assert bool((got[:, :, 0, 1] == 1).all()) and float(got.sum()) == 32.0
    add = torch.randn(1, 32, 2, 2)
    assert torch.equal(BO.pool_backward(x, torch.ones(1, 32, 1, 1), torch.float32, add=add), add + got)


@pytest.mark.parametrize("norm", ["BN", "FrozenBN", ""])
def test_read_out_per_norm(norm):
    """engine.losses.norm_param_grads on the call's q and r: weight and bias on running statistics for BN, the conv bias without a norm,
    nothing for FrozenBN -- against autograd through the convolution's own folded expression."""
    from dd3d_amd.engine.losses import norm_param_grads
    from dd3d_amd.layers import fold_norm
    dla = BC.mini_dla(norm)
    gen = torch.Generator().manual_seed(4)
    for conv in (dla.level2.project, dla.level4.tree1.tree1.conv1, dla.level5.root.conv):
        k, s = conv.weight.shape[-1], conv.stride
        x = torch.randn(2, conv.weight.shape[1], 6, 8, generator=gen, dtype=torch.float64)
        g = torch.randn(2, conv.weight.shape[0], 6 // s, 8 // s, generator=gen, dtype=torch.float64)
        y = torch.randn(g.shape, generator=gen, dtype=torch.float64)
        n = conv.norm
        leaves = {}
        if conv.bias is not None:
            leaves["bias"] = conv.bias.detach().double().requires_grad_(True)
        if n is not None and isinstance(n.weight, torch.nn.Parameter):
            leaves["norm.weight"], leaves["norm.bias"] = n.weight.detach().double().requires_grad_(True), n.bias.detach().double().requires_grad_(True)
        c = F.conv2d(x, conv.weight.detach().double(), leaves.get("bias"), stride=s, padding=(k - 1) // 2)
        if n is not None:
            nw, nb = leaves.get("norm.weight", n.weight.detach().double()), leaves.get("norm.bias", n.bias.detach().double())
            c = (c - n.running_mean.double()[None, :, None, None]) * (nw * torch.rsqrt(n.running_var.double() + n.eps))[None, :, None, None] + nb[None, :, None, None]
        if leaves:
            (c * g * (y > 0)).sum().backward()
        scale = fold_norm(conv, None)[0]
        res = BO.layer_grads(x, y, g, conv.weight.detach(), scale, s, torch.float64)
        got = norm_param_grads(conv, n, scale.double(), res["q"], res["r"])
        assert set(got) == set(leaves) == {"BN": {"norm.weight", "norm.bias"}, "": {"bias"}, "FrozenBN": set()}[norm]
        for kk, v in got.items():
            # (norm_param_grads takes rstd and the centre from the module's float32 statistics: float32 rounding of those, as in the FPN's test)
            assert float((v - leaves[kk].grad).abs().max()) <= 1e-6 * max(1.0, float(leaves[kk].grad.abs().max())), (norm, kk)


def _dry_plan(model, B=1, H=128, W=256, **kw):
    from dd3d_amd.engine.losses import LossPlan
    return LossPlan(model, B, H, W, device="cpu", dry_run=True, **kw)


TREE_CALLS = ["root", "tree2.conv2", "tree2.conv1", "tree1.conv2", "project", "tree1.conv1", "pool"]
INNER2_CALLS = ["root", "tree2.conv2", "tree2.conv1", "tree1.conv2", "tree1.conv1"]
WANT_OPS = [f"level5.{c}" for c in TREE_CALLS] + [f"level4.tree2.{c}" for c in INNER2_CALLS] + [f"level4.tree1.{c}" for c in TREE_CALLS] + \
    [f"level3.tree2.{c}" for c in INNER2_CALLS] + [f"level3.tree1.{c}" for c in TREE_CALLS] + [f"level2.{c}" for c in TREE_CALLS]


@pytest.mark.parametrize("name", list(BC.CONFIGS))
def test_dry_run_plan_ops_handovers_and_keys(name):
    from dd3d_amd import hip
    exp, over = BC.CONFIGS[name]
    model = GC.cpu_model(exp, over)
    with_f, plan = _dry_plan(model, fpn_grads=True), _dry_plan(model, backbone_grads=True)
    assert plan.with_backbone_grads and plan.with_fpn_grads and plan.keep_tower_outputs and not with_f.with_backbone_grads
    base = [op.name for op in with_f.ops]
    assert [op.name for op in plan.ops] == base + ["backbone_grads." + t for t in WANT_OPS] and base[-1] == "fpn_grads.lateral3"
    assert list(plan.backbone_layers) == WANT_OPS and all(op.branch == 0 for op in plan.ops[len(base):])  # one graph on the main stream
    assert sorted(plan.bufs) == sorted(with_f.bufs)  # the forward keeps its buffers
    L = plan.backbone_layers
    same = lambda a, b: a is not None and b is not None and a.data_ptr() == b.data_ptr() and tuple(a.shape) == tuple(b.shape)
    F_ = {n: plan.backbone_feature_grads[n][0] for n in ("level3", "level4", "level5")}
    g_of, add_of, res_of = (lambda k: L[k].keep[0]), (lambda k: L[k].keep[3]), (lambda k: L[k].keep[4])

    def depth1(p, G_out, oc, ic, root_dim, x_add, bottom_add):
        """the hand-overs inside a stride-2 depth-1 tree `p` whose root reads root_dim channels"""
        D = L[p + ".root"].da
        assert same(g_of(p + ".root"), G_out) and D.shape[-1] == root_dim and L[p + ".root"].Cin == root_dim
        assert same(g_of(p + ".tree2.conv2"), D[..., :oc]) and L[p + ".tree2.conv2"].args.g_pitch == root_dim
        assert same(g_of(p + ".tree2.conv1"), L[p + ".tree2.conv2"].da)
        assert same(add_of(p + ".tree2.conv1"), D[..., oc:2 * oc]) and same(res_of(p + ".tree2.conv1")[0], D[..., :oc])  # x1: root slice, tree2's residual
        assert L[p + ".tree2.conv1"].src["res_y"] == L[p + ".tree2.conv2"].src["y"]  # masked by the stored x2
        assert same(g_of(p + ".tree1.conv2"), L[p + ".tree2.conv1"].da) and same(g_of(p + ".project"), L[p + ".tree2.conv1"].da)
        assert L[p + ".project"].src["y"] == L[p + ".tree1.conv2"].src["y"]  # the residual's gradient: G_x1 masked by the stored x1
        assert (add_of(p + ".project") is None) if bottom_add is None else same(add_of(p + ".project"), bottom_add)
        assert same(g_of(p + ".tree1.conv1"), L[p + ".tree1.conv2"].da) and L[p + ".tree1.conv1"].stride == 2
        assert (add_of(p + ".tree1.conv1") is None) if x_add is None else same(add_of(p + ".tree1.conv1"), x_add)
        pool = L[p + ".pool"]
        assert same(pool.keep[0], L[p + ".project"].da) and same(pool.keep[1], L[p + ".tree1.conv1"].da) and pool.keep[2] is None and pool.C == ic
        assert pool.src["x"] == L[p + ".tree1.conv1"].src["x"]
        return pool.da

    def depth2(p, G_out, oc, ic, x_add):
        """level3 / level4: tree2 (root over [x2 | x1 | bottom | t1]) first, then tree1, which shares the pooled bottom"""
        q, root_dim = p + ".tree2", 3 * oc + ic
        D = L[q + ".root"].da
        assert same(g_of(q + ".root"), G_out) and D.shape[-1] == root_dim and L[q + ".root"].src["x"] == (p + ".cat", 0, root_dim)
        assert same(g_of(q + ".tree2.conv2"), D[..., :oc]) and same(add_of(q + ".tree2.conv1"), D[..., oc:2 * oc]) and same(res_of(q + ".tree2.conv1")[0], D[..., :oc])
        assert same(g_of(q + ".tree1.conv2"), L[q + ".tree2.conv1"].da)
        c1 = L[q + ".tree1.conv1"]  # stride 1, bottom = x = t1: root slice, tree1's residual, conv1's input gradient
        assert c1.stride == 1 and same(c1.keep[3], D[..., 2 * oc + ic:]) and same(c1.keep[4][0], L[q + ".tree2.conv1"].da)
        assert c1.src["x"] == (p + ".cat", 2 * oc + ic, oc) and c1.src["res_y"] == (p + ".cat", oc, oc)
        r = p + ".tree1"
        assert L[r + ".root"].src["y"] == (p + ".cat", 2 * oc + ic, oc) and L[r + ".project"].src["x"] == (p + ".cat", 2 * oc, ic)  # t1; the shared bottom
        return depth1(r, c1.da, oc, ic, 2 * oc, x_add, D[..., 2 * oc:2 * oc + ic])

    g = depth1("level5", F_["level5"], 512, 256, 1280, F_["level4"], L["level5.root"].da[..., 1024:1280])
    assert L["level5.project"].src["x"] == ("level5.cat", 1024, 256)
    g = depth2("level4", g, 256, 128, F_["level3"])
    assert L["level4.tree2.root"].Cin == 896
    g = depth2("level3", g, 128, 64, None)
    assert L["level3.tree2.root"].Cin == 448
    g = depth1("level2", g, 64, 32, 128, None, None)
    assert L["level2.project"].src["x"] == ("level2.bottom", 0, 32) and L["level2.tree1.conv1"].src["x"] == ("level1", 0, 32)
    assert same(g, plan.level1_grad) and tuple(g.shape) == (1, 64, 128, 32)
    # exact key sets
    ff, fp = with_f.fpn_grads()
    feats, params = plan.backbone_grads()
    assert list(feats) == ["backbone_level1"] and feats["backbone_level1"].shape == (1, 32, 64, 128) and feats["backbone_level1"].dtype == torch.float32
    named = dict(model.named_parameters())
    assert sorted(params) == BO.param_names(model.backbone.bottom_up) and len(params) == 34  # FrozenBN owns nothing: the 34 filters
    assert all(params[k].shape == named[k].shape and params[k].dtype == torch.float32 for k in params)
    assert list(plan.fpn_grads()[0]) == list(ff) and sorted(plan.fpn_grads()[1]) == sorted(fp) and not any(k in fp for k in params)
    # reads: every stored buffer once, each still the buffer of its name
    assert len(set(plan.backbone_reads)) == len(plan.backbone_reads) == 24 and all(n in plan.bufs for n in plan.backbone_reads)
    assert set(plan.backbone_reads) == {"level1.0", "level2.bottom"} | {f"level{n}.{s}" for n in (2, 5) for s in ("cat", "out", "tree1.mid", "tree2.mid")} | \
        {f"level{n}.{s}" for n in (3, 4) for s in ("cat", "tree2.out", "tree1.cat", "tree1.tree1.mid", "tree1.tree2.mid", "tree2.tree1.mid", "tree2.tree2.mid")}
    # the slab: one for every call of the plan, sized for the largest user, within the budget
    part, qpart = plan.tower_slab
    convs = [lay for k, lay in L.items() if not k.endswith(".pool")]
    assert all(lay.part.data_ptr() == part.data_ptr() for lay in convs + list(plan.fpn_layers.values()) + list(plan.tower_layers.values()))
    assert all(part.numel() >= lay.n_slices * lay.Cout * lay.ksize**2 * lay.Cin and qpart.numel() >= lay.n_slices * lay.Cout for lay in convs)
    assert 4 * part.numel() <= hip.TG_SLAB_BYTES + 4 * 9 * 256 * 256 * len(plan.features)  # (the towers' rule rounds up once per pyramid level)
    with pytest.raises(RuntimeError, match="backbone_grads"):
        with_f.backbone_grads()


def test_slab_budget_at_the_measured_sizes():
    """1 and 4 x 384 x 1280 KITTI and 6 x 896 x 1600 nuScenes: the largest weight-gradient call's partials stay within DD3D_TG_SLAB_BYTES."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import dla_slab_words
    dla = GC.cpu_model("dd3d_kitti_dla34").backbone.bottom_up
    for B, H, W in ((1, 384, 1280), (4, 384, 1280), (6, 896, 1600)):
        rows, qrows = dla_slab_words(B, dla, H // 2, W // 2)
        assert 0 < 4 * rows <= hip.TG_SLAB_BYTES and qrows > 0, (B, H, W, rows)
    assert hip.backbone_grad_slices(1, 12, 40, 512, 512, 3, 1) == 3 and hip.backbone_grad_slices(6, 28, 50, 512, 512, 3, 1) == 17


def test_every_call_shape_of_the_measured_sizes_is_accepted(hiplib):
    """Every convolution of level2 .. level5 at 1 and 4 x 384 x 1280 and at the 6 x 896 x 1600 nuScenes sample (whose level1 tensor has
    2.15 million pixels) goes through the library's own shape check and slice count, which agrees with the Python mirror; the pixel
    limit is DD3D_BG_MAX_PIXELS and nothing smaller."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import _dla_tree_calls
    dla = GC.cpu_model("dd3d_kitti_dla34").backbone.bottom_up
    bare = hip.BackboneGradArgs()
    for B, Hp, Wp in ((1, 384, 1280), (4, 384, 1280), (6, 896, 1600)):
        H, W, n_calls = Hp // 2, Wp // 2, 0
        for lvl in range(2, 6):
            for k, s, h, w_, ci, co in _dla_tree_calls(getattr(dla, f"level{lvl}"), H, W):
                bare.B, bare.H, bare.W, bare.Cin, bare.Cout, bare.ksize, bare.stride = B, h, w_, ci, co, k, s
                n = hiplib.dd3d_backbone_grad_slices(C.byref(bare))
                assert n >= 1 and n == hip.backbone_grad_slices(B, h, w_, ci, co, k, s), (B, Hp, Wp, lvl, k, s, h, w_, ci, co, hiplib.dd3d_last_error())
                assert B * h * w_ <= hip.BG_MAX_PIXELS
                n_calls += 1
            H, W = H // 2, W // 2
        assert n_calls == 34
    assert 6 * 448 * 800 > (1 << 31) // 2048  # (the towers' and the FPN's pixel limit would have refused level2.tree1.conv1 here)
    bare.B, bare.H, bare.W, bare.Cin, bare.Cout, bare.ksize, bare.stride = 1, 8192, 8192, 32, 64, 3, 2
    assert hiplib.dd3d_backbone_grad_slices(C.byref(bare)) >= 1  # exactly DD3D_BG_MAX_PIXELS
    bare.B = 2
    assert hiplib.dd3d_backbone_grad_slices(C.byref(bare)) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_backbone_grad_slices")


def test_other_plans_are_unchanged():
    model = GC.cpu_model("dd3d_kitti_dla34")
    plain, with_f, with_b = _dry_plan(model), _dry_plan(model, fpn_grads=True), _dry_plan(model, backbone_grads=True)
    names = [op.name for op in plain.ops]
    assert not any("grads" in n for n in names) and not hasattr(plain, "backbone_layers") and not hasattr(with_f, "backbone_layers")
    fn = [op.name for op in with_f.ops]
    assert fn[:len(names)] == names and not any(n.startswith("backbone_grads") for n in fn) and fn[-1] == "fpn_grads.lateral3"
    assert [op.name for op in with_b.ops][:len(fn)] == fn
    assert not with_f.with_backbone_grads and with_f.with_fpn_grads and not _dry_plan(model, tower_grads=True).with_fpn_grads
    assert with_b.tower_slab[0].numel() >= with_f.tower_slab[0].numel()
    assert [lay.n_slices for lay in with_b.fpn_layers.values()] == [lay.n_slices for lay in with_f.fpn_layers.values()]


def test_backbone_grad_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    cls, pcls = hip.BackboneGradArgs, hip.PoolGradArgs
    names, pnames = [f[0] for f in cls._fields_], [f[0] for f in pcls._fields_]
    assert names == ["x", "y", "g", "w", "scale", "add", "res_g", "res_y", "da", "part", "qpart", "dw_level", "dw", "q", "r", "B", "H", "W", "Cin", "Cout", "ksize",
                     "stride", "g_pitch", "add_pitch", "res_pitch", "da_pitch", "x_mode", "x_pitch", "y_mode", "y_pitch", "res_y_mode", "res_y_pitch", "n_slices",
                     "dgrad_rows", "dgrad_group", "x_plane_scale", "y_plane_scale", "res_y_plane_scale"]
    assert pnames == ["x", "g", "res_g", "res_y", "add", "da", "B", "H", "W", "C", "x_mode", "x_pitch", "res_y_mode", "res_y_pitch", "g_pitch", "res_pitch",
                      "add_pitch", "da_pitch", "x_plane_scale", "res_y_plane_scale"]
    out = (C.c_int64 * 64)()
    n = hiplib.dd3d_backbone_grad_layout(out, 64)
    assert n == len(names) + len(pnames) + 2 and out[0] == C.sizeof(cls) and out[len(names) + 1] == C.sizeof(pcls)
    assert [out[i + 1] for i in range(len(names))] == [getattr(cls, f).offset for f in names]
    assert [out[len(names) + 2 + i] for i in range(len(pnames))] == [getattr(pcls, f).offset for f in pnames] and out[n] == -1
    assert hiplib.dd3d_backbone_grad_layout(out, 8) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_backbone_grad_layout")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(dd3d_backbone_grad_args));', '  printf("psize %zu\\n", sizeof(dd3d_pool_grad_args));',
             '  printf("maxcin %d\\n", DD3D_BG_MAX_CIN);', '  printf("maxcout %d\\n", DD3D_BG_MAX_COUT);', '  printf("unit %d\\n", DD3D_BG_UNIT);',
             '  printf("minunits %d\\n", DD3D_BG_MIN_UNITS_PER_SLICE);', '  printf("slab %lld\\n", (long long)DD3D_TG_SLAB_BYTES);',
             '  printf("tiles %d\\n", DD3D_BG_MIN_TILES);', '  printf("maxpix %ld\\n", (long)DD3D_BG_MAX_PIXELS);']
    lines += [f'  printf("{f} %zu\\n", offsetof(dd3d_backbone_grad_args, {f}));' for f in names]
    lines += [f'  printf("p_{f} %zu\\n", offsetof(dd3d_pool_grad_args, {f}));' for f in pnames] + ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) and int(got["psize"]) == C.sizeof(pcls)
    assert int(got["maxcin"]) == hip.BG_MAX_CIN and int(got["maxcout"]) == hip.BG_MAX_COUT and int(got["unit"]) == hip.BG_UNIT
    assert int(got["minunits"]) == hip.BG_MIN_UNITS_PER_SLICE and int(got["slab"]) == hip.TG_SLAB_BYTES and int(got["tiles"]) == hip.BG_MIN_TILES
    assert int(got["maxpix"]) == hip.BG_MAX_PIXELS
    for f in names:
        assert int(got[f]) == getattr(cls, f).offset, f
    for f in pnames:
        assert int(got["p_" + f]) == getattr(pcls, f).offset, f
    assert all(e in hip.EXPORTS for e in ("dd3d_backbone_wgrad", "dd3d_backbone_dgrad", "dd3d_backbone_grad_slices", "dd3d_maxpool2x2_backward",
                                          "dd3d_backbone_grad_layout"))


def test_unsupported_models_raise_before_anything_is_built():
    from dd3d_amd.engine.losses import check_dla_backward
    v99 = GC.cpu_model("dd3d_kitti_v99")
    with pytest.raises(NotImplementedError, match="V2-99"):
        _dry_plan(v99, backbone_grads=True)
    for variant, word in (("DLA-60", "Bottleneck"), ("DLA-X-60-C", "BottleneckX")):
        m = GC.cpu_model("dd3d_kitti_dla34", {"FE": {"BACKBONE": {"NAME": variant}}})
        with pytest.raises(NotImplementedError, match=word):
            _dry_plan(m, backbone_grads=True)
    model = GC.cpu_model("dd3d_kitti_dla34")
    model.force_generic_dla = True
    with pytest.raises(NotImplementedError, match="force_generic_dla"):
        _dry_plan(model, backbone_grads=True)
    model.force_generic_dla = False
    for math, word in ((2, "bf16x2"), (3, "bf16")):
        model.math = {2: "bf16x2", 3: "bf16"}[math]
        with pytest.raises(NotImplementedError, match=word):
            _dry_plan(model, backbone_grads=True)
    model.math = None
    _dry_plan(model, fpn_grads=True)  # the other plans of these models are not affected
    check_dla_backward(model.backbone.bottom_up, model)
