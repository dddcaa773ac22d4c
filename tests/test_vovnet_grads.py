"""VoVNet-V2 backbone backward without a GPU (engine.LossPlan(vovnet_grads=True), engine.losses.vovnet_backward): the statements of the
3x3 ceil-mode pool backward and of the eSE gate backward (tests/vovnet_grad_oracle.py) against torch autograd, the dry-run plan's calls,
their order and the buffers they bind, the parameter names, the struct layouts against a compiled C program, the unsupported variants."""
import ctypes as C
import os
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import loss_grad_cases as GC
from tests import vovnet_grad_oracle as VG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dry_plan(model, B=1, H=128, W=256, **kw):
    from dd3d_amd.engine.losses import LossPlan
    return LossPlan(model, B, H, W, device="cpu", dry_run=True, **kw)


def pool_input(kind, B, C_, hw, seed=0):
    """The stored input of a 3x3 stride-2 pool.  "random": seeded normals; "negative": all below zero; "relu": rectified normals (windows
    of zeros tie, as the stored activations do); "ties": small integers, so that most windows hold their maximum several times; "equal":
    one value everywhere."""
    gen = torch.Generator().manual_seed(seed)
    h, w = hw
    if kind == "equal":
        return torch.full((B, C_, h, w), 0.75)
    if kind == "ties":
        return torch.randint(0, 3, (B, C_, h, w), generator=gen).float()
    x = torch.randn(B, C_, h, w, generator=gen)
    return torch.relu(x - 0.5) if kind == "relu" else -x.abs() - 0.1 if kind == "negative" else x


# 3x3: one window; 4x5: the last window overhangs (two rows / columns wide); 7x8: odd and even sizes; 9x9: four windows a side.  The
# forward's rule drops a last window that would start outside the map ((Ho - 1) * 2 >= H); without padding that never happens for a 3x3
# stride-2 pool (the last start is 2 * ceil((H - 3) / 2) <= H - 2), which test_pool_output_size_rule_is_torchs pins for H = 3 .. 39.
POOL_SIZES = [(3, 3), (4, 5), (7, 8), (9, 9), (16, 32)]


def test_pool_output_size_rule_is_torchs():
    from dd3d_amd import hip
    for n in range(3, 40):
        want = F.max_pool2d(torch.zeros(1, 1, n, 3), 3, 2, ceil_mode=True).shape[2]
        assert VG.pool3_out(n) == hip.pool3_out(n) == want, n
    assert [VG.pool3_out(n) for n in (3, 4, 5, 7, 8, 9)] == [1, 2, 2, 3, 4, 4]


@pytest.mark.parametrize("kind", ["random", "negative", "relu", "ties", "equal"])
@pytest.mark.parametrize("hw", POOL_SIZES)
def test_pool_backward_restatement_equals_torch_autograd_bit_for_bit(kind, hw):
    """The gather in ascending (oy, ox) with the first maximum in row-major window order IS torch's CPU max_pool2d backward in float32:
    equal bits, ties and all-zero windows included."""
    x = pool_input(kind, 2, 32, hw, seed=7)
    gen = torch.Generator().manual_seed(8)
    g = torch.randn(2, 32, VG.pool3_out(hw[0]), VG.pool3_out(hw[1]), generator=gen)
    leaf = x.clone().requires_grad_(True)
    y = F.max_pool2d(leaf, 3, 2, ceil_mode=True)
    assert y.shape == g.shape
    y.backward(g)
    mine = VG.pool3_backward(x, g, torch.float32)
    assert torch.equal(mine, leaf.grad), (kind, hw)
    add = torch.randn(x.shape, generator=gen)
    with_add = VG.pool3_backward(x, g, torch.float32, add=add)
    # a pixel no window selects keeps `add` bit for bit; the selected ones differ from it
    untouched = leaf.grad == 0
    assert torch.equal(with_add[untouched], add[untouched])


def test_pool_backward_first_maximum_wins_on_constructed_ties():
    x = torch.full((1, 32, 7, 8), 0.75)
    g = torch.arange(1, 1 + 3 * 4, dtype=torch.float32).view(1, 1, 3, 4).expand(1, 32, 3, 4).contiguous()
    da = VG.pool3_backward(x, g)
    want = torch.zeros_like(x)
    want[:, :, 0:6:2, 0:8:2] = g  # the top-left corner of every window
    assert torch.equal(da, want)
    x[:, :, 2, 2] = 1.0  # one pixel shared by four windows: it collects all four gradients in ascending (oy, ox)
    da = VG.pool3_backward(x, g)
    assert torch.equal(da[0, 0, 2, 2], ((g[0, 0, 0, 0] + g[0, 0, 0, 1]) + g[0, 0, 1, 0]) + g[0, 0, 1, 1])


@pytest.mark.parametrize("identity", [False, True])
def test_ese_formulas_against_float64_autograd_of_the_osa_module(identity):
    vov = VG.mini_vovnet()
    sname = "stage2"
    gen = torch.Generator().manual_seed(3)
    mods = list(vov.stage2.named_children())
    k = 1 if identity else 0
    mname, m = mods[k]
    assert m.identity == identity
    from oracle import vovnet_oracle as VO
    from tests import whole_model_grad_oracle as WO
    sd = VG.state(vov, torch.float64)
    xin = (torch.relu(torch.randn(2, m.in_ch, 6, 10, generator=gen))).double().requires_grad_(True)
    with WO.intercepted() as rec:
        out = VO._osa(sd, f"backbone.bottom_up.{sname}.{mname}", mname, xin, len(m.layers), m.identity)
    xt = rec["F"].out[-1]
    xt.retain_grad()
    G = torch.randn(out.shape, generator=gen).double()
    (out * G).sum().backward()
    p = f"backbone.bottom_up.{sname}.{mname}.ese.fc"
    mine = VG.ese_backward(xt.detach(), G, sd[p + ".weight"].detach(), sd[p + ".bias"].detach(), torch.float64)
    z = mine["z"]
    assert float(((z.abs() - 3).abs()).min()) > 1e-3
    assert bool((z <= -3).any()) and bool((z >= 3).any()) and bool(((z > -3) & (z < 3)).any())  # all three regions of the hard sigmoid
    tol = lambda ref: 1e-12 * max(1.0, float(ref.abs().max()))
    assert float((mine["g_xt"] - xt.grad).abs().max()) <= tol(xt.grad)
    assert float((mine["d_fc_w"] - sd[p + ".weight"].grad.reshape(m.concat_ch, m.concat_ch)).abs().max()) <= tol(sd[p + ".weight"].grad)
    assert float((mine["d_fc_b"] - sd[p + ".bias"].grad).abs().max()) <= tol(sd[p + ".bias"].grad)


def _want_ops(vov):
    ops = []
    names = list(vov.stage_names)
    for si in reversed(range(len(names))):
        stage = getattr(vov, names[si])
        for mname, m in reversed(list(stage.named_children())):
            ops += [f"{names[si]}.{mname}.{c}" for c in ["ese", "concat"] + [str(i) for i in reversed(range(1, len(m.layers)))] + (["sum"] if m.identity else []) + ["0"]]
        if stage.has_pool:
            ops.append(names[si] + ".pool")
    return ops + ["stem_3", "stem_2"]


def test_dry_plan_calls_order_and_bound_buffers():
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import EseGrads, Pool3Grads, SumGrads, VovnetConvGrads
    model = GC.cpu_model("dd3d_kitti_v99")
    vov = model.backbone.bottom_up
    plan, with_f = _dry_plan(model, vovnet_grads=True), _dry_plan(model, fpn_grads=True)
    names, fn = [op.name for op in plan.ops], [op.name for op in with_f.ops]
    assert names[:len(fn)] == fn and not any(n.startswith("vovnet_grads") for n in fn)  # the fpn_grads plan, then the new calls alone
    assert names[len(fn):] == ["vovnet_grads." + k for k in _want_ops(vov)] == ["vovnet_grads." + k for k in plan.vovnet_layers]
    assert plan.with_fpn_grads and plan.with_vovnet_grads and not plan.with_backbone_grads and not with_f.with_vovnet_grads
    L = plan.vovnet_layers
    B = 1
    for key, lay in L.items():
        for ref in lay.src.values():
            buf = plan.bufs[ref[0]]
            assert ref[1] % 32 == 0 and ref[1] + ref[2] <= buf.pitch, (key, ref)
        if isinstance(lay, EseGrads):
            xt = plan.bufs[lay.src["xt"][0]]
            assert (lay.H, lay.W, lay.C) == (xt.H, xt.W, xt.pitch) and lay.g_xt.shape == (B, xt.H, xt.W, xt.pitch) and 1 <= lay.rsplit <= hip.EG_MAX_RSPLIT
        elif isinstance(lay, Pool3Grads):
            x = plan.bufs[lay.src["x"][0]]
            assert (lay.H, lay.W, lay.C) == (x.H, x.W, x.pitch) and lay.da.shape == (B, x.H, x.W, x.pitch)
            assert lay.args.add and (lay.Ho, lay.Wo) == (VG.pool3_out(x.H), VG.pool3_out(x.W))  # the FPN's gradient at the stage output is added
        elif isinstance(lay, SumGrads):
            assert key.endswith(".sum") and lay.da.shape == lay.keep[0].shape == lay.keep[1].shape
        else:
            assert isinstance(lay, VovnetConvGrads)
            x, y = plan.bufs[lay.src["x"][0]], plan.bufs[lay.src["y"][0]]
            assert (lay.H, lay.W) == (x.H, x.W) and (lay.Ho, lay.Wo) == (y.H, y.W) and lay.Cin == lay.src["x"][2] and lay.Cout == lay.src["y"][2]
            assert lay.Cin <= hip.VG_MAX_CIN and lay.Cout <= hip.VG_MAX_COUT and lay.da.shape == (B, x.H, x.W, lay.Cin)
            assert lay.args.n_slices == hip.backbone_grad_slices(B, lay.H, lay.W, lay.Cin, lay.Cout, lay.ksize, lay.stride)
    # the module input's three terms: (the concat gradient's slice + G_out under identity, one elementwise launch), then layer 0's own
    first, second, head = L["stage5.OSA5_1.0"], L["stage5.OSA5_3.0"], L["stage5.OSA5_3.sum"]
    assert "stage5.OSA5_1.sum" not in L and first.args.add == L["stage5.OSA5_1.concat"].da.data_ptr() and first.args.add_pitch == 768 + 5 * 224
    assert head.call[:2] == (L["stage5.OSA5_3.concat"].da.data_ptr(), L["stage5.OSA5_3.ese"].args.g) and head.call[3:] == (4 * 8, 1024, 2144, 1024, 1024)
    assert second.args.add == head.da.data_ptr() and second.args.add_pitch == 1024
    widest = L["stage5.OSA5_3.concat"]
    assert (widest.Cin, widest.Cout, widest.ksize) == (2144, 1024, 1) and L["stage5.OSA5_3.4"].Cin == 224 and L["stage5.OSA5_2.0"].Cin == 1024
    # layer i reads D_cat[slice i] + the input gradient of layer i + 1
    l4, l3 = L["stage3.OSA3_2.4"], L["stage3.OSA3_2.3"]
    assert l3.args.g == l4.da.data_ptr() and l4.args.add == L["stage3.OSA3_2.concat"].da[..., 512 + 3 * 160:].data_ptr()
    # the stem: stem_3 is the stride-2 call into the first concat buffer's input slice
    assert (L["stem_3"].stride, L["stem_3"].Cin, L["stem_3"].Cout, L["stem_2"].stride) == (2, 64, 128, 1) and L["stem_3"].src["y"][0] == "stage2.OSA2_1.cat"
    feats, params = plan.vovnet_grads()
    assert list(feats) == ["backbone_stem_1"] and feats["backbone_stem_1"].shape == (1, 64, 64, 128) and feats["backbone_stem_1"].dtype == torch.float32
    assert len(set(plan.vovnet_reads)) == len(plan.vovnet_reads) and all(n in plan.bufs for n in plan.vovnet_reads)
    assert set(plan.vovnet_reads) == {"stem.0", "stem.1", "stage2.out", "stage3.out", "stage4.out"} | \
        {f"{s}.{m}.{t}" for s in vov.stage_names for m, _ in getattr(vov, s).named_children() for t in ("cat", "xt")}
    part, qpart = plan.tower_slab
    convs = [lay for lay in L.values() if isinstance(lay, VovnetConvGrads)]
    assert all(lay.part.data_ptr() == part.data_ptr() for lay in convs + list(plan.fpn_layers.values()) + list(plan.tower_layers.values()))
    assert all(part.numel() >= lay.n_slices * lay.Cout * lay.ksize**2 * lay.Cin and qpart.numel() >= lay.n_slices * lay.Cout for lay in convs)
    with pytest.raises(RuntimeError, match="vovnet_grads"):
        with_f.vovnet_grads()


def test_param_grad_names():
    """param_grads of a dry plan: named_parameters() of backbone.bottom_up minus stem.stem_1/*, each of its parameter's shape."""
    model = GC.cpu_model("dd3d_kitti_v99")
    plan = _dry_plan(model, vovnet_grads=True)
    _, params = plan.vovnet_grads()
    named = dict(model.named_parameters())
    want = VG.vovnet_param_names(model)
    assert sorted(params) == want and len(want) == 130  # 16 modules x (5 layers + concat + fc weight + fc bias) + stem_2 + stem_3
    assert [k for k in named if k.startswith("backbone.bottom_up.") and k not in params] == ["backbone.bottom_up.stem.stem_1/conv.weight"]
    assert all(params[k].shape == named[k].shape and params[k].dtype == torch.float32 for k in params)
    assert not any(k in plan.fpn_grads()[1] for k in params)
    bn = GC.cpu_model("dd3d_kitti_v99", {"FE": {"BACKBONE": {"NORM": "BN"}}})
    _, params = _dry_plan(bn, vovnet_grads=True).vovnet_grads()
    assert sorted(params) == VG.vovnet_param_names(bn) and len(params) == 130 + 2 * (16 * 6 + 2)  # BN: weight and bias of every norm but stem_1's


def test_slab_budget_at_the_measured_sizes():
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import _vovnet_conv_calls, vovnet_slab_words
    vov = GC.cpu_model("dd3d_kitti_v99").backbone.bottom_up
    for B, H, W in ((1, 384, 1280), (4, 384, 1280), (6, 896, 1600)):
        rows, qrows = vovnet_slab_words(B, vov, H // 2, W // 2)
        assert 0 < 4 * rows <= hip.TG_SLAB_BYTES and qrows > 0, (B, H, W, rows)
    calls = _vovnet_conv_calls(vov, 192, 640)
    assert len(calls) == 16 * 6 + 2 and max(c[4] for c in calls) == hip.VG_MAX_CIN and max(c[5] for c in calls) == hip.VG_MAX_COUT
    assert max(c[4] for c in calls if c[0] == 3) == 1024 and sorted({c[5] for c in calls if c[0] == 3}) == [64, 128, 160, 192, 224]


def test_vovnet_grad_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    structs = (("dd3d_ese_grad_args", hip.EseGradArgs), ("dd3d_pool3_grad_args", hip.Pool3GradArgs))
    assert [f[0] for f in hip.EseGradArgs._fields_] == ["xt", "g", "fc_w", "fc_b", "part", "m", "z", "s", "dz", "u", "g_xt", "d_fc_w", "d_fc_b", "B", "HW", "C",
                                                        "rsplit", "xt_mode", "xt_pitch", "g_pitch", "gxt_pitch", "xt_plane_scale", "reserved"]
    assert [f[0] for f in hip.Pool3GradArgs._fields_] == ["x", "g", "add", "da", "B", "H", "W", "C", "x_mode", "x_pitch", "g_pitch", "add_pitch", "da_pitch",
                                                          "x_plane_scale"]
    out = (C.c_int64 * 64)()
    n = hiplib.dd3d_vovnet_grad_layout(out, 64)
    assert n == sum(len(cls._fields_) + 1 for _, cls in structs) and out[n] == -1
    i = 0
    for _, cls in structs:
        assert out[i] == C.sizeof(cls)
        assert [out[i + 1 + j] for j in range(len(cls._fields_))] == [getattr(cls, f[0]).offset for f in cls._fields_]
        i += 1 + len(cls._fields_)
    assert hiplib.dd3d_vovnet_grad_layout(out, 8) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_vovnet_grad_layout")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {',
             '  printf("maxcin %d\\n", DD3D_VG_MAX_CIN);', '  printf("maxcout %d\\n", DD3D_VG_MAX_COUT);', '  printf("rsplit %d\\n", DD3D_EG_MAX_RSPLIT);']
    for cname, cls in structs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f[0]} %zu\\n", offsetof({cname}, {f[0]}));' for f in cls._fields_]
    lines += ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert (int(got["maxcin"]), int(got["maxcout"]), int(got["rsplit"])) == (hip.VG_MAX_CIN, hip.VG_MAX_COUT, hip.EG_MAX_RSPLIT)
    for cname, cls in structs:
        assert int(got[cname]) == C.sizeof(cls)
        for f in cls._fields_:
            assert int(got[f"{cname}.{f[0]}"]) == getattr(cls, f[0]).offset, (cname, f[0])
    assert all(e in hip.EXPORTS for e in ("dd3d_vovnet_conv_wgrad", "dd3d_vovnet_conv_dgrad", "dd3d_vovnet_conv_grad_slices", "dd3d_vovnet_add", "dd3d_ese_backward",
                                          "dd3d_maxpool3x3s2_ceil_backward", "dd3d_vovnet_grad_layout"))
    # the wide entry points' slice rule is the backbone's, under their own limits
    a = hip.BackboneGradArgs()
    for (B, h, w, ci, co, k, s) in ((1, 4, 8, 2144, 1024, 1, 1), (2, 8, 16, 1024, 224, 3, 1), (1, 64, 128, 64, 128, 3, 2), (4, 24, 80, 1312, 32, 1, 1)):
        a.B, a.H, a.W, a.Cin, a.Cout, a.ksize, a.stride = B, h, w, ci, co, k, s
        assert hiplib.dd3d_vovnet_conv_grad_slices(C.byref(a)) == hip.backbone_grad_slices(B, h, w, ci, co, k, s), (B, h, w, ci, co, k, s)
    assert hiplib.dd3d_backbone_grad_slices(C.byref(a)) == -1  # (Cin 1312: past the DLA entry points' limit, which stays)
    a.Cin = 2176
    assert hiplib.dd3d_vovnet_conv_grad_slices(C.byref(a)) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_vovnet_conv_grad_slices")
    a.Cin, a.Cout = 64, 1056
    assert hiplib.dd3d_vovnet_conv_grad_slices(C.byref(a)) == -1
    assert hiplib.dd3d_vovnet_conv_grad_slices(None) == -1


def test_unsupported_variants_raise():
    from dd3d_amd.engine.losses import check_vovnet_backward
    dla = GC.cpu_model("dd3d_kitti_dla34")
    with pytest.raises(NotImplementedError, match="stem_grads"):
        _dry_plan(dla, vovnet_grads=True)
    for name, word in (("V-19-slim-eSE", "multiple of 32"), ("V-19-dw-eSE", "depthwise"), ("V-19-slim-dw-eSE", "depthwise")):
        m = GC.cpu_model("dd3d_kitti_v99", {"FE": {"BACKBONE": {"NAME": name}}})
        with pytest.raises(NotImplementedError, match=word):
            _dry_plan(m, vovnet_grads=True)
    v99 = GC.cpu_model("dd3d_kitti_v99")
    for math in ("bf16x2", "bf16"):
        v99.math = math
        with pytest.raises(NotImplementedError, match=math):
            _dry_plan(v99, vovnet_grads=True)
    v99.math = None
    for name in ("V-19-eSE", "V-39-eSE", "V-57-eSE", "V-99-eSE"):
        check_vovnet_backward(GC.cpu_model("dd3d_kitti_v99", {"FE": {"BACKBONE": {"NAME": name}}}).backbone.bottom_up)
    with pytest.raises(NotImplementedError, match="V2-99"):  # the DLA flags keep raising for this model
        _dry_plan(v99, backbone_grads=True)
    _dry_plan(v99, fpn_grads=True)


def test_compute_losses_takes_vovnet_grads_as_a_keyword_of_its_own():
    """The flag is no further level of the chain head_grads .. stem_grads (the named parameters stay that chain); anything else is refused."""
    import inspect
    from dd3d_amd.modeling.dd3d import DD3D
    assert "vovnet_grads" in inspect.signature(DD3D.get_loss_plan).parameters
    model = GC.cpu_model("dd3d_kitti_v99")
    with pytest.raises(TypeError, match="vovnet_grad"):
        model.compute_losses([], vovnet_grad=True)
