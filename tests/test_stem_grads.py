"""DLA-34 stem backward without a GPU: the layer oracle's restated form against torch autograd and against central differences, the
three-call chain against the whole-model oracle's one autograd pass for every backbone norm, the library's own shape check and slice count on every call shape of the
measured sizes, the struct layout against the header compiled as C."""
import ctypes as C
import os
import subprocess

import pytest
import torch

from tests import stem_grad_cases as SC
from tests import stem_grad_oracle as SO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _layer_inputs(layer, norm, hw=(7, 9), B=2, seed=0):
    k, s, cin, cout = SO.SHAPES[layer]
    gen = torch.Generator().manual_seed(100 + seed)
    p = SC.stem_params(norm, seed)[layer]
    if k == 7:
        p["w"] = torch.randn(cout, cin, k, k, generator=gen, dtype=F64) / 12.0  # (the layer alone: all four input channels are live)
    x = torch.randn(B, cin, hw[0], hw[1], generator=gen, dtype=F64)
    ho, wo = (hw[0] + s - 1) // s, (hw[1] + s - 1) // s
    g = torch.randn(B, cout, ho, wo, generator=gen, dtype=F64)
    return p, x, g, s


@pytest.mark.parametrize("norm", ["BN", ""])
@pytest.mark.parametrize("layer", list(SO.SHAPES))
def test_restated_layer_equals_autograd(layer, norm):
    """gm, dw_level, dw, q, r, da and the norm read-out on the forward's own output are autograd through F.conv2d + norm + ReLU."""
    p, x, g, s = _layer_inputs(layer, norm)
    y = SO.forward_layer(x, p, s, F64)
    assert tuple(y.shape[2:]) == ((x.shape[2] + s - 1) // s, (x.shape[3] + s - 1) // s) and 0.2 < float((y > 0).double().mean()) < 0.8
    res = SO.layer_grads(x, y, g, p["w"], SO.fold(p, F64)[0], s, F64)
    got, ref = SO.read_out(p, res, F64), SO.autograd_layer(x, p, g, s, F64)
    got["x"] = res["da"]
    assert sorted(got) == sorted(ref) == sorted(["w", "x"] + (["gamma", "beta"] if norm else ["b"]))
    for k in ref:
        assert got[k].shape == ref[k].shape and float(ref[k].abs().max()) > 0.0, k
        assert float((got[k] - ref[k]).abs().max()) <= 1e-12 * max(1.0, float(ref[k].abs().max())), (layer, norm, k)


@pytest.mark.parametrize("layer", list(SO.SHAPES))
def test_central_differences_per_family(layer):
    """d <g, y> / d theta by central differences in float64, a few entries per family: filter, conv bias / norm bias, norm weight, input."""
    for norm in ("BN", ""):
        p, x, g, s = _layer_inputs(layer, norm, hw=(5, 6), B=1, seed=3)
        y = SO.forward_layer(x, p, s, F64)
        res = SO.layer_grads(x, y, g, p["w"], SO.fold(p, F64)[0], s, F64)
        got = SO.read_out(p, res, F64)
        got["x"] = res["da"]
        loss = lambda q, xx: float((SO.forward_layer(xx, q, s, F64) * g).sum())
        h = 1e-6
        for key in got:
            t = x if key == "x" else p[key]
            for idx in torch.randperm(t.numel(), generator=torch.Generator().manual_seed(7))[:4].tolist():
                def at(d):
                    v = t.clone()
                    v.view(-1)[idx] += d
                    return loss(p if key == "x" else dict(p, **{key: v}), v if key == "x" else x)
                fd = (at(h) - at(-h)) / (2 * h)
                assert abs(fd - float(got[key].reshape(-1)[idx])) <= 1e-6 * max(1.0, abs(fd)), (layer, norm, key, idx)


@pytest.mark.parametrize("norm", ["FrozenBN", "BN", ""])
def test_three_call_chain_equals_the_whole_model_oracle(norm):
    """The three-call chain on the whole-model oracle forward's own activations (whole_model_grad_oracle.whole_model_grads, natural masks:
    oracle.dd3d_oracle's DLA-34 stem with its padding, its three-channel image, its norm and the model's parameter names) gives the stem
    parameters' gradients of that one autograd pass to 1e-9 of each family's maximum, for every backbone norm, with exactly the keys the
    norm owns: nothing for FrozenBN beside the filters, norm weight and bias for BN, the conv bias for "".  The chain is fed the
    oracle's ReLU outputs 0 .. 2, the normalised image and the retained backbone_level1 gradient."""
    from tests import whole_model_grad_oracle as WO
    case = dict(WO.CASES["kitti_dla34"], overrides={"FE": {"BACKBONE": {"NORM": norm}}}, B=2, H=128, W=128)
    model = WO.case_model(case)
    inputs, gt = WO.case_inputs(case, model)
    ex = {}
    params, at = SO.whole_model_grads_with_stem(model if norm else SO.WithIdentityNorms(model), model.cfg, inputs, gt, F64, extras=ex)
    named = dict(model.named_parameters())
    assert sorted(params) == sorted(named)
    pfx = "backbone.bottom_up."
    own = {"FrozenBN": ("weight", ), "BN": ("weight", "norm.weight", "norm.bias"), "": ("weight", "bias")}[norm]
    want = sorted(f"{pfx}{l}.{k}" for l in SO.STEM_LAYERS for k in own)
    assert sorted(k for k in named if k.startswith(tuple(pfx + l + "." for l in SO.STEM_LAYERS))) == want
    sp = SO.model_stem_params(model)
    base, l0, l1 = ex["relu_out"][:3]
    assert base.shape[1:] == (16, 128, 128) and l1.shape[1:] == (32, 64, 64)
    img = torch.stack([(x["image"].to(F64) - model.pixel_mean.to(F64).view(3, 1, 1)) / model.pixel_std.to(F64).view(3, 1, 1) for x in inputs])
    img4 = torch.cat([img, torch.zeros_like(img[:, :1])], 1)
    # the restated forward is the oracle's: the same three tensors from the model's own parameters
    f0 = SO.forward_layer(img4, sp["base_layer"], 1, F64)
    f1 = SO.forward_layer(f0, sp["level0.0"], 1, F64)
    for a, b in ((f0, base), (f1, l0), (SO.forward_layer(f1, sp["level1.0"], 2, F64), l1)):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    raw, tens = SO.stem_chain(img4, sp, at["backbone_level1"], F64, stored={"base": base, "level0.0": l0, "level1.0": l1})
    for key in ("backbone_level0", "backbone_base_layer"):
        assert float((tens[key] - at[key]).abs().max()) <= 1e-9 * float(at[key].abs().max()) and float(at[key].abs().max()) > 0, key
    got = {}
    for l in SO.STEM_LAYERS:
        for k, v in SO.read_out(sp[l], raw[l], F64).items():
            name = f"{pfx}{l}.{SO.PARAM_NAME[k]}"
            if name in named:  # (a FrozenBN norm's weight and bias are buffers: the read-out has them, the model does not own them)
                got[name] = v[:, :3] if name.endswith("base_layer.weight") else v
    assert sorted(got) == want
    fams = {}
    for k in want:
        fams.setdefault(k.rsplit(".", 2)[-2] + "." + k.rsplit(".", 1)[-1] if ".norm." in k else k.rsplit(".", 1)[-1], []).append(k)
    for fam, ks in sorted(fams.items()):
        gmax = max(float(params[k].abs().max()) for k in ks)
        dev = max(float((got[k] - params[k]).abs().max()) for k in ks)
        assert all(got[k].shape == named[k].shape for k in ks) and gmax > 0.0 and dev <= 1e-9 * gmax, (norm, fam, dev, gmax)


def _bare(shape):
    from dd3d_amd import hip
    a = hip.StemGradArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.ksize, a.stride = shape
    return a


def test_measured_call_shapes_pass_the_library_check_and_fit_the_slab(hiplib):
    """Every call shape of 1 and 4 KITTI images and the nuScenes sample: the library's slice count is the Python rule's, a slice is at most
    32 x 196 words, and the rows fit the plan's shared slab without growing it."""
    from dd3d_amd import hip
    for name, (B, Hp, Wp) in SC.MEASURED.items():
        for shape in SC.call_shapes(B, Hp, Wp):
            n = hiplib.dd3d_stem_grad_slices(C.byref(_bare(shape)))
            _, H, W, cin, cout, k, s = shape
            assert n == hip.stem_grad_slices(*shape) and n >= 1, (name, shape, hiplib.dd3d_last_error())
            assert cout * k * k * cin <= 32 * 196 and n * cout * k * k * cin * 4 <= hip.TG_SLAB_BYTES, (name, shape, n)
            units = B * ((H + s - 1) // s) * (((W + s - 1) // s + 63) // 64)
            assert hip.SG_MIN_UNITS_PER_SLICE <= -(-units // n) <= hip.SG_MAX_UNITS_PER_SLICE
    assert hip.stem_grad_slices(1, 1, 1, 16, 16, 3, 1) == 1 and hip.stem_grad_slices(2, 9, 331, 16, 32, 3, 2) == 4
    assert hip.stem_grad_slices(1, 384, 1280, 4, 16, 7, 1) == 512 and hip.stem_grad_slices(6, 896, 1664, 4, 16, 7, 1) == 2184
    # past the slab's byte budget the slices grow instead of the slab: 2^26 pixels of the 7 x 7 would be 16384 slices of 64 units
    n = hip.stem_grad_slices(1, 8192, 8192, 4, 16, 7, 1)
    assert n == hiplib.dd3d_stem_grad_slices(C.byref(_bare((1, 8192, 8192, 4, 16, 7, 1)))) and n < 16384 and n * 16 * 196 * 4 <= hip.TG_SLAB_BYTES


def test_other_shapes_are_rejected_by_the_shape_query(hiplib):
    from dd3d_amd import hip
    for shape in ((1, 8, 8, 3, 16, 7, 1), (1, 8, 8, 16, 16, 3, 2), (1, 8, 8, 32, 32, 3, 1), (1, 8, 8, 16, 32, 1, 2), (1, 8, 8, 4, 16, 7, 2),
                  (0, 8, 8, 16, 16, 3, 1), (1, 0, 8, 16, 16, 3, 1), (1, 8, 0, 16, 16, 3, 1), (1, 8193, 8192, 16, 16, 3, 1)):
        assert hiplib.dd3d_stem_grad_slices(C.byref(_bare(shape))) == -1, shape
        assert hiplib.dd3d_last_error().decode().startswith("dd3d_stem_grad_slices"), shape
    assert hiplib.dd3d_stem_grad_slices(None) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_stem_grad_slices")
    assert hip.STEM_GRAD_SHAPES == tuple(SO.SHAPES.values())


def test_stem_grad_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    cls = hip.StemGradArgs
    names = [f[0] for f in cls._fields_]
    assert names == ["x", "y", "g", "w", "scale", "da", "part", "qpart", "dw_level", "dw", "q", "r", "B", "H", "W", "Cin", "Cout", "ksize", "stride", "x_pitch",
                     "g_pitch", "da_pitch", "y_mode", "y_pitch", "n_slices", "wgrad_blocks", "y_plane_scale"]
    out = (C.c_int64 * 32)()
    n = hiplib.dd3d_stem_grad_layout(out, 32)
    assert n == len(names) + 1 and out[0] == C.sizeof(cls) and out[n] == -1
    assert [out[i + 1] for i in range(len(names))] == [getattr(cls, f).offset for f in names]
    assert hiplib.dd3d_stem_grad_layout(out, 8) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_stem_grad_layout")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(dd3d_stem_grad_args));',
             '  printf("unit %d\\n", DD3D_SG_UNIT);', '  printf("target %d\\n", DD3D_SG_TARGET_SLICES);', '  printf("minunits %d\\n", DD3D_SG_MIN_UNITS_PER_SLICE);',
             '  printf("maxunits %d\\n", DD3D_SG_MAX_UNITS_PER_SLICE);']
    lines += [f'  printf("{f} %zu\\n", offsetof(dd3d_stem_grad_args, {f}));' for f in names] + ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    assert (int(got["unit"]), int(got["target"]), int(got["minunits"]), int(got["maxunits"])) == (hip.SG_UNIT, hip.SG_TARGET_SLICES,
                                                                                                 hip.SG_MIN_UNITS_PER_SLICE, hip.SG_MAX_UNITS_PER_SLICE)
    for f in names:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert all(e in hip.EXPORTS for e in ("dd3d_stem_wgrad", "dd3d_stem_dgrad", "dd3d_stem_grad_slices", "dd3d_stem_grad_layout"))


# ------------------------------------------------------------------------------------------------ the plan and the public interface
def _dry_plan(model, B=1, H=128, W=256, **kw):
    from dd3d_amd.engine.losses import LossPlan
    return LossPlan(model, B, H, W, device="cpu", dry_run=True, **kw)


STEM_OPS = ["stem_grads.level1.0", "stem_grads.level0.0", "stem_grads.base_layer"]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("exp", ["dd3d_kitti_dla34", "dd3d_nusc_dla34"])
def test_dry_run_plan_order_handovers_keys_reads_and_slab(exp, fused, monkeypatch):
    """LossPlan(stem_grads=True) on both released DLA-34 configs, with the fused stem (the KEEP launch stores base and level0.0) and launch
    by launch: the three calls behind the last backbone call in their order, every hand-over, the exact key sets, the reads, the slab."""
    from dd3d_amd import hip
    from tests import loss_grad_cases as GC
    monkeypatch.setenv("DD3D_FUSED_STEM", "1" if fused else "0")
    model = GC.cpu_model(exp)
    with_b, plan = _dry_plan(model, backbone_grads=True), _dry_plan(model, stem_grads=True)
    assert plan.fused_stem == fused and plan.with_stem_grads and plan.with_backbone_grads and plan.with_fpn_grads and not with_b.with_stem_grads
    names, bn = [op.name for op in plan.ops], [op.name for op in with_b.ops]
    assert names == bn + STEM_OPS and bn[-1].startswith("backbone_grads.")  # nothing else moves: one more tail on the same stream
    stem_ops = [op for op in plan.ops if (getattr(op, "desc", None) or {}).get("kind") == "fused_stem"]
    assert len(stem_ops) == (1 if fused else 0)
    if fused:  # the KEEP launch writes the two buffers the backward reads; the plan without the flag keeps the plain launch
        keep = stem_ops[0].desc["keep"]
        assert keep[0].buf is plan.bufs["base"] and keep[1].buf is plan.bufs["level0.0"] and stem_ops[0].keep_args is not None
        plain = [op for op in with_b.ops if (getattr(op, "desc", None) or {}).get("kind") == "fused_stem"][0]
        assert plain.keep_args is None and plain.desc["keep"] is None and "base" not in with_b.bufs and "level0.0" not in with_b.bufs
    L = plan.stem_layers
    assert list(L) == ["level1.0", "level0.0", "base_layer"]
    same = lambda a, b: a.data_ptr() == b.data_ptr() and tuple(a.shape) == tuple(b.shape) and a.stride() == b.stride()
    l1, l0, lb = L["level1.0"], L["level0.0"], L["base_layer"]
    # hand-overs: g of a call is the call before's da; x is the f32 buffer of the layer's input; the mask is the layer's stored output
    assert same(l1.keep[1], plan.level1_grad) and same(l0.keep[1], l1.da) and same(lb.keep[1], l0.da) and lb.da is None
    assert same(l1.keep[0], plan.bufs["level0.0"].t) and same(l0.keep[0], plan.bufs["base"].t) and same(lb.keep[0], plan.bufs["img4"].t)
    assert [(l.ksize, l.stride, l.Cin, l.Cout) for l in (lb, l0, l1)] == list(hip.STEM_GRAD_SHAPES)
    assert [(l.H, l.W) for l in (l1, l0, lb)] == [(128, 256)] * 3 and tuple(l1.da.shape) == tuple(l0.da.shape) == (1, 128, 256, 16)
    assert [l.src for l in (l1, l0, lb)] == [dict(x=("level0.0", 0, 16), y=("level1.0", 0, 32)), dict(x=("base", 0, 16), y=("level0.0", 0, 16)),
                                             dict(x=("img4", 0, 4), y=("base", 0, 16))]
    assert (l1.with_wgrad, l1.with_dgrad, l0.with_wgrad, l0.with_dgrad, lb.with_wgrad, lb.with_dgrad) == (True, True, True, True, True, False)
    w7 = lb.keep[2]
    assert tuple(w7.shape) == (16, 7, 7, 4) and float(w7[..., 3].abs().max()) == 0.0
    assert torch.equal(w7[..., :3], model.backbone.bottom_up.base_layer.weight.detach().float().permute(0, 2, 3, 1))
    # exact key sets: param_grads covers all named parameters, grads gains exactly the two new keys
    bt, bp = plan.backbone_grads()
    st, sp = plan.stem_grads()
    assert list(st) == ["backbone_level0", "backbone_base_layer"] and all(v.shape == (1, 16, 128, 256) and v.dtype == torch.float32 for v in st.values())
    named = dict(model.named_parameters())
    pfx = "backbone.bottom_up."
    assert sorted(sp) == sorted(pfx + k for k in ("base_layer.weight", "level0.0.weight", "level1.0.weight"))  # FrozenBN owns nothing
    assert all(sp[k].shape == named[k].shape and sp[k].dtype == torch.float32 for k in sp) and sp[pfx + "base_layer.weight"].shape == (16, 3, 7, 7)
    everything = dict(plan.predictor_grads()[1], **plan.tower_grads()[1])
    everything.update(plan.fpn_grads()[1])
    everything.update(bp)
    assert not any(k in everything for k in sp)
    everything.update(sp)
    assert sorted(everything) == sorted(named)
    assert list(with_b.backbone_grads()[0]) == list(bt) and sorted(with_b.backbone_grads()[1]) == sorted(bp)
    # reads: the four stem tensors, each still the buffer of its name
    assert plan.stem_reads == ["img4", "base", "level0.0", "level1.0"] and all(n in plan.bufs for n in plan.stem_reads)
    assert plan.backbone_reads == with_b.backbone_reads
    # the slab: the plan's one slab, not grown for the stem
    part, qpart = plan.tower_slab
    assert part.numel() == with_b.tower_slab[0].numel() and qpart.numel() == with_b.tower_slab[1].numel()
    for lay in L.values():
        assert lay.part.data_ptr() == part.data_ptr() and lay.qpart.data_ptr() == qpart.data_ptr()
        assert lay.n_slices * lay.Cout * lay.ksize**2 * lay.Cin <= part.numel() and lay.n_slices * lay.Cout <= qpart.numel()
        assert lay.Cout * lay.ksize**2 * lay.Cin <= 32 * 196
    with pytest.raises(RuntimeError, match="stem_grads"):
        with_b.stem_grads()


def test_bn_and_normless_backbones_add_their_per_channel_parameters():
    from tests import loss_grad_cases as GC
    pfx = "backbone.bottom_up."
    for norm, extra in (("BN", ("norm.weight", "norm.bias")), ("", ("bias", ))):
        model = GC.cpu_model("dd3d_kitti_dla34", {"FE": {"BACKBONE": {"NORM": norm}}})
        sp = _dry_plan(model, stem_grads=True).stem_grads()[1]
        want = [pfx + f"{l}.{k}" for l in ("base_layer", "level0.0", "level1.0") for k in ("weight", ) + extra]
        assert sorted(sp) == sorted(want)
        named = dict(model.named_parameters())
        assert all(sp[k].shape == named[k].shape for k in sp)


def test_plans_without_the_flag_are_unchanged(monkeypatch):
    """Op for op and buffer for buffer: the forward plan and every loss plan short of stem_grads build what they built before."""
    from dd3d_amd.engine.forward import ForwardPlan
    from tests import loss_grad_cases as GC
    model = GC.cpu_model("dd3d_kitti_dla34")
    fwd = ForwardPlan(model, 1, 128, 256, device="cpu", dry_run=True)
    assert "base" not in fwd.bufs and "level0.0" not in fwd.bufs and not any("stem_grads" in op.name for op in fwd.ops)
    stem = [op for op in fwd.ops if (getattr(op, "desc", None) or {}).get("kind") == "fused_stem"]
    assert len(stem) == 1 and stem[0].keep_args is None
    for kw in (dict(), dict(grads=True), dict(pred_grads=True), dict(tower_grads=True), dict(fpn_grads=True), dict(backbone_grads=True)):
        plan = _dry_plan(model, **kw)
        assert not plan.with_stem_grads and not hasattr(plan, "stem_layers") and not any(op.name.startswith("stem_grads") for op in plan.ops), kw
        assert "base" not in plan.bufs and "level0.0" not in plan.bufs, kw
    full = _dry_plan(model, stem_grads=True)
    assert [op.name for op in full.ops][:len(plan.ops)] == [op.name for op in plan.ops]
    assert sorted(set(full.bufs) - set(plan.bufs)) == ["base", "level0.0"]


def test_unsupported_models_raise_before_anything_is_built():
    from tests import loss_grad_cases as GC
    with pytest.raises(NotImplementedError, match="V2-99"):
        _dry_plan(GC.cpu_model("dd3d_kitti_v99"), stem_grads=True)
    for variant, word in (("DLA-60", "Bottleneck"), ("DLA-X-60-C", "BottleneckX")):
        with pytest.raises(NotImplementedError, match=word):
            _dry_plan(GC.cpu_model("dd3d_kitti_dla34", {"FE": {"BACKBONE": {"NAME": variant}}}), stem_grads=True)
    model = GC.cpu_model("dd3d_kitti_dla34")
    model.force_generic_dla = True
    with pytest.raises(NotImplementedError, match="force_generic_dla"):
        _dry_plan(model, stem_grads=True)
    model.force_generic_dla = False
    for math in ("bf16x2", "bf16"):
        model.math = math
        with pytest.raises(NotImplementedError, match=math):
            _dry_plan(model, stem_grads=True)
    model.math = None
    for hw in ((127, 256), (128, 255)):  # an odd canvas (never produced by the padding to the FPN's size divisibility)
        with pytest.raises(NotImplementedError, match="even canvas"):
            _dry_plan(model, H=hw[0], W=hw[1], stem_grads=True)
    with pytest.raises(RuntimeError):
        model.train()


def test_keep_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    cls = hip.StemKeepArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {', '  printf("size %zu\\n", sizeof(dd3d_stem_keep_args));',
             '  printf("stemsize %zu\\n", sizeof(dd3d_stem_args));']
    names = [f[0] for f in cls._fields_]
    assert names == ["stem", "keep_base", "keep_level0", "keep_base_pitch", "keep_level0_pitch"]
    lines += [f'  printf("{f} %zu\\n", offsetof(dd3d_stem_keep_args, {f}));' for f in names] + ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) and int(got["stemsize"]) == C.sizeof(hip.StemArgs) and cls.stem.offset == 0
    for f in names:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert "dd3d_stem_fused_keep_f16x2" in hip.EXPORTS
    assert hiplib.dd3d_stem_fused_keep_f16x2(None, None) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_stem_fused_keep_f16x2")
    a = cls()
    assert hiplib.dd3d_stem_fused_keep_f16x2(C.byref(a), None) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_stem_fused_keep_f16x2: null pointer")


@pytest.mark.parametrize("name", ["kitti_dla34", "nusc_dla34", "kitti_dla34_bn"])
def test_pinned_cases_meet_the_sign_conditions_in_the_stem(name):
    """The float32 oracle forward against the float64 one on the pinned whole-model cases, in the three stem ReLUs: a sign differs only
    where |pre64| <= 2^-16 of its tensor's largest magnitude; with the stem counted, at most 1e-4 of all ReLU elements differ."""
    from tests import whole_model_grad_oracle as WO
    from tests.test_whole_model_grads import reference
    ref = reference(name)
    assert WO.stem_relus(ref.model) == 3 and [tuple(p.shape[1:2]) for p in ref.pre[:3]] == [(16, ), (16, ), (32, )]
    rep = SO.stem_sign_report(ref.pre32, ref.pre)
    for label, n, bad, far in rep:
        print(f"[stem_grads] {name} signs {label}: {bad} of {n} float32 signs differ from the float64 forward's, {far} beyond 2^-16 of the tensor's maximum")
        assert far == 0, (name, label, bad, far)
    total = sum(p.numel() for p in ref.pre)
    bad_all = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(ref.pre, ref.pre32))
    assert bad_all <= WO.SIGN_CAP * total and sum(r[1] for r in rep) > 0
