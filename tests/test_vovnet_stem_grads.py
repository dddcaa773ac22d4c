"""VoVNet-V2 stem_1 backward without a GPU (dd3d_vovnet_stem_wgrad, LossPlan(vovnet_stem_grads=True),
DD3D.compute_losses(vovnet_stem_grads=True)): the new entry points and the library's own shape check and slice count, dry plans of both
released V2-99 configs -- param_grads' keys are named_parameters() --, the call's bindings and place, the errors, and the sign
condition of the GPU whole-model test on the reference alone."""
import ctypes as C
import inspect

import pytest
import torch

from tests import loss_grad_cases as GC
from tests import vovnet_stem_grad_cases as VS
from tests import whole_model_grad_oracle as WO

PFX = VS.STEM1


def _dry_plan(model, B=1, H=128, W=256, **kw):
    from dd3d_amd.engine.losses import LossPlan
    return LossPlan(model, B, H, W, device="cpu", dry_run=True, **kw)


def _bare(shape):
    from dd3d_amd import hip
    a = hip.StemGradArgs()
    a.B, a.H, a.W, a.Cin, a.Cout, a.ksize, a.stride = shape
    return a


# ------------------------------------------------------------------------------------------------ ABI
def test_new_entry_points_and_the_slice_rule(hiplib):
    from dd3d_amd import hip
    assert all(e in hip.EXPORTS for e in ("dd3d_vovnet_stem_wgrad", "dd3d_vovnet_stem_grad_slices"))
    assert hip.VOVNET_STEM_GRAD_SHAPE == VS.SHAPE == (3, 2, 4, 64) and hip.VOVNET_STEM_GRAD_SHAPE not in hip.STEM_GRAD_SHAPES
    assert hip.STEM_GRAD_SHAPES == ((7, 1, 4, 16), (3, 1, 16, 16), (3, 2, 16, 32))
    k, s, cin, cout = VS.SHAPE
    sizes = [(B, hw[0], hw[1]) for hw, B, _ in VS.SEAM_CASES.values()] + list(VS.MEASURED.values()) + [(1, 128, 256), (1, 127, 255), (1, 8192, 8192)]
    for B, H, W in sizes:
        n = hiplib.dd3d_vovnet_stem_grad_slices(C.byref(_bare((B, H, W, cin, cout, k, s))))
        assert n == hip.vovnet_stem_grad_slices(B, H, W) == hip.stem_grad_slices(B, H, W, cin, cout, k, s) and n >= 1, (B, H, W, hiplib.dd3d_last_error())
        assert n * cout * k * k * cin * 4 <= hip.TG_SLAB_BYTES
    assert [hip.vovnet_stem_grad_slices(B, hw[0], hw[1]) for hw, B, _ in VS.SEAM_CASES.values()] == list(VS.SLICES.values())
    assert hip.vovnet_stem_grad_slices(1, 384, 1280) == 240 and hip.vovnet_stem_grad_slices(6, 896, 1600) == 546  # 1920 units, 8 a slice; 34944 units, 64 a slice


def test_shape_queries_reject_each_others_shapes(hiplib):
    from dd3d_amd import hip
    for k, s, cin, cout in hip.STEM_GRAD_SHAPES:
        assert hiplib.dd3d_vovnet_stem_grad_slices(C.byref(_bare((1, 8, 8, cin, cout, k, s)))) == -1, (k, s, cin, cout)
        assert hiplib.dd3d_last_error().decode().startswith("dd3d_vovnet_stem_grad_slices"), hiplib.dd3d_last_error()
    for shape in ((1, 8, 8, 4, 64, 3, 1), (1, 8, 8, 3, 64, 3, 2), (1, 8, 8, 4, 32, 3, 2), (1, 8, 8, 4, 64, 7, 2), (0, 8, 8, 4, 64, 3, 2), (1, 0, 8, 4, 64, 3, 2),
                  (1, 8, 0, 4, 64, 3, 2), (1, 8193, 8192, 4, 64, 3, 2)):
        assert hiplib.dd3d_vovnet_stem_grad_slices(C.byref(_bare(shape))) == -1, shape
        assert hiplib.dd3d_last_error().decode().startswith("dd3d_vovnet_stem_grad_slices"), shape
    assert hiplib.dd3d_vovnet_stem_grad_slices(None) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_vovnet_stem_grad_slices")
    # the DLA stem's query keeps rejecting stem_1's shape
    assert hiplib.dd3d_stem_grad_slices(C.byref(_bare((1, 8, 8, 4, 64, 3, 2)))) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_stem_grad_slices")
    # the entry point checks its arguments before anything is launched: no device is needed to be refused
    assert hiplib.dd3d_vovnet_stem_wgrad(None, None) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_vovnet_stem_wgrad")
    assert hiplib.dd3d_vovnet_stem_wgrad(C.byref(_bare((1, 8, 8, 16, 32, 3, 2))), None) == -1
    assert hiplib.dd3d_last_error().decode().startswith("dd3d_vovnet_stem_wgrad: (ksize, stride, Cin, Cout)")


# ------------------------------------------------------------------------------------------------ dry plans
def _check_dry_plan(model, bn=False):
    plan = _dry_plan(model, vovnet_stem_grads=True)
    assert plan.with_vovnet_stem_grads and plan.with_vovnet_grads and plan.with_fpn_grads and not plan.with_backbone_grads
    tensors, sp = plan.vovnet_stem_grads()
    assert list(tensors) == []
    named = dict(model.named_parameters())
    want = [PFX + "conv.weight"] + ([PFX + "norm.weight", PFX + "norm.bias"] if bn else [])
    assert sorted(sp) == sorted(want) and sp[PFX + "conv.weight"].shape == (64, 3, 3, 3)
    everything = dict(plan.predictor_grads()[1], **plan.tower_grads()[1])
    everything.update(plan.fpn_grads()[1])
    everything.update(plan.vovnet_grads()[1])
    assert not any(k in everything for k in sp)
    everything.update(sp)
    assert sorted(everything) == sorted(named)
    assert all(everything[k].shape == named[k].shape and everything[k].dtype == torch.float32 for k in named)
    return plan


@pytest.mark.parametrize("exp", ["dd3d_kitti_v99", "dd3d_nusc_v99"])
def test_dry_plan_param_grads_are_named_parameters(exp):
    _check_dry_plan(GC.cpu_model(exp))
    _check_dry_plan(GC.cpu_model(exp, {"FE": {"BACKBONE": {"NORM": "BN"}}}), bn=True)


@pytest.mark.variants
@pytest.mark.parametrize("name", ["V-19-eSE", "V-39-eSE", "V-57-eSE"])
def test_dry_plan_param_grads_of_the_other_covered_specs(name):
    _check_dry_plan(GC.cpu_model("dd3d_kitti_v99", {"FE": {"BACKBONE": {"NAME": name}}}))
    _check_dry_plan(GC.cpu_model("dd3d_kitti_v99", {"FE": {"BACKBONE": {"NAME": name, "NORM": "BN"}}}), bn=True)


def test_the_call_its_bindings_and_its_place():
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import GradCall, VovnetStemGrads
    model = GC.cpu_model("dd3d_kitti_v99")
    plan, with_v = _dry_plan(model, vovnet_stem_grads=True), _dry_plan(model, vovnet_grads=True)
    names, vn = [op.name for op in plan.ops], [op.name for op in with_v.ops]
    assert names == vn + ["vovnet_stem_grads.stem_1"] and vn[-1] == "vovnet_grads.stem_2"  # one more call behind stem_2's, nothing else moves
    assert sorted(plan.bufs) == sorted(with_v.bufs)  # everything it reads is in the parent's plan already
    assert list(plan.vovnet_stem_layers) == ["stem_1"] and not hasattr(with_v, "vovnet_stem_layers") and not with_v.with_vovnet_stem_grads
    lay = plan.vovnet_stem_layers["stem_1"]
    assert isinstance(lay, VovnetStemGrads) and isinstance(lay, GradCall) and not hasattr(lay, "da")
    assert lay.ENTRIES == (("dd3d_vovnet_stem_wgrad", "vovnet_stem_wgrad"), ) and lay.with_wgrad and not lay.with_dgrad
    a, img, s0 = lay.args, plan.bufs["img4"], plan.bufs["stem.0"]
    assert (a.ksize, a.stride, a.Cin, a.Cout) == hip.VOVNET_STEM_GRAD_SHAPE and (a.B, a.H, a.W) == (1, 128, 256) == (img.B, img.H, img.W)
    assert a.x == img.t.data_ptr() and a.x_pitch == 4 == img.pitch and (lay.Ho, lay.Wo) == (64, 128) == (s0.H, s0.W)
    bind = (a.y_mode, a.y or 0, a.y_pitch, a.y_plane_scale)  # (a dry plan's buffers have no device address)
    from dd3d_amd.engine.losses import act_binding
    assert bind == act_binding(plan, s0.view()) and a.y_mode == hip.PG_ACT_F16X2 and s0.view().np > 0  # the stored split planes
    assert a.g == plan.stem1_grad.data_ptr() == plan.vovnet_layers["stem_2"].da.data_ptr() and a.g_pitch == 64
    assert lay.src == dict(x=("img4", 0, 4), y=("stem.0", 0, 64)) and plan.vovnet_stem_reads == ["img4", "stem.0"]
    w = lay.keep[2]
    conv = getattr(model.backbone.bottom_up.stem, "stem_1/conv")
    assert tuple(w.shape) == (64, 3, 3, 4) and float(w[..., 3].abs().max()) == 0.0 and torch.equal(w[..., :3], conv.weight.detach().float().permute(0, 2, 3, 1))
    from dd3d_amd.layers import fold_norm
    assert torch.equal(lay.scale.cpu(), fold_norm(conv, getattr(model.backbone.bottom_up.stem, "stem_1/norm"))[0].float().cpu())
    # the slab: the plan's one slab, not grown for the call
    part, qpart = plan.tower_slab
    assert part.numel() == with_v.tower_slab[0].numel() and qpart.numel() == with_v.tower_slab[1].numel()
    assert a.part == part.data_ptr() and a.qpart == qpart.data_ptr() and a.n_slices == lay.n_slices == hip.vovnet_stem_grad_slices(1, 128, 256) == 16
    assert lay.n_slices * 64 * 36 <= part.numel() and lay.n_slices * 64 <= qpart.numel()
    for B, H, W in VS.MEASURED.values():  # the measured canvases: the VoVNet backward's slab holds the call
        from dd3d_amd.engine.losses import vovnet_slab_words
        rows, qrows = vovnet_slab_words(B, model.backbone.bottom_up, H // 2, W // 2)
        n = hip.vovnet_stem_grad_slices(B, H, W)
        assert n * 64 * 36 <= rows and n * 64 <= qrows, (B, H, W, n, rows, qrows)
    with pytest.raises(RuntimeError, match="vovnet_stem_grads"):
        with_v.vovnet_stem_grads()


# ------------------------------------------------------------------------------------------------ errors and the public interface
def test_errors_and_keywords():
    from dd3d_amd.modeling.dd3d import DD3D
    sig = inspect.signature(DD3D.get_loss_plan).parameters
    assert sig["vovnet_stem_grads"].default is False and sig["vovnet_grads"].default is False
    assert "vovnet_stem_grads" not in inspect.signature(DD3D.compute_losses).parameters  # (taken from **branch: the named flags are pinned)
    with pytest.raises(NotImplementedError, match="stem_grads=True"):
        _dry_plan(GC.cpu_model("dd3d_kitti_dla34"), vovnet_stem_grads=True)
    v99 = GC.cpu_model("dd3d_kitti_v99")
    for bad in ("vovnet_stem_grad", "vovnet_stems_grads", "stem1_grads"):
        with pytest.raises(TypeError, match=bad):
            v99.compute_losses([], **{bad: True})
    for name, word in (("V-19-slim-eSE", "multiple of 32"), ("V-19-dw-eSE", "depthwise")):  # whatever vovnet_grads raises for
        with pytest.raises(NotImplementedError, match=word):
            _dry_plan(GC.cpu_model("dd3d_kitti_v99", {"FE": {"BACKBONE": {"NAME": name}}}), vovnet_stem_grads=True)
    for math in ("bf16x2", "bf16"):
        v99.math = math
        with pytest.raises(NotImplementedError, match=math):
            _dry_plan(v99, vovnet_stem_grads=True)
    v99.math = None
    plan = _dry_plan(v99, vovnet_stem_grads=True, batch_stats=True)
    assert plan.batch_stats and plan.with_vovnet_stem_grads and [op.name for op in plan.ops][-1] == "vovnet_stem_grads.stem_1"
    assert sorted(plan.vovnet_stem_grads()[1]) == [PFX + "conv.weight"]


def test_planes_off_raises_as_for_vovnet_grads(monkeypatch):
    monkeypatch.setenv("DD3D_PLANES", "0")  # (the three-term arithmetic on f32 NHWC tensors)
    model = GC.cpu_model("dd3d_kitti_v99")
    model.math = "bf16x3"
    with pytest.raises(NotImplementedError, match="split-plane"):
        _dry_plan(model, vovnet_stem_grads=True)


# ------------------------------------------------------------------------------------------------ the sign condition, on the reference alone
def test_stem_1_signs_of_the_plan_emulator_stay_within_the_conditions():
    """The GPU whole-model test takes stem_1's ReLU mask from the plan's stored tensor and holds the plan to SIGN_NEAR / SIGN_CAP.  Here the
    plan emulator (float32 torch on the dry plan's own packed operands) stands for the kernels on the same case: its stem_1 output equals
    the float64 forward's within STORED_TOL, a sign differs only where |pre64| <= 2^-16 of the tensor's maximum, and with stem_1 counted at
    most 1e-4 of all ReLU elements differ (the other calls: the float32 oracle forward, as tests/test_whole_model_grads.py counts them)."""
    from dd3d_amd.engine.forward import ForwardPlan
    from tests.plan_emulator import emulate
    from tests.test_whole_model_grads import reference
    ref = reference("kitti_v99")
    case = WO.CASES["kitti_v99"]
    assert (case["B"], case["H"], case["W"]) == (1, 128, 256) and len(ref.pre) == case["relus"]
    plan = ForwardPlan(ref.model, *ref.model.canvas_size(ref.inputs), device="cpu", dry_run=True)
    ref.model.stage_inputs(ref.inputs, plan=plan)
    first = next(op.name for op in plan.ops if (getattr(op, "desc", None) or {}).get("kind") == "conv")
    with torch.no_grad():
        done = emulate(plan, stop_before=(first, ))  # preprocess and stem_1 alone
    assert "stem_1/conv" in done, done
    got, pre = plan.bufs["stem.0"].nchw().double(), ref.pre[0]
    assert tuple(got.shape) == tuple(pre.shape) == (1, 64, 64, 128)
    err, tol = float((got - pre.clamp(min=0)).abs().max()), WO.STORED_TOL * max(1.0, float(pre.abs().max()))
    assert err <= tol, (err, tol)
    bad = (got > 0) != (pre > 0)
    far = bad & (pre.abs() > WO.SIGN_NEAR * float(pre.abs().max()))
    total = sum(p.numel() for p in ref.pre)
    others = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(ref.pre[1:], ref.pre32[1:]))
    print(f"[vovnet_stem_grads] kitti_v99 stem_1 signs: {int(bad.sum())} of {pre.numel()} emulated signs differ from the float64 forward's, "
          f"{int(far.sum())} beyond 2^-16 of the tensor's maximum; {others} more in the other {len(ref.pre) - 1} calls of {total} elements")
    assert int(far.sum()) == 0 and int(bad.sum()) + others <= WO.SIGN_CAP * total
