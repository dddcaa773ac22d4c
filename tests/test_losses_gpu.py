"""Loss engine on the MI355X (csrc/losses.hip, engine.LossPlan): targets bit for bit against the CPU oracle (tests/loss_oracle.py), the
loss kernel at its C-ABI seam on the committed reference head maps, DD3D.compute_losses end to end (keys, order, values against the
oracle fed the plan's own head maps), determinism, graph replay vs launch by launch, and the full-size geometries."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import loss_oracle as LO

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _model(exp, overrides=None, weights=None):
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import META_ARCH_REGISTRY, get_cfg
    from dd3d_amd.synthetic import load_calib, make_state_dict
    cfg = get_cfg(exp, overrides)
    m = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
    if weights:
        m.load_state_dict(make_state_dict(m, calib=load_calib(weights)))
    return m.to("cuda").eval()


def _gt(model, inputs, **kw):
    from dd3d_amd.synthetic import make_gt_instances
    nusc = hasattr(model, "attr_logits")
    return make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES,
                             num_attributes=model.attr_logits.out_channels if nusc else None, **kw)


def _oracle_targets(model, level_hw, gt):
    from dd3d_amd.engine.losses import feature_locations
    strides = [s.stride for s in model.backbone_output_shape]
    locs = [feature_locations(h, w, strides[l], model.feature_locations_offset) for l, (h, w) in enumerate(level_hw)]
    nusc = hasattr(model, "attr_logits")
    pt = model.cfg.DD3D.FCOS3D.PREPARE_TARGET
    t = LO.prepare_targets(locs, LO.gt_dicts(gt, not model.only_box2d, nusc), strides, model.num_classes, list(model.cfg.DD3D.SIZES_OF_INTEREST),
                           bool(pt.CENTER_SAMPLE), float(pt.POS_RADIUS), not model.only_box2d, nusc,
                           model.attr_logits.out_channels if nusc else 3)
    return locs, t


def _assert_targets_equal(got, ref, box3d, nusc):
    for k in ("labels", "target_inds", "im_inds", "fpn_levels", "pos_inds"):
        assert torch.equal(got[k].cpu(), ref[k]), k
    for k in ("box2d_reg_targets", "locations"):
        assert torch.equal(got[k].cpu(), ref[k]), k
    if box3d:
        b = got["box3d_targets"]
        g3 = torch.cat([b.quat, b.proj_ctr, b.depth, b.size, b.inv_intrinsics.reshape(-1, 9)], 1).cpu()
        assert torch.equal(g3, ref["box3d"])
    if nusc:
        assert torch.equal(got["attributes"].cpu(), ref["attributes"])
        assert torch.equal(got["speeds"].cpu(), ref["speeds"], ) or np.array_equal(got["speeds"].cpu().numpy(), ref["speeds"].numpy(), equal_nan=True)


def _ctr_ieee(t):
    """compute_ctrness_targets (fcos2d.py:20-27) with every operation correctly rounded to f32 (each f64 result rounded once)."""
    r = t["box2d_reg_targets"].double()
    lr = (torch.minimum(r[:, 0], r[:, 2]) / torch.maximum(r[:, 0], r[:, 2])).float()
    tb = (torch.minimum(r[:, 1], r[:, 3]) / torch.maximum(r[:, 1], r[:, 3])).float()
    c = torch.sqrt((lr * tb).double()).float()
    return torch.where(t["labels"] != t["num_classes"], c, torch.zeros_like(c))


def _close(got, ref, rel, absz=1e-6):
    assert list(got) == list(ref), (list(got), list(ref))
    for k in ref:
        g, r = float(got[k]), float(ref[k])
        if r == 0.0:
            assert abs(g) <= absz, (k, g, r)
        else:
            assert abs(g - r) <= rel * abs(r), (k, g, r, abs(g - r) / abs(r))


def _maps_nchw(plan):
    """The plan's head maps in the reference's NCHW per-level form (the keys of the golden files)."""
    C_ = plan.model.num_classes
    out = {}
    for l in range(len(plan.features)):
        cl = plan.cls_maps[l].t.permute(0, 3, 1, 2).cpu()
        out[f"logits{l}"] = cl[:, :C_]
        if plan.nusc:
            A = plan.loss_args.num_attr
            out[f"attr{l}"], out[f"speed{l}"] = cl[:, C_:C_ + A], cl[:, C_ + A:C_ + A + 1]
        b2 = plan.b2d_maps[l].t.permute(0, 3, 1, 2).cpu()
        out[f"box2d_reg{l}"], out[f"centerness{l}"] = b2[:, :4], b2[:, 4:5]
        if plan.box3d_on:
            C3 = 1 if plan.model.cfg.DD3D.FCOS3D.CLASS_AGNOSTIC_BOX3D else C_
            b3 = plan.b3d_maps[l].t.permute(0, 3, 1, 2).cpu()
            for k, (c0, n) in {"quat": (0, 4), "ctr": (4, 2), "depth": (6, 1), "size": (7, 3), "conf": (10, 1)}.items():
                out[f"{k}{l}"] = b3[:, c0 * C3:(c0 + n) * C3]
    return out


def _seam(model, maps, inv_K, gt, level_hw):
    """dd3d_loss_assign + dd3d_loss_terms called directly on head maps given in NCHW (laid out as ForwardPlan._heads writes them)."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import _Targets, _fill_common, feature_locations, pack_gt
    dev = "cuda"
    B, L, C_ = maps["logits0"].shape[0], len(level_hw), model.num_classes
    nusc, box3d = hasattr(model, "attr_logits"), not model.only_box2d
    strides = [s.stride for s in model.backbone_output_shape]
    a = hip.LossArgs()
    nloc = _fill_common(a, model.cfg, model, level_hw, strides, B, hip.LOSS_MAX_GT)
    keep = []

    def nhwc(parts):
        t = torch.cat(parts, 1).permute(0, 2, 3, 1)
        pitch = (t.shape[-1] + 3) // 4 * 4
        buf = torch.zeros(t.shape[:-1] + (pitch, ), dtype=torch.float32)
        buf[..., :t.shape[-1]] = t
        buf = buf.contiguous().to(dev)
        keep.append(buf)
        return buf.data_ptr(), pitch

    A = model.attr_logits.out_channels if nusc else 0
    for l in range(L):
        a.cls[l], a.cls_pitch = nhwc([maps[f"logits{l}"]] + ([maps[f"attr{l}"], maps[f"speed{l}"]] if nusc else []))
        a.box2d[l], a.b2d_pitch = nhwc([maps[f"box2d_reg{l}"], maps[f"centerness{l}"]])
        if box3d:
            a.box3d[l], a.b3d_pitch = nhwc([maps[f"{k}{l}"] for k in ("quat", "ctr", "depth", "size", "conf")])
    a.attr_off, a.num_attr, a.speed_off = (C_, A, C_ + A) if nusc else (0, 0, -1)
    locs = torch.cat([feature_locations(h, w, strides[l], model.feature_locations_offset) for l, (h, w) in enumerate(level_hw)]).to(dev)
    canon = torch.tensor([list(r) for r in model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES], dtype=torch.float32, device=dev)
    iK = inv_K.reshape(B, 9).contiguous().to(dev)
    off, recs = pack_gt(gt, hip.LOSS_MAX_GT, box3d, nusc, A, C_)
    g_off = torch.from_numpy(off).to(dev)
    g = torch.from_numpy(recs if recs.shape[0] else np.zeros((1, hip.LOSS_GT_FIELDS), np.float32)).to(dev)
    keep += [locs, canon, iK, g_off, g]
    a.locations, a.canon_sizes, a.inv_K, a.gt_off, a.gt = locs.data_ptr(), canon.data_ptr(), iK.data_ptr(), g_off.data_ptr(), g.data_ptr()
    t = _Targets(a, B * nloc, box3d, nusc, dev)
    nb = (B * nloc + hip.LOSS_BLOCK - 1) // hip.LOSS_BLOCK
    partials = torch.zeros((nb, hip.LOSS_TERMS), device=dev)
    out = torch.zeros(hip.LOSS_OUT, device=dev)
    npos = torch.zeros(1, dtype=torch.int32, device=dev)
    a.partials, a.n_partials, a.out, a.num_pos = partials.data_ptr(), nb, out.data_ptr(), npos.data_ptr()
    L_ = hip.lib()
    hip.check(L_.dd3d_loss_assign(C.byref(a), hip.current_stream()), "assign")
    hip.check(L_.dd3d_loss_terms(C.byref(a), hip.current_stream()), "terms")
    torch.cuda.synchronize()
    from dd3d_amd.engine.losses import OUT_INDEX, loss_keys
    n = int(npos.cpu())
    o = out.cpu()
    return {k: o[OUT_INDEX[k]] for k in loss_keys(box3d, nusc, n)}, t


GOLDEN_CASES = {
    # file: (experiment, overrides, dataset, image sizes)
    "dla34_kitti_128x384_b2_ragged": ("dd3d_kitti_dla34", None, "kitti", [(128, 384), (115, 362)]),
    "dla34_nusc_128x224_b6": ("dd3d_nusc_dla34", None, "nusc", [(128, 224)] * 6),
    "dla34_kitti_box2d_only_128x256_b2": ("dd3d_kitti_dla34", {"MODEL": {"BOX3D_ON": False}}, "kitti", [(128, 256)] * 2),
    "dla34_kitti_variant_ctr_half_distance": ("dd3d_kitti_dla34", {"DD3D": {"FEATURE_LOCATIONS_OFFSET": "half", "FCOS3D": {
        "PREDICT_DISTANCE": True, "SCALE_DEPTH_BY_FOCAL_LENGTHS": False}}}, "kitti", [(128, 256)]),
    "dla34_kitti_variant_egocentric_agnostic": ("dd3d_kitti_dla34", {"DD3D": {"FCOS3D": {"PREDICT_ALLOCENTRIC_ROT": False,
                                                                                          "CLASS_AGNOSTIC_BOX3D": True}}}, "kitti", [(128, 256)]),
    "dla34_kitti_variant_plain_heads": ("dd3d_kitti_dla34", {"DD3D": {"FCOS2D": {"USE_SCALE": False}, "FCOS3D": {"USE_SCALE": False,
                                                                                                              "PER_LEVEL_PREDICTORS": True}}}, "kitti", [(128, 256)]),
}


def _golden_case(name):
    from dd3d_amd.synthetic import make_inputs
    exp, over, ds, sizes = GOLDEN_CASES[name]
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    model = _model(exp, over)
    maps = {k: torch.from_numpy(z[k]) for k in z.files if k[:-1] in ("logits", "box2d_reg", "centerness", "quat", "ctr", "depth", "size", "conf",
                                                                      "attr", "speed")}
    B = maps["logits0"].shape[0]
    inputs = make_inputs(B, sizes[0][0], sizes[0][1], dataset=ds)
    for x, (h, w) in zip(inputs, sizes):
        x["image"] = x["image"][:, :h, :w]
    if model.only_box2d and maps.get("quat0") is not None:
        maps = {k: v for k, v in maps.items() if k[:-1] in ("logits", "box2d_reg", "centerness")}
    level_hw = [tuple(maps[f"logits{l}"].shape[-2:]) for l in range(len([k for k in maps if k.startswith("logits")]))]
    K = torch.stack([x["intrinsics"] for x in inputs]).float()
    return model, maps, inputs, level_hw, torch.linalg.inv(K)


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_loss_kernels_at_seam_on_reference_head_maps(hiplib, name):
    model, maps, inputs, level_hw, inv_K = _golden_case(name)
    gt = _gt(model, inputs, empty_images=(1, ) if len(inputs) > 2 else (), quirk_images=(len(inputs) - 1, ) if len(inputs) > 3 else ())
    got, t = _seam(model, maps, inv_K, gt, level_hw)
    _, ref_t = _oracle_targets(model, level_hw, gt)
    assert torch.equal(t.labels.cpu().long(), ref_t["labels"]) and torch.equal(t.box2d_reg.cpu(), ref_t["box2d_reg_targets"])
    # centerness targets: the kernel rounds like IEEE f32 division and square root; torch's vectorised CPU sqrt is off by one ulp on a
    # few inputs, so the bit-for-bit comparison is against the IEEE statement, and torch's values are within one ulp
    assert torch.equal(t.ctr.cpu(), _ctr_ieee(ref_t))
    assert torch.allclose(t.ctr.cpu(), ref_t["ctr"], rtol=2.0**-23, atol=0.0)
    assert int((ref_t["labels"] != model.num_classes).sum()) > 20  # not a vacuous comparison
    ref = LO.losses(maps, ref_t, inv_K, dict(LO.settings(model), num_levels=len(level_hw)))
    _close(got, ref, 5e-6)


def test_prepare_targets_adversarial_gt_bit_exact(hiplib):
    """Area ties, edges on the grid, the first-GT quirk, an image without GT and an image with 512 GT."""
    from dd3d_amd.engine.losses import feature_locations
    from dd3d_amd.synthetic import make_inputs
    model = _model("dd3d_kitti_dla34")
    inputs = make_inputs(4, 384, 1280)
    gt = _gt(model, inputs, n_per_image=40, empty_images=(1, ), quirk_images=(2, ))
    gt[3] = _gt(model, inputs[3:], n_per_image=512, seed=77)[0]
    # exact ties: the same box twice (lowest index wins) and a second box of the same area elsewhere
    b = gt[0].gt_boxes.tensor
    b[5] = b[4]
    level_hw = [(48, 160), (24, 80), (12, 40), (6, 20), (3, 10)]
    strides = [8, 16, 32, 64, 128]
    locs = [feature_locations(h, w, s) for (h, w), s in zip(level_hw, strides)]
    got = model.prepare_targets([l.cuda() for l in locs], gt, level_hw)
    _, ref = _oracle_targets(model, level_hw, gt)
    _assert_targets_equal(got, ref, True, False)
    n = sum(h * w for h, w in level_hw)
    lab = ref["labels"].view(-1)
    assert bool((ref["target_inds"][ref["im_inds"] == 1] == -1).all())
    assert bool((lab[ref["im_inds"] == 2] == model.num_classes).all())  # the quirk image has no positive
    assert int((lab[ref["im_inds"] == 3] != model.num_classes).sum()) > 0 and n > 0
    with pytest.raises(ValueError, match="512"):
        model.prepare_targets([l.cuda() for l in locs], _gt(model, inputs[:1], n_per_image=513), level_hw)


@pytest.mark.parametrize("exp,weights,B,H,W,ds", [("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti"),
                                                   ("dd3d_nusc_dla34", "dla34_nusc", 6, 128, 224, "nusc")])
def test_compute_losses_end_to_end(hiplib, exp, weights, B, H, W, ds):
    from dd3d_amd.synthetic import make_inputs
    model = _model(exp, weights=weights)
    inputs = make_inputs(B, H, W, dataset=ds)
    gt = _gt(model, inputs, empty_images=(1, ))
    for x, g in zip(inputs, gt):
        x["instances"] = g
    losses = model.compute_losses(inputs)
    plan = model.get_loss_plan(*model.canvas_size(inputs))
    assert all(v.dim() == 0 and v.dtype == torch.float32 and v.device.type == "cuda" for v in losses.values())
    level_hw = [(f.H, f.W) for f in plan.features]
    _, ref_t = _oracle_targets(model, level_hw, gt)
    _assert_targets_equal(plan.target_dict(), ref_t, True, ds != "kitti")
    inv_K = plan.inv_K.view(-1, 3, 3).cpu()
    ref = LO.losses(_maps_nchw(plan), ref_t, inv_K, dict(LO.settings(model), num_levels=len(level_hw)))
    _close(losses, ref, 5e-6)
    # bitwise the same on a second call, and the captured graph equals launch-by-launch execution
    again = model.compute_losses(inputs)
    assert all(torch.equal(again[k], losses[k]) for k in losses)
    model.use_graph = False
    model.invalidate_plans()
    eager = model.compute_losses(inputs)
    assert all(torch.equal(eager[k], losses[k]) for k in losses)


def test_compute_losses_without_positives_key_order(hiplib):
    from dd3d_amd.synthetic import make_inputs
    model = _model("dd3d_kitti_dla34", weights="dla34_kitti")
    inputs = make_inputs(2, 128, 256)
    for x, g in zip(inputs, _gt(model, inputs, empty_images=(0, 1))):
        x["instances"] = g
    losses = model.compute_losses(inputs)
    assert list(losses) == ["loss_cls", "loss_box2d_reg", "loss_centerness", "loss_box3d_quat", "loss_box3d_proj_ctr", "loss_box3d_depth",
                            "loss_box3d_size", "loss_conf3d"]
    assert float(losses["loss_cls"]) > 0 and all(float(losses[k]) == 0.0 for k in list(losses)[1:])
    with pytest.raises(NotImplementedError):
        model.train()


@pytest.mark.parametrize("exp,weights,B,H,W,ds", [("dd3d_kitti_dla34", "dla34_kitti", 4, 384, 1280, "kitti"),
                                                   ("dd3d_nusc_dla34", "dla34_nusc", 6, 896, 1600, "nusc")])
def test_compute_losses_full_size(hiplib, exp, weights, B, H, W, ds):
    from dd3d_amd.synthetic import make_inputs
    model = _model(exp, weights=weights)
    inputs = make_inputs(B, H, W, dataset=ds)
    gt = _gt(model, inputs, n_per_image=48, quirk_images=(B - 1, ))
    for x, g in zip(inputs, gt):
        x["instances"] = g
    losses = model.compute_losses(inputs)
    plan = model.get_loss_plan(*model.canvas_size(inputs))
    level_hw = [(f.H, f.W) for f in plan.features]
    _, ref_t = _oracle_targets(model, level_hw, gt)
    _assert_targets_equal(plan.target_dict(), ref_t, True, ds != "kitti")
    ref = LO.losses(_maps_nchw(plan), ref_t, plan.inv_K.view(-1, 3, 3).cpu(), dict(LO.settings(model), num_levels=len(level_hw)))
    _close(losses, ref, 5e-6)


# ---------------------------------------------------------------------------------------------- away from the released settings
from tests import loss_grad_cases as GC  # noqa: E402  (imports GOLDEN_CASES from this module)


def _forward_close(got, case, what, nan_keys=()):
    """The project's bar of this seam: every loss within 5e-6 (relative) of the float32 CPU oracle; a key of `nan_keys` is NaN on both
    sides.  Prints each loss's distance from the float32 and the float64 oracle."""
    ref, ref64 = case.losses(torch.float32), case.losses(torch.float64)
    assert list(got) == list(ref), (list(got), list(ref))
    for k in ref:
        g, r, r64 = float(got[k]), float(ref[k]), float(ref64[k])
        print(f"[losses] {what} {k}: kernel {g:.9g} oracle32 {r:.9g} rel {abs(g - r) / max(abs(r), 1e-30):.2e}; against float64 {abs(g - r64) / max(abs(r64), 1e-30):.2e}"
              f" (oracle32 against float64 {abs(r - r64) / max(abs(r64), 1e-30):.2e})")
    for k in ref:
        g, r = float(got[k]), float(ref[k])
        if k in nan_keys:
            assert np.isnan(g) and np.isnan(r), (what, k, g, r)
    _close({k: v for k, v in got.items() if k not in nan_keys}, {k: v for k, v in ref.items() if k not in nan_keys}, 5e-6)


def _assert_seam_targets(t, case):
    """Labels, box2d_reg and the centerness targets of the assignment kernel bit for bit, as in
    test_loss_kernels_at_seam_on_reference_head_maps."""
    ref_t = case.targets
    assert torch.equal(t.labels.cpu().long(), ref_t["labels"]) and torch.equal(t.box2d_reg.cpu(), ref_t["box2d_reg_targets"])
    assert torch.equal(t.ctr.cpu(), _ctr_ieee(ref_t))
    assert torch.allclose(t.ctr.cpu(), ref_t["ctr"], rtol=2.0**-23, atol=0.0)


@pytest.mark.parametrize("name,key", GC.SETTINGS_ROWS)
def test_loss_kernels_at_seam_away_from_the_released_settings(hiplib, name, key):
    """Every row of loss_grad_cases.SETTINGS: the focal loss's powf branch and its alpha switch, plain L1, another temperature and
    other weights in the loss kernel; CENTER_SAMPLE off and other radii in the assignment kernel, whose targets are compared bit for bit."""
    case = GC.settings_case(name, key)
    got, t = _seam(case.model, case.maps, case.inv_K, case.gt, case.level_hw)
    _assert_seam_targets(t, case)
    assert case.num_pos > 20 and int(t.flags.cpu()) == 0
    if key == "no_center_sample" and "nusc" in name:  # the first-box quirk belongs to centre sampling: without it the quirk image has positives
        B = len(case.gt)
        assert int(((case.targets["im_inds"] == B - 1) & (case.targets["labels"] != case.model.num_classes)).sum()) > 0
        assert int(((GC.golden_case(name).targets["im_inds"] == B - 1) & (GC.golden_case(name).targets["labels"] != case.model.num_classes)).sum()) == 0
    _forward_close(got, case, f"{name}:{key}")


@pytest.mark.parametrize("gamma", GC.SATURATED_GAMMAS)
@pytest.mark.parametrize("H,W", [(4, 4), (1, 257)])
def test_loss_kernels_on_saturated_logits(hiplib, H, W, gamma):
    """Logits of +-60 on positives and whole background rows of -60: 1 - p_t is exactly 0 or 1 in float32."""
    case = GC.handmade_case(H, W, gamma=gamma)
    got, t = _seam(case.model, case.maps, case.inv_K, case.gt, case.level_hw)
    _assert_seam_targets(t, case)
    assert all(np.isfinite(float(v)) for v in got.values())
    _forward_close(got, case, f"saturated{H}x{W}:gamma{gamma}")


@pytest.mark.parametrize("name", GC.POISONED_CASES)
def test_loss_kernels_on_the_renormalised_path(hiplib, name):
    """One positive with an all-zero quaternion (loss_grad_cases.poisoned_case) decodes to NaN and sets the batch-wide trigger; every
    other positive goes through the renormalised branch of decoded_quat.  The families the oracle makes NaN are NaN, the others meet
    the bar; the flag is 1 here and 0 on the clean case.  (What this does and does not prove: test_loss_grads_gpu.py.)"""
    case, clean = GC.poisoned_case(name), GC.golden_case(name)
    got, t = _seam(case.model, case.maps, case.inv_K, case.gt, case.level_hw)
    assert int(t.flags.cpu()) == 1
    nan = {k for k, v in case.losses(torch.float64).items() if bool(torch.isnan(v))}
    assert nan == {"loss_conf3d", "loss_box3d_quat"}
    _forward_close(got, case, "poisoned:" + name, nan_keys=nan)
    _, t0 = _seam(clean.model, clean.maps, clean.inv_K, clean.gt, clean.level_hw)
    assert int(t0.flags.cpu()) == 0


# ---------------------------------------------------------------------------------------------- against the reference's own modules
from tests import test_losses_golden as TG  # noqa: E402


@pytest.mark.parametrize("name", list(TG.CASES))
def test_prepare_targets_matches_reference_golden(hiplib, name):
    from dd3d_amd.engine.losses import feature_locations
    model, g, maps, level_hw, gt = TG.load_case(name)
    model = model.to("cuda")
    strides = [s.stride for s in model.backbone_output_shape]
    locs = [feature_locations(h, w, strides[l], model.feature_locations_offset).cuda() for l, (h, w) in enumerate(level_hw)]
    got = model.prepare_targets(locs, gt, level_hw)
    TG.golden_targets_equal(got, g, not model.only_box2d, hasattr(model, "attr_logits"))


@pytest.mark.parametrize("name", list(TG.CASES))
def test_loss_kernels_at_seam_match_reference_golden(hiplib, name):
    """The loss kernels fed the reference's own head maps and K^-1: within 5e-6 of the reference's loss modules."""
    model, g, maps, level_hw, gt = TG.load_case(name)
    got, _ = _seam(model.to("cuda"), maps, torch.from_numpy(g["inv_K"]), gt, level_hw)
    TG.assert_losses_close(got, g, 5e-6)


@pytest.mark.parametrize("name", list(TG.CASES))
def test_compute_losses_matches_reference_golden(hiplib, name):
    """End to end from the uint8 images: keys in the reference's order, values within 1e-4 of the reference's (2e-4 on the nuScenes
    sample, whose head maps this forward reproduces to ~1e-5 of their range, not ~1e-6: the same offset in the f32-equivalent arithmetic;
    the kernels themselves are within 5e-6 of the reference on the reference's own maps, test_loss_kernels_at_seam_match_reference_golden)."""
    from dd3d_amd.synthetic import load_calib, make_state_dict
    from tests.golden.make_golden import case_inputs
    model, g, maps, level_hw, gt = TG.load_case(name)
    exp, geometry = TG.CASES[name][1], TG.CASES[name][3]
    model.load_state_dict(make_state_dict(model, calib=load_calib("dla34_nusc" if "nusc" in exp else "dla34_kitti")))
    model = model.to("cuda")
    inputs = case_inputs(*geometry)
    for x, inst in zip(inputs, gt):
        x["instances"] = inst
    TG.assert_losses_close(model.compute_losses(inputs), g, 2e-4 if "nusc" in exp else 1e-4)
