"""CPU tests of the loss engine's host side and of the oracle it is tested against (tests/loss_oracle.py): the reference behaviours
the issue lists (area ties, strict / inclusive comparisons, centre sampling, the first-GT quirk, images without GT, target order,
tridet's smooth-L1, the unclamped disentangled loss, the attribute mean, denominators, key order), Boxes3D.from_vectors, GT packing
and its cap, the C / ctypes layout of dd3d_loss_args."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loss_oracle as LO


def _gt(boxes, classes=None):
    b = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    return {"boxes": b, "classes": torch.tensor(classes if classes is not None else [0] * len(b))}


def _targets(gt, locs, strides=(8, ), sizes=(), center=True, radius=1.5):
    return LO.prepare_targets(locs, gt, list(strides), 3, list(sizes), center, radius, box3d=False)


def test_area_ties_pick_lowest_index_and_background_points_at_gt0():
    loc = [torch.tensor([[16.0, 16.0], [100.0, 100.0]])]
    t = _targets([_gt([[0, 0, 32, 32], [0, 0, 32, 32], [8, 8, 40, 40]], [2, 1, 0])], loc, center=False)
    assert t["labels"].tolist() == [2, 3] and t["target_inds"].tolist() == [0, 0]
    # the background location is measured to GT 0
    assert t["box2d_reg_targets"][1].tolist() == [100.0, 100.0, -68.0, -68.0]


def test_strict_inside_and_inclusive_size_ranges():
    loc = [torch.tensor([[0.0, 16.0], [64.0, 16.0], [32.0, 16.0]])]
    t = _targets([_gt([[0, 0, 64, 32]])], loc, center=False)
    assert t["labels"].tolist() == [3, 3, 0]  # on the left / right edge: not inside (strict > 0)
    loc2 = [torch.tensor([[64.0, 64.0]]), torch.tensor([[64.0, 64.0]])]
    # max regression distance exactly 64: inside [-1, 64] of level 0 AND [64, INF] of level 1
    t2 = LO.prepare_targets(loc2, [_gt([[0, 0, 128, 128]])], [8, 16], 3, [64], False, 1.5, box3d=False)
    assert t2["labels"].tolist() == [0, 0]


def test_center_sampling_region_and_first_gt_quirk():
    loc = [torch.tensor([[50.0, 50.0], [61.0, 50.0], [63.0, 50.0]])]
    t = LO.prepare_targets(loc, [_gt([[0, 0, 100, 100]])], [8], 3, [], True, 1.5, box3d=False)
    assert t["labels"].tolist() == [0, 0, 3]  # centre region 50 -+ 8 * 1.5 = (38, 62), strict, clipped to the box
    # the FIRST GT has x1 + x2 == 0: the whole image has no positive, whatever its other boxes
    q = LO.prepare_targets(loc, [_gt([[-10, 0, 10, 20], [0, 0, 100, 100]])], [8], 3, [], True, 1.5, box3d=False)
    assert (q["labels"] == 3).all()


def test_image_without_gt_and_level_first_order():
    loc = [torch.tensor([[8.0, 8.0], [24.0, 8.0]]), torch.tensor([[16.0, 16.0]])]
    t = LO.prepare_targets(loc, [_gt([[0, 0, 40, 40]], [1]), {"boxes": torch.zeros((0, 4)), "classes": torch.zeros(0, dtype=torch.long)}],
                           [8, 16], 3, [64], False, 1.5, box3d=False)
    assert t["im_inds"].tolist() == [0, 0, 1, 1, 0, 1] and t["fpn_levels"].tolist() == [0, 0, 0, 0, 1, 1]
    assert t["target_inds"].tolist() == [0, 0, -1, -1, 0, -1] and t["labels"].tolist()[2:4] == [3, 3]


def test_smooth_l1_is_tridets_not_its_docstring():
    x = torch.tensor([0.0, 0.0, 0.0])
    y = torch.tensor([0.04, 0.05, 0.2])
    l = LO.smooth_l1_loss(x, y, 0.05)
    assert torch.allclose(l, torch.tensor([0.5 * 0.04**2, 0.05 - 0.025, 0.2 - 0.025]))  # jumps at n = beta
    assert torch.equal(LO.smooth_l1_loss(x, y, 1e-6), y)


def test_losses_from_maps_keys_denominators_and_unclamped_groups():
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import META_ARCH_REGISTRY, get_cfg
    model = META_ARCH_REGISTRY.get("NuscenesDD3D")(get_cfg("dd3d_nusc_dla34"))
    p = dict(LO.settings(model), num_levels=1, beta=0.05)
    g = torch.Generator().manual_seed(0)
    C_, H, W = 10, 4, 4
    maps = {"logits0": torch.randn(1, C_, H, W, generator=g), "box2d_reg0": torch.rand(1, 4, H, W, generator=g) * 20,
            "centerness0": torch.randn(1, 1, H, W, generator=g), "quat0": torch.randn(1, 4 * C_, H, W, generator=g),
            "ctr0": torch.randn(1, 2 * C_, H, W, generator=g), "depth0": torch.randn(1, C_, H, W, generator=g) * 1000,
            "size0": torch.randn(1, 3 * C_, H, W, generator=g), "conf0": torch.randn(1, C_, H, W, generator=g),
            "attr0": torch.randn(1, 3, H, W, generator=g), "speed0": torch.rand(1, 1, H, W, generator=g)}
    loc = [torch.tensor([[x * 8.0, y * 8.0] for y in range(H) for x in range(W)])]
    K = torch.tensor([[700.0, 0, 16], [0, 700.0, 16], [0, 0, 1]])
    gt = {"boxes": torch.tensor([[0.0, 0.0, 30.0, 30.0]]), "classes": torch.tensor([4]), "quat": torch.tensor([[1.0, 0, 0, 0]]),
          "proj_ctr": torch.tensor([[15.0, 15.0]]), "depth": torch.tensor([[300.0]]), "size": torch.tensor([[1.0, 2.0, 1.5]]),
          "inv_K": torch.linalg.inv(K)[None], "attributes": torch.tensor([3]), "speeds": torch.tensor([float("nan")])}
    t = LO.prepare_targets(loc, [gt], [8], C_, [], True, 1.5, True, True, 3)
    out = LO.losses(maps, t, torch.linalg.inv(K)[None], p)
    assert list(out) == ["loss_cls", "loss_box2d_reg", "loss_centerness", "loss_conf3d", "loss_box3d_quat", "loss_box3d_proj_ctr",
                         "loss_box3d_depth", "loss_box3d_size", "loss_attr", "loss_speed"]
    assert float(out["loss_attr"]) == 0.0 and float(out["loss_speed"]) == 0.0  # invalid attribute, NaN speed
    # a depth error of hundreds of metres: far above MAX_LOSS_PER_GROUP_DISENT (20) * weight, since the clamp is discarded
    assert float(out["loss_box3d_depth"]) > 2 * 20.0
    from dd3d_amd.engine.losses import loss_keys
    assert loss_keys(True, True, 0)[3:] == ["loss_box3d_quat", "loss_box3d_proj_ctr", "loss_box3d_depth", "loss_box3d_size", "loss_conf3d",
                                            "loss_attr", "loss_speed"]
    assert loss_keys(False, False, 5) == ["loss_cls", "loss_box2d_reg", "loss_centerness"]


def test_boxes3d_from_vectors_matches_its_definition():
    from dd3d_amd.structures import Boxes3D
    K = np.array([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]])
    vecs = [np.array([0.9, 0.1, -0.3, 0.2, 1.5, 1.2, 20.0, 1.6, 3.9, 1.5]), np.array([1.0, 0, 0, 0, -4.0, 1.0, 35.5, 0.6, 0.8, 1.7])]
    b = Boxes3D.from_vectors(vecs, K)
    for i, v in enumerate(vecs):
        pc = K.dot(v[4:7])
        assert torch.equal(b.proj_ctr[i], torch.tensor(pc[:2] / pc[-1], dtype=torch.float32))
        assert torch.equal(b.quat[i], torch.tensor(v[:4], dtype=torch.float32)) and float(b.depth[i]) == np.float32(v[6])
    assert b.inv_intrinsics.dtype == torch.float64 and torch.equal(b.inv_intrinsics[1], torch.from_numpy(np.linalg.inv(K)))
    e = Boxes3D.from_vectors([], K)
    assert e.quat.shape == (0, 4) and e.proj_ctr.shape == (0, 2) and e.depth.shape == (0, 1) and e.inv_intrinsics.shape == (0, 3, 3)


def test_gt_packing_layout_and_cap():
    from dd3d_amd import get_cfg, hip
    from dd3d_amd.engine.losses import pack_gt
    from dd3d_amd.synthetic import make_gt_instances, make_inputs
    cfg = get_cfg("dd3d_nusc_dla34")
    inputs = make_inputs(3, 64, 96, dataset="nusc")
    gt = make_gt_instances(inputs, 10, cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, n_per_image=5, empty_images=(1, ), num_attributes=3)
    off, recs = pack_gt(gt, 512, True, True, 3, 10)
    assert off.tolist() == [0, 5, 5, 10] and recs.shape == (10, hip.LOSS_GT_FIELDS)
    g = gt[2]
    assert np.array_equal(recs[5:, 0:4], g.gt_boxes.tensor.numpy()) and recs[5:, 4].view(np.int32).tolist() == g.gt_classes.tolist()
    assert np.array_equal(recs[5:, 17:26], g.gt_boxes3d.inv_intrinsics.float().reshape(-1, 9).numpy())  # float64 K^-1 -> float32
    assert recs[5:, 5].view(np.int32).tolist() == g.gt_attributes.tolist()
    big = make_gt_instances(inputs[:1], 10, cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, n_per_image=513)
    with pytest.raises(ValueError, match="512"):
        pack_gt(big, 512, True, False, 3, 10)
    # classes and attributes index head-map rows and canonical sizes on the device: out of range raises, as the reference's indexing does
    bad = make_gt_instances(inputs[:1], 10, cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, n_per_image=4, num_attributes=3)
    for field, value, what in (("gt_classes", 11, "gt_classes"), ("gt_classes", -1, "gt_classes"), ("gt_attributes", 4, "gt_attributes"),
                               ("gt_attributes", -1, "gt_attributes")):
        keep = getattr(bad[0], field).clone()
        getattr(bad[0], field)[2] = value
        with pytest.raises(ValueError, match=what):
            pack_gt(bad, 512, True, True, 3, 10)
        setattr(bad[0], field, keep)
    bad[0].gt_classes[1] = 10  # = num_classes: background, as in the reference
    pack_gt(bad, 512, True, True, 3, 10)


def test_loss_args_layout_matches_header(hiplib):
    from dd3d_amd import hip
    out = (C.c_int64 * 64)()
    n = hiplib.dd3d_loss_layout(out, 64)
    names = ["cls", "box2d", "box3d", "locations", "gt_off", "gt", "inv_K", "canon_sizes", "labels", "target_inds", "box2d_reg", "ctr_target",
             "box3d_t", "attributes", "speeds", "flags", "partials", "out", "num_pos", "H", "W", "loc_off", "soi_lo", "soi_hi", "radius",
             "num_levels", "B", "num_classes", "max_gt", "n_partials", "cls_pitch", "b2d_pitch", "b3d_pitch", "attr_off", "num_attr",
             "speed_off", "center_sample", "class_agnostic_3d", "scale_depth_by_focal", "allocentric", "depth_is_distance", "min_depth",
             "max_depth", "focal_factor", "focal_alpha", "focal_gamma", "smooth_l1_beta", "conf3d_temperature", "weight_box3d",
             "weight_conf3d", "weight_attr", "weight_speed"]
    assert n == len(names) + 1 and [f[0] for f in hip.LossArgs._fields_] == names
    assert out[0] == C.sizeof(hip.LossArgs)
    assert [out[i + 1] for i in range(len(names))] == [getattr(hip.LossArgs, f).offset for f in names]


def test_loss_config_keys_and_loc_loss_type_guard():
    from dd3d_amd import get_cfg
    from dd3d_amd.engine.losses import check_loss_config
    c = get_cfg("dd3d_kitti_dla34")
    assert (c.DD3D.FCOS2D.LOSS.ALPHA, c.DD3D.FCOS2D.LOSS.GAMMA, c.DD3D.FCOS2D.LOSS.LOC_LOSS_TYPE) == (0.25, 2.0, "giou")
    assert (c.DD3D.FCOS3D.LOSS.SMOOTH_L1_BETA, c.DD3D.FCOS3D.LOSS.WEIGHT_BOX3D, c.DD3D.FCOS3D.PREPARE_TARGET.POS_RADIUS) == (0.05, 2.0, 1.5)
    n = get_cfg("dd3d_nusc_v99")
    assert (n.DD3D.NUSC.LOSS.WEIGHT_ATTR, n.DD3D.NUSC.LOSS.WEIGHT_SPEED) == (0.2, 0.2)
    check_loss_config(c)
    with pytest.raises(ValueError, match="giou"):
        check_loss_config(get_cfg("dd3d_kitti_dla34", {"DD3D": {"FCOS2D": {"LOSS": {"LOC_LOSS_TYPE": "iou"}}}}))


def test_focal_gamma_range_guard():
    """GAMMA == 0 and GAMMA >= 1 are supported; between 0 and 1 the derivative of (1 - p_t)^gamma is infinite at 1 - p_t == 0 (a
    logit beyond about +-17 in float32) and below 0 the loss itself is, in the reference as well: shown here on torch, and refused."""
    from dd3d_amd import get_cfg
    from dd3d_amd.engine.losses import check_loss_config
    from tests import loss_oracle as LO
    for gamma in (0.0, 1.0, 1.5, 2.0, 3.0):
        check_loss_config(get_cfg("dd3d_kitti_dla34", {"DD3D": {"FCOS2D": {"LOSS": {"GAMMA": gamma}}}}))
        x = torch.tensor([60.0, -60.0, 60.0, -60.0], requires_grad=True)
        LO.sigmoid_focal_loss(x, torch.tensor([1.0, 0.0, 0.0, 1.0]), 0.25, gamma).backward()
        assert bool(torch.isfinite(x.grad).all()), gamma
    for gamma in (0.5, 0.999, -1.0, float("nan")):
        with pytest.raises(ValueError, match="GAMMA"):
            check_loss_config(get_cfg("dd3d_kitti_dla34", {"DD3D": {"FCOS2D": {"LOSS": {"GAMMA": gamma}}}}))
    x = torch.tensor([60.0, -60.0], requires_grad=True)
    LO.sigmoid_focal_loss(x, torch.tensor([1.0, 0.0]), 0.25, 0.5).backward()
    assert not bool(torch.isfinite(x.grad).all())  # what the guard keeps out


def test_model_still_refuses_train_and_has_the_loss_api():
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import META_ARCH_REGISTRY, get_cfg
    m = META_ARCH_REGISTRY.get("DD3D")(get_cfg("dd3d_kitti_dla34"))
    with pytest.raises(NotImplementedError):
        m.train()
    assert callable(m.compute_losses) and callable(m.prepare_targets) and m.canvas_size([{"image": torch.zeros(3, 100, 300)}]) == (1, 128, 384)
