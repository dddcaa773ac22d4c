"""Golden targets and losses from the reference's OWN training modules: DD3DTargetPreparer / NuscenesDD3DTargetPreparer
(tridet/modeling/dd3d/prepare_targets.py, nuscenes_dd3d.py), FCOS2DLoss, FCOS3DLoss and NuscenesLoss, run on the CPU over the
third-party shims of ref_shims.py, fed the reference's eval-mode head maps already committed with the forward goldens.  fvcore's
sigmoid_focal_loss and smooth_l1_loss (which the shims leave unimplemented: the forward never calls them) are independent statements of
fvcore's published functions, patched into sys.modules before the reference's loss modules are imported.  Also Boxes3D.from_vectors
(boxes3d.py:175-218) on a few vectors.  Run in the build container only (the reference tree does not exist on the GPU box):

    python tests/golden/make_loss_golden.py      ->  tests/golden/losses_*.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests.golden import ref_shims  # noqa: E402
from tests.golden.make_golden import VARIANTS, case_inputs  # noqa: E402

# name: (head-map golden, experiment, overrides, case_inputs arguments (B, H, W, ragged, dataset), GT options)
CASES = {
    "kitti_ragged": ("dla34_kitti_128x384_b2_ragged", "dd3d_kitti_dla34", None, (2, 128, 384, True, "kitti"), dict(n_per_image=24)),
    "kitti_ragged_nopos": ("dla34_kitti_128x384_b2_ragged", "dd3d_kitti_dla34", None, (2, 128, 384, True, "kitti"), dict(empty_images=(0, 1))),
    # (no image without GT here: the reference's nuScenes preparer appends no attribute targets for one and misaligns the rest)
    "nusc_b6": ("dla34_nusc_128x224_b6", "dd3d_nusc_dla34", None, (6, 128, 224, False, "nusc"), dict(n_per_image=24, quirk_images=(5, ))),
    "kitti_box2d_only": ("dla34_kitti_box2d_only_128x256_b2", "dd3d_kitti_dla34", {"MODEL": {"BOX3D_ON": False}}, (2, 128, 256, False, "kitti"),
                         dict(n_per_image=24, empty_images=(1, ))),
}
for _v, _over in VARIANTS.items():
    CASES[f"kitti_variant_{_v}"] = (f"dla34_kitti_variant_{_v}", "dd3d_kitti_dla34", _over, (1, 128, 256, False, "kitti"), dict(n_per_image=24))
GT_SEED = 2000
TARGET_KEYS = ("labels", "box2d_reg_targets", "locations", "target_inds", "im_inds", "fpn_levels", "pos_inds")


def sigmoid_focal_loss(inputs, targets, alpha=-1, gamma=2, reduction="none"):
    """[ext] fvcore.nn.sigmoid_focal_loss (fvcore/nn/focal_loss.py), stated independently."""
    import torch.nn.functional as F
    p = torch.sigmoid(inputs)
    ce = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce * ((1 - p_t)**gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss


def smooth_l1_loss(input, target, beta, reduction="none"):
    """[ext] fvcore.nn.smooth_l1_loss (fvcore/nn/smooth_l1_loss.py), stated independently: 0.5 n^2 / beta below beta."""
    if beta < 1e-5:
        loss = torch.abs(input - target)
    else:
        n = torch.abs(input - target)
        loss = torch.where(n < beta, 0.5 * n**2 / beta, n - 0.5 * beta)
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss


class LevelList(list):
    """Per-level head maps.  FCOS3DLoss's no-positive branch calls `box3d_quat.sum()` on the per-level LIST (fcos3d.py:217-225), which
    raises AttributeError as released; `.sum()` here supplies the evident intent (the sum over the levels) so that the branch's keys and
    zeros can be recorded.  The positive branch never calls it."""
    def sum(self):
        return torch.stack([x.sum() for x in self]).sum()


def install():
    ref_shims.install()
    sys.modules["fvcore.nn"].sigmoid_focal_loss = sigmoid_focal_loss
    sys.modules["fvcore.nn.smooth_l1_loss"].smooth_l1_loss = smooth_l1_loss


def gt_instances(model, inputs, opts):
    from dd3d_amd.synthetic import make_gt_instances
    nusc = hasattr(model, "attr_logits")
    return make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, seed=GT_SEED,
                             num_attributes=model.attr_logits.out_channels if nusc else None, **opts)


def to_reference(gt, box3d, nusc):
    """dd3d_amd Instances -> the reference's Instances / Boxes / Boxes3D (same arrays; K^-1 stays float64 as its mapper makes it)."""
    from detectron2.structures import Boxes, Instances
    from tridet.structures.boxes3d import Boxes3D
    out = []
    for g in gt:
        r = Instances(g.image_size)
        r.gt_boxes = Boxes(g.gt_boxes.tensor.clone())
        r.gt_classes = g.gt_classes.clone()
        if box3d:
            b = g.gt_boxes3d
            r.gt_boxes3d = Boxes3D(b.quat.clone(), b.proj_ctr.clone(), b.depth.clone(), b.size.clone(), b.inv_intrinsics.clone())
        if nusc:
            r.gt_attributes, r.gt_speeds = g.gt_attributes.clone(), g.gt_speeds.clone()
        out.append(r)
    return out


def run_case(name):
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import META_ARCH_REGISTRY, get_cfg
    maps_file, exp, over, ci, opts = CASES[name]
    cfg = get_cfg(exp, over)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
    box3d, nusc = not model.only_box2d, hasattr(model, "attr_logits")
    install()
    from tridet.modeling.dd3d.fcos2d import FCOS2DLoss
    from tridet.modeling.dd3d.fcos3d import FCOS3DLoss
    from tridet.modeling.dd3d.nuscenes_dd3d import NuscenesDD3DTargetPreparer, NuscenesLoss
    from tridet.modeling.dd3d.prepare_targets import DD3DTargetPreparer
    from tridet.utils.tensor2d import compute_features_locations
    z = np.load(os.path.join(HERE, maps_file + ".npz"))
    L = len([k for k in z.files if k.startswith("logits")])
    m = lambda k: LevelList(torch.from_numpy(z[f"{k}{l}"]) for l in range(L))
    inputs = case_inputs(*ci)
    gt = gt_instances(model, inputs, opts)
    shapes = model.backbone_output_shape
    feature_shapes = [tuple(z[f"logits{l}"].shape[-2:]) for l in range(L)]
    locations = [compute_features_locations(h, w, shapes[l].stride, dtype=torch.float32, offset=cfg.DD3D.FEATURE_LOCATIONS_OFFSET)
                 for l, (h, w) in enumerate(feature_shapes)]
    K = torch.stack([x["intrinsics"] for x in inputs]).float()
    inv_K = K.inverse()  # core.py:93
    with torch.no_grad():
        prep = (NuscenesDD3DTargetPreparer if nusc else DD3DTargetPreparer)(cfg, shapes)
        targets = prep(locations, to_reference(gt, box3d, nusc), feature_shapes)
        losses = {}
        l2, info = FCOS2DLoss(cfg)(m("logits"), m("box2d_reg"), m("centerness"), targets)
        losses.update(l2)
        if box3d:
            losses.update(FCOS3DLoss(cfg)(m("quat"), m("ctr"), m("depth"), m("size"), m("conf"), None, inv_K, info, targets))
        if nusc:
            losses.update(NuscenesLoss(cfg)(m("attr"), m("speed"), info, targets))
    out = {"inv_K": inv_K.numpy(), "loss_keys": np.array(list(losses)), "loss_values": np.array([float(v) for v in losses.values()], np.float64)}
    out["gt_off"] = np.cumsum([0] + [len(g) for g in gt]).astype(np.int64)
    cat = lambda f: torch.cat([f(g) for g in gt]).numpy()
    out["gt_boxes"], out["gt_classes"] = cat(lambda g: g.gt_boxes.tensor.reshape(-1, 4)), cat(lambda g: g.gt_classes)
    if box3d:
        for f, k in (("quat", 4), ("proj_ctr", 2), ("depth", 1), ("size", 3)):
            out["gt_" + f] = cat(lambda g: getattr(g.gt_boxes3d, f).reshape(len(g), k))
        out["gt_inv_K"] = cat(lambda g: g.gt_boxes3d.inv_intrinsics.reshape(len(g), 3, 3))
    if nusc:
        out["gt_attributes"], out["gt_speeds"] = cat(lambda g: g.gt_attributes), cat(lambda g: g.gt_speeds)
    for k in TARGET_KEYS:
        out["t_" + k] = targets[k].numpy()
    if box3d:
        b = targets["box3d_targets"]
        for f in ("quat", "proj_ctr", "depth", "size", "inv_intrinsics"):
            out["t_box3d_" + f] = getattr(b, f).numpy()
    if nusc:
        out["t_attributes"], out["t_speeds"] = targets["attributes"].numpy(), targets["speeds"].numpy()
    path = os.path.join(HERE, f"losses_{name}.npz")
    np.savez_compressed(path, **out)
    print(name, "->", path, f"{os.path.getsize(path) / 1024:.0f} KB; positives", len(targets["pos_inds"]),
          {k: round(float(v), 6) for k, v in losses.items()})


def from_vectors_golden():
    install()
    from tridet.structures.boxes3d import Boxes3D
    rng = np.random.default_rng(5)
    K = np.array([[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]])
    vecs = [np.concatenate([q / np.linalg.norm(q), [rng.uniform(-10, 10), rng.uniform(-2, 3), rng.uniform(3, 70)], rng.uniform(0.5, 5, 3)])
            for q in rng.normal(size=(7, 4))]
    b = Boxes3D.from_vectors(vecs, K)
    e = Boxes3D.from_vectors([], K)
    out = {"vecs": np.stack(vecs), "K": K, "quat": b.quat.numpy(), "proj_ctr": b.proj_ctr.numpy(), "depth": b.depth.numpy(), "size": b.size.numpy(),
           "inv_intrinsics": b.inv_intrinsics.numpy(), "empty_shapes": np.array([tuple(t.shape) + (0, ) * (3 - t.dim()) for t in
                                                                                (e.quat, e.proj_ctr, e.depth, e.size, e.inv_intrinsics)])}
    path = os.path.join(HERE, "losses_from_vectors.npz")
    np.savez_compressed(path, **out)
    print("from_vectors ->", path)


if __name__ == "__main__":
    only = sys.argv[1:]
    for n in CASES:
        if not only or n in only:
            run_case(n)
    if not only or "from_vectors" in only:
        from_vectors_golden()
