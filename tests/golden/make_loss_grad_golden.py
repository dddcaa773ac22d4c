"""Golden head-map gradients from the reference's OWN loss modules: FCOS2DLoss, FCOS3DLoss and NuscenesLoss run on the CPU over the
shims of ref_shims.py (as make_loss_golden.py runs them), on the committed reference head maps as leaves that require grad, and
torch autograd of the sum of the returned loss dict.  The shim's scipy matrix_to_quaternion detaches; it is replaced here by the
differentiable statement of pytorch3d's function (oracle/dd3d_oracle.py), before the reference's geometry module is imported.  Stored per
case: the positives' rows of every family (level-first target order, as the losses flatten the maps) and the dense logits gradient --
every other row is zero.  Run in the build container only (the reference tree does not exist on the GPU box):

    python tests/golden/make_loss_grad_golden.py      ->  tests/golden/loss_grads_*.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests.golden import make_loss_golden as MG  # noqa: E402
from tests.golden.make_golden import case_inputs  # noqa: E402

CASES = ("kitti_ragged", "kitti_ragged_nopos", "nusc_b6", "kitti_variant_egocentric_agnostic")
FAMILIES = ("logits", "box2d_reg", "centerness", "quat", "ctr", "depth", "size", "conf", "attr", "speed")


def install():
    MG.install()
    from oracle.dd3d_oracle import matrix_to_quaternion
    sys.modules["pytorch3d.transforms.rotation_conversions"].matrix_to_quaternion = matrix_to_quaternion
    geo = sys.modules.get("tridet.utils.geometry")
    if geo is not None and hasattr(geo, "matrix_to_quaternion"):
        geo.matrix_to_quaternion = matrix_to_quaternion


def run_case(name):
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import META_ARCH_REGISTRY, get_cfg
    maps_file, exp, over, ci, opts = MG.CASES[name]
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
    fams = [k for k in FAMILIES if f"{k}0" in z.files and (box3d or k in FAMILIES[:3]) and (nusc or k not in FAMILIES[8:])]
    leaf = {k: [torch.from_numpy(z[f"{k}{l}"]).clone().requires_grad_(True) for l in range(L)] for k in fams}
    m = lambda k: MG.LevelList(leaf[k])
    inputs = case_inputs(*ci)
    gt = MG.gt_instances(model, inputs, opts)
    shapes = model.backbone_output_shape
    feature_shapes = [tuple(z[f"logits{l}"].shape[-2:]) for l in range(L)]
    locations = [compute_features_locations(h, w, shapes[l].stride, dtype=torch.float32, offset=cfg.DD3D.FEATURE_LOCATIONS_OFFSET)
                 for l, (h, w) in enumerate(feature_shapes)]
    inv_K = torch.stack([x["intrinsics"] for x in inputs]).float().inverse()
    with torch.no_grad():
        prep = (NuscenesDD3DTargetPreparer if nusc else DD3DTargetPreparer)(cfg, shapes)
        targets = prep(locations, MG.to_reference(gt, box3d, nusc), feature_shapes)
    losses = {}
    l2, info = FCOS2DLoss(cfg)(m("logits"), m("box2d_reg"), m("centerness"), targets)
    losses.update(l2)
    if box3d:
        losses.update(FCOS3DLoss(cfg)(m("quat"), m("ctr"), m("depth"), m("size"), m("conf"), None, inv_K, info, targets))
    if nusc:
        losses.update(NuscenesLoss(cfg)(m("attr"), m("speed"), info, targets))
    flat_leaves = [t for k in fams for t in leaf[k]]
    grads = torch.autograd.grad(sum(losses.values()), flat_leaves, allow_unused=True)
    grads = [torch.zeros_like(t) if g is None else g for t, g in zip(flat_leaves, grads)]
    pos = targets["pos_inds"]
    out = {"pos_inds": pos.numpy(), "loss_keys": np.array(list(losses)), "loss_values": np.array([float(v) for v in losses.values()], np.float64)}
    for i, k in enumerate(fams):
        g = torch.cat([x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]) for x in grads[i * L:(i + 1) * L]])  # fcos2d.py:179-181
        assert bool(torch.isfinite(g).all()), k
        if k == "logits":
            out["dense_logits"] = g.numpy()
        else:
            rest = torch.ones(g.shape[0], dtype=torch.bool)
            rest[pos] = False
            assert float(g[rest].abs().max() if rest.any() else 0.0) == 0.0, k  # nothing off the positives
            out["pos_" + k] = g[pos].numpy()
    path = os.path.join(HERE, f"loss_grads_{name}.npz")
    np.savez_compressed(path, **out)
    print(name, "->", path, f"{os.path.getsize(path) / 1024:.0f} KB; positives", len(pos))


if __name__ == "__main__":
    only = sys.argv[1:]
    for n in CASES:
        if not only or n in only:
            run_case(n)
