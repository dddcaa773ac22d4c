"""Golden tower gradients under BATCH statistics from the reference's OWN modules: make_tower_grad_golden.py with `ref.fcos2d_head.train()`
and everything else in eval() -- the released configs' training forward, where cls_tower and box2d_tower (DD3D.FCOS2D.NORM: BN) normalise
with the batch's mean and variance per pyramid level and FCOS3D (FrozenBN) keeps its running statistics.  Same seeded FPN features of a
64 x 128 canvas, target preparer, loss modules and torch autograd of the sum of the loss dict with the five features as leaves.  Stored
per case: the loss values, the gradient of every tower parameter under its state-dict name and the gradient at the five features (of a
tensor with more than SAMPLE_CAP entries a seeded sample of positions, predictor_grad_cases.tower_sample), and the running statistics the
one training forward leaves in the eight norms x five levels of the two BN towers.  Needs the reference tree; no test runs it:

    python tests/golden/make_tower_bn_golden.py      ->  tests/golden/tower_bn_grads_*.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

from tests import predictor_grad_cases as PC  # noqa: E402
from tests import tower_grad_oracle as TO  # noqa: E402
from tests.golden import make_loss_golden as MG  # noqa: E402
from tests.golden.make_golden import build_reference_model  # noqa: E402
from tests.golden.make_loss_grad_golden import install  # noqa: E402


def run_case(name):
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import get_cfg
    exp, tag, B, ds = PC.REFERENCE_CASES[name]
    cfg = get_cfg(exp)
    sd, feats, inputs, gt = PC.reference_inputs(name)
    install()
    ref = build_reference_model(cfg)
    install()  # (the model's import of the geometry module happened in between: patch its matrix_to_quaternion as well)
    ref.load_state_dict(sd, strict=True)
    ref.eval()
    ref.fcos2d_head.train()  # the BN towers: batch statistics, and the running ones move
    nusc = hasattr(ref, "attr_logits")
    for p in ref.parameters():
        p.requires_grad_(True)
    feats = [f.clone().requires_grad_(True) for f in feats]
    from tridet.utils.tensor2d import compute_features_locations
    logits, box2d_reg, centerness, extra = ref.fcos2d_head(feats)
    quat, ctr, depth, size, conf, _ = ref.fcos3d_head(feats)
    shapes = ref.backbone_output_shape
    feature_shapes = [tuple(f.shape[-2:]) for f in feats]
    locations = [compute_features_locations(h, w, shapes[l].stride, dtype=torch.float32, offset=cfg.DD3D.FEATURE_LOCATIONS_OFFSET)
                 for l, (h, w) in enumerate(feature_shapes)]
    inv_K = torch.stack([x["intrinsics"] for x in inputs]).float().inverse()
    with torch.no_grad():
        targets = ref.prepare_targets(locations, MG.to_reference(gt, True, nusc), feature_shapes)
    m = MG.LevelList
    losses = {}
    l2, info = ref.fcos2d_loss(m(logits), m(box2d_reg), m(centerness), targets)
    losses.update(l2)
    losses.update(ref.fcos3d_loss(m(quat), m(ctr), m(depth), m(size), m(conf), None, inv_K, info, targets))
    if nusc:
        attr = [ref.attr_logits(x) for x in extra["cls_tower_out"]]
        speed = [ref.speed(x) for x in extra["cls_tower_out"]]
        losses.update(ref.nuscenes_loss(m(attr), m(speed), info, targets))
    sum(losses.values()).backward()
    out = {"loss_keys": np.array(list(losses)), "loss_values": np.array([float(v) for v in losses.values()], np.float64),
           "pos_inds": targets["pos_inds"].numpy()}
    named = dict(ref.named_parameters())
    for k in sorted(named):
        if TO.TOWER_PARAM.match(k):
            g = named[k].grad
            assert g is not None and bool(torch.isfinite(g).all()), k
            out["param:" + k] = g.reshape(-1)[PC.tower_sample(g.shape)].numpy()
    for l, f in enumerate(feats):
        out[f"feature:{l}"] = f.grad.reshape(-1)[PC.tower_sample(f.shape)].numpy()
    moved = 0
    for k, v in ref.state_dict().items():
        if k.startswith(("fcos2d_head.cls_tower", "fcos2d_head.box2d_tower")) and k.endswith(("running_mean", "running_var")):
            out["stat:" + k] = v.detach().numpy().copy()
            moved += int(not torch.equal(v, sd[k]))
    assert moved == 2 * 8 * len(feats), moved  # every norm of the two towers saw exactly its own level
    path = os.path.join(HERE, f"tower_bn_grads_{name}.npz")
    np.savez_compressed(path, **out)
    print(name, "->", path, f"{os.path.getsize(path) / 1024:.0f} KB; positives", len(targets["pos_inds"]),
          {k: round(float(v), 5) for k, v in losses.items()}, "tower parameters", sum(k.startswith("param:") for k in out))


if __name__ == "__main__":
    only = sys.argv[1:]
    for n in PC.REFERENCE_CASES:
        if not only or n in only:
            run_case(n)
