"""Golden dense-depth loss dicts from the reference's OWN classes: tridet.modeling.dd3d.dense_depth.DD3DDenseDepth in training mode with
its real DenseDepthL1Loss, run on the CPU over the third-party shims of ref_shims.py (the recipe of make_golden.dense_depth_golden: the
shims, the `in_strides` fix, ref.train(); every norm of the config is frozen, so train == eval arithmetic).  Run in the build container
only (the reference tree does not exist on the GPU box):

    python tests/golden/make_dense_depth_loss_golden.py      ->  tests/golden/dense_depth_loss_*.npz

Each case runs the reference twice: once with an all-zero ground truth to read its own level-0 map, then with the ground truth
dd3d_amd.synthetic.make_depth_maps builds around that map (base +- d: both branches of the smooth-L1 at level 0).  A fixture holds the
loss dict, the ground-truth maps, the reference's valid-pixel count, the head's RAW per-level maps (a few hundred values per image: the
tests up-sample them with oracle.dense_depth_oracle.aligned_bilinear, which this script checks to be bit-identical to what the
reference's loss module was called with) and, per level, delta = 1e-3 * max|map| (the per-pixel bar of tests/test_dense_depth.py) and
n_cut = the number of valid pixels whose |map - gt| lies within delta of beta.

The intrinsics have a short focal length (the synthetic KITTI one x 0.1, x 0.125 for the second image), which puts the focal-scaled
level-0 map (3 .. 20) inside [MIN_DEPTH, MAX_DEPTH] and delta (0.02) well below beta, so that the ground truth stays clear of the
beta +- delta band at level 0 (make_depth_maps' `gap` = 1.05 delta).  Without focal scaling (the third case) the synthetic head's level-0
map would reach 155, outside the range and with delta above beta; that case therefore runs with the head's per-level Scale and Offset
parameters times 0.1 (`case_state_dict`: the same state dict goes to the reference and to the model under test), which puts the unscaled
level-0 map at 2.5 .. 15.5.  Every fixture has n_cut / N <= 1 % at every level (asserted here and in tests/test_dense_depth_loss.py).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

EXPERIMENT, CALIB = "dd3d_kitti_dla34", "dla34_kitti"
B, H, W = 2, 128, 256
GT_SEED = 3000
BASE_OVERRIDES = {"MODEL": {"META_ARCHITECTURE": "DD3DDenseDepth"},
                  "DD3D": {"IN_FEATURES": ["p3", "p4", "p5", "p6", "p7"], "FCOS3D": {"DEPTH_HEAD": {"LOSS_TYPE": "L1", "LOSS_WEIGHT": 1.0}}}}
# name -> overrides on top of BASE_OVERRIDES; every case is the ragged batch (second image smaller than the canvas)
CASES = {
    "ragged": {},
    "ragged_min0": {"DD3D": {"FCOS3D": {"MIN_DEPTH": 0.0}}},  # the padding (and every no-return pixel) counts
    "half_noscale": {"DD3D": {"FEATURE_LOCATIONS_OFFSET": "half", "FCOS3D": {"SCALE_DEPTH_BY_FOCAL_LENGTHS": False}}},
}


# name -> factor on the head's Scale / Offset parameters (the range of the raw per-level maps)
HEAD_RANGE = {"half_noscale": 0.1}


def case_state_dict(name, sd):
    """The synthetic state dict of a case: `sd` with the dense-depth head's output range adjusted where the case asks for it."""
    f = HEAD_RANGE.get(name)
    if f is None:
        return sd
    out = dict(sd)
    for k, v in sd.items():
        if k.startswith("fcos3d_head.scales_depth.") or k.startswith("fcos3d_head.offsets_depth."):
            out[k] = v * f
    return out


def fixture_path(name):
    return os.path.join(HERE, f"dense_depth_loss_{name}.npz")


def _merge(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = _merge(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else v
    return out


def case_overrides(name):
    return _merge(BASE_OVERRIDES, CASES[name])


def case_inputs():
    """The ragged batch of every case, without ground truth."""
    from dd3d_amd.synthetic import make_inputs
    inputs = make_inputs(B, H, W)
    for x, s in zip(inputs, (0.1, 0.125)):
        x["intrinsics"] = x["intrinsics"] * torch.tensor([[s], [s], [1.0]])
    inputs[1]["image"] = inputs[1]["image"][:, :H - 13, :W - 22].contiguous()
    inputs[1]["height"], inputs[1]["width"] = H - 13, W - 22
    return inputs


def golden(name):
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import META_ARCH_REGISTRY, get_cfg
    from dd3d_amd.synthetic import load_calib, make_depth_maps, make_state_dict
    from oracle.dense_depth_oracle import aligned_bilinear
    from tests.golden import ref_shims
    from tests.golden.make_golden import TRAINING_ONLY_KEYS
    cfg = get_cfg(EXPERIMENT, _merge(TRAINING_ONLY_KEYS, case_overrides(name)))
    ours = META_ARCH_REGISTRY.get("DD3DDenseDepth")(cfg)
    sd = case_state_dict(name, make_state_dict(ours, calib=load_calib(CALIB)))
    assert any(k.startswith("fcos3d_head.scales_depth.") for k in sd) and any(k.startswith("fcos3d_head.offsets_depth.") for k in sd)
    ref_shims.install()
    sys.modules["detectron2.config.config"] = sys.modules["detectron2.config"]
    from tridet.modeling.dd3d.dense_depth import DD3DDenseDepth
    ref = DD3DDenseDepth(cfg)
    ref.load_state_dict(sd, strict=True)
    ref.train()
    # the released class reads self.in_strides in forward (dense_depth.py:142) but only its HEAD defines it (make_golden.dense_depth_golden)
    ref.in_strides = ref.fcos3d_head.in_strides
    raw, preds, gts = [], [], []
    ref.fcos3d_head.register_forward_hook(lambda mod, args, out: raw.append([t.detach().clone() for t in out]))
    ref.depth_loss.register_forward_pre_hook(lambda mod, args: (preds.append(args[0].detach().clone()), gts.append(args[1].detach().clone())) and None)
    c3 = cfg.DD3D.FCOS3D
    beta = float(c3.LOSS.SMOOTH_L1_BETA)
    inputs = case_inputs()
    for x in inputs:
        x["depth"] = torch.zeros(x["image"].shape[-2:])
    with torch.no_grad():
        ref(inputs)
    level0 = preds[0]
    delta0 = 1e-3 * float(level0.abs().max())
    gap = 1.05 * delta0 if 1.05 * delta0 < 0.8 * beta else 1e-3
    # (the ground truth is built for the config's released range, whatever the case's MIN_DEPTH override)
    depth = make_depth_maps(inputs, seed=GT_SEED, valid_fraction=0.5, base=[level0[i] for i in range(B)], min_depth=0.1,
                            max_depth=float(c3.MAX_DEPTH), beta=beta, gap=gap)
    for x, d in zip(inputs, depth):
        x["depth"] = d
    del raw[:], preds[:], gts[:]
    with torch.no_grad():
        losses = ref(inputs)
    L = len(losses)
    assert len(preds) == L == 5 and len(raw) == 1 and list(losses) == [f"loss_dense_depth_lvl_{l}" for l in range(L)]
    gt = gts[0]
    assert gt.shape == (B, H, W) and all(torch.equal(g_, gt) for g_ in gts)
    M = ((gt < ref.depth_loss.min_depth).to(torch.float32) + (gt > ref.depth_loss.max_depth).to(torch.float32)) == 0.  # dense_depth_loss.py:29-33
    # the oracle's up-sampling of the raw maps is what the reference's loss module saw, bit for bit
    offset = cfg.DD3D.FEATURE_LOCATIONS_OFFSET
    K = torch.stack([x["intrinsics"] for x in inputs])
    for l, (r, s) in enumerate(zip(raw[0], ref.in_strides)):
        m = aligned_bilinear(r, s, offset).squeeze(1)
        if c3.SCALE_DEPTH_BY_FOCAL_LENGTHS:
            inv_K = K.inverse()
            px = torch.norm(torch.stack([inv_K[:, 0, 0], inv_K[:, 1, 1]], dim=-1), dim=-1)
            m = m / (px * c3.SCALE_DEPTH_BY_FOCAL_LENGTHS_FACTOR).reshape(-1, 1, 1)
        assert torch.equal(m, preds[l]), f"level {l}: the oracle's up-sampling differs from the reference's"
    delta = [1e-3 * float(p.abs().max()) for p in preds]
    n_cut = [int((((p[M] - gt[M]).abs() - beta).abs() <= d).sum()) for p, d in zip(preds, delta)]
    assert all(n <= 0.01 * int(M.sum()) for n in n_cut), (n_cut, int(M.sum()))
    out = {"losses": np.array([float(v) for v in losses.values()], dtype=np.float32), "valid_count": np.int64(int(M.sum())),
           "delta": np.array(delta, dtype=np.float64), "n_cut": np.array(n_cut, dtype=np.int64), "gap": np.float64(gap)}
    for i, d in enumerate(depth):
        out[f"gt{i}"] = d.numpy()
    for l, r in enumerate(raw[0]):
        out[f"raw{l}"] = r.numpy()
    path = fixture_path(name)
    np.savez_compressed(path, **out)
    print(name, "->", path, f"{os.path.getsize(path) / 1024:.0f} KB; valid {int(M.sum())} of {M.numel()}, losses", out["losses"].tolist(), "delta",
          [round(d, 4) for d in delta], "n_cut", n_cut, "gap", round(gap, 4), "level-0 range", float(level0.min()), float(level0.max()))


if __name__ == "__main__":
    for name in (sys.argv[1:] or list(CASES)):
        golden(name)
