"""Deterministic synthetic weights and inputs (there are no datasets / checkpoints offline).

SURVEY.md section 8d: seeded reference-style initialisation, *randomised* (Frozen)BN statistics so that norm folding
is really exercised, and classifier gains calibrated once (offline, tests/golden/calibrate_synthetic.py ->
dd3d_amd/data/synth_calib_*.json) so that roughly 1 % of the (location, class) scores pass PRE_NMS_THRESH --
otherwise a random network yields no candidates (or all of them) and decode / NMS are not exercised.

Used by bench.py, __graft_entry__.smoke() and the tests; the same state_dict feeds the HIP path and the oracle.
"""
import json
import os

import torch

_DATA_DIR = os.path.join(os.path.dirname(__file__), "data")

KITTI_K = [[721.5377, 0.0, 609.5593], [0.0, 721.5377, 172.854], [0.0, 0.0, 1.0]]  # KITTI cam-2 intrinsics
NUSC_K = [[1266.4, 0.0, 816.3], [0.0, 1266.4, 491.5], [0.0, 0.0, 1.0]]


def calib_path(tag):
    """The package ships the calibrations of the four benchmarked / tested configurations (DLA-34 and V2-99, KITTI and nuScenes); the
    other backbone specs' files live with the tests that emulate them (tests/data, named by DD3D_CALIB_DIR -- tests/conftest.py)."""
    p = os.path.join(_DATA_DIR, f"synth_calib_{tag}.json")
    extra = os.environ.get("DD3D_CALIB_DIR")
    if not os.path.exists(p) and extra and os.path.exists(os.path.join(extra, f"synth_calib_{tag}.json")):
        return os.path.join(extra, f"synth_calib_{tag}.json")
    return p


SHIPPED_CALIBS = ("dla34_kitti", "dla34_nusc", "v99_kitti", "v99_nusc")


def load_calib(tag, required=False):
    """Calibration of one synthetic configuration ({} when there is none: the state dict is then uncalibrated and a random network
    yields no candidates -- or all of them).  `required`: raise instead, naming where the file is expected."""
    p = calib_path(tag)
    if os.path.exists(p):
        with open(p) as f:
            return json.load(f)
    if required:
        raise FileNotFoundError(
            f"no synthetic calibration '{tag}': the package ships {', '.join(SHIPPED_CALIBS)} (dd3d_amd/data/synth_calib_*.json); the other "
            "backbone specs' files live under tests/data and are found through DD3D_CALIB_DIR (tests/conftest.py sets it) -- "
            f"expected {os.path.basename(p)} in {_DATA_DIR} or $DD3D_CALIB_DIR={os.environ.get('DD3D_CALIB_DIR')!r}")
    return {}


def make_state_dict(model, seed=0, calib=None):
    """Return a CPU state_dict for ``model`` (any dd3d_amd meta-arch): conv weights keep the model's own seeded
    initialisation (re-drawn here under ``seed``), every norm gets random affine + statistics.
    ``calib`` maps a norm prefix -> [mean, std] of its input activation (measured once with the oracle) and the
    predictor prefixes -> [gain, bias]."""
    from dd3d_amd.layers import BatchNorm2d, Conv2d, FrozenBatchNorm2d
    calib = calib or {}
    g = torch.Generator().manual_seed(seed)
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    for name, mod in model.named_modules():
        if isinstance(mod, Conv2d):
            w = sd[name + ".weight"]
            fan_out = w.shape[0] * w.shape[2] * w.shape[3]
            fan_in = w.shape[1] * w.shape[2] * w.shape[3]
            is_pred = mod.norm is None and mod.bias is not None and name.split(".")[0] in ("fcos2d_head", "fcos3d_head") \
                or name in ("attr_logits", "speed") or ".box3d_depth." in name
            if is_pred:  # kaiming_uniform_(a=1): U(-sqrt(3/fan_in), +)
                bound = (3.0 / fan_in)**0.5
                w.copy_((torch.rand(w.shape, generator=g) * 2 - 1) * bound)
            else:  # kaiming_normal_(fan_out, relu)
                w.copy_(torch.randn(w.shape, generator=g) * (2.0 / fan_out)**0.5)
            if name + ".bias" in sd:
                sd[name + ".bias"].copy_(torch.randn(w.shape[0], generator=g) * 0.02)
            if name in calib:  # predictor gain / bias
                gain, bias = calib[name]
                w.mul_(gain)
                if name + ".bias" in sd:
                    sd[name + ".bias"].add_(bias)
        elif isinstance(mod, (BatchNorm2d, FrozenBatchNorm2d)):
            n = mod.num_features
            m0, s0, gain = (list(calib.get(name, [0.0, 1.0])) + [1.0])[:3]  # gain: per-level equalisation of the logits
            sd[name + ".weight"].copy_((torch.rand(n, generator=g) + 0.5) * gain)
            sd[name + ".bias"].copy_(torch.randn(n, generator=g) * 0.1 * gain)
            sd[name + ".running_mean"].copy_(m0 + torch.randn(n, generator=g) * 0.1 * s0)
            sd[name + ".running_var"].copy_((torch.rand(n, generator=g) + 0.5) * s0 * s0)
    return sd


def make_inputs(B=1, H=384, W=1280, dataset="kitti", seed=1000, out_hw=None, device="cpu"):
    """``batched_inputs`` with the schema of DefaultDatasetMapper (tridet/data/dataset_mappers/dataset_mapper.py:100-201):
    uint8 (3,H,W) BGR ``image``, 3x3 float32 ``intrinsics`` (already adjusted for the resize), ``height``/``width``."""
    if dataset == "kitti":
        K = torch.tensor(KITTI_K) * torch.tensor([[1270.0 / 1224.0], [384.0 / 370.0], [1.0]])
    else:
        K = torch.tensor(NUSC_K) * torch.tensor([[1593.0 / 1600.0], [896.0 / 900.0], [1.0]])
    out = []
    for i in range(B):
        g = torch.Generator().manual_seed(seed + i)
        img = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g)
        d = {"image": img.to(device), "intrinsics": K.clone().float(), "height": H, "width": W, "image_id": i,
             "file_name": f"synthetic_{seed + i}.png"}
        if out_hw is not None:
            d["height"], d["width"] = out_hw
        if dataset != "kitti":
            # nuScenes-shaped extras (dataset_mapper.py:155-165): 6 cameras per sample (yaw 0, +-55, +-110, 180 deg around the
            # vertical axis of the ego frame, composed with the camera-to-vehicle axis swap) times one ego pose per sample
            from dd3d_amd.structures import Pose
            cam, sample = i % 6, i // 6
            yaw = [0.0, 55.0, -55.0, 110.0, -110.0, 180.0][cam]
            cam_to_vehicle = Pose((0.5, -0.5, 0.5, -0.5), (1.5, 0.2 * (cam - 2.5), 1.6))  # z fwd, x right, y down -> x fwd, y left, z up
            ego = Pose.from_yaw(17.0 * sample + 5.0, (410.0 + 13.0 * sample, 1180.0 - 7.0 * sample, 0.0))
            d["pose"] = ego * Pose.from_yaw(yaw) * cam_to_vehicle
            d["sample_token"] = f"s{sample}"
        out.append(d)
    return out


def make_gt_instances(inputs, num_classes, canonical_sizes, seed=2000, n_per_image=24, empty_images=(), quirk_images=(), num_attributes=None):
    """Seeded ground truth for `inputs` (make_inputs' batch): per image an ``Instances`` with gt_boxes, gt_classes and gt_boxes3d
    (built by Boxes3D.from_vectors from float64 intrinsics, as tridet/data/transform_utils.py:116 does) and, with `num_attributes`,
    gt_attributes / gt_speeds (nuScenes; attribute == num_attributes means "none", some speeds NaN, half of them below 0.08 m/s).  The boxes cover every FPN
    level's size range, include pairs of equal area and edges on the stride-8 grid (locations exactly on a box edge);
    `empty_images` get no GT, `quirk_images` a FIRST box with x1 + x2 == 0 (prepare_targets.py:190)."""
    import numpy as np
    from dd3d_amd.structures import Boxes, Boxes3D, Instances
    out = []
    for i, x in enumerate(inputs):
        H, W = int(x["image"].shape[-2]), int(x["image"].shape[-1])
        K = np.asarray(x["intrinsics"], dtype=np.float64)
        rng = np.random.default_rng(seed + i)
        n = 0 if i in empty_images else n_per_image
        boxes = []
        for j in range(n):
            side = float(np.exp(rng.uniform(np.log(6.0), np.log(max(H, W) * 1.2))))  # every size range, [-1, 64] .. [512, INF]
            w, h = side * rng.uniform(0.6, 1.4), side * rng.uniform(0.6, 1.4)
            cx, cy = rng.uniform(0, W), rng.uniform(0, H)
            b = [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2]
            if j % 4 == 1:  # edges on the location grid
                b = [float(np.round(v / 8.0) * 8.0) for v in b]
                if b[2] <= b[0]:
                    b[2] = b[0] + 8.0
                if b[3] <= b[1]:
                    b[3] = b[1] + 8.0
            if j % 6 == 5 and boxes:  # the same width and height as the previous box, shifted: equal areas on the overlap
                p = boxes[-1]
                dx, dy = float(np.round(rng.uniform(-0.3, 0.3) * (p[2] - p[0]))), float(np.round(rng.uniform(-0.3, 0.3) * (p[3] - p[1])))
                b = [p[0] + dx, p[1] + dy, p[2] + dx, p[3] + dy]
            boxes.append(b)
        if n and i in quirk_images:
            half = (boxes[0][2] - boxes[0][0]) / 2.0
            boxes[0] = [-half, boxes[0][1], half, boxes[0][3]]
        boxes = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
        classes = rng.integers(0, num_classes, size=n)
        vecs = []
        for j in range(n):
            q = rng.normal(size=4)
            q /= np.linalg.norm(q)
            z = rng.uniform(4.0, 60.0)
            u, v = (boxes[j, 0] + boxes[j, 2]) / 2.0, (boxes[j, 1] + boxes[j, 3]) / 2.0
            t = np.linalg.solve(K, np.array([u, v, 1.0])) * z
            size = np.asarray(canonical_sizes[classes[j]], dtype=np.float64) * rng.uniform(0.7, 1.3, size=3)
            vecs.append(np.concatenate([q, t, size]))
        inst = Instances((H, W))
        inst.gt_boxes = Boxes(torch.from_numpy(boxes))
        inst.gt_classes = torch.from_numpy(classes.astype(np.int64))
        inst.gt_boxes3d = Boxes3D.from_vectors(vecs, K)
        if num_attributes is not None:
            inst.gt_attributes = torch.from_numpy(rng.integers(0, num_attributes + 1, size=n).astype(np.int64))
            sp = rng.uniform(0.0, 12.0, size=n).astype(np.float32)
            slow = rng.uniform(size=n) < 0.5  # slow objects: errors on both sides of the speed loss's beta (0.05) for predictions near 0
            sp[slow] = rng.uniform(0.0, 0.08, size=int(slow.sum())).astype(np.float32)
            sp[rng.uniform(size=n) < 0.25] = np.nan
            inst.gt_speeds = torch.from_numpy(sp)
        out.append(inst)
    return out


def make_depth_maps(inputs, seed=3000, valid_fraction=0.5, base=None, min_depth=0.1, max_depth=80.0, beta=0.05, below_fraction=0.05,
                    above_fraction=0.10, gap=1e-3):
    """Seeded, LiDAR-like sparse ground-truth depth for `inputs` (make_inputs' batch; DD3DDenseDepth.compute_losses reads it as
    x["depth"]): per image a float32 (Hi, Wi) map that is 0 where there is no return, below `min_depth` on `below_fraction` of the
    pixels (min_depth - U(0.01, 1): negative values and, for min_depth > 0.01, small positive ones), above `max_depth` on
    `above_fraction` of them, and inside the range on `valid_fraction` of them.

    Without `base` the in-range values are uniform over the range.  With `base` (per image a map of at least the image's size, e.g. a
    level of predict_dense_depth) they are base +- d, on pixels whose base value lies far enough inside the range for that (fewer than
    `valid_fraction` of the pixels when the base leaves the range on many): |d| is below `beta` on about half of them and above it on the
    others, so that a prediction equal to `base` takes both branches of the smooth-L1, and no pixel has | |d| - beta | < gap -- counted on
    the float32 difference of the stored value and the base."""
    out = []
    for i, x in enumerate(inputs):
        H, W = int(x["image"].shape[-2]), int(x["image"].shape[-1])
        n = H * W
        g = torch.Generator().manual_seed(seed + i)
        perm = torch.randperm(n, generator=g)
        rand = lambda k: torch.rand(k, generator=g)
        n_below, n_above, n_valid = int(below_fraction * n), int(above_fraction * n), int(valid_fraction * n)
        below, above, rest = perm[:n_below], perm[n_below:n_below + n_above], perm[n_below + n_above:]
        depth = torch.zeros(n, dtype=torch.float32)
        depth[below] = min_depth - (0.01 + 0.99 * rand(n_below))
        depth[above] = max_depth + 0.01 + 40.0 * rand(n_above)
        if base is None:
            idx = rest[:n_valid]
            depth[idx] = min_depth + 0.01 + (max_depth - min_depth - 0.02) * rand(idx.numel())
        else:
            b = torch.as_tensor(base[i]).detach().to("cpu", torch.float32)[:H, :W].reshape(-1)
            assert b.numel() == n, f"base map {i} is smaller than its image"
            margin = 4.0 * beta + gap
            ok = (b[rest] > min_depth + margin) & (b[rest] < max_depth - margin)
            idx = rest[ok][:n_valid]
            k = idx.numel()
            slack = 1e-5 + 1e-6 * max(abs(min_depth), abs(max_depth))  # the stored sum is rounded to float32: |d| moves by half an ulp of the base
            lo = rand(k) * max(beta - gap - slack, 0.0)
            hi = beta + gap + slack + rand(k) * (3.0 * beta - gap - slack)
            mag = torch.where(rand(k) < 0.5, lo, hi)
            sign = torch.where(rand(k) < 0.5, -torch.ones(k), torch.ones(k))
            depth[idx] = b[idx] + sign * mag
            assert bool((((depth[idx] - b[idx]).abs() - beta).abs() >= gap).all())
        out.append(depth.reshape(H, W))
    return out
