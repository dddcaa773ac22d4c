"""Cases shared by the CPU and GPU tests of the loss backward: the committed reference head maps of tests/test_losses_gpu.GOLDEN_CASES
with seeded ground truth (at the released settings, at every row of SETTINGS, and with one poisoned quaternion that switches the batch
to the renormalised decode), the reference-golden cases, and hand-built maps that put one positive on each non-smooth point of the loss
or saturate the focal loss.
Everything here is built on the CPU; the float64 / float32 autograd references are computed once per case and shared."""
import functools
import os

import numpy as np
import torch

from tests import loss_grad_oracle as GO
from tests import loss_oracle as LO

# Settings rows: every loss setting of dd3d_loss_args away from its released value, one group per row (config overrides).  The table
# stands above the import of tests.test_losses_gpu because that module parametrises over it and imports this one in turn.
_F2, _F3 = (lambda d: {"DD3D": {"FCOS2D": {"LOSS": d}}}), (lambda d: {"DD3D": {"FCOS3D": {"LOSS": d}}})
_PT = lambda d: {"DD3D": {"FCOS3D": {"PREPARE_TARGET": d}}}
SETTINGS = {
    "gamma1.5_alpha_off": _F2({"ALPHA": -1.0, "GAMMA": 1.5}),
    "gamma0_alpha0.6": _F2({"ALPHA": 0.6, "GAMMA": 0.0}),
    "gamma1": _F2({"GAMMA": 1.0}),
    "gamma3": _F2({"GAMMA": 3.0}),
    "beta_tiny": _F3({"SMOOTH_L1_BETA": 1e-6}),
    "beta0.5_T3_weights": _F3({"SMOOTH_L1_BETA": 0.5, "CONF_3D_TEMPERATURE": 3.0, "WEIGHT_BOX3D": 0.7, "WEIGHT_CONF3D": 1.3}),
    "no_center_sample": _PT({"CENTER_SAMPLE": False}),
    "radius2.5_depth1_40": {"DD3D": {"FCOS3D": {"PREPARE_TARGET": {"POS_RADIUS": 2.5}, "MIN_DEPTH": 1.0, "MAX_DEPTH": 40.0}}},
    "radius0.5": _PT({"POS_RADIUS": 0.5}),
}
SETTINGS_KITTI, SETTINGS_NUSC = "dla34_kitti_128x384_b2_ragged", "dla34_nusc_128x224_b6"
NUSC_WEIGHTS = {"DD3D": {"NUSC": {"LOSS": {"WEIGHT_ATTR": 0.4, "WEIGHT_SPEED": 2.5}}}}  # added to every nuScenes row
SETTINGS_ROWS = [(SETTINGS_KITTI, k) for k in SETTINGS] + [(SETTINGS_NUSC, k) for k in ("gamma1.5_alpha_off", "beta0.5_T3_weights", "no_center_sample")]
SATURATED_GAMMAS = (0.0, 1.0, 1.5, 2.0, 3.0)
POISONED_CASES = (SETTINGS_KITTI, SETTINGS_NUSC)

from tests.test_losses_gpu import GOLDEN_CASES  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
MAP_KEYS = GO.FAMILIES
# GT seed per case: chosen on the CPU so that at most 3 % of the positives sit within the kink margin (test_loss_grads.py counts them)
GT_SEEDS = {name: 2000 for name in GOLDEN_CASES}
KINK_CAP = 0.03


def merged(*overrides):
    """The config overrides (nested dicts, None allowed) merged in order into a new dict."""
    out = {}
    for o in overrides:
        for k, v in (o or {}).items():
            out[k] = merged(out.get(k), v) if isinstance(v, dict) else v
    return out


def cpu_model(exp, overrides=None):
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import META_ARCH_REGISTRY, get_cfg
    cfg = get_cfg(exp, overrides)
    return META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg).eval()


def oracle_targets(model, level_hw, gt):
    from dd3d_amd.engine.losses import feature_locations
    strides = [s.stride for s in model.backbone_output_shape]
    locs = [feature_locations(h, w, strides[l], model.feature_locations_offset) for l, (h, w) in enumerate(level_hw)]
    nusc, box3d = hasattr(model, "attr_logits"), not model.only_box2d
    pt = model.cfg.DD3D.FCOS3D.PREPARE_TARGET
    return LO.prepare_targets(locs, LO.gt_dicts(gt, box3d, nusc), strides, model.num_classes, list(model.cfg.DD3D.SIZES_OF_INTEREST),
                              bool(pt.CENTER_SAMPLE), float(pt.POS_RADIUS), box3d, nusc, model.attr_logits.out_channels if nusc else 3)


class Case:
    """model (CPU), maps (NCHW, float32), gt, level_hw, inv_K (B, 3, 3), targets and settings of the oracle; g64 / g32 / kink lazily."""
    def __init__(self, model, maps, gt, level_hw, inv_K):
        self.model, self.maps, self.gt, self.level_hw, self.inv_K = model, maps, gt, level_hw, inv_K
        self.targets = oracle_targets(model, level_hw, gt)
        self.p = dict(LO.settings(model), num_levels=len(level_hw))
        self._ref = {}

    @property
    def num_pos(self):
        return int(self.targets["pos_inds"].numel())

    def ref(self, dtype=torch.float64, upstream=None):
        key = (dtype, None if upstream is None else tuple(float(v) for v in upstream))
        if key not in self._ref:
            self._ref[key] = GO.head_grads(self.maps, self.targets, self.inv_K, self.p, upstream, dtype)
        return self._ref[key]

    def losses(self, dtype=torch.float32):
        """The loss dict of LO.losses on the case's maps in `dtype`, computed once."""
        key = ("losses", dtype)
        if key not in self._ref:
            maps = {k: v.to(dtype) for k, v in self.maps.items()}
            with torch.no_grad():
                self._ref[key] = LO.losses(maps, GO._cast(self.targets, dtype), self.inv_K.to(dtype), self.p)
        return self._ref[key]

    @functools.cached_property
    def kink(self):
        return GO.near_kink(self.maps, self.targets, self.inv_K, self.p)

    def keep_rows(self):
        """Rows (targets) compared against the bar: everything but the positives within the kink margin."""
        keep = torch.ones(self.targets["labels"].numel(), dtype=torch.bool)
        keep[self.targets["pos_inds"][self.kink]] = False
        return keep


def _maps_of(z, model):
    box3d = not model.only_box2d
    return {k: torch.from_numpy(z[k]) for k in z.files if k[:-1] in MAP_KEYS and (box3d or k[:-1] in ("logits", "box2d_reg", "centerness"))}


def _committed_case(name, extra=None):
    from dd3d_amd.synthetic import make_gt_instances, make_inputs
    exp, over, ds, sizes = GOLDEN_CASES[name]
    model = cpu_model(exp, merged(over, extra) or None)
    maps = _maps_of(np.load(os.path.join(GOLDEN, name + ".npz")), model)
    B = maps["logits0"].shape[0]
    inputs = make_inputs(B, sizes[0][0], sizes[0][1], dataset=ds)
    for x, (h, w) in zip(inputs, sizes):
        x["image"] = x["image"][:, :h, :w]
    nusc = hasattr(model, "attr_logits")
    gt = make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, seed=GT_SEEDS[name],
                           num_attributes=model.attr_logits.out_channels if nusc else None, empty_images=(1, ) if B > 2 else (),
                           quirk_images=(B - 1, ) if B > 3 else ())
    level_hw = [tuple(maps[f"logits{l}"].shape[-2:]) for l in range(len([k for k in maps if k.startswith("logits")]))]
    K = torch.stack([x["intrinsics"] for x in inputs]).float()
    return Case(model, maps, gt, level_hw, torch.linalg.inv(K))


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """A case of tests/test_losses_gpu.GOLDEN_CASES: the committed reference head maps with seeded synthetic GT (an image without GT
    and a quirk image where the batch is large enough, as the forward's seam test has them)."""
    return _committed_case(name)


@functools.lru_cache(maxsize=None)
def settings_case(name, key):
    """golden_case(name) with the model built at row `key` of SETTINGS (the case's own overrides merged with the row's, and with
    NUSC_WEIGHTS on a nuScenes case): the kernels (through _fill_common) and the oracle (through LO.settings) both read model.cfg."""
    return _committed_case(name, merged(SETTINGS[key], NUSC_WEIGHTS if GOLDEN_CASES[name][2] == "nusc" else None))


def poisoned_target(case, image=None):
    """The positive (index into pos_inds) whose quaternion poisoned_case zeroes: the first one off the kink mask that sits in the
    middle half of its block of 256 targets (and in an image other than `image`, when given)."""
    pos = case.targets["pos_inds"]
    ok = ~case.kink & ((pos % 256) >= 64) & ((pos % 256) < 192)
    if image is not None:
        ok &= case.targets["im_inds"][pos] != image
    return int(torch.nonzero(ok)[0])


@functools.lru_cache(maxsize=None)
def poisoned_case(name):
    """golden_case(name) with the four quat channels of ONE positive's own class zeroed (a nuScenes positive outside image 0).  That
    box decodes to NaN, which sets the batch-wide renormalisation trigger of an allocentric decode: every other positive then goes
    through the renormalised branch with finite numbers.  `poisoned` is the positive's index into pos_inds."""
    clean = golden_case(name)
    j = poisoned_target(clean, image=0 if GOLDEN_CASES[name][2] == "nusc" else None)
    n, p = int(clean.targets["pos_inds"][j]), clean.p
    C3 = 1 if p["class_agnostic"] else p["num_classes"]
    c3 = 0 if p["class_agnostic"] else int(clean.targets["labels"][n])
    maps = {k: v.clone() for k, v in clean.maps.items()}
    # target n -> level, image, pixel (level-first, then image, then H*W)
    B, off = maps["logits0"].shape[0], 0
    for l, (h, w) in enumerate(clean.level_hw):
        if n < off + B * h * w:
            b, pix = divmod(n - off, h * w)
            for k in range(4):
                maps[f"quat{l}"][b, k * C3 + c3, pix // w, pix % w] = 0.0
            break
        off += B * h * w
    case = Case(clean.model, maps, clean.gt, clean.level_hw, clean.inv_K)
    case.poisoned, case.kink = j, clean.kink  # (the kink mask of the clean maps: the poisoned row is compared on its NaN pattern)
    return case


REFERENCE_CASES = ("kitti_ragged", "kitti_ragged_nopos", "nusc_b6", "kitti_variant_egocentric_agnostic")


@functools.lru_cache(maxsize=None)
def reference_case(name):
    """A case of tests/test_losses_golden.CASES (the GT and K^-1 the reference's own loss modules were run on) and its gradient golden
    tests/golden/loss_grads_<name>.npz (make_loss_grad_golden.py)."""
    from tests import test_losses_golden as TG
    model, g, maps, level_hw, gt = TG.load_case(name)
    c = Case(model, maps, gt, level_hw, torch.from_numpy(g["inv_K"]))
    c.golden = np.load(os.path.join(GOLDEN, f"loss_grads_{name}.npz"))
    return c


# ---------------------------------------------------------------------------------------------- hand-built non-smooth points
def _quat_for(target_ego, K_inv, ctr_xy):
    """The allocentric quaternion whose egocentric rotation at the viewing ray through `ctr_xy` is `target_ego` (3x3): R_local^T R."""
    ray = K_inv.double() @ torch.tensor([ctr_xy[0], ctr_xy[1], 1.0], dtype=torch.float64)
    z = ray / ray.norm()
    y = torch.tensor([0., 1., 0.], dtype=torch.float64) - z[1] * z
    y = y / y.norm()
    Rl = torch.stack([torch.linalg.cross(y, z), y, z], dim=-1)
    from oracle.dd3d_oracle import matrix_to_quaternion
    return matrix_to_quaternion((Rl.T @ target_ego.double())[None])[0]


@functools.lru_cache(maxsize=None)
def handmade_case(H=4, W=4, class_agnostic=False, nusc=True, gamma=None):
    """One level of H x W locations (stride 8) -- 4 x 4: one block; 1 x 257: N = 257 targets, two blocks, the last positive alone in
    the second -- with one GT box per positive location and head-map rows set to hit, one positive each: the four candidates of
    matrix_to_quaternion (identity, then 180 degrees about x, y, z), a depth below MIN_DEPTH, above MAX_DEPTH and exactly on MAX_DEPTH,
    a saturated tanh, every GIoU side larger and smaller than its target plus an exact tie, a post-ReLU zero, an invalid attribute and a
    NaN speed.
    With `gamma` (FCOS2D.LOSS.GAMMA) the saturated variant instead: fewer positives, so that background locations remain at 4 x 4 --
    an identity rotation, a GIoU side larger, a target-class logit of +60, one of -60, a background-class logit of +60 on a positive
    and the invalid attribute -- and two background locations whose whole logit rows are -60: 1 - p_t is exactly 0 (or 1) there."""
    over = {"DD3D": {"SIZES_OF_INTEREST": [], "FCOS3D": {"CLASS_AGNOSTIC_BOX3D": bool(class_agnostic)}}}  # one level: one size range
    if gamma is not None:
        over = merged(over, {"DD3D": {"FCOS2D": {"LOSS": {"GAMMA": float(gamma)}}}})
    model = cpu_model("dd3d_nusc_dla34" if nusc else "dd3d_kitti_dla34", over)
    C_ = int(model.num_classes)
    C3 = 1 if class_agnostic else C_
    A = model.attr_logits.out_channels if nusc else 0
    g = torch.Generator().manual_seed(7 + H * W)
    r = lambda *s: torch.randn(*s, generator=g)
    maps = {"logits0": r(1, C_, H, W), "box2d_reg0": torch.rand(1, 4, H, W, generator=g) * 6 + 1, "centerness0": r(1, 1, H, W),
            "quat0": r(1, 4 * C3, H, W), "ctr0": r(1, 2 * C3, H, W), "depth0": r(1, C3, H, W), "size0": r(1, 3 * C3, H, W) * 0.3,
            "conf0": r(1, C3, H, W)}
    if nusc:
        maps.update(attr0=r(1, A, H, W), speed0=torch.rand(1, 1, H, W, generator=g))
    K = torch.tensor([[80.0, 0, 4.0 * W], [0, 80.0, 4.0 * H], [0, 0, 1]])
    iK = torch.linalg.inv(K)
    canon = model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES
    c3 = model.cfg.DD3D.FCOS3D
    # depth channel value that decodes to `z` metres: depth / (pixel_size * factor)
    px = float(torch.sqrt(iK[0, 0]**2 + iK[1, 1]**2)) * float(c3.SCALE_DEPTH_BY_FOCAL_LENGTHS_FACTOR)
    maps["depth0"] = (1.0 + 0.1 * maps["depth0"]) * 15.0 * px  # decodes to about 15 m
    from dd3d_amd.structures import Boxes, Boxes3D, Instances
    rot = lambda ax: torch.diag(torch.tensor([1.0 if i == ax else -1.0 for i in range(3)]))
    specs = [dict(R=torch.eye(3)), dict(R=rot(0)), dict(R=rot(1)), dict(R=rot(2)), dict(depth=float(c3.MIN_DEPTH) * 0.5),
             dict(depth=float(c3.MAX_DEPTH) * 1.5), dict(depth_exact=float(c3.MAX_DEPTH)), dict(size=30.0), dict(reg="larger"), dict(reg="smaller"),
             dict(reg="tie"), dict(reg="zero"), dict(attr=A, speed=float("nan"))]
    if gamma is not None:
        specs = [specs[0], specs[8], dict(logit=60.0), dict(logit=-60.0), dict(bg_logit=60.0), specs[-1]]
        for idx in (1, H * W - 2):  # background locations (the positives sit on multiples of step >= 2 and on the last target)
            maps["logits0"][0, :, idx // W, idx % W] = -60.0
    step = max(1, (H * W) // len(specs))
    boxes, classes, quats, ctrs, deps, sizes_, attrs, speeds = [], [], [], [], [], [], [], []
    for j, sp in enumerate(specs):
        idx = j * step if j + 1 < len(specs) else H * W - 1  # the last positive is the last target
        y, x = idx // W, idx % W
        lx, ly = 8.0 * x, 8.0 * y
        cls = j % C_
        ch = lambda comp: comp * C3 + (0 if class_agnostic else cls)
        # a box of 6 x 6 around the location, off centre: only this location falls inside; level 0 takes every size (one level)
        boxes.append([lx - 2.0, ly - 3.0, lx + 4.0, ly + 3.0])
        classes.append(cls)
        tgt = torch.tensor([2.0, 3.0, 4.0, 3.0])  # l, t, r, b targets of this location
        if "reg" in sp:
            v = {"larger": tgt + torch.tensor([1.0, 2.0, 0.5, 1.5]), "smaller": tgt - torch.tensor([1.0, 2.0, 0.5, 1.5]),
                 "tie": torch.tensor([2.0, 3.5, 4.0, 2.5]), "zero": torch.tensor([0.0, 3.5, 4.5, 0.0])}[sp["reg"]]
            maps["box2d_reg0"][0, :, y, x] = v
        if "R" in sp:
            cxy = (lx + float(maps["ctr0"][0, ch(0), y, x]), ly + float(maps["ctr0"][0, ch(1), y, x]))
            qa = _quat_for(sp["R"], iK, cxy)
            for k in range(4):
                maps["quat0"][0, ch(k), y, x] = float(qa[k]) * 1.7  # (unnormalised: the two normalisations take part)
        if "depth" in sp:
            maps["depth0"][0, ch(0), y, x] = sp["depth"] * px
        if "depth_exact" in sp:  # a channel value that the decode's own float32 division maps exactly onto the bound
            want = torch.tensor(sp["depth_exact"], dtype=torch.float32)
            pxf = torch.sqrt(iK[0, 0] * iK[0, 0] + iK[1, 1] * iK[1, 1]) * torch.tensor(float(c3.SCALE_DEPTH_BY_FOCAL_LENGTHS_FACTOR))
            v = want * pxf
            for _ in range(8):
                if float(v / pxf) == float(want):
                    break
                v = torch.nextafter(v, torch.tensor(float("inf")) if float(v / pxf) < float(want) else torch.tensor(-float("inf")))
            assert float(v / pxf) == float(want)
            maps["depth0"][0, ch(0), y, x] = v
        if "size" in sp:
            maps["size0"][0, ch(0), y, x] = sp["size"]
        if "logit" in sp:
            maps["logits0"][0, cls, y, x] = sp["logit"]
        if "bg_logit" in sp:
            maps["logits0"][0, (cls + 1) % C_, y, x] = sp["bg_logit"]
        tq = torch.nn.functional.normalize(r(4), dim=0)
        quats.append(tq.tolist())
        ctrs.append([lx + 0.5, ly - 0.25])
        deps.append([12.0 + j])
        sizes_.append([float(v) * 1.1 for v in canon[cls]])
        attrs.append(sp.get("attr", j % A if A else 0))
        speeds.append(sp.get("speed", 0.3 * j))
    inst = Instances((8 * H, 8 * W))
    n = len(specs)
    inst.gt_boxes = Boxes(torch.tensor(boxes, dtype=torch.float32))
    inst.gt_classes = torch.tensor(classes)
    inst.gt_boxes3d = Boxes3D(torch.tensor(quats), torch.tensor(ctrs), torch.tensor(deps), torch.tensor(sizes_), iK[None].expand(n, 3, 3).double())
    if nusc:
        inst.gt_attributes, inst.gt_speeds = torch.tensor(attrs), torch.tensor(speeds, dtype=torch.float32)
    case = Case(model, maps, [inst], [(H, W)], iK[None])
    case.specs = specs
    return case
