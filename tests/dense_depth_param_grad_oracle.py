"""CPU oracle of DD3DDenseDepth's composed training backward (tests/test_dense_depth_param_grads.py,
tests/test_dense_depth_param_grads_gpu.py): ONE torch autograd pass from the sum of the loss dict to every parameter of the model, through
the oracle forward the goldens pin to the reference (oracle.dense_depth_oracle.dense_depth_forward, run under
whole_model_grad_oracle.intercepted: its ReLUs take their derivative from given masks, the tower norms may use the batch's statistics)
and the differentiable statement of the loss (dense_depth_grad_oracle.losses on the forward's raw maps).

Nothing comes from the kernels but the signs of the plan's stored ReLU outputs (`plan_masks`, validated by value like
whole_model_grad_oracle.plan_masks) and, for the fixture, how far the plan's up-sampled maps are from the oracle's (`remove_kinks`).

The fixture.  The smooth-L1 derivative jumps at |v - gt| = beta; `remove_kinks` takes out every pixel within KINK_MARGIN + the plan's own
distance of that jump at any level, so kernel and oracle take the same branch everywhere.  On the quadratic branch the derivative is
(v - gt) / beta: the FORWARD's rounding of v enters the gradient amplified by 1 / beta = 20, which no bar made of the oracle's own
float32 error holds for a forward in 16-bit terms -- the loss backward's own tests compare that branch at the seam, on given maps
(tests/test_dense_depth_grads_gpu.py).  So the ground truth here lies on the linear branch: `ground_truth` draws it with
make_depth_maps from two sub-ranges of the valid depths, one below and one above everything the network predicts on the batch (both signs
of the derivative occur), and the tests assert that no kept pixel is within beta of a prediction.
"""
import torch

from oracle import dd3d_oracle as O
from oracle import dense_depth_oracle as DDO
from tests import dense_depth_grad_oracle as GO
from tests import dense_depth_loss_oracle as DO
from tests import whole_model_grad_oracle as WO
from tests.golden import make_dense_depth_loss_golden as G

F64, F32 = torch.float64, torch.float32
KINK_MARGIN = GO.KINK_MARGIN
KINK_CAP = 0.02      # the removed share of the valid pixels, the cap of tests/test_dense_depth_grads_gpu.py
CPU_SCAN_EXTRA = 1e-2  # what the CPU scan of the seeds allows for the plan's distance from the oracle's maps
# The synthetic heads predict depths all over the valid range (-36 .. 164 on the DLA-34 batch): the cases shrink the per-level Scale by
# HEAD_SCALE and set every Offset to HEAD_OFFSET, which puts all five levels' predictions into one band around the middle of the range
# and leaves room for ground truth on either side of it.
HEAD_SCALE, HEAD_OFFSET = 0.1, 40.0


# ------------------------------------------------------------------------------------------------- the cases
def _merge(a, b):
    return G._merge(a, b) if b else a


V99_OUTPUTS = ["p2", "p3", "p4", "p5", "p6"]  # every FPN output of the V2-99 trunk (LastLevelP6): DD3DDenseDepth reads them all
# exp / weights: the experiment and the calibration of the synthetic weights; overrides: on top of the dense-depth head's; sizes: per-image
# (h, w) on the canvas H x W (the second image of the DLA cases is ragged); gt_seed: make_depth_maps' (scanned on the CPU, see
# tests/test_dense_depth_param_grads.py); flag: the deepest flag of compute_losses
_DLA = dict(exp="dd3d_kitti_dla34", weights="dla34_kitti", H=128, W=256, sizes=[(128, 256), (100, 200)], gt_seed=3100, flag="stem_grads", batch_stats=False)
CASES = {
    "dla34_frozenbn_none": dict(_DLA, overrides={"DD3D": {"FCOS3D": {"NORM": "FrozenBN"}}}),
    "dla34_frozenbn_half": dict(_DLA, overrides={"DD3D": {"FEATURE_LOCATIONS_OFFSET": "half", "FCOS3D": {"NORM": "FrozenBN"}}}),
    "dla34_bn_none": dict(_DLA, overrides={"DD3D": {"FCOS3D": {"NORM": "BN"}}}),
    "dla34_bn_half": dict(_DLA, overrides={"DD3D": {"FEATURE_LOCATIONS_OFFSET": "half", "FCOS3D": {"NORM": "BN"}}}),
    "dla34_bn_batch_stats": dict(_DLA, overrides={"DD3D": {"FCOS3D": {"NORM": "BN"}}}, batch_stats=True),
    "v99": dict(exp="dd3d_kitti_v99", weights="v99_kitti", H=128, W=256, sizes=[(128, 256), (128, 256)], gt_seed=3100, flag="vovnet_stem_grads",
                batch_stats=False, overrides={"DD3D": {"IN_FEATURES": V99_OUTPUTS}}),
}


def case_overrides(case):
    """The dense-depth head on the case's experiment: the meta-architecture, every FPN output, the loss settings, focal scaling on."""
    base = _merge(G.BASE_OVERRIDES, {"DD3D": {"FCOS3D": {"SCALE_DEPTH_BY_FOCAL_LENGTHS": True}}})
    return _merge(base, case["overrides"])


def cpu_model(case):
    """The case's CPU model with its synthetic weights."""
    from dd3d_amd.synthetic import load_calib, make_state_dict
    from tests import loss_grad_cases as GC
    m = GC.cpu_model(case["exp"], case_overrides(case))
    sd = make_state_dict(m, calib=load_calib(case["weights"]))
    for k in sd:  # the predictions into one band inside the valid depths (see `ground_truth`)
        if k.startswith("fcos3d_head.scales_depth."):
            sd[k] = sd[k] * HEAD_SCALE
        elif k.startswith("fcos3d_head.offsets_depth."):
            sd[k] = torch.full_like(sd[k], HEAD_OFFSET)
    m.load_state_dict(sd)
    return m


def case_images(case, seed=1000):
    """The case's batch without ground truth: make_inputs' images, cut to the case's per-image sizes."""
    from dd3d_amd.synthetic import make_inputs
    inputs = make_inputs(len(case["sizes"]), case["H"], case["W"], seed=seed)
    for x, (h, w) in zip(inputs, case["sizes"]):
        if (h, w) != (case["H"], case["W"]):
            x["image"] = x["image"][:, :h, :w].contiguous()
            x["height"], x["width"] = h, w
    return inputs


def loss_settings(model):
    """What dense_depth_grad_oracle.losses takes behind the ground truth."""
    c3 = model.cfg.DD3D.FCOS3D
    factor = float(model.scale_depth_by_focal_lengths_factor) if model.scale_depth_by_focal_lengths else None
    return dict(strides=[s.stride for s in model.backbone_output_shape], offset=model.feature_locations_offset, factor=factor,
                min_depth=float(c3.MIN_DEPTH), max_depth=float(c3.MAX_DEPTH), beta=float(c3.LOSS.SMOOTH_L1_BETA), weight=float(c3.DEPTH_HEAD.LOSS_WEIGHT))


def ground_truth(inputs, maps64, s, seed):
    """Per-image make_depth_maps ground truth on the linear branch of every level: the even pixels (row + column) from the valid depths
    below everything the network predicts on the batch, the odd ones from those above it, each sub-range 4 * beta away from the
    predictions.  `maps64`: the float64 oracle's up-sampled maps."""
    from dd3d_amd.synthetic import make_depth_maps
    lo, hi = min(float(m.min()) for m in maps64), max(float(m.max()) for m in maps64)
    gap = 4.0 * s["beta"]
    assert s["min_depth"] + 2.0 < lo - gap and hi + gap < s["max_depth"] - 2.0, (lo, hi)
    # (no draw beyond the far end of a sub-range: it would fall among the predictions; beyond the other end it leaves the valid depths)
    near = make_depth_maps(inputs, seed=seed, min_depth=s["min_depth"] + 1.0, max_depth=lo - gap, beta=s["beta"], above_fraction=0.0)
    far = make_depth_maps(inputs, seed=seed + 50, min_depth=hi + gap, max_depth=s["max_depth"] - 1.0, beta=s["beta"], below_fraction=0.0)
    out = []
    for a, b in zip(near, far):
        yy, xx = torch.meshgrid(torch.arange(a.shape[0]), torch.arange(a.shape[1]), indexing="ij")
        out.append(torch.where((yy + xx) % 2 == 0, a, b))
    return out


def remove_kinks(depths, maps64, s, H, W, extra):
    """dense_depth_grad_oracle.remove_kinks on the padded canvas with the margin KINK_MARGIN + `extra`, evaluated on the float64 oracle's
    maps: (per-image maps with the removed pixels at 0, the removed share of the valid pixels, the share of the kept valid pixels within
    beta of a prediction at any level)."""
    gt = DO.pad_depth(depths, H, W)
    kept, removed = GO.remove_kinks(gt, maps64, s["min_depth"], s["max_depth"], s["beta"], margin=KINK_MARGIN + extra)
    M = DO.valid_mask(kept, s["min_depth"], s["max_depth"])
    quad = torch.zeros_like(M)
    for m in maps64:
        quad |= (m.float() - kept).abs() < s["beta"]
    share = float((quad & M).sum()) / max(int(M.sum()), 1)
    return [kept[i, :d.shape[0], :d.shape[1]].clone() for i, d in enumerate(depths)], removed, share


# ------------------------------------------------------------------------------------------------- the autograd pass
def is_dla(model):
    return WO.is_dla(model)


def bn_leaf_names(model):
    """The weights of the box3d tower's trainable BatchNorm2d layers: the norms batch_stats=True puts on the batch's statistics."""
    from dd3d_amd.layers import BatchNorm2d
    return sorted(k + ".weight" for k, m in model.named_modules() if k.startswith("fcos3d_head.box3d_tower.") and isinstance(m, BatchNorm2d))


def param_grads(model_cpu, inputs, depths, dtype, masks=None, batch_stats=False, extras=None, backward=True):
    """d (sum of the loss dict) / d (every named parameter of `model_cpu`) by one autograd pass in `dtype`: the state-dict tensors are the
    leaves, the images are cast to `dtype`.  Returns
      ({parameter name: gradient},
       {dense_depth<l>: at the head's per-level outputs; box3d_tower_out<l>: at the tower outputs the predictors read; feature<l>: at the
        FPN outputs; backbone_<name>: the FPN's part at a backbone output feature; DLA: backbone_level1 / backbone_level0 /
        backbone_base_layer, VoVNet: backbone_stem_1 -- at the stem's post-ReLU tensors, none masked by its own ReLU},
       [the ReLU pre-activations in call order, detached]).
    `masks`: one boolean tensor per ReLU call (trunk, then per level the tower layers).  `extras`: a dict that receives losses, raw (the
    per-level raw maps), maps (up-sampled, focal-scaled) and relu_out, detached.  `backward=False`: the forward alone."""
    cfg = model_cpu.cfg
    sd = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v.detach()) for k, v in model_cpu.state_dict().items()}
    names = [k for k, _ in model_cpu.named_parameters()]
    for k in names:
        sd[k].requires_grad_(True)
    batch = [dict(x, image=x["image"].to(dtype)) for x in inputs]
    bn_leaves = [sd[k] for k in bn_leaf_names(model_cpu)] if batch_stats else []
    tower_out, conv2d = {}, O.conv2d

    def watched_conv2d(sd_, name, x, *a, **k):
        if name.startswith("fcos3d_head.dense_depth."):  # the predictor reads an alias of the tower's output: its gradient is kept there
            x = x.view_as(x)
            tower_out[int(name.rsplit(".", 1)[-1])] = x
        return conv2d(sd_, name, x, *a, **k)

    O.conv2d = watched_conv2d
    try:
        with WO.intercepted(masks, bn_leaves) as rec:
            _, stages = DDO.dense_depth_forward(sd, cfg, batch)
    finally:
        O.conv2d = conv2d
    fn = rec["F"]
    if batch_stats and fn.bn_calls != len(bn_leaves):
        raise ValueError(f"{fn.bn_calls} batch-statistics norm calls for {len(bn_leaves)} tower norms")
    if masks is not None and len(masks) != len(fn.pre):
        raise ValueError(f"{len(masks)} masks for {len(fn.pre)} ReLU calls")
    raw = stages["raw"]
    s = loss_settings(model_cpu)
    H, W = stages["images"].shape[-2:]
    gt = DO.pad_depth(depths, int(H), int(W))
    K = torch.stack([x["intrinsics"].float() for x in inputs])
    values = GO.losses(raw, gt, s["strides"], s["offset"], K, s["factor"], s["min_depth"], s["max_depth"], s["beta"], s["weight"])
    total = sum(values)
    at = {f"dense_depth{l}": v for l, v in enumerate(raw)}
    at.update({f"box3d_tower_out{l}": tower_out[l] for l in range(len(raw))})
    at.update({f"feature{l}": v for l, v in enumerate(rec["features"])})
    at.update({f"backbone_{n}": v for n, v in rec["bottom_up"].items()})
    if is_dla(model_cpu):
        assert WO.stem_relus(model_cpu) == 3
        at.update(backbone_base_layer=fn.out[0], backbone_level0=fn.out[1], backbone_level1=fn.out[2])
    else:
        at.update(backbone_stem_1=fn.out[0])
    if extras is not None:
        extras.update(losses=[v.detach() for v in values], raw=[v.detach() for v in raw], relu_out=[v.detach() for v in fn.out],
                      maps=[m.detach() for m in GO.upsampled_maps([v.detach() for v in raw], s["strides"], s["offset"], K, s["factor"])])
    pre = [v.detach() for v in fn.pre]
    if not backward:
        return {}, {}, pre
    for v in at.values():
        v.retain_grad()
    total.backward()
    zero = lambda v: torch.zeros_like(v) if v.grad is None else v.grad
    return {k: zero(sd[k]).detach() for k in names}, {k: zero(v).detach() for k, v in at.items()}, pre


# ------------------------------------------------------------------------------------------------- the masks of a plan's stored tensors
def relu_sites(plan):
    """One (label, Buf, first channel, channels, stored_is_pre) per ReLU call of the oracle forward of `plan.model`, in call order: the
    trunk -- DLA-34: the stem's three stored tensors, the trees (whole_model_grad_oracle._tree_sites); a VoVNet: stem_1's `stem.0`, then
    vovnet_grad_oracle.vovnet_sites -- P7's ReLU of the stored p6, then per level the tower layers' own output buffers."""
    model = plan.model
    dla, fpn = model.backbone.bottom_up, model.backbone
    if is_dla(model):
        from tests import stem_grad_oracle as SO
        sites = [(n, plan.bufs[n], 0, None, False) for n in SO.STEM_BUFFERS]
        for lvl in range(2, 6):
            sites += [(n, plan.bufs[n], c0, c, False) for n, c0, c in WO._tree_sites(getattr(dla, f"level{lvl}"), f"level{lvl}")]
    else:
        from tests import vovnet_grad_oracle as VG
        mine = VG.vovnet_sites(plan)
        assert mine[0] is None and all(x is not None for x in mine[1:])
        sites = [("stem.0", plan.bufs["stem.0"], 0, None, False)] + mine[1:]
    if fpn.top_block is not None and fpn.top_block.num_levels == 2:
        n = f"p{fpn.stages[-1] + 1}"
        sites.append((n, plan.bufs[n], 0, None, True))
    depth = 1 + max(i for (_, i) in plan.tower_info)
    for l in range(len(plan.features)):
        for i in range(depth):
            v = plan.tower_info[("box3d", i)]["y"][l]
            sites.append((f"box3d_tower.{i}[{l}]", v.buf, v.c0, v.C, False))
    return sites


def plan_masks(plan, pre64, report=None):
    """One boolean mask per ReLU call from the sign of the plan's decoded stored tensor, the mapping validated by value as
    whole_model_grad_oracle.plan_masks does (STORED_TOL); `report` receives (label, elements, sign disagreements with the float64
    forward, of them beyond SIGN_NEAR of the tensor's maximum) per call."""
    from tests.util import decode
    sites = relu_sites(plan)
    if len(sites) != len(pre64):
        raise ValueError(f"{len(sites)} plan tensors for {len(pre64)} ReLU calls of the oracle forward")
    masks = []
    for k, ((label, buf, c0, n, stored_is_pre), pre) in enumerate(zip(sites, pre64)):
        got = decode(buf, c0, n).double()
        ref = pre.double() if stored_is_pre else pre.double().clamp(min=0)
        if tuple(got.shape) != tuple(ref.shape):
            raise ValueError(f"ReLU call {k} ({label}): stored {tuple(got.shape)}, oracle {tuple(ref.shape)}")
        err, tol = float((got - ref).abs().max()), WO.STORED_TOL * max(1.0, float(ref.abs().max()))
        if not err <= tol:
            raise ValueError(f"ReLU call {k} ({label}): the stored tensor is {err:.3e} from the oracle's (bar {tol:.3e})")
        mask = got > 0
        masks.append(mask)
        if report is not None:
            bad = mask != (pre > 0)
            far = bad & (pre.abs() > WO.SIGN_NEAR * float(pre.abs().max()))
            report.append((label, pre.numel(), int(bad.sum()), int(far.sum())))
    return masks


def plan_maps(plan, s, inputs):
    """The plan's raw maps of the last run up-sampled on the CPU (float32, the oracle's aligned_bilinear and focal division)."""
    raw = [m.t[..., 0].unsqueeze(1).float().cpu() for m in plan.dd_raw]
    K = torch.stack([x["intrinsics"].float() for x in inputs])
    return GO.upsampled_maps(raw, s["strides"], s["offset"], K, s["factor"])


# ------------------------------------------------------------------------------------------------- stages and families
def stage_and_family(name):
    """(stage, family) of a parameter name for the comparison's rows."""
    from tests import backbone_grad_oracle as BO
    from tests import fpn_grad_oracle as FO
    from tests import tower_grad_oracle as TO
    if name.startswith(("fcos3d_head.dense_depth.", "fcos3d_head.scales_depth.", "fcos3d_head.offsets_depth.")):
        return "predictors", WO.predictor_family_of(name)
    if name.startswith("fcos3d_head.box3d_tower."):
        return "towers", TO.family_of(name)
    if name.startswith("backbone.bottom_up."):
        top = name.split(".")[2]
        if top in ("base_layer", "level0", "level1"):
            return "stem", BO.family_of(name)
        if top.startswith("level"):
            return "backbone " + top, BO.family_of(name)
        from tests import vovnet_grad_oracle as VG
        return "vovnet " + top.split("/")[0], VG.family_of(name)
    if name.startswith("backbone."):
        return "fpn", FO.family_of(name)
    raise KeyError(name)
