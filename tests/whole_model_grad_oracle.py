"""CPU oracle of the composed training backward (tests/test_whole_model_grads.py, tests/test_whole_model_grads_gpu.py): ONE torch autograd
pass from the summed loss dict down to the model's parameters, through the oracle forward the goldens pin to the reference
(oracle.dd3d_oracle.dd3d_forward, stop_after_heads; the nuScenes heads of oracle.nuscenes_oracle) and the loss oracle
(tests.loss_oracle.losses; the summed scalar is loss_grad_oracle.summed_loss, the statement head_grads differentiates too).

The stage oracles (loss_grad_oracle, predictor_grad_oracle, tower_grad_oracle, fpn_grad_oracle, backbone_grad_oracle) each take the
gradient the previous stage's KERNELS produced; this one takes nothing from the kernels but the signs of the stored ReLU outputs.

ReLU signs.  A ReLU's derivative jumps at 0, and the HIP forward (two- or three-term 16-bit products, float32 accumulation) rounds a
handful of pre-activations of ~1e-7 relative size onto the other side than a float64 forward does.  The kernels mask by the STORED
output; so does the reference: `masks` forces the derivative of every ReLU call (in the oracle forward's call order) to a given boolean
tensor, the forward value stays clamp(min=0).  `plan_masks` reads the masks off a LossPlan's stored tensors and validates the mapping
from call index to plan buffer by value.
"""
import contextlib
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import dd3d_oracle as O
from oracle import nuscenes_oracle as NO
from oracle import vovnet_oracle as VO
from tests import loss_grad_cases as GC
from tests import loss_grad_oracle as GO
from tests import loss_oracle as LO
from tests.util import decode

STORED_TOL = 1e-4  # tests/test_forward_gpu.py: a stored activation within 1e-4 * max(1, max|ref|) of the oracle's
SIGN_NEAR = 2.0**-16  # a mask may differ from the float64 sign only where |pre| <= SIGN_NEAR * max|pre| of its tensor ...
SIGN_CAP = 1e-4       # ... and on at most this share of all ReLU elements


class _MaskedRelu(torch.autograd.Function):
    """relu in the forward; in the backward the given mask decides, not the sign of the input."""
    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return x.clamp(min=0)

    @staticmethod
    def backward(ctx, g):
        (mask, ) = ctx.saved_tensors
        # relu's own backward kernel on the 0 / 1 mask: the same memory layout of the result, hence the same order of every later sum
        return torch.ops.aten.threshold_backward(g, mask.to(g.dtype), 0), None


class _Functional:
    """Stands for torch.nn.functional inside the oracle modules: every relu call is recorded (input and output, call order) and, with
    `masks`, differentiated through masks[call index].  `batch_stats`: the weight leaves of the norms that normalise with the batch's
    statistics, as nn.BatchNorm2d does in train() (the head towers' norms under compute_losses(batch_stats=True)); every other
    batch_norm call goes through unchanged."""
    def __init__(self, masks, batch_stats=()):
        self.masks, self.pre, self.out = masks, [], []
        self.batch_stats, self.bn_calls = {id(w) for w in batch_stats}, 0

    def __getattr__(self, name):
        return getattr(F, name)

    def batch_norm(self, x, running_mean, running_var, weight=None, bias=None, training=False, momentum=0.1, eps=1e-5):
        if id(weight) not in self.batch_stats:
            return F.batch_norm(x, running_mean, running_var, weight, bias, training=training, momentum=momentum, eps=eps)
        self.bn_calls += 1  # (clones: train() would update the running statistics in place, the state dict keeps its own)
        return F.batch_norm(x, running_mean.clone(), running_var.clone(), weight, bias, training=True, momentum=0.1, eps=eps)

    def relu(self, x, inplace=False):
        k = len(self.pre)
        if self.masks is None:
            y = F.relu(x)
        else:
            if k >= len(self.masks) or tuple(self.masks[k].shape) != tuple(x.shape):
                raise ValueError(f"ReLU call {k}: no mask of shape {tuple(x.shape)}")
            y = _MaskedRelu.apply(x, self.masks[k])
        self.pre.append(x)
        self.out.append(y)
        return y


@contextlib.contextmanager
def intercepted(masks=None, batch_stats=()):
    """The oracle forward under observation: its ReLUs and batch norms go through a _Functional; the FPN reads aliases of the backbone features and the
    heads read aliases of the FPN outputs, so that the gradient AT an alias is the consumer's contribution alone (what the kernels'
    backbone_<name> and feature<l> are: the FPN's part without the next tree's, the towers' part without P6's)."""
    fn = _Functional(masks, batch_stats)
    rec = {"F": fn, "bottom_up": None, "features": None, "cls_tower_out": None}
    saved = (O.F, NO.F, O.fpn_forward, O.dd3d_backbone, O.fcos2d_head, VO.F)

    def fpn_forward(sd, bottom_up, *a, **k):
        rec["bottom_up"] = OrderedDict((n, v.view_as(v)) for n, v in bottom_up.items())
        return saved[2](sd, rec["bottom_up"], *a, **k)

    def dd3d_backbone(*a, **k):
        feats, strides, bu = saved[3](*a, **k)
        rec["features"] = [f.view_as(f) for f in feats]
        return rec["features"], strides, bu

    def fcos2d_head(*a, **k):
        res = saved[4](*a, **k)
        rec["cls_tower_out"] = res[3]
        return res

    O.F, NO.F, O.fpn_forward, O.dd3d_backbone, O.fcos2d_head, VO.F = fn, fn, fpn_forward, dd3d_backbone, fcos2d_head, fn
    try:
        yield rec
    finally:
        O.F, NO.F, O.fpn_forward, O.dd3d_backbone, O.fcos2d_head, VO.F = saved


def is_dla(model):
    return hasattr(model.backbone.bottom_up, "level1")


def stem_relus(model):
    """How many ReLU calls the DLA stem makes (base_layer, level0, level1): the last of them is the level1 tensor."""
    dla = model.backbone.bottom_up
    return 1 + len(dla.level0) + len(dla.level1)


def free_relus(model):
    """The leading ReLU calls no compared quantity depends on: the DLA stem (the backward stops at level1), every ReLU of a VoVNet
    (vovnet.py:99-161: three stem layers, then `layers` 3x3s and the 1x1 concat per OSA module; its backward stops at the backbone's
    output features)."""
    if is_dla(model):
        return stem_relus(model)
    _, _, _, layers, blocks = VO.SPECS[model.cfg.FE.BACKBONE.NAME]
    assert model.cfg.FE.BACKBONE.NAME not in VO.DW_SPECS
    return 3 + sum(blocks) * (layers + 1)


def whole_model_grads(model_cpu, cfg, inputs, gt, dtype, masks=None, inv_K=None, extras=None, backward=True, batch_stats=False):
    """d (sum of the loss dict) / d (every named parameter of `model_cpu`) by one autograd pass in `dtype`: the state-dict tensors are
    the leaves, the images are cast to `dtype`.  Returns
      ({parameter name: gradient},
       {backbone_level1 (DLA): at the stem's post-ReLU output, not masked by that tensor's own ReLU; backbone_<name>: the FPN's part at a
        backbone output feature; feature<l>: the heads' part at an FPN output; <head map><l>: at the maps the losses read},
       [the ReLU pre-activations in call order, detached]).
    `masks`: one boolean tensor per ReLU call that replaces the derivative's own sign test.  `inv_K` (B, 3, 3): default, the float32
    inverse of the inputs' intrinsics.  `extras`: a dict that receives losses, maps, targets, p, inv_K, relu_out, features and bottom_up (detached).
    `backward=False`: the forward alone (the pre-activations and the extras; both gradient dicts empty).  `batch_stats`: the head towers'
    trainable BatchNorm2d layers (tower_bn_oracle.bn_prefixes) normalise with the batch's statistics, per level, and the backward goes
    through both statistics: the forward of the reference's train() in the towers, every other norm on its running statistics."""
    nusc = hasattr(model_cpu, "attr_logits")
    sd = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v.detach()) for k, v in model_cpu.state_dict().items()}
    names = [k for k, _ in model_cpu.named_parameters()]
    for k in names:
        sd[k].requires_grad_(True)
    batch = [dict(x, image=x["image"].to(dtype)) for x in inputs]
    if inv_K is None:
        inv_K = torch.linalg.inv(torch.stack([x["intrinsics"] for x in inputs]).float())
    bn_leaves = []
    if batch_stats:
        from tests import tower_bn_oracle as TB
        bn_leaves = [sd[p + ".weight"] for p in sorted(TB.bn_prefixes(model_cpu))]
    with intercepted(masks, bn_leaves) as rec:
        _, st = O.dd3d_forward(sd, cfg, batch, stop_after_heads=True)
        keys = [k for k in GO.FAMILIES[:8] if k in st]
        if nusc:
            st["attr"], st["speed"] = NO.nuscenes_heads(sd, rec["cls_tower_out"])
            keys += ["attr", "speed"]
    fn = rec["F"]
    if batch_stats and fn.bn_calls != len(bn_leaves):  # per-level norms: one call each
        raise ValueError(f"{fn.bn_calls} batch-statistics norm calls for {len(bn_leaves)} tower norms")
    if masks is not None and len(masks) != len(fn.pre):
        raise ValueError(f"{len(masks)} masks for {len(fn.pre)} ReLU calls")
    L = len(st["logits"])
    maps = {f"{k}{l}": st[k][l] for k in keys for l in range(L)}
    level_hw = [tuple(st["logits"][l].shape[-2:]) for l in range(L)]
    targets = GC.oracle_targets(model_cpu, level_hw, gt)
    p = dict(LO.settings(model_cpu), num_levels=L)
    total, losses = GO.summed_loss(maps, targets, inv_K, p, None, dtype)
    at = {"backbone_level1": fn.out[stem_relus(model_cpu) - 1]} if is_dla(model_cpu) else {}
    at.update({f"backbone_{n}": v for n, v in rec["bottom_up"].items()})
    at.update({f"feature{l}": v for l, v in enumerate(rec["features"])})
    at.update(maps)
    if backward:
        for v in at.values():
            v.retain_grad()
        total.backward()
    zero = lambda v: torch.zeros_like(v) if v.grad is None else v.grad
    if extras is not None:
        extras.update(losses={k: v.detach() for k, v in losses.items()}, maps={k: v.detach() for k, v in maps.items()}, targets=targets, p=p,
                      inv_K=inv_K, relu_out=[v.detach() for v in fn.out], features=[v.detach() for v in rec["features"]],
                      bottom_up=OrderedDict((n, v.detach()) for n, v in rec["bottom_up"].items()))
    if not backward:
        return {}, {}, [v.detach() for v in fn.pre]
    return {k: zero(sd[k]) for k in names}, {k: zero(v).detach() for k, v in at.items()}, [v.detach() for v in fn.pre]


def natural_masks(pre):
    return [v > 0 for v in pre]


# ------------------------------------------------------------------------------------------------- the masks of a plan's stored tensors
def _tree_sites(m, name):
    """The ReLU calls of oracle.dd3d_oracle._tree in call order as (plan buffer, first channel, channels) of BackboneLowering._tree's
    buffers: conv1 of tree1 (mid), x1, conv1 of tree2 (mid), x2, the root's output -- x1 and x2 live in the root's concat buffer, a
    depth-2 tree's inner tree1 writes its output into the outer concat buffer."""
    def depth1(m, name, cat, dst):
        oc = m.out_channels
        return [(name + ".tree1.mid", 0, None), (cat, oc, oc), (name + ".tree2.mid", 0, None), (cat, 0, oc), dst]

    if m.levels == 1:
        return depth1(m, name, name + ".cat", (name + ".out", 0, None))
    oc, ic = m.out_channels, m.in_channels
    off = 2 * oc + (ic if m.level_root else 0)
    return depth1(m.tree1, name + ".tree1", name + ".tree1.cat", (name + ".cat", off, oc)) + \
        depth1(m.tree2, name + ".tree2", name + ".cat", (name + ".tree2.out", 0, None))


def relu_sites(plan):
    """One entry per ReLU call of the oracle forward of `plan.model` (DLA-34 or a VoVNet, the FPN with P6 or P6/P7, the FCOS heads,
    nuScenes' speed head last): None for the calls of free_relus (no compared quantity depends on those signs), else
    (label, Buf, first channel, channels, stored_is_pre) -- `stored_is_pre`: the plan stores the ReLU's INPUT (p6; P7 reads its ReLU)."""
    model = plan.model
    dla, fpn = model.backbone.bottom_up, model.backbone
    sites = [None] * free_relus(model)
    for lvl in range(2, 6) if is_dla(model) else ():
        sites += [(n, plan.bufs[n], c0, c, False) for n, c0, c in _tree_sites(getattr(dla, f"level{lvl}"), f"level{lvl}")]
    if fpn.top_block is not None and fpn.top_block.num_levels == 2:
        n = f"p{fpn.stages[-1] + 1}"
        sites.append((n, plan.bufs[n], 0, None, True))
    L = len(plan.features)
    view = lambda label, v: (label, v.buf, v.c0, v.C, False)
    depth = lambda t: 1 + max(i for (tn, i) in plan.tower_info if tn == t)
    for l in range(L):  # fcos2d_head: per level the cls tower, the box2d tower, box2d_reg (stored post-ReLU)
        for t in ("cls", "box2d"):
            sites += [view(f"{t}_tower.{i}[{l}]", plan.tower_info[(t, i)]["y"][l]) for i in range(depth(t))]
        sites.append((f"box2d_reg{l}", plan.b2d_maps[l], 0, 4, False))
    if plan.box3d_on:
        for l in range(L):
            sites += [view(f"box3d_tower.{i}[{l}]", plan.tower_info[("box3d", i)]["y"][l]) for i in range(depth("box3d"))]
    if plan.nusc:
        C_, A = int(model.num_classes), int(plan.loss_args.num_attr)
        sites += [(f"speed{l}", plan.cls_maps[l], C_ + A, 1, False) for l in range(L)]
    return sites


def plan_masks(plan, pre64, report=None):
    """One boolean mask per ReLU call: the sign of the plan's DECODED STORED tensor of that call (tests.util.decode), the oracle's own
    sign for the stem.  The mapping (relu_sites) is checked by value: the decoded tensor must have the call's shape and agree with the
    float64 ReLU output (with p6: its input) within STORED_TOL * max(1, max|ref|), the forward tests' bar; anything else raises.
    `report`: a list that receives (label, elements, sign disagreements, disagreements with |pre| > SIGN_NEAR * max|pre|) per call."""
    sites = relu_sites(plan)
    if len(sites) != len(pre64):
        raise ValueError(f"{len(sites)} plan tensors for {len(pre64)} ReLU calls of the oracle forward")
    masks = []
    for k, (site, pre) in enumerate(zip(sites, pre64)):
        if site is None:
            masks.append(pre > 0)
            continue
        label, buf, c0, n, stored_is_pre = site
        got = decode(buf, c0, n).double()
        ref = pre.double() if stored_is_pre else pre.double().clamp(min=0)
        if tuple(got.shape) != tuple(ref.shape):
            raise ValueError(f"ReLU call {k} ({label}): stored {tuple(got.shape)}, oracle {tuple(ref.shape)}")
        err, tol = float((got - ref).abs().max()), STORED_TOL * max(1.0, float(ref.abs().max()))
        if not err <= tol:
            raise ValueError(f"ReLU call {k} ({label}): the stored tensor is {err:.3e} from the oracle's (bar {tol:.3e})")
        mask = got > 0
        masks.append(mask)
        if report is not None:
            bad = mask != (pre > 0)
            far = bad & (pre.abs() > SIGN_NEAR * float(pre.abs().max()))
            report.append((label, pre.numel(), int(bad.sum()), int(far.sum())))
    return masks


# ------------------------------------------------------------------------------------------------- stages, families and the cases
def predictor_family_of(name):
    return "weight" if name.endswith(".weight") else "scale" if name.endswith(".scale") else "offset" if "offsets_" in name else "bias"


def stage_and_family(name, backbone_grads=True):
    """(stage, family) of a parameter name, the family as the stage's own test defines it; None for the stem, which has no backward,
    and for the whole bottom-up network where the backward stops at the FPN (`backbone_grads` False)."""
    from tests import backbone_grad_oracle as BO
    from tests import fpn_grad_oracle as FO
    from tests import predictor_grad_oracle as PO
    from tests import tower_grad_oracle as TO
    if PO.PREDICTOR_PARAM.match(name):
        return "predictors", predictor_family_of(name)
    if TO.TOWER_PARAM.match(name):
        return "towers", TO.family_of(name)
    if name.startswith("backbone.bottom_up."):
        top = name.split(".")[2]
        if top in ("base_layer", "level0", "level1") or not backbone_grads:
            return None
        if top in ("level2", "level3", "level4", "level5"):
            return "backbone " + top, BO.family_of(name)
        raise KeyError(name)
    if name.startswith("backbone."):
        return "fpn", FO.family_of(name)
    raise KeyError(name)


def tensor_family_of(key):
    """The family of a key of the tensor gradients: the key without its level (feature, logits, ...), the backbone features by name."""
    return key if key.startswith("backbone_") else key.rstrip("0123456789")


BN_EVERYWHERE = {"FE": {"BACKBONE": {"NORM": "BN"}, "FPN": {"NORM": "BN"}}}  # the towers' norm is BN in the released configs
_KITTI = dict(exp="dd3d_kitti_dla34", weights="dla34_kitti", overrides=None, B=2, H=128, W=384, ds="kitti", gt_seed=2004, n_per_image=24, positives=150, relus=99,
              grads="backbone_grads")
# One entry per case of the GPU test.  `ref`: the cases that share a CPU reference (model, inputs, GT, batch_stats).  GT seeds: scanned on the CPU for
# a batch with no positive inside loss_grad_oracle.KINK_MARGIN of a non-smooth point of the loss on the float64 oracle's head maps (one
# such positive moves every parameter upstream of it by far more than rounding) -- tests/test_whole_model_grads.py pins seed, positive
# count and the empty kink mask.  nuScenes: six boxes per image; with the default 24 every seed of 2000 .. 2011 has 2 to 13 kink positives.
CASES = {
    "kitti_dla34": dict(_KITTI, ref="kitti_dla34", math=None, act_scale=None),
    "kitti_dla34_bf16x3": dict(_KITTI, ref="kitti_dla34", math="bf16x3", act_scale=None),
    "kitti_dla34_plane_scale_1": dict(_KITTI, ref="kitti_dla34", math=None, act_scale=1.0),
    "nusc_dla34": dict(exp="dd3d_nusc_dla34", weights="dla34_nusc", overrides=None, B=6, H=128, W=224, ds="nusc", gt_seed=2007, n_per_image=6, positives=183,
                       relus=104, grads="backbone_grads", ref="nusc_dla34", math=None, act_scale=None),
    "kitti_dla34_bn": dict(_KITTI, overrides=BN_EVERYWHERE, ref="kitti_dla34_bn", math=None, act_scale=None),
    # V2-99: LastLevelP6, four stages; its backward stops at the backbone's output features (fpn_grads).  Float64 oracle: 4 s on 16 threads.
    "kitti_v99": dict(exp="dd3d_kitti_v99", weights="v99_kitti", overrides=None, B=1, H=128, W=256, ds="kitti", gt_seed=2000, n_per_image=24, positives=170,
                      relus=164, grads="fpn_grads", ref="kitti_v99", math=None, act_scale=None),
}
# Batch statistics in the head towers (compute_losses(batch_stats=True)): the head maps change, so the seeds were scanned again on the
# float64 train-mode forward (2000 .. 2015: 2002, 2004 and 2010 leave no positive inside the kink margin; 2004 keeps the batch of the
# running-statistics cases).
CASES["kitti_dla34_batch_stats"] = dict(_KITTI, ref="kitti_dla34_batch_stats", math=None, act_scale=None, batch_stats=True)
REFERENCES = sorted({c["ref"] for c in CASES.values()})


def case_inputs(case, model):
    """(inputs, gt) of a case: the seeded synthetic batch, the second image without GT."""
    from dd3d_amd.synthetic import make_gt_instances, make_inputs
    inputs = make_inputs(case["B"], case["H"], case["W"], dataset=case["ds"])
    gt = make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, seed=case["gt_seed"], n_per_image=case["n_per_image"],
                           num_attributes=model.attr_logits.out_channels if hasattr(model, "attr_logits") else None, empty_images=(1, ))
    return inputs, gt


def case_model(case):
    """The case's CPU model with its synthetic weights."""
    from dd3d_amd.synthetic import load_calib, make_state_dict
    m = GC.cpu_model(case["exp"], case["overrides"])
    m.load_state_dict(make_state_dict(m, calib=load_calib(case["weights"])))
    return m
