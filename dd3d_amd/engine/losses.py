"""Loss engine: target assignment and the training loss dict of DD3D / NuscenesDD3D on the MI355X, and on request the gradient of
the dict's weighted sum with respect to the head maps (csrc/loss_grads.hip) and, one layer further down, with respect to the predictor
layer's parameters and the tower outputs it reads (csrc/predictor_grads.hip), and one layer further again through the head towers to
their parameters and the FPN outputs (csrc/tower_grads.hip), and one stage further through the FPN to its parameters and the backbone's
output features (csrc/fpn_grads.hip), and one stage further again through the DLA-34 backbone's level5 .. level2 to their parameters
and the stem's output (csrc/backbone_grads.hip), and last through the stem -- base_layer, level0, level1 -- to its parameters
(csrc/stem_grads.hip); for the VoVNet-V2 backbones, behind the FPN through stage5 .. stage2, stem_3 and stem_2 (csrc/vovnet_grads.hip and
the wide entry points of csrc/backbone_grads.hip) and last stem_1's filter (dd3d_vovnet_stem_wgrad, csrc/stem_grads.hip).  With
batch_stats=True the head towers whose norm is a trainable BatchNorm2d use the batch's statistics, forward and backward
(csrc/tower_bn.hip); with fpn_batch_stats=True the FPN's lateral and output norms do (csrc/fpn_bn.hip), with backbone_batch_stats=True the DLA-34 bottom-up network's (csrc/backbone_bn.hip).  There is no optimiser or model.train().  The chain behind the loss backward (flags, stage builders, read-outs) is the
mixin ``BackwardStages``: ``LossPlan`` and the dense-depth network's ``DenseDepthLossPlan`` (dense_depth_loss.py) both run it.

``LossPlan`` reuses the forward plan's trunk and heads (ForwardPlan._trunk / _heads) and, in place of the inference post-processing,
runs two launches of csrc/losses.hip: the assignment (DD3DTargetPreparer, prepare_targets.py:28-235) and the per-target loss terms with
their single-block finalize (FCOS2DLoss fcos2d.py:159-239, FCOS3DLoss fcos3d.py:191-299, NuscenesLoss nuscenes_dd3d.py:199-265).  The
ground truth of a call is packed into one pinned host mirror and shipped with one asynchronous copy, beside the image metadata.

`assign_targets` is the same assignment kernel on its own, for DD3D.prepare_targets (the reference's call signature).
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from dd3d_amd import hip
from dd3d_amd.engine.forward import ForwardPlan
from dd3d_amd.engine.ops import CallOp
from dd3d_amd.engine.plan import PlanBase

INF = 100000000.0  # prepare_targets.py:8
LOSS_KEYS_2D = ("loss_cls", "loss_box2d_reg", "loss_centerness")
# FCOS3DLoss returns its keys in a different order with and without positives (fcos3d.py:217-225 vs :297)
LOSS_KEYS_3D = ("loss_conf3d", "loss_box3d_quat", "loss_box3d_proj_ctr", "loss_box3d_depth", "loss_box3d_size")
LOSS_KEYS_3D_EMPTY = ("loss_box3d_quat", "loss_box3d_proj_ctr", "loss_box3d_depth", "loss_box3d_size", "loss_conf3d")
LOSS_KEYS_NUSC = ("loss_attr", "loss_speed")
OUT_INDEX = {"loss_cls": 0, "loss_box2d_reg": 1, "loss_centerness": 2, "loss_box3d_quat": 3, "loss_box3d_proj_ctr": 4, "loss_box3d_depth": 5,
             "loss_box3d_size": 6, "loss_conf3d": 7, "loss_attr": 8, "loss_speed": 9}


def loss_keys(box3d, nusc, num_pos):
    """Keys of the reference's loss dict, in its order (core.py:103-111, nuscenes_dd3d.py:385-397)."""
    keys = list(LOSS_KEYS_2D)
    if box3d:
        keys += LOSS_KEYS_3D if num_pos > 0 else LOSS_KEYS_3D_EMPTY
    if nusc:
        keys += LOSS_KEYS_NUSC
    return keys


def feature_locations(h, w, stride, offset="none"):
    """tridet/utils/tensor2d.py:6-25 compute_features_locations: (x, y), row-major, x fastest."""
    sx = torch.arange(0, w * stride, step=stride, dtype=torch.float32)
    sy = torch.arange(0, h * stride, step=stride, dtype=torch.float32)
    yy, xx = torch.meshgrid(sy, sx, indexing="ij")
    loc = torch.stack((xx.reshape(-1), yy.reshape(-1)), dim=1)
    if offset == "half":
        loc = loc + stride // 2
    return loc


def sizes_of_interest(cfg, num_levels):
    """prepare_targets.py:19-25: [-1, s0], [s0, s1], ..., [s_last, INF]; one range per level."""
    soi, prev = [], -1
    for s in cfg.DD3D.SIZES_OF_INTEREST:
        soi.append([prev, s])
        prev = s
    soi.append([prev, INF])
    if len(soi) != num_levels:
        raise ValueError(f"DD3D.SIZES_OF_INTEREST gives {len(soi)} size ranges for {num_levels} feature levels")
    return soi


def check_loss_config(cfg):
    loc = str(cfg.DD3D.FCOS2D.LOSS.LOC_LOSS_TYPE)
    if loc != "giou":
        raise ValueError(f"DD3D.FCOS2D.LOSS.LOC_LOSS_TYPE = {loc!r}: the loss engine implements 'giou' (every reference config's choice) only")
    gamma = float(cfg.DD3D.FCOS2D.LOSS.GAMMA)
    if not (gamma == 0.0 or gamma >= 1.0):
        # (1 - p_t)^gamma at 1 - p_t == 0, which float32 reaches for any logit beyond about +-17: infinite below 0, and between 0 and 1
        # its derivative gamma * 0^(gamma - 1) is, which makes the location's logit gradients non-finite (in torch autograd as well)
        raise ValueError(f"DD3D.FCOS2D.LOSS.GAMMA = {gamma}: the focal loss needs GAMMA == 0 or GAMMA >= 1 (below 0 the loss, and between 0 "
                         "and 1 its gradient, is not finite at a confidently classified logit)")


def pack_gt(gt_instances, max_gt, box3d, nusc, num_attr, num_classes):
    """Ground truth of a batch -> (offsets [B + 1] int32, records [n, LOSS_GT_FIELDS] float32) in the layout of dd3d_loss_args.gt.
    Each instance needs gt_boxes and gt_classes; gt_boxes3d (any object with the reference's Boxes3D fields: quat, proj_ctr, depth,
    size, inv_intrinsics, which may be float64) when `box3d`; gt_attributes and gt_speeds when `nusc`.  Classes outside
    [0, num_classes] and attributes outside [0, num_attr] raise ValueError."""
    off = [0]
    recs = []
    for i, inst in enumerate(gt_instances):
        boxes = inst.gt_boxes.tensor if hasattr(inst.gt_boxes, "tensor") else inst.gt_boxes
        boxes = torch.as_tensor(boxes).detach().to("cpu", torch.float32).reshape(-1, 4)
        n = boxes.shape[0]
        if n > max_gt:
            raise ValueError(f"image {i} has {n} ground-truth boxes; the loss engine holds at most {max_gt} per image (G_max = {max_gt})")
        r = np.zeros((n, hip.LOSS_GT_FIELDS), dtype=np.float32)
        if n:
            r[:, 0:4] = boxes.numpy()
            # the kernels index head-map rows and the canonical sizes with these (the reference raises an IndexError on them)
            cls = torch.as_tensor(inst.gt_classes).to("cpu", torch.int64).reshape(-1)
            if cls.numel() != n or bool(((cls < 0) | (cls > num_classes)).any()):
                raise ValueError(f"image {i}: gt_classes must hold {n} values in [0, {num_classes}] ({num_classes} = background)")
            r[:, 4] = cls.to(torch.int32).numpy().view(np.float32)
            if nusc:
                att = torch.as_tensor(inst.gt_attributes).to("cpu", torch.int64).reshape(-1)
                if att.numel() != n or bool(((att < 0) | (att > num_attr)).any()):
                    raise ValueError(f"image {i}: gt_attributes must hold {n} values in [0, {num_attr}] ({num_attr} = no attribute)")
                r[:, 5] = att.to(torch.int32).numpy().view(np.float32)
                r[:, 6] = torch.as_tensor(inst.gt_speeds).to("cpu", torch.float32).numpy()
            else:
                r[:, 5] = np.array([num_attr], dtype=np.int32).view(np.float32)[0]
                r[:, 6] = np.nan
            if box3d:
                b3 = inst.gt_boxes3d
                f = lambda t, k: torch.as_tensor(t).detach().to("cpu", torch.float32).reshape(n, k).numpy()
                r[:, 7:11] = f(b3.quat, 4)
                r[:, 11:13] = f(b3.proj_ctr, 2)
                r[:, 13:14] = f(b3.depth, 1)
                r[:, 14:17] = f(b3.size, 3)
                r[:, 17:26] = f(b3.inv_intrinsics, 9)
        recs.append(r)
        off.append(off[-1] + n)
    return np.asarray(off, dtype=np.int32), (np.concatenate(recs, 0) if recs else np.zeros((0, hip.LOSS_GT_FIELDS), np.float32))


class _Targets:
    """Device buffers of the assignment's outputs for N targets, and the dd3d_loss_args fields that point at them."""
    def __init__(self, a, N, box3d, nusc, device):
        self.labels = torch.zeros(N, dtype=torch.int32, device=device)
        self.target_inds = torch.zeros(N, dtype=torch.int32, device=device)
        self.box2d_reg = torch.zeros((N, 4), dtype=torch.float32, device=device)
        self.ctr = torch.zeros(N, dtype=torch.float32, device=device)
        self.box3d = torch.zeros((N, hip.LOSS_BOX3D_FIELDS), dtype=torch.float32, device=device) if box3d else None
        self.attributes = torch.zeros(N, dtype=torch.int32, device=device) if nusc else None
        self.speeds = torch.zeros(N, dtype=torch.float32, device=device) if nusc else None
        self.flags = torch.zeros(1, dtype=torch.int32, device=device)
        a.labels, a.target_inds = self.labels.data_ptr(), self.target_inds.data_ptr()
        a.box2d_reg, a.ctr_target, a.flags = self.box2d_reg.data_ptr(), self.ctr.data_ptr(), self.flags.data_ptr()
        a.box3d_t = self.box3d.data_ptr() if box3d else None
        a.attributes = self.attributes.data_ptr() if nusc else None
        a.speeds = self.speeds.data_ptr() if nusc else None

    def as_dict(self, locations, B, num_levels, level_sizes, num_classes):
        """The reference's targets dict (prepare_targets.py:65-80, nuscenes_dd3d.py:93-97) as device tensors."""
        from dd3d_amd.structures import Boxes3D
        dev = self.labels.device
        labels = self.labels.long()
        loc_lv = torch.split(locations, level_sizes)
        out = {
            "labels": labels,
            "box2d_reg_targets": self.box2d_reg,
            "locations": torch.cat([lv.repeat(B, 1) for lv in loc_lv]),
            "target_inds": self.target_inds.long(),
            "im_inds": torch.cat([torch.arange(B, device=dev).repeat_interleave(n) for n in level_sizes]),
            "fpn_levels": torch.cat([torch.full((B * n, ), l, dtype=torch.long, device=dev) for l, n in enumerate(level_sizes)]),
            "pos_inds": torch.nonzero(labels != num_classes).squeeze(1),
        }
        if self.box3d is not None:
            t = self.box3d
            out["box3d_targets"] = Boxes3D(t[:, 0:4], t[:, 4:6], t[:, 6:7], t[:, 7:10], t[:, 10:19].reshape(-1, 3, 3))
        if self.attributes is not None:
            out["attributes"] = self.attributes.long()
            out["speeds"] = self.speeds
        return out


def _fill_common(a, cfg, model, level_hw, strides, B, max_gt):
    """Geometry, size ranges, centre sampling and the FCOS3D decode / loss settings of dd3d_loss_args."""
    L = len(level_hw)
    if L > hip.MAX_LEVELS:
        raise ValueError(f"{L} feature levels exceed {hip.MAX_LEVELS}")
    soi = sizes_of_interest(cfg, L)
    pt = cfg.DD3D.FCOS3D.PREPARE_TARGET
    off = 0
    for l, (h, w) in enumerate(level_hw):
        a.H[l], a.W[l] = int(h), int(w)
        a.loc_off[l] = off
        off += int(h) * int(w)
        a.soi_lo[l], a.soi_hi[l] = float(soi[l][0]), float(soi[l][1])
        a.radius[l] = float(strides[l] * pt.POS_RADIUS)  # prepare_targets.py:196 (python float, then f32 like the tensor op)
    a.loc_off[L] = off
    a.num_levels, a.B, a.num_classes, a.max_gt = L, B, int(model.num_classes), int(max_gt)
    a.center_sample = int(bool(pt.CENTER_SAMPLE))
    c3 = cfg.DD3D.FCOS3D
    a.class_agnostic_3d = int(bool(c3.CLASS_AGNOSTIC_BOX3D))
    a.scale_depth_by_focal = int(bool(c3.SCALE_DEPTH_BY_FOCAL_LENGTHS))
    a.allocentric = int(bool(c3.PREDICT_ALLOCENTRIC_ROT))
    a.depth_is_distance = int(bool(c3.PREDICT_DISTANCE))
    a.min_depth, a.max_depth, a.focal_factor = float(c3.MIN_DEPTH), float(c3.MAX_DEPTH), float(c3.SCALE_DEPTH_BY_FOCAL_LENGTHS_FACTOR)
    l2, l3 = cfg.DD3D.FCOS2D.LOSS, c3.LOSS
    a.focal_alpha, a.focal_gamma = float(l2.ALPHA), float(l2.GAMMA)
    a.smooth_l1_beta, a.conf3d_temperature = float(l3.SMOOTH_L1_BETA), float(l3.CONF_3D_TEMPERATURE)
    a.weight_box3d, a.weight_conf3d = float(l3.WEIGHT_BOX3D), float(l3.WEIGHT_CONF3D)
    nusc = getattr(getattr(cfg.DD3D, "NUSC", None), "LOSS", None)
    a.weight_attr = float(nusc.WEIGHT_ATTR) if nusc is not None and hasattr(model, "attr_logits") else 0.0
    a.weight_speed = float(nusc.WEIGHT_SPEED) if nusc is not None and hasattr(model, "attr_logits") else 0.0
    return off


def model_is_nusc(model):
    return hasattr(model, "attr_logits")


def num_attributes(model):
    return int(model.attr_logits.out_channels) if model_is_nusc(model) else 0


def assign_targets(model, locations, gt_instances, feature_shapes, max_gt=hip.LOSS_MAX_GT):
    """DD3DTargetPreparer.__call__ (prepare_targets.py:28-91) / NuscenesDD3DTargetPreparer.__call__ on the device: one launch of
    dd3d_loss_assign on the current stream.  `locations`: per-level (H*W, 2) tensors; `feature_shapes`: per-level (H, W)."""
    cfg, dev = model.cfg, model.device
    check_loss_config(cfg)
    level_hw = [(int(s[0]), int(s[1])) for s in feature_shapes]
    strides = [s.stride for s in model.backbone_output_shape]
    B = len(gt_instances)
    box3d, nusc = not model.only_box2d, model_is_nusc(model)
    a = hip.LossArgs()
    nloc = _fill_common(a, cfg, model, level_hw, strides, B, max_gt)
    loc = torch.cat([torch.as_tensor(x).reshape(-1, 2).to(dev, torch.float32) for x in locations]).contiguous()
    if loc.shape[0] != nloc:
        raise ValueError(f"{loc.shape[0]} locations for feature shapes {level_hw} ({nloc} locations)")
    off, recs = pack_gt(gt_instances, max_gt, box3d, nusc, num_attributes(model), int(model.num_classes))
    gt_off = torch.from_numpy(off).to(dev)
    gt = torch.from_numpy(recs).to(dev) if recs.shape[0] else torch.zeros((1, hip.LOSS_GT_FIELDS), dtype=torch.float32, device=dev)
    a.locations, a.gt_off, a.gt = loc.data_ptr(), gt_off.data_ptr(), gt.data_ptr()
    a.num_attr = num_attributes(model)
    t = _Targets(a, B * nloc, box3d, nusc, dev)
    hip.check(hip.lib().dd3d_loss_assign(C.byref(a), hip.current_stream()), "loss_assign")
    return t.as_dict(loc, B, len(level_hw), [h * w for h, w in level_hw], model.num_classes)


HEAD_KEYS_2D = ("logits", "box2d_reg", "centerness")
HEAD_KEYS_3D = ("quat", "ctr", "depth", "size", "conf")
HEAD_KEYS_NUSC = ("attr", "speed")
BOX3D_COMPONENTS = {"quat": (0, 4), "ctr": (4, 2), "depth": (6, 1), "size": (7, 3), "conf": (10, 1)}  # first component, count (x C3 channels)


def fill_grad_args(d_cls, d_b2d, d_b3d, upstream, denoms):
    """dd3d_loss_grad_args over per-level NHWC gradient buffers (d_b3d None: 2D only)."""
    g = hip.LossGradArgs()
    for l in range(len(d_cls)):
        g.d_cls[l], g.d_box2d[l] = d_cls[l].data_ptr(), d_b2d[l].data_ptr()
        g.d_box3d[l] = d_b3d[l].data_ptr() if d_b3d is not None else None
    g.upstream, g.denoms = upstream.data_ptr(), denoms.data_ptr()
    return g


def unpack_head_grads(d_cls, d_b2d, d_b3d, num_classes, num_attr, class_agnostic):
    """NHWC / pitch gradient buffers -> {key<l>: NCHW tensor} (copies; attr / speed when num_attr > 0, the 3D keys when d_b3d)."""
    out = {}
    C_ = num_classes
    for l in range(len(d_cls)):
        cl = d_cls[l].permute(0, 3, 1, 2)
        out[f"logits{l}"] = cl[:, :C_].clone()
        if num_attr:
            out[f"attr{l}"], out[f"speed{l}"] = cl[:, C_:C_ + num_attr].clone(), cl[:, C_ + num_attr:C_ + num_attr + 1].clone()
        b2 = d_b2d[l].permute(0, 3, 1, 2)
        out[f"box2d_reg{l}"], out[f"centerness{l}"] = b2[:, :4].clone(), b2[:, 4:5].clone()
        if d_b3d is not None:
            C3 = 1 if class_agnostic else C_
            b3 = d_b3d[l].permute(0, 3, 1, 2)
            for k, (c0, n) in BOX3D_COMPONENTS.items():
                out[f"{k}{l}"] = b3[:, c0 * C3:(c0 + n) * C3].clone()
    return out


def pred_act_mode(plan):
    """DD3D_PG_ACT_* of the storage a plan keeps its tower outputs in; the reduced modes have no loader."""
    if not plan.use_planes:
        return hip.PG_ACT_F32
    if plan.math == hip.MATH_F16X2:
        return hip.PG_ACT_F16X2
    if plan.math == hip.MATH_BF16X3:
        return hip.PG_ACT_BF16X3
    name = {hip.MATH_BF16X2: "bf16x2", hip.MATH_BF16: "bf16"}.get(plan.math, str(plan.math))
    raise NotImplementedError(f"predictor gradients read f32, f16x2 or bf16x3 tower outputs; the arithmetic mode {name!r} has no loader")


class GradCall:
    """What the gradient calls below share: the guarded allocator of their outputs, the pitch rule of the NHWC tensors they are handed,
    the weight-gradient outputs of the convolution calls and the launch.

    `ENTRIES`: (library entry, label of its error check) of the launches in their order -- the weight gradient, run when `with_wgrad`,
    then the input gradient, run when `with_dgrad`; a call of one launch lists one entry.  `_raw` holds (tensor, numel) of every tensor
    the call allocates and its kernels write: `numel` words of output, then `guard` words the kernels must leave at `fill`."""
    ENTRIES = ()
    with_wgrad = with_dgrad = True

    def __init__(self, device, fill, guard):
        self._raw, self._new = [], (device, float(fill), guard)

    def out(self, *shape):
        device, fill, guard = self._new
        numel = int(np.prod(shape))
        t = torch.full((numel + guard, ), fill, dtype=torch.float32, device=device)
        self._raw.append((t, numel))
        return t[:numel].view(*shape)

    @staticmethod
    def pitch(t):
        """Words between two pixels of an NHWC tensor or channel slice (torch leaves the stride of a dimension of size one arbitrary:
        a tensor one pixel wide whose stride is below its channel count has the channel count)."""
        return int(t.stride(-2)) if t.shape[-2] > 1 or t.stride(-2) >= t.shape[-1] else int(t.shape[-1])

    def wgrad_outputs(self, a, slab, Cout, KK, level=(), total=()):
        """The weight gradient's outputs and their six addresses in `a`: the partials `part` [n_slices, Cout, KK] and `qpart`
        [n_slices, Cout] -- the shared `slab`, or the call's own -- then `dw_level` [*level, Cout, KK], `dw` [*total, Cout, KK] and the
        per-channel sums `q`, `r` [*level, Cout]."""
        if slab is None:
            slab = (self.out(self.n_slices, Cout, KK), self.out(self.n_slices, Cout))
        self.part, self.qpart = slab
        assert self.part.numel() >= self.n_slices * Cout * KK and self.qpart.numel() >= self.n_slices * Cout
        self.dw_level, self.dw = self.out(*level, Cout, KK), self.out(*total, Cout, KK)
        self.q, self.r = self.out(*level, Cout), self.out(*level, Cout)
        a.part, a.qpart, a.dw_level, a.dw = (t.data_ptr() for t in (self.part, self.qpart, self.dw_level, self.dw))
        a.q, a.r = self.q.data_ptr(), self.r.data_ptr()

    def launch(self, lib, st):
        for (entry, label), on in zip(self.ENTRIES, (self.with_wgrad, self.with_dgrad)):
            if on:
                hip.check(getattr(lib, entry)(C.byref(self.args), st), label)

    def guards_intact(self, fill):
        return all(bool((t[n:] == fill).all()) for t, n in self._raw)


class PredGroupGrads(GradCall):
    """Buffers and dd3d_pred_grad_args of one predictor group (the predictors fused into one head map, reading one tower).

    `act`: per-level device address of the tower output in the storage `act_mode` names; `g`, `maps`: per-level NHWC tensors of pitch
    `g_pitch`; `w`: per-level [n, 3, 3, Cin] filters, the SAME tensor on the levels that share a module; `bias`, `scale`: per-level [n];
    `lo`: [n] or None; `slot`: int32 [n] or None.  Outputs are allocated here, filled with `fill` and followed by `guard` words of it."""
    ENTRIES = (("dd3d_predictor_wgrad", "predictor_wgrad"), ("dd3d_predictor_dgrad", "predictor_dgrad"))

    def __init__(self, device, B, level_hw, Cin, n, g_pitch, act, act_mode, act_pitch, plane_scale, g, maps, w, bias, scale, lo=None, slot=None,
                 fill=0.0, guard=0):
        GradCall.__init__(self, device, fill, guard)
        L = len(level_hw)
        self.B, self.level_hw, self.Cin, self.n, self.L = B, list(level_hw), Cin, n, L
        self.keep = (g, maps, w, bias, scale, lo, slot)
        a = hip.PredGradArgs()
        out = self.out
        K9 = 9 * Cin
        self.n_slices = hip.pred_grad_slices(B, level_hw)
        self.part, self.qpart = out(self.n_slices, n, K9), out(self.n_slices, n)
        self.dw_level, self.dw, self.db = out(L, n, K9), out(L, n, K9), out(L, n)
        self.q, self.r = out(L, n), out(L, n)
        self.dscale, self.doffset = out(L, hip.PG_MAX_SLOTS), out(L, hip.PG_MAX_SLOTS)
        self.da = [out(B, h, w_, Cin) for h, w_ in level_hw]
        for l, (h, w_) in enumerate(level_hw):
            a.act[l] = act[l] or None
            a.g[l], a.map[l] = g[l].data_ptr(), (maps[l].data_ptr() if maps is not None else None)
            a.w[l], a.bias[l], a.scale[l] = w[l].data_ptr(), bias[l].data_ptr(), scale[l].data_ptr()
            a.da[l] = self.da[l].data_ptr()
            a.H[l], a.W[l] = int(h), int(w_)
        a.lo = lo.data_ptr() if lo is not None else None
        a.slot = slot.data_ptr() if slot is not None else None
        a.part, a.qpart, a.dw_level, a.dw, a.db = (t.data_ptr() for t in (self.part, self.qpart, self.dw_level, self.dw, self.db))
        a.q, a.r, a.dscale, a.doffset = (t.data_ptr() for t in (self.q, self.r, self.dscale, self.doffset))
        a.num_levels, a.B, a.Cin, a.n, a.g_pitch = L, int(B), int(Cin), int(n), int(g_pitch)
        a.act_mode, a.act_pitch, a.n_slices, a.plane_scale = int(act_mode), int(act_pitch), self.n_slices, float(plane_scale)
        self.args = a
        # the first level of every distinct filter: the rows of dw / db that are written
        self.owners = [l for l in range(L) if all(w[m].data_ptr() != w[l].data_ptr() for m in range(l))]


def act_binding(plan, view):
    """(DD3D_PG_ACT_* mode, device address, pitch, plane scale) of the storage a plan keeps `view` in: its split planes where it has
    them, else f32 NHWC.  The reduced modes have no loader (pred_act_mode names them)."""
    if view.np and plan.use_planes:
        return pred_act_mode(plan), view.pptr, 0, float(view.buf.plane_scale)
    return hip.PG_ACT_F32, view.ptr, int(view.pitch), 1.0


class TowerLayerGrads(GradCall):
    """Buffers and dd3d_tower_grad_args of one tower layer over all levels.

    `x`, `y`: per level (mode, device address, pitch, plane scale) of the layer's input and stored output (one mode per side); `g`:
    per-level NHWC gradient tensors of pitch `g_pitch`; `w`: the [Cout, 3, 3, Cin] filter; `scale`: per-level [Cout]; `da_add`: per-level
    [B, h, w, Cin] tensors or None; `slab`: (part, qpart) shared with other layers that run in stream order, or None to allocate them.
    Outputs are allocated here, filled with `fill` and followed by `guard` words of it."""
    ENTRIES = (("dd3d_tower_wgrad", "tower_wgrad"), ("dd3d_tower_dgrad", "tower_dgrad"))

    def __init__(self, device, B, level_hw, Cin, Cout, x, y, g, g_pitch, w, scale, da_add=None, slab=None, fill=0.0, guard=0, dgrad_rows=0):
        GradCall.__init__(self, device, fill, guard)
        L = len(level_hw)
        self.B, self.level_hw, self.Cin, self.Cout, self.L = B, list(level_hw), Cin, Cout, L
        self.keep = (g, w, scale, da_add, slab)
        a = hip.TowerGradArgs()
        self.n_slices = hip.tower_grad_slices(B, level_hw, Cin, Cout)
        self.wgrad_outputs(a, slab, Cout, 9 * Cin, level=(L, ))  # one filter for all levels: dw is their sum
        self.da = [self.out(B, h, w_, Cin) for h, w_ in level_hw]
        for l, (h, w_) in enumerate(level_hw):
            a.x[l], a.y[l] = x[l][1] or None, y[l][1] or None
            a.g[l], a.scale[l], a.da[l] = g[l].data_ptr(), scale[l].data_ptr(), self.da[l].data_ptr()
            a.da_add[l] = da_add[l].data_ptr() if da_add is not None else None
            a.H[l], a.W[l] = int(h), int(w_)
        a.w = w.data_ptr()
        a.num_levels, a.B, a.Cin, a.Cout, a.g_pitch = L, int(B), int(Cin), int(Cout), int(g_pitch)
        a.x_mode, a.x_pitch, a.x_plane_scale = int(x[0][0]), int(x[0][2]), float(x[0][3])
        a.y_mode, a.y_pitch, a.y_plane_scale = int(y[0][0]), int(y[0][2]), float(y[0][3])
        assert all(v[0] == x[0][0] and v[2:] == x[0][2:] for v in x) and all(v[0] == y[0][0] and v[2:] == y[0][2:] for v in y)
        a.n_slices, a.dgrad_rows = self.n_slices, int(dgrad_rows)
        self.args = a


class FpnConvGrads(GradCall):
    """Buffers and dd3d_fpn_grad_args of one FPN convolution per level (k x k, stride 1 or 2, a filter per level, no ReLU).

    `in_hw`: per-level INPUT sizes; `x`: per level (mode, device address, pitch, plane scale) of the convolution's input, or None for a
    call that only runs the input gradient; `g`: per-level NHWC gradient tensors at the convolution's output, pitch `g_pitch`; `w`:
    per-level [Cout, k, k, Cin] filters; `scale`: per-level [Cout]; `mask`: per-level bindings like `x` of a stored tensor of the input's
    shape, or None; `add`: per-level [B, h, w, Cin] tensors (entries may be None) or None; `pool`: per level None, a [B, 2h, 2w, Cin]
    tensor, or "prev" for the input gradient of the level before (the transposed top-down path inside one call); `slab`: (part, qpart)
    shared with other calls that run in stream order, or None to allocate them.  Outputs are allocated here, filled with `fill` and
    followed by `guard` words of it."""
    ENTRIES = (("dd3d_fpn_wgrad", "fpn_wgrad"), ("dd3d_fpn_dgrad", "fpn_dgrad"))

    def __init__(self, device, B, in_hw, Cin, Cout, ksize, stride, x, g, g_pitch, w, scale, mask=None, add=None, pool=None, in_relu=False, slab=None,
                 fill=0.0, guard=0, dgrad_rows=0, wgrad=True, dgrad=True):
        GradCall.__init__(self, device, fill, guard)
        L = len(in_hw)
        self.B, self.in_hw, self.Cin, self.Cout, self.L, self.ksize, self.stride = B, list(in_hw), Cin, Cout, L, ksize, stride
        self.out_hw = [((h + stride - 1) // stride, (w_ + stride - 1) // stride) for h, w_ in in_hw]
        self.keep = (g, w, scale, add, pool, slab)
        self.with_wgrad, self.with_dgrad = bool(wgrad), bool(dgrad)
        a = hip.FpnGradArgs()
        self.n_slices = hip.fpn_grad_slices(B, in_hw, Cin, Cout, ksize, stride)
        self.part = self.qpart = self.dw_level = self.dw = self.q = self.r = None
        if wgrad:
            self.wgrad_outputs(a, slab, Cout, ksize * ksize * Cin, level=(L, ), total=(L, ))  # a filter per level
        self.da = [self.out(B, h, w_, Cin) for h, w_ in in_hw] if dgrad else None
        for l, (h, w_) in enumerate(in_hw):
            a.x[l] = (x[l][1] or None) if x is not None else None
            a.g[l], a.w[l], a.scale[l] = g[l].data_ptr(), w[l].data_ptr(), scale[l].data_ptr()
            a.mask[l] = (mask[l][1] or None) if mask is not None and mask[l] is not None else None
            a.add[l] = add[l].data_ptr() if add is not None and add[l] is not None else None
            src = pool[l] if pool is not None else None
            if isinstance(src, str):
                assert src == "prev" and l > 0 and dgrad
                src = self.da[l - 1]
            a.pool[l] = src.data_ptr() if src is not None else None
            a.pool_H[l], a.pool_W[l] = (int(src.shape[1]), int(src.shape[2])) if src is not None else (0, 0)
            a.da[l] = self.da[l].data_ptr() if dgrad else None
            a.H[l], a.W[l] = int(h), int(w_)
        a.num_levels, a.B, a.Cin, a.Cout, a.g_pitch = L, int(B), int(Cin), int(Cout), int(g_pitch)
        a.ksize, a.stride, a.in_relu = int(ksize), int(stride), int(bool(in_relu))
        a.x_mode, a.x_pitch, a.x_plane_scale = (int(x[0][0]), int(x[0][2]), float(x[0][3])) if x is not None else (0, 0, 1.0)
        m0 = next((m for m in (mask or []) if m is not None), None)
        a.mask_mode, a.mask_pitch, a.mask_plane_scale = (int(m0[0]), int(m0[2]), float(m0[3])) if m0 is not None else (0, 0, 1.0)
        assert x is None or all(v[0] == x[0][0] and v[2:] == x[0][2:] for v in x)
        a.n_slices, a.dgrad_rows = self.n_slices, int(dgrad_rows)
        self.args = a


class BackboneConvGrads(GradCall):
    """Buffers and dd3d_backbone_grad_args of ONE backbone convolution (k x k, stride 1 or 2; csrc/backbone_grads.hip).

    `H`, `W`: the INPUT's sizes; `x`, `y`: (mode, device address, pitch, plane scale) of the stored input and of the stored output whose
    ReLU the gradient crosses (`y` None: no mask; `x` None for a call that only runs the input gradient); `g`: [B, Ho, Wo, Cout] f32
    gradient at the output, possibly a channel slice of a wider tensor (its pitch is the tensor's stride); `w`: [Cout, k, k, Cin]; `scale`:
    [Cout]; `add`: [B, H, W, Cin] (a slice may be given) or None; `res`: (gradient [B, H, W, Cin], binding of the stored tensor that masks
    it) or None; `da`: a [B, H, W, Cin] slice of a wider gradient buffer to write into, or None to allocate it; `slab`: (part, qpart)
    shared with other calls that run in stream order, or None to allocate them.  Outputs are allocated here, filled with `fill` and
    followed by `guard` words of it."""
    ENTRIES = (("dd3d_backbone_wgrad", "backbone_wgrad"), ("dd3d_backbone_dgrad", "backbone_dgrad"))

    def __init__(self, device, B, H, W, Cin, Cout, ksize, stride, x, y, g, w, scale, add=None, res=None, da=None, slab=None, fill=0.0, guard=0,
                 dgrad_rows=0, dgrad_group=0, wgrad=True, dgrad=True):
        GradCall.__init__(self, device, fill, guard)
        self.B, self.H, self.W, self.Cin, self.Cout, self.ksize, self.stride = B, int(H), int(W), Cin, Cout, ksize, stride
        self.Ho, self.Wo = (self.H + stride - 1) // stride, (self.W + stride - 1) // stride
        self.keep = (g, w, scale, add, res, slab)
        self.scale = scale
        self.with_wgrad, self.with_dgrad = bool(wgrad), bool(dgrad)
        a = hip.BackboneGradArgs()
        pitch = self.pitch
        assert tuple(g.shape) == (B, self.Ho, self.Wo, Cout) and g.stride(-1) == 1, (tuple(g.shape), (B, self.Ho, self.Wo, Cout))
        self.n_slices = hip.backbone_grad_slices(B, self.H, self.W, Cin, Cout, ksize, stride)
        self.part = self.qpart = self.dw_level = self.dw = self.q = self.r = None
        if wgrad:
            self.wgrad_outputs(a, slab, Cout, ksize * ksize * Cin)
        if dgrad:
            self.da = self.out(B, self.H, self.W, Cin) if da is None else da
            assert tuple(self.da.shape) == (B, self.H, self.W, Cin) and self.da.stride(-1) == 1
            a.da, a.da_pitch = self.da.data_ptr(), pitch(self.da)
        else:
            self.da = None
        a.x = (x[1] or None) if x is not None else None
        a.y = (y[1] or None) if y is not None else None
        self.masked = y is not None
        a.g, a.w, a.scale, a.g_pitch = g.data_ptr(), w.data_ptr(), scale.data_ptr(), pitch(g)
        if add is not None:
            assert tuple(add.shape) == (B, self.H, self.W, Cin) and add.stride(-1) == 1
            a.add, a.add_pitch = add.data_ptr(), pitch(add)
        if res is not None:
            rg, ry = res
            assert tuple(rg.shape) == (B, self.H, self.W, Cin) and rg.stride(-1) == 1
            a.res_g, a.res_pitch, a.res_y = rg.data_ptr(), pitch(rg), ry[1] or None
            a.res_y_mode, a.res_y_pitch, a.res_y_plane_scale = int(ry[0]), int(ry[2]), float(ry[3])
        else:
            a.res_y_plane_scale = 1.0
        a.B, a.H, a.W, a.Cin, a.Cout, a.ksize, a.stride = int(B), self.H, self.W, int(Cin), int(Cout), int(ksize), int(stride)
        a.x_mode, a.x_pitch, a.x_plane_scale = (int(x[0]), int(x[2]), float(x[3])) if x is not None else (0, 0, 1.0)
        a.y_mode, a.y_pitch, a.y_plane_scale = (int(y[0]), int(y[2]), float(y[3])) if y is not None else (0, 0, 1.0)
        a.n_slices, a.dgrad_rows, a.dgrad_group = self.n_slices, int(dgrad_rows), int(dgrad_group)
        self.args = a


class PoolGrads(GradCall):
    """Buffers and dd3d_pool_grad_args of one 2x2 max-pool backward: `x` the binding of the pool's stored input ([B, H, W, C]), `g` the
    gradient at the pooled tensor (None with `res` alone), `res`: (a second part of it, binding of the stored tensor that masks it) or
    None, `add` [B, H, W, C] or None.  `da` is allocated here (filled with `fill`, followed by `guard` words)."""
    ENTRIES = (("dd3d_maxpool2x2_backward", "maxpool2x2_backward"), )

    def __init__(self, device, B, H, W, Cc, x, g, add=None, res=None, fill=0.0, guard=0):
        GradCall.__init__(self, device, fill, guard)
        self.B, self.H, self.W, self.C = B, int(H), int(W), int(Cc)
        self.keep = (g, add, res)
        self.da = self.out(B, self.H, self.W, self.C)
        pitch = self.pitch
        a = hip.PoolGradArgs()
        a.x, a.da, a.res_y_plane_scale = x[1] or None, self.da.data_ptr(), 1.0
        for t in ([g] if g is not None else []) + ([res[0]] if res is not None else []):
            assert tuple(t.shape) == (B, self.H // 2, self.W // 2, self.C) and t.stride(-1) == 1
        if g is not None:
            a.g, a.g_pitch = g.data_ptr(), pitch(g)
        if res is not None:
            a.res_g, a.res_pitch, a.res_y = res[0].data_ptr(), pitch(res[0]), res[1][1] or None
            a.res_y_mode, a.res_y_pitch, a.res_y_plane_scale = int(res[1][0]), int(res[1][2]), float(res[1][3])
        a.B, a.H, a.W, a.C = int(B), self.H, self.W, self.C
        a.x_mode, a.x_pitch, a.x_plane_scale = int(x[0]), int(x[2]), float(x[3])
        a.da_pitch = self.C
        if add is not None:
            assert tuple(add.shape) == (B, self.H, self.W, self.C) and add.stride(-1) == 1
            a.add, a.add_pitch = add.data_ptr(), pitch(add)
        self.args = a


class StemConvGrads(GradCall):
    """Buffers and dd3d_stem_grad_args of ONE stem convolution (csrc/stem_grads.hip): (ksize, stride, Cin, Cout) one of
    hip.STEM_GRAD_SHAPES.

    `H`, `W`: the INPUT's sizes; `x`: [B, H, W, Cin] f32, possibly a channel slice of a wider tensor (None for a call that only runs the
    input gradient); `y`: (mode, device address, pitch, plane scale) of the stored output whose ReLU the gradient crosses; `g`:
    [B, Ho, Wo, Cout] f32 gradient at the output (a slice may be given); `w`: [Cout, k, k, Cin]; `scale`: [Cout]; `da`: a [B, H, W, Cin]
    slice of a wider gradient buffer to write into, or None to allocate it; `slab`: (part, qpart) shared with other calls that run in
    stream order, or None to allocate them; `wgrad_blocks`: blocks of the weight gradient's main launch (0: one per slice).  Outputs are
    allocated here, filled with `fill` and followed by `guard` words of it."""
    ENTRIES = (("dd3d_stem_wgrad", "stem_wgrad"), ("dd3d_stem_dgrad", "stem_dgrad"))

    def __init__(self, device, B, H, W, Cin, Cout, ksize, stride, x, y, g, w, scale, da=None, slab=None, fill=0.0, guard=0, wgrad_blocks=0,
                 wgrad=True, dgrad=True):
        GradCall.__init__(self, device, fill, guard)
        self.B, self.H, self.W, self.Cin, self.Cout, self.ksize, self.stride = B, int(H), int(W), Cin, Cout, ksize, stride
        self.Ho, self.Wo = (self.H + stride - 1) // stride, (self.W + stride - 1) // stride
        self.keep = (x, g, w, scale, slab)
        self.scale = scale
        self.with_wgrad, self.with_dgrad = bool(wgrad), bool(dgrad)
        a = hip.StemGradArgs()
        pitch = self.pitch
        assert tuple(g.shape) == (B, self.Ho, self.Wo, Cout) and g.stride(-1) == 1, (tuple(g.shape), (B, self.Ho, self.Wo, Cout))
        self.n_slices = hip.stem_grad_slices(B, self.H, self.W, Cin, Cout, ksize, stride)
        self.part = self.qpart = self.dw_level = self.dw = self.q = self.r = self.da = None
        if wgrad:
            assert tuple(x.shape) == (B, self.H, self.W, Cin) and x.stride(-1) == 1, (tuple(x.shape), (B, self.H, self.W, Cin))
            self.wgrad_outputs(a, slab, Cout, ksize * ksize * Cin)
            a.x, a.x_pitch = x.data_ptr(), pitch(x)
        if dgrad:
            self.da = self.out(B, self.H, self.W, Cin) if da is None else da
            assert tuple(self.da.shape) == (B, self.H, self.W, Cin) and self.da.stride(-1) == 1
            a.da, a.da_pitch = self.da.data_ptr(), pitch(self.da)
        a.y, a.y_mode, a.y_pitch, a.y_plane_scale = y[1] or None, int(y[0]), int(y[2]), float(y[3])
        a.g, a.w, a.scale, a.g_pitch = g.data_ptr(), w.data_ptr(), scale.data_ptr(), pitch(g)
        a.B, a.H, a.W, a.Cin, a.Cout, a.ksize, a.stride = int(B), self.H, self.W, int(Cin), int(Cout), int(ksize), int(stride)
        a.n_slices, a.wgrad_blocks = self.n_slices, int(wgrad_blocks)
        self.args = a


class VovnetStemGrads(GradCall):
    """Buffers and dd3d_stem_grad_args of the VoVNet-V2 stem_1's weight gradient (dd3d_vovnet_stem_wgrad, csrc/stem_grads.hip):
    (ksize, stride, Cin, Cout) = hip.VOVNET_STEM_GRAD_SHAPE.  There is no input gradient: the image has none.

    `H`, `W`: the INPUT's sizes; `x`: [B, H, W, 4] f32 normalised image, possibly a channel slice of a wider tensor; `y`: (mode, device
    address, pitch, plane scale) of stem_1's stored output, whose ReLU the gradient crosses; `g`: [B, Ho, Wo, 64] f32 gradient at that
    output (a slice may be given); `w`: [64, 3, 3, 4]; `scale`: [64]; `slab`: (part, qpart) shared with other calls that run in stream
    order, or None to allocate them; `wgrad_blocks`: blocks of the main launch (0: one per slice).  Outputs are allocated here, filled
    with `fill` and followed by `guard` words of it."""
    ENTRIES = (("dd3d_vovnet_stem_wgrad", "vovnet_stem_wgrad"), )
    with_dgrad = False

    def __init__(self, device, B, H, W, x, y, g, w, scale, slab=None, fill=0.0, guard=0, wgrad_blocks=0):
        GradCall.__init__(self, device, fill, guard)
        ksize, stride, Cin, Cout = hip.VOVNET_STEM_GRAD_SHAPE
        self.B, self.H, self.W, self.Cin, self.Cout, self.ksize, self.stride = B, int(H), int(W), Cin, Cout, ksize, stride
        self.Ho, self.Wo = (self.H + stride - 1) // stride, (self.W + stride - 1) // stride
        self.keep = (x, g, w, scale, slab)
        self.scale = scale
        a = hip.StemGradArgs()
        pitch = self.pitch
        assert tuple(g.shape) == (B, self.Ho, self.Wo, Cout) and g.stride(-1) == 1, (tuple(g.shape), (B, self.Ho, self.Wo, Cout))
        assert tuple(x.shape) == (B, self.H, self.W, Cin) and x.stride(-1) == 1, (tuple(x.shape), (B, self.H, self.W, Cin))
        assert tuple(w.shape) == (Cout, ksize, ksize, Cin) and w.is_contiguous(), tuple(w.shape)
        self.n_slices = hip.vovnet_stem_grad_slices(B, self.H, self.W)
        self.wgrad_outputs(a, slab, Cout, ksize * ksize * Cin)
        a.x, a.x_pitch = x.data_ptr(), pitch(x)
        a.y, a.y_mode, a.y_pitch, a.y_plane_scale = y[1] or None, int(y[0]), int(y[2]), float(y[3])
        a.g, a.w, a.scale, a.g_pitch = g.data_ptr(), w.data_ptr(), scale.data_ptr(), pitch(g)
        a.B, a.H, a.W, a.Cin, a.Cout, a.ksize, a.stride = int(B), self.H, self.W, int(Cin), int(Cout), int(ksize), int(stride)
        a.n_slices, a.wgrad_blocks = self.n_slices, int(wgrad_blocks)
        self.args = a


class VovnetConvGrads(BackboneConvGrads):
    """BackboneConvGrads through dd3d_vovnet_conv_wgrad / dd3d_vovnet_conv_dgrad: the same call and kernels under the limits
    hip.VG_MAX_CIN / hip.VG_MAX_COUT."""
    ENTRIES = (("dd3d_vovnet_conv_wgrad", "vovnet_conv_wgrad"), ("dd3d_vovnet_conv_dgrad", "vovnet_conv_dgrad"))


class SumGrads(GradCall):
    """One dd3d_vovnet_add launch: `da` [B, H, W, C] = a + b, two f32 NHWC gradients of that shape (slices may be given).  `da` is
    allocated here (filled with `fill`, followed by `guard` words)."""
    def __init__(self, device, a, b, fill=0.0, guard=0):
        GradCall.__init__(self, device, fill, guard)
        assert tuple(a.shape) == tuple(b.shape) and a.dim() == 4 and a.stride(-1) == 1 and b.stride(-1) == 1, (tuple(a.shape), tuple(b.shape))
        self.keep = (a, b)
        self.da = self.out(*a.shape)
        self.call = (a.data_ptr(), b.data_ptr(), self.da.data_ptr(), int(a.numel() // a.shape[-1]), int(a.shape[-1]), self.pitch(a), self.pitch(b),
                     int(a.shape[-1]))

    def launch(self, lib, st):  # (positional arguments: there is no args struct to pass by reference)
        hip.check(lib.dd3d_vovnet_add(*self.call, st), "vovnet_add")


class EseGrads(GradCall):
    """Buffers and dd3d_ese_grad_args of one eSE gate's backward (csrc/vovnet_grads.hip): `xt` the binding of the stored pre-eSE tensor
    ([B, H, W, C]), `g` the gradient at the module output ([B, H, W, C], a slice may be given), `fc_w` [C, C] and `fc_b` [C] on the
    device.  Outputs are allocated here, filled with `fill` and followed by `guard` words of it: g_xt [B, H, W, C] (not masked by xt's own
    ReLU), d_fc_w [C, C], d_fc_b [C], and the per-image vectors m, z, s, dz, u [B, C]."""
    ENTRIES = (("dd3d_ese_backward", "ese_backward"), )

    def __init__(self, device, B, H, W, Cc, xt, g, fc_w, fc_b, rsplit=None, fill=0.0, guard=0):
        GradCall.__init__(self, device, fill, guard)
        self.B, self.H, self.W, self.C = B, int(H), int(W), int(Cc)
        self.keep = (g, fc_w, fc_b)
        out = self.out
        HW = self.H * self.W
        self.rsplit = hip.ese_grad_rsplit(HW) if rsplit is None else int(rsplit)
        assert tuple(g.shape) == (B, self.H, self.W, self.C) and g.stride(-1) == 1, (tuple(g.shape), (B, self.H, self.W, self.C))
        assert tuple(fc_w.shape) == (self.C, self.C) and tuple(fc_b.shape) == (self.C, ) and fc_w.is_contiguous()
        self.part = out(B, self.rsplit, 2, self.C)
        self.m, self.z, self.s, self.dz, self.u = (out(B, self.C) for _ in range(5))
        self.g_xt, self.d_fc_w, self.d_fc_b = out(B, self.H, self.W, self.C), out(self.C, self.C), out(self.C)
        self.da = self.g_xt
        a = hip.EseGradArgs()
        a.xt, a.xt_mode, a.xt_pitch, a.xt_plane_scale = xt[1] or None, int(xt[0]), int(xt[2]), float(xt[3])
        a.g, a.g_pitch = g.data_ptr(), self.pitch(g)
        a.fc_w, a.fc_b = fc_w.data_ptr(), fc_b.data_ptr()
        a.part, a.m, a.z, a.s, a.dz, a.u = (t.data_ptr() for t in (self.part, self.m, self.z, self.s, self.dz, self.u))
        a.g_xt, a.gxt_pitch, a.d_fc_w, a.d_fc_b = self.g_xt.data_ptr(), self.C, self.d_fc_w.data_ptr(), self.d_fc_b.data_ptr()
        a.B, a.HW, a.C, a.rsplit = int(B), HW, self.C, self.rsplit
        self.args = a


class Pool3Grads(GradCall):
    """Buffers and dd3d_pool3_grad_args of one MaxPool2d(3, 2, ceil_mode=True) backward: `x` the binding of the pool's stored input
    ([B, H, W, C]), `g` the gradient at the pooled tensor ([B, pool3_out(H), pool3_out(W), C], a slice may be given), `add` [B, H, W, C] or
    None.  `da` is allocated here (filled with `fill`, followed by `guard` words)."""
    ENTRIES = (("dd3d_maxpool3x3s2_ceil_backward", "maxpool3x3s2_ceil_backward"), )

    def __init__(self, device, B, H, W, Cc, x, g, add=None, fill=0.0, guard=0):
        GradCall.__init__(self, device, fill, guard)
        self.B, self.H, self.W, self.C = B, int(H), int(W), int(Cc)
        self.Ho, self.Wo = hip.pool3_out(self.H), hip.pool3_out(self.W)
        self.keep = (g, add)
        self.da = self.out(B, self.H, self.W, self.C)
        pitch = self.pitch
        assert tuple(g.shape) == (B, self.Ho, self.Wo, self.C) and g.stride(-1) == 1, (tuple(g.shape), (B, self.Ho, self.Wo, self.C))
        a = hip.Pool3GradArgs()
        a.x, a.g, a.g_pitch, a.da, a.da_pitch = x[1] or None, g.data_ptr(), pitch(g), self.da.data_ptr(), self.C
        a.B, a.H, a.W, a.C = int(B), self.H, self.W, self.C
        a.x_mode, a.x_pitch, a.x_plane_scale = int(x[0]), int(x[2]), float(x[3])
        if add is not None:
            assert tuple(add.shape) == (B, self.H, self.W, self.C) and add.stride(-1) == 1
            a.add, a.add_pitch = add.data_ptr(), pitch(add)
        self.args = a


class TowerBnGrads(GradCall):
    """Buffers and dd3d_tower_bn_args of one batch-statistics tower layer's norm backward over all levels (csrc/tower_bn.hip): the
    segments are the levels.  `raw`: per-level [B, h, w, C] f32 views' (address, pitch) of the stored convolution output; `y`: per level
    (mode, device address, pitch, plane scale) of the stored layer output; `g`: per-level NHWC gradient tensors at y, pitch `g_pitch`;
    `stats`: per-level [BN_STAT_ROWS, C] tensors the forward wrote; `part`: the scratch rows shared with the forward's statistics.
    Outputs are allocated here, filled with `fill` and followed by `guard` words of it: qp [L, 2, C] (q, p) and gc, per level [B, h, w, C]."""
    ENTRIES = (("dd3d_bn_backward_reduce", "bn_backward_reduce"), ("dd3d_bn_backward_apply", "bn_backward_apply"))

    def __init__(self, device, B, level_hw, Cc, raw, y, g, g_pitch, stats, part, fill=0.0, guard=0):
        GradCall.__init__(self, device, fill, guard)
        L = len(level_hw)
        self.B, self.level_hw, self.C, self.L = B, list(level_hw), Cc, L
        self.keep = (g, stats, part)
        self.qp = self.out(L, 2, Cc)
        self.gc = [self.out(B, h, w_, Cc) for h, w_ in level_hw]
        a = hip.TowerBnArgs()
        for l, (h, w_) in enumerate(level_hw):
            a.c[l], a.y[l], a.g[l], a.stats[l] = raw[l][0] or None, y[l][1] or None, g[l].data_ptr(), stats[l].data_ptr()
            a.qp[l], a.gc[l], a.N[l] = self.qp[l].data_ptr(), self.gc[l].data_ptr(), int(B * h * w_)
        assert all(v[0] == y[0][0] and v[2:] == y[0][2:] for v in y) and all(r[1] == raw[0][1] for r in raw)
        a.num_segs, a.C, a.c_pitch, a.g_pitch = L, int(Cc), int(raw[0][1]), int(g_pitch)
        a.y_mode, a.y_pitch, a.plane_scale = int(y[0][0]), int(y[0][2]), float(y[0][3])
        self.n_slices = hip.bn_slices([B * h * w_ for h, w_ in level_hw])
        assert part.numel() >= self.n_slices * 2 * Cc
        a.part, a.n_slices = part.data_ptr(), int(part.numel() // (2 * Cc))
        self.args = a


class FpnBnGrads(TowerBnGrads):
    """TowerBnGrads without the mask, for the FPN's norms (csrc/fpn_bn.hip; no ReLU follows them): the segments are the stages, finest
    first, no stored output is bound.  qp [L, 2, C] holds (d beta, d gamma) of every stage's norm, gc the gradient at its raw convolution."""
    ENTRIES = (("dd3d_bn_backward_reduce_linear", "bn_backward_reduce_linear"), ("dd3d_bn_backward_apply_linear", "bn_backward_apply_linear"))

    def __init__(self, device, B, level_hw, Cc, raw, g, g_pitch, stats, part, fill=0.0, guard=0):
        TowerBnGrads.__init__(self, device, B, level_hw, Cc, raw, [(hip.PG_ACT_F32, 0, 0, 1.0)] * len(level_hw), g, g_pitch, stats, part, fill=fill,
                              guard=guard)


class BackboneBnGrads(TowerBnGrads):
    """The norm backward of ONE convolution of the DLA-34 bottom-up network under backbone_batch_stats (csrc/backbone_bn.hip; the widths
    16 .. 512): one segment.  `y`: (mode, device address, pitch, plane scale) of the stored tensor whose sign masks `g` -- the layer's own
    output behind a ReLU, the block's output for a project (its gradient is the residual's share G * [x1 > 0]) -- or None for no mask.
    qp [1, 2, C] holds (d beta, d gamma), gc[0] the dense gradient [B, h, w, C] at the raw convolution output."""
    ENTRIES = (("dd3d_backbone_bn_backward_reduce", "backbone_bn_backward_reduce"), ("dd3d_backbone_bn_backward_apply", "backbone_bn_backward_apply"))
    LINEAR = (("dd3d_backbone_bn_backward_reduce_linear", "backbone_bn_backward_reduce_linear"),
              ("dd3d_backbone_bn_backward_apply_linear", "backbone_bn_backward_apply_linear"))

    def __init__(self, device, B, hw, Cc, raw, y, g, stats, part, fill=0.0, guard=0):
        assert tuple(g.shape) == (B, hw[0], hw[1], Cc) and g.stride(-1) == 1, (tuple(g.shape), (B, hw[0], hw[1], Cc))
        self.masked = y is not None
        if not self.masked:
            self.ENTRIES = self.LINEAR
        TowerBnGrads.__init__(self, device, B, [hw], Cc, [raw], [y if self.masked else (hip.PG_ACT_F32, 0, 0, 1.0)], [g], self.pitch(g), [stats], part,
                              fill=fill, guard=guard)


def check_backbone_batch_stats(model, B, Hp, Wp, stem_grads=False):
    """What LossPlan(backbone_batch_stats=True) refuses before anything is built: a bottom-up network without trainable BatchNorm2d (the
    flag must not be a silent no-op), everything but the DLA-34 lowering (VoVNet, the Bottleneck variants, force_generic_dla), a level
    with one value per channel (in torch's words), the arithmetic modes and lowerings without split planes, and an odd canvas under
    stem_grads."""
    import os
    from dd3d_amd.modeling.dla import DLA, BasicBlock
    cfg, net = model.cfg, model.backbone.bottom_up
    if str(cfg.FE.BACKBONE.NORM) != "BN":
        raise ValueError(f"backbone_batch_stats needs FE.BACKBONE.NORM = 'BN' (it is {str(cfg.FE.BACKBONE.NORM)!r}): the bottom-up network has no norm "
                         "that uses batch statistics")
    if not isinstance(net, DLA):
        raise NotImplementedError(f"backbone_batch_stats covers the DLA-34 bottom-up network; {type(net).__name__} (the VoVNet-V2 family) has no "
                                  "batch-statistics lowering")
    if net.block is not BasicBlock:
        raise NotImplementedError(f"backbone_batch_stats covers BasicBlock trees (DLA-34); the {net.block.__name__} DLA variants have no "
                                  "batch-statistics lowering")
    if max(net.levels) > 2 or net.residual_root:
        raise NotImplementedError("backbone_batch_stats covers trees at most two deep without a residual root (DLA-34)")
    if getattr(model, "force_generic_dla", False):
        raise NotImplementedError("backbone_batch_stats follows the DLA-34 lowering; force_generic_dla has no batch-statistics form")
    bad = [int(c) for c in net.channels if not hip.backbone_bn_width_ok(int(c))]
    if bad:
        raise NotImplementedError(f"backbone_batch_stats takes 16, multiples of 32 up to 256 and multiples of 256 up to {hip.BBN_MAX_C} channels "
                                  f"(a level has {bad[0]})")
    mode = plan_math(model)
    if mode in (hip.MATH_BF16X2, hip.MATH_BF16):
        name = {hip.MATH_BF16X2: "bf16x2", hip.MATH_BF16: "bf16"}[mode]
        raise NotImplementedError(f"backbone_batch_stats stores f16x2 or bf16x3 planes; the arithmetic mode {name!r} has no apply")
    for on, what in ((mode == hip.MATH_F32, "DD3D_MATH=f32"), (mode == hip.MATH_BF16X3 and os.environ.get("DD3D_PLANES", "1") == "0", "DD3D_PLANES=0"),
                     (os.environ.get("DD3D_PLANES_ONLY", "1") == "0", "DD3D_PLANES_ONLY=0")):
        if on:
            raise NotImplementedError(f"backbone_batch_stats is built on the split-plane trees; {what} selects a lowering with f32 twins, which has "
                                      "no batch-statistics form")
    if stem_grads and (int(Hp) % 2 or int(Wp) % 2):
        raise NotImplementedError(f"backbone_batch_stats with stem gradients needs an even canvas ({Hp} x {Wp}): the stem's lowering sizes level1 as "
                                  "floor(H / 2), the stride-2 backward as ceil(H / 2)")
    h, w = int(Hp), int(Wp)
    for i, c in enumerate(net.channels):
        if i:
            h, w = h // 2, w // 2
        if B * h * w < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size [{B}, {c}, {h}, {w}] "
                             f"(level{i} of the bottom-up network on a {Hp} x {Wp} canvas)")


def plan_math(model):
    """The DD3D_MATH_* a plan of `model` will run on (ForwardPlan._trunk's rule), known before the plan exists."""
    from dd3d_amd.engine.tiling import MATH_NAMES, default_math
    m = getattr(model, "math", None)
    return default_math() if m is None else MATH_NAMES[m] if isinstance(m, str) else int(m)


def check_fpn_batch_stats(model, B, Hp, Wp, backbone_covered=False):
    """What LossPlan(fpn_batch_stats=True) refuses before anything is built: an FPN without trainable BatchNorm2d (the flag must not be a
    silent no-op), a bottom-up network that would need batch statistics too, a stage with one value per channel (in torch's words),
    widths the kernels do not take, another fuse type, and the lowerings without the fused split-plane FPN."""
    import math
    import os
    cfg, fpn = model.cfg, model.backbone
    if str(cfg.FE.FPN.NORM) != "BN":
        raise ValueError(f"fpn_batch_stats needs FE.FPN.NORM = 'BN' (it is {str(cfg.FE.FPN.NORM)!r}): the FPN has no norm that uses batch statistics")
    if str(cfg.FE.BACKBONE.NORM) == "BN" and not backbone_covered:  # (backbone_batch_stats=True gives the bottom-up network's)
        raise NotImplementedError("fpn_batch_stats covers the FPN; FE.BACKBONE.NORM = 'BN' would need batch statistics in the bottom-up network as well")
    if fpn._fuse_type != "sum":
        raise NotImplementedError(f"fpn_batch_stats implements FE.FPN FUSE_TYPE 'sum' (it is {fpn._fuse_type!r})")
    Cf = int(getattr(fpn, f"fpn_output{fpn.stages[0]}").out_channels)
    if Cf % 32 or Cf > hip.BN_MAX_C:
        raise NotImplementedError(f"fpn_batch_stats needs FE.FPN.OUT_CHANNELS to be a multiple of 32 up to {hip.BN_MAX_C} (it is {Cf})")
    for s in fpn.stages:
        h, w = math.ceil(Hp / 2**s), math.ceil(Wp / 2**s)
        if B * h * w < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size [{B}, {Cf}, {h}, {w}] "
                             f"(FPN stage {s} on a {Hp} x {Wp} canvas)")
    mode = plan_math(model)
    if mode in (hip.MATH_BF16X2, hip.MATH_BF16):
        name = {hip.MATH_BF16X2: "bf16x2", hip.MATH_BF16: "bf16"}[mode]
        raise NotImplementedError(f"fpn_batch_stats stores f16x2 or bf16x3 planes; the arithmetic mode {name!r} has no apply")
    for on, what in ((mode == hip.MATH_F32, "DD3D_MATH=f32"), (mode == hip.MATH_BF16X3 and os.environ.get("DD3D_PLANES", "1") == "0", "DD3D_PLANES=0"),
                     (os.environ.get("DD3D_PLANES_ONLY", "1") == "0", "DD3D_PLANES_ONLY=0")):
        if on:
            raise NotImplementedError(f"fpn_batch_stats is built on the fused split-plane FPN; {what} selects the round-3 FPN lowering, which has no "
                                      "batch-statistics form (separate top-down launches on f32 laterals)")


def check_batch_stats(model, B, Hp, Wp, fpn_covered=False, backbone_covered=False):
    """What LossPlan(batch_stats=True) refuses before anything is built: a level with one value per channel (the reference raises there
    too, in torch's words) and trunk norms that would need batch statistics as well (`fpn_covered`: fpn_batch_stats=True gives the FPN's;
    `backbone_covered`: backbone_batch_stats=True the bottom-up network's)."""
    import math
    cfg = model.cfg
    for key, node in (("FE.BACKBONE.NORM", cfg.FE.BACKBONE), ("FE.FPN.NORM", cfg.FE.FPN)):
        if str(node.NORM) == "BN" and not (fpn_covered and key == "FE.FPN.NORM") and not (backbone_covered and key == "FE.BACKBONE.NORM"):
            raise NotImplementedError(f"batch_stats covers the head towers; {key} = 'BN' would need batch statistics in the trunk as well")
    for s in model.backbone_output_shape:
        h, w = math.ceil(Hp / s.stride), math.ceil(Wp / s.stride)
        if B * h * w < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size [{B}, {s.channels}, {h}, {w}] "
                             f"(stride {s.stride} on a {Hp} x {Wp} canvas)")


def slice_binding(bind, c0, npix):
    """The binding (mode, address, pitch, plane scale) of the channel slice that starts at channel `c0` of a stored buffer with `npix`
    pixels: f32 moves the pointer by channels, split planes by whole 32-channel chunk images (f16x2: 128, bf16x3: 192 bytes a pixel)."""
    mode, addr, pitch, scale = bind
    if not addr or not c0:
        return bind
    if mode == hip.PG_ACT_F32:
        return (mode, addr + 4 * c0, pitch, scale)
    assert c0 % 32 == 0, c0
    return (mode, addr + (c0 // 32) * npix * (128 if mode == hip.PG_ACT_F16X2 else 192), pitch, scale)


def filter_copy(conv, device, cin=None):
    """The [Cout, k, k, Cin] float32 copy of a convolution's filter the gradient kernels read, on `device`; with `cin` the input channels
    are padded with zero filters up to that width (a buffer's pad channels, the image's fourth channel)."""
    w = conv.weight.detach().float()
    if cin is not None and w.shape[1] < cin:
        w = torch.cat([w, torch.zeros(w.shape[0], cin - w.shape[1], *w.shape[2:], dtype=w.dtype, device=w.device)], 1)
    return w.permute(0, 2, 3, 1).contiguous().to(device)


def check_dla_backward(dla, model=None):
    """NotImplementedError naming what the backbone backward does not cover (it covers BackboneLowering._tree: DLA-34)."""
    from dd3d_amd.modeling.dla import DLA, BasicBlock
    if not isinstance(dla, DLA):
        raise NotImplementedError(f"backbone gradients cover the DLA-34 backbone; {type(dla).__name__} (the V2-99 family) has no backward")
    if dla.block is not BasicBlock:
        raise NotImplementedError(f"backbone gradients cover BasicBlock trees (DLA-34); the {dla.block.__name__} DLA variants have no backward")
    if max(dla.levels) > 2 or dla.residual_root:
        raise NotImplementedError("backbone gradients cover trees at most two deep without a residual root (DLA-34)")
    if model is not None and getattr(model, "force_generic_dla", False):
        raise NotImplementedError("backbone gradients follow the DLA-34 lowering; force_generic_dla has no backward")


def _dla_tree_calls(m, H, W):
    """(ksize, stride, input H, W, Cin, Cout) of every convolution of a tree whose input is H x W."""
    s = m.stride
    Ho, Wo = H // s, W // s
    if m.levels == 2:
        return _dla_tree_calls(m.tree1, H, W) + _dla_tree_calls(m.tree2, Ho, Wo)
    oc, ic = m.out_channels, m.in_channels
    calls = [(1, 1, Ho, Wo, m.root_dim, oc), (3, 1, Ho, Wo, oc, oc), (3, 1, Ho, Wo, oc, oc), (3, 1, Ho, Wo, oc, oc), (3, s, H, W, ic, oc)]
    if m.project is not None:
        calls.append((1, 1, Ho, Wo, ic, oc))
    return calls


def dla_slab_words(B, dla, H1, W1):
    """Floats of (part, qpart) the largest weight-gradient call of the backbone backward needs; H1 x W1: the level1 tensor."""
    rows = qrows = 0
    H, W = H1, W1
    for lvl in range(2, 6):
        tree = getattr(dla, f"level{lvl}")
        for k, s, h, w_, ci, co in _dla_tree_calls(tree, H, W):
            n = hip.backbone_grad_slices(B, h, w_, ci, co, k, s)
            rows, qrows = max(rows, n * co * k * k * ci), max(qrows, n * co)
        H, W = H // 2, W // 2
    return rows, qrows


def dla_backward(device, B, dla, G, acts, vec, slab=None, fill=0.0, guard=0, bn=None):
    """The calls of the DLA-34 backward in their order, level5 down to level2 (include/dd3d_hip.h states the mathematics).  Per depth-1
    tree: root, tree2.conv2, tree2.conv1, tree1.conv2, project, tree1.conv1, pool; a depth-2 tree runs its tree2 first, then its tree1.

    `G`: {level<n>: [B, h, w, C] gradient the FPN sends to a backbone output feature}; level5's is required; `acts`: {name of a stored
    buffer of BackboneLowering._tree (<tree>.cat, <tree>.tree1.mid, <tree>.tree2.mid, <tree>.bottom, <tree>.out) and "level1" for the
    tensor level2 reads: ((mode, address, pitch, plane scale) of the WHOLE buffer, H, W, C)}; `vec`: host vector -> device.  Returns
    ({key: BackboneConvGrads or PoolGrads}, the gradient [B, h1, w1, C1] at the level1 tensor); a convolution's layer carries its module
    as `conv` and what it reads as `src` = {operand: (buffer name, first channel, channels)}.

    `bn` (backbone_batch_stats): dict(layers={key: dict(raw=(address, pitch), stats=tensor)}, part=scratch, ones={C: [C] ones}).  Then a
    BackboneBnGrads sits between each layer's incoming gradient and its convolution gradients (the layer's `bn`, run in front of it): it
    masks G by the stored tensor the running-statistics call would mask it by -- the layer's own output; for a project the block's
    output x1, whose ReLU the residual's share crossed -- and returns G_c; the convolution calls run on g := G_c without a mask, scale
    ones.  `add` and `res` (the residual's share G * [x1 > 0], masked on the way by the stored x1) are what they were."""
    from dd3d_amd.layers import fold_norm
    check_dla_backward(dla)
    layers, common = OrderedDict(), dict(fill=fill, guard=guard)

    def bind(ref):
        key, c0, _ = ref
        b, h, w_, _ = acts[key]
        return slice_binding(b, c0, B * h * w_)

    def conv(key, mod, x, y, g, stride, add=None, res=None):
        k, cin, cout = int(mod.weight.shape[-1]), int(mod.weight.shape[1]), int(mod.weight.shape[0])
        assert x[2] == cin and (y is None or y[2] == cout), (key, x, y)
        H, W = acts[x[0]][1], acts[x[0]][2]
        norm_call, yb, scale = None, bind(y) if y is not None else None, None
        if bn is not None:
            rec = bn["layers"][key]
            norm_call = BackboneBnGrads(device, B, ((H + stride - 1) // stride, (W + stride - 1) // stride), cout, rec["raw"], yb, g, rec["stats"], bn["part"],
                                        **common)
            g, yb, scale = norm_call.gc[0], None, bn["ones"][cout]
        lay = BackboneConvGrads(device, B, H, W, cin, cout, k, stride, bind(x), yb, g, filter_copy(mod, device),
                                vec(fold_norm(mod, None)[0]) if scale is None else scale, add=add, res=(res[0], bind(res[1])) if res is not None else None,
                                slab=slab, **common)
        lay.bn = norm_call
        lay.conv, lay.norm, lay.src = mod, getattr(mod, "norm", None), dict(x=x, y=y, res_y=res[1] if res is not None else None)
        layers[key] = lay
        return lay.da

    def tree1(m, name, x, dst, G_out, cat=None, bottom=None, bottom_add=None, x_add=None, x_slice=None):
        """A depth-1 tree: returns (the gradient at its input, the gradient over its root's concat buffer)."""
        oc, ic, s = m.out_channels, m.in_channels, m.stride
        own = cat is None
        cat = cat or name + ".cat"
        dst = dst or (name + ".out", 0, oc)
        Dcat = conv(name + ".root", m.root.conv, (cat, 0, acts[cat][3]), dst, G_out, 1)
        x2, x1, mid1, mid2 = (cat, 0, oc), (cat, oc, oc), (name + ".tree1.mid", 0, oc), (name + ".tree2.mid", 0, oc)
        if own and m.level_root:
            bottom, bottom_add = (cat, 2 * oc, ic), Dcat[..., 2 * oc:2 * oc + ic]
        D2, D1 = Dcat[..., :oc], Dcat[..., oc:2 * oc]
        Gmid2 = conv(name + ".tree2.conv2", m.tree2.conv2, mid2, x2, D2, 1)
        Gx1 = conv(name + ".tree2.conv1", m.tree2.conv1, x1, mid2, Gmid2, 1, add=D1, res=(D2, x2))
        Gmid1 = conv(name + ".tree1.conv2", m.tree1.conv2, mid1, x1, Gx1, 1)
        if s == 2:
            Gbottom, res = bottom_add, None
            if m.project is not None:  # (the gradient at `residual` is Gx1 * [x1 > 0]: the call masks it by the stored x1)
                Gbottom = conv(name + ".project", m.project, bottom or (name + ".bottom", 0, ic), x1, Gx1, 1, add=bottom_add)
            else:  # the pooled tensor is the residual itself
                res = (Gx1, bind(x1))
            Cx = conv(name + ".tree1.conv1", m.tree1.conv1, x, mid1, Gmid1, 2, add=x_add)
            H, W = acts[x[0]][1], acts[x[0]][2]
            pool = PoolGrads(device, B, H, W, ic, bind(x), Gbottom, add=Cx, res=res, **common)
            pool.src = dict(x=x, res_y=x1 if res is not None else None)
            layers[name + ".pool"] = pool
            return pool.da, Dcat
        assert x_add is None or x_slice is None, name
        A = Dcat[..., x_slice[0]:x_slice[0] + x_slice[1]] if x_slice is not None else x_add
        if m.project is not None:  # bottom = x: the project's input gradient joins x's
            A = conv(name + ".project", m.project, x, x1, Gx1, 1, add=A)
            return conv(name + ".tree1.conv1", m.tree1.conv1, x, mid1, Gmid1, 1, add=A), Dcat
        return conv(name + ".tree1.conv1", m.tree1.conv1, x, mid1, Gmid1, 1, add=A, res=(Gx1, x1)), Dcat

    def tree(m, name, x, G_out, x_add):
        if m.levels == 1:
            return tree1(m, name, x, None, G_out, x_add=x_add)[0]
        oc, ic = m.out_channels, m.in_channels
        cat2 = name + ".cat"
        off, bottom = 2 * oc, None
        if m.level_root:
            bottom, off = (cat2, off, ic), off + ic
        t1 = (cat2, off, oc)
        G_t1, Dcat2 = tree1(m.tree2, name + ".tree2", t1, None, G_out, cat=cat2, x_slice=(off, oc))
        return tree1(m.tree1, name + ".tree1", x, t1, G_t1, bottom=bottom, bottom_add=Dcat2[..., 2 * oc:2 * oc + ic] if m.level_root else None,
                     x_add=x_add)[0]

    out_name = lambda lvl: f"level{lvl}"
    g = G["level5"]
    for lvl in (5, 4, 3, 2):
        m = getattr(dla, f"level{lvl}")
        if lvl == 2:
            x = ("level1", 0, m.in_channels)
        else:
            p = getattr(dla, f"level{lvl - 1}")
            x = (f"level{lvl - 1}.out" if p.levels == 1 else f"level{lvl - 1}.tree2.out", 0, m.in_channels)
        g = tree(m, out_name(lvl), x, g, G.get(f"level{lvl - 1}"))
    return layers, g


def conv_param_grads(named, lay, conv, norm, dw, scale, q, r):
    """{parameter name: gradient of the parameter's shape} of ONE convolution and its norm from the outputs of the call `lay` that ran its
    backward: the filter's from `dw` (lay.Cout x k x k x lay.Cin words; the gradients of the buffer's pad channels are dropped), the
    per-channel parameters' from `scale`, `q` and `r` (norm_param_grads); `named`: {id(parameter): name}."""
    params = {}
    k, cin = lay.ksize, int(conv.weight.shape[1])
    if id(conv.weight) in named:
        # (a copy even where the permuted view is contiguous already -- a 1 x 1 filter over all of the buffer's channels: the read-outs
        # return copies, never the plan's own memory, which the next run overwrites)
        params[named[id(conv.weight)]] = dw.view(lay.Cout, k, k, lay.Cin)[..., :cin].permute(0, 3, 1, 2).clone(memory_format=torch.contiguous_format)
    got = norm_param_grads(conv, norm, scale, q, r)
    for key, p in (("norm.weight", getattr(norm, "weight", None)), ("norm.bias", getattr(norm, "bias", None)), ("bias", conv.bias)):
        if key in got and id(p) in named:
            params[named[id(p)]] = got[key]
    return params


def dla_param_grads(named, layers, prefix=""):
    """{parameter name: gradient of the parameter's shape} from the layers of `dla_backward`; `named`: {id(parameter): name}."""
    params = {}
    for lay in layers.values():
        if getattr(lay, "conv", None) is None:
            continue
        norm_call = getattr(lay, "bn", None)
        if norm_call is None:
            params.update(conv_param_grads(named, lay, lay.conv, lay.norm, lay.dw, lay.scale, lay.q, lay.r))
            continue
        # batch statistics: d gamma = p, d beta = q of the norm's backward; the convolution call's own q / r are by-products (q: the sum
        # of G_c, a conv bias' gradient -- zero up to rounding, the norm removes the mean)
        params.update(conv_param_grads(named, lay, lay.conv, None, lay.dw, lay.scale, lay.q, lay.r))
        for p, v in ((lay.norm.weight, norm_call.qp[0, 1]), (lay.norm.bias, norm_call.qp[0, 0])):
            if id(p) in named:
                params[named[id(p)]] = v.clone()
    return params


def check_vovnet_backward(vov, model=None):
    """NotImplementedError naming what the VoVNet backward does not cover (it covers BackboneLowering._vovnet for the specs whose channel
    counts are multiples of 32: V-19-eSE, V-39-eSE, V-57-eSE, V-99-eSE)."""
    from dd3d_amd.modeling.vovnet import VoVNet
    if not isinstance(vov, VoVNet):
        raise NotImplementedError(f"vovnet_grads covers the VoVNet-V2 backbones; {type(vov).__name__} has its own backward: use stem_grads=True")
    if any(dw for _, _, dw in vov.stem_seqs):
        raise NotImplementedError("vovnet_grads: the depthwise specs (V-19-dw-eSE, V-19-slim-dw-eSE) have no backward for their depthwise 3x3 layers")
    for sname in vov.stage_names:
        for mname, m in getattr(vov, sname).named_children():
            if m.depthwise or m.conv_reduction is not None:
                raise NotImplementedError(f"vovnet_grads: {sname}.{mname} is depthwise; the depthwise 3x3 layers and conv_reduction have no backward")
            for what, ch in (("in_ch", m.in_ch), ("stage_ch", m.stage_ch), ("concat_ch", m.concat_ch)):
                if ch % 32:
                    raise NotImplementedError(f"vovnet_grads: {sname}.{mname}.{what} = {ch} is not a multiple of 32 (the slim specs): the gradient "
                                              "kernels have no zero-padded channel handling")


def _vovnet_geometry(vov, H1, W1):
    """{stage name: (H, W) of its tensors} from the size H1 x W1 of stem_1's output."""
    H, W = (H1 + 1) // 2, (W1 + 1) // 2  # stem_3: 3x3, stride 2, padding 1
    hw = {}
    for sname in vov.stage_names:
        if getattr(vov, sname).has_pool:
            H, W = hip.pool3_out(H), hip.pool3_out(W)
        hw[sname] = (H, W)
    return hw


def _vovnet_conv_calls(vov, H1, W1):
    """(ksize, stride, input H, W, Cin, Cout) of every convolution of the VoVNet backward; H1 x W1: stem_1's output."""
    from dd3d_amd.modeling.vovnet import seq_conv
    stem = [getattr(vov.stem, c) for c, _, _ in vov.stem_seqs]
    calls = [(3, int(cv.stride), H1, W1, int(cv.weight.shape[1]), int(cv.weight.shape[0])) for cv in stem[1:]]
    hw = _vovnet_geometry(vov, H1, W1)
    for sname in vov.stage_names:
        H, W = hw[sname]
        for _, m in getattr(vov, sname).named_children():
            cin = m.in_ch
            for layer in m.layers:
                calls.append((3, 1, H, W, cin, m.stage_ch))
                cin = m.stage_ch
            calls.append((1, 1, H, W, int(seq_conv(m.concat).weight.shape[1]), m.concat_ch))
    return calls


def vovnet_slab_words(B, vov, H1, W1):
    """Floats of (part, qpart) the largest weight-gradient call of the VoVNet backward needs; H1 x W1: stem_1's output."""
    rows = qrows = 0
    for k, s, h, w_, ci, co in _vovnet_conv_calls(vov, H1, W1):
        n = hip.backbone_grad_slices(B, h, w_, ci, co, k, s)
        rows, qrows = max(rows, n * co * k * k * ci), max(qrows, n * co)
    return rows, qrows


def vovnet_backward(device, B, vov, G, acts, vec, slab=None, fill=0.0, guard=0, stages=None, stem=True):
    """The calls of the VoVNet-V2 backward in their order, the last stage down to stem_2 (include/dd3d_hip.h states the mathematics).  Per
    OSA module, last to first: eSE, the concat 1x1 (weight gradient, then the input gradient over the whole concat width into one D_cat),
    layers n-1 .. 1 (layer i's incoming gradient is D_cat[slice i] + the input gradient of layer i+1, masked by the stored concat-buffer
    slice while staged), under `identity` the module input's sum T = D_cat[x] + G_out (one elementwise launch), layer 0 (its input
    gradient adds T, or D_cat[x] without the identity: (D_cat[x] + G_out) + dgrad).
    Between stages the 3x3 pool backward, adding the FPN's gradient at the pool's input; after stage2 stem_3 (stride 2) and stem_2.

    `G`: {stage<n>: [B, h, w, C] gradient the FPN sends to a stage output}; the last stage's is required; `acts`: {name of a stored buffer
    of BackboneLowering._vovnet (<stage>.<module>.cat, <stage>.<module>.xt, <stage>.out, stem.0, stem.1): ((mode, address, pitch, plane
    scale) of the WHOLE buffer, H, W, C)}; `vec`: host vector -> device; `stages`: a run of consecutive stage names (default: all); `stem`:
    go on through stem_3 and stem_2 when the run starts at stage2.  Returns ({key: EseGrads, VovnetConvGrads, SumGrads or Pool3Grads}, the gradient
    at the tensor the chain ends at: stem_1's stored output, not masked by its own ReLU, or the first stage's input); a convolution's
    layer carries its module as `conv`, its norm as `norm` and what it reads as `src` = {operand: (buffer name, first channel, channels)}."""
    from dd3d_amd.layers import fold_norm
    from dd3d_amd.modeling.vovnet import seq_conv, seq_norm
    check_vovnet_backward(vov)
    layers, common = OrderedDict(), dict(fill=fill, guard=guard)

    def bind(ref):
        key, c0, _ = ref
        b, h, w_, _ = acts[key]
        return slice_binding(b, c0, B * h * w_)

    def conv(key, mod, norm, x, y, g, add=None):
        k, cin, cout, stride = int(mod.weight.shape[-1]), int(mod.weight.shape[1]), int(mod.weight.shape[0]), int(mod.stride)
        assert x[2] == cin and y[2] == cout, (key, x, y)
        H, W = acts[x[0]][1], acts[x[0]][2]
        lay = VovnetConvGrads(device, B, H, W, cin, cout, k, stride, bind(x), bind(y), g, filter_copy(mod, device), vec(fold_norm(mod, norm)[0]),
                              add=add, slab=slab, **common)
        lay.conv, lay.norm, lay.src = mod, norm, dict(x=x, y=y)
        layers[key] = lay
        return lay.da

    names = list(stages or vov.stage_names)
    g = G[names[-1]]
    for si in reversed(range(len(names))):
        sname = names[si]
        stage = getattr(vov, sname)
        mods = list(stage.named_children())
        for mname, m in reversed(mods):
            cat, xt = f"{sname}.{mname}.cat", f"{sname}.{mname}.xt"
            n, pin, pst, pcc = len(m.layers), m.in_ch, m.stage_ch, m.concat_ch
            H, W, catC = acts[cat][1:]
            assert catC == pin + n * pst and acts[xt][1:] == (H, W, pcc), (cat, acts[cat][1:], acts[xt][1:])
            fc = m.ese.fc
            ese = EseGrads(device, B, H, W, pcc, bind((xt, 0, pcc)), g, vec(fc.weight.reshape(pcc, pcc)), vec(fc.bias), **common)
            ese.fc, ese.src = fc, dict(xt=(xt, 0, pcc))
            layers[f"{sname}.{mname}.ese"] = ese
            Dcat = conv(f"{sname}.{mname}.concat", seq_conv(m.concat), seq_norm(m.concat), (cat, 0, catC), (xt, 0, pcc), ese.g_xt)
            gl = Dcat[..., pin + (n - 1) * pst:]
            for i in reversed(range(n)):
                x = (cat, pin + (i - 1) * pst, pst) if i else (cat, 0, pin)
                add = Dcat[..., x[1]:x[1] + x[2]]
                if i == 0 and m.identity:  # the module input's three terms: (D_cat[x] + G_out) + layer 0's input gradient
                    head = SumGrads(device, add, g, **common)
                    head.src = {}
                    layers[f"{sname}.{mname}.sum"] = head
                    add = head.da
                gl = conv(f"{sname}.{mname}.{i}", seq_conv(m.layers[i]), seq_norm(m.layers[i]), x, (cat, pin + i * pst, pst), gl, add=add)
            g = gl  # the gradient at the module's input: the previous module's G_out
        if stage.has_pool and si > 0:
            prev = names[si - 1]
            b, h, w_, c = acts[prev + ".out"]
            pool = Pool3Grads(device, B, h, w_, c, bind((prev + ".out", 0, c)), g, add=G.get(prev), **common)
            pool.src = dict(x=(prev + ".out", 0, c))
            layers[sname + ".pool"] = pool
            g = pool.da
    if stem and not getattr(vov, names[0]).has_pool:
        first = f"{names[0]}.{next(iter(getattr(vov, names[0]).named_children()))[0]}.cat"
        (c2, n2, _), (c3, n3, _) = vov.stem_seqs[1], vov.stem_seqs[2]
        s2, s3 = getattr(vov.stem, c2), getattr(vov.stem, c3)
        g = conv("stem_3", s3, getattr(vov.stem, n3), ("stem.1", 0, int(s3.weight.shape[1])), (first, 0, int(s3.weight.shape[0])), g)
        g = conv("stem_2", s2, getattr(vov.stem, n2), ("stem.0", 0, int(s2.weight.shape[1])), ("stem.1", 0, int(s2.weight.shape[0])), g)
    return layers, g


def vovnet_param_grads(named, layers):
    """{parameter name: gradient of the parameter's shape} from the layers of `vovnet_backward`; `named`: {id(parameter): name}."""
    params = {}
    for lay in layers.values():
        fc = getattr(lay, "fc", None)
        if fc is not None:
            if id(fc.weight) in named:
                params[named[id(fc.weight)]] = lay.d_fc_w.view(fc.weight.shape).clone()
            if id(fc.bias) in named:
                params[named[id(fc.bias)]] = lay.d_fc_b.clone()
            continue
        # (nothing to drop: conv() asserts lay.Cin is the filter's own width; and no "bias" entry can occur: modeling/vovnet.py builds
        # every convolution with bias=False)
        if getattr(lay, "conv", None) is not None:
            params.update(conv_param_grads(named, lay, lay.conv, lay.norm, lay.dw, lay.scale, lay.q, lay.r))
    return params


def norm_param_grads(conv, norm, scale, q, r):
    """Gradients of one level's share of a tower layer's per-channel parameters from the kernels' sums q = sum g and r = sum g * conv:
    {"norm.weight", "norm.bias", "bias"} as far as the modules have them as parameters.  The forward is layers.fold_norm's:
    y = (conv + b - mean) * w * rstd + beta, with w * rstd = `scale`; without a norm y = conv + b."""
    out = {}
    b = conv.bias.detach().float().to(q.device) if conv.bias is not None else None
    if norm is not None and isinstance(norm.weight, torch.nn.Parameter):
        rstd = torch.rsqrt(norm.running_var.float() + norm.eps).to(q.device)
        centre = -norm.running_mean.float().to(q.device) if b is None else b - norm.running_mean.float().to(q.device)
        out["norm.weight"] = rstd * (r + centre * q)
        out["norm.bias"] = q.clone()
    if b is not None:
        out["bias"] = scale.to(q.device) * q if norm is not None else q.clone()
    return out


def _fpn_calls(fpn, acts):
    """(ksize, stride, input sizes per level, Cin) of every weight-gradient call of the FPN backward."""
    names, stages = list(fpn.in_features), list(fpn.stages)
    calls = [(3, 1, [acts[f"t{s}"][1:3] for s in stages], acts[f"t{stages[0]}"][3])]
    calls += [(1, 1, [acts[n][1:3]], acts[n][3]) for n in names]
    if fpn.top_block is not None:
        calls += [(3, 2, [acts[f"p{stages[-1] + i}"][1:3]], acts[f"p{stages[-1]}"][3]) for i in range(fpn.top_block.num_levels)]
    return calls


def fpn_slab_words(B, fpn, acts):
    """Floats of (part, qpart) the largest weight-gradient call of the FPN backward needs."""
    Cf = acts[f"t{fpn.stages[0]}"][3]
    n = [(hip.fpn_grad_slices(B, hw, ci, Cf, k, s), k * k * ci) for k, s, hw, ci in _fpn_calls(fpn, acts)]
    return max(sl * Cf * kk for sl, kk in n), max(sl * Cf for sl, _ in n)


def fpn_backward(device, B, fpn, G, acts, vec, slab=None, fill=0.0, guard=0, bn=None):
    """The calls of the FPN backward in their order (include/dd3d_hip.h states the mathematics): the top block (P7, then P6) down to D
    of the coarsest stage; the output convolutions (all weight gradients in one call, a filter per level; the input gradients finest
    stage first, each adding the 2x2 sums of the finer stage's: the transposed top-down path); the laterals, coarsest stage first.

    `G`: {p<s>: [B, h, w, Cf] gradient at every FPN output}; `acts`: {t<s> (stored top-down sum), p<s> (the coarsest stage's output and
    p6), backbone feature name: ((mode, address, pitch, plane scale), H, W, C)} as stored; `vec`: host vector -> device.  Returns
    ({key: FpnConvGrads}, {feature name: (gradient [B, h, w, C], real channels)}); a layer's `conv` is its module (`outputs`: a list).

    `bn` (fpn_batch_stats): {"outputs" / "laterals": dict(raw=[(address, pitch)], stats=[tensor], part=scratch, ones=[C]) per stage, finest
    first}.  Then the norms' backward runs in front of the convolutions': one FpnBnGrads over all stages on D and the output raws before
    `outputs`, one on T (the transposed top-down sums already added) and the lateral raws before the laterals; the convolution calls run
    on g := G_c with scale ones.  A convolution layer's `bn` is its FpnBnGrads (else None), `bn_index` its stages' rows of bn.qp."""
    from dd3d_amd.layers import fold_norm
    if fpn._fuse_type != "sum":
        raise NotImplementedError("FPN gradients implement FUSE_TYPE 'sum' (as the forward)")
    names, stages = list(fpn.in_features), list(fpn.stages)  # finest first
    Cf = acts[f"t{stages[0]}"][3]
    layers, common = OrderedDict(), dict(slab=slab, fill=fill, guard=guard)

    filt = lambda conv, cin: filter_copy(conv, device, cin)  # the input channels padded with zero filters up to the buffer's width
    scale_of = lambda conv: vec(fold_norm(conv, None)[0])
    hw = lambda k: (acts[k][1], acts[k][2])
    s5 = stages[-1]
    D_top = G[f"p{s5}"]
    if fpn.top_block is not None:
        tb = fpn.top_block
        D6 = G[f"p{s5 + 1}"]
        if tb.num_levels == 2:  # P7 reads relu(p6): the stored p6, rectified while staged; the same stored p6 masks its input gradient
            p6 = acts[f"p{s5 + 1}"][0]
            lay = FpnConvGrads(device, B, [hw(f"p{s5 + 1}")], Cf, Cf, 3, 2, [p6], [G[f"p{s5 + 2}"]], Cf, [filt(tb.p7, Cf)], [scale_of(tb.p7)], mask=[p6],
                               add=[D6], in_relu=True, **common)
            lay.conv = tb.p7
            layers["top_block.p7"] = lay
            D6 = lay.da[0]
        lay = FpnConvGrads(device, B, [hw(f"p{s5}")], Cf, Cf, 3, 2, [acts[f"p{s5}"][0]], [D6], Cf, [filt(tb.p6, Cf)], [scale_of(tb.p6)], add=[D_top],
                           **common)
        lay.conv = tb.p6
        layers["top_block.p6"] = lay
        D_top = lay.da[0]
    D = [G[f"p{s}"] for s in stages[:-1]] + [D_top]
    convs = [getattr(fpn, f"fpn_output{s}") for s in stages]
    stage_hw = [hw(f"t{s}") for s in stages]

    def norm_backward(rec, g):
        return FpnBnGrads(device, B, stage_hw, Cf, rec["raw"], g, Cf, rec["stats"], rec["part"], fill=fill, guard=guard)

    out_bn = norm_backward(bn["outputs"], D) if bn is not None else None
    lay = FpnConvGrads(device, B, stage_hw, Cf, Cf, 3, 1, [acts[f"t{s}"][0] for s in stages], D if out_bn is None else out_bn.gc, Cf,
                       [filt(c, Cf) for c in convs], [scale_of(c) for c in convs] if out_bn is None else [bn["outputs"]["ones"]] * len(stages),
                       pool=[None] + ["prev"] * (len(stages) - 1), **common)
    lay.conv, lay.bn, lay.bn_index = convs, out_bn, list(range(len(stages)))
    layers["outputs"] = lay
    T = lay.da
    lat_bn = norm_backward(bn["laterals"], T) if bn is not None else None
    if lat_bn is not None:
        T = lat_bn.gc
    backbone = OrderedDict()
    for idx in reversed(range(len(stages))):
        n, conv = names[idx], getattr(fpn, f"fpn_lateral{stages[idx]}")
        cin = acts[n][3]
        lay = FpnConvGrads(device, B, [hw(n)], cin, Cf, 1, 1, [acts[n][0]], [T[idx]], Cf, [filt(conv, cin)],
                           [scale_of(conv) if lat_bn is None else bn["laterals"]["ones"]], **common)
        lay.conv, lay.bn, lay.bn_index = conv, lat_bn, [idx]
        layers[f"lateral{stages[idx]}"] = lay
        backbone[n] = (lay.da[0], int(conv.weight.shape[1]))
    return layers, backbone


def fpn_param_grads(named, layers):
    """{parameter name: gradient of the parameter's shape} from the layers of `fpn_backward`; `named`: {id(parameter): name}.  The
    gradients of the buffers' pad channels are dropped."""
    params = {}
    for lay in layers.values():
        convs = lay.conv if isinstance(lay.conv, list) else [lay.conv]
        bn = getattr(lay, "bn", None)
        for l, conv in enumerate(convs):
            if bn is None:
                params.update(conv_param_grads(named, lay, conv, getattr(conv, "norm", None), lay.dw[l], lay.keep[2][l], lay.q[l], lay.r[l]))
                continue
            # batch statistics: d gamma = p, d beta = q of the norm's backward; the GEMM call's own q / r are by-products (q: the sum of G_c,
            # a conv bias' gradient -- zero up to rounding, the norm removes the mean)
            params.update(conv_param_grads(named, lay, conv, None, lay.dw[l], lay.keep[2][l], lay.q[l], lay.r[l]))
            qp = bn.qp[lay.bn_index[l]]
            for p, v in ((conv.norm.weight, qp[1]), (conv.norm.bias, qp[0])):
                if id(p) in named:
                    params[named[id(p)]] = v.clone()
    return params


def assemble_tower_grads(model, layers, feature_grads):
    """TowerLayerGrads of every (tower, layer) -> ({feature<l>: NCHW}, {parameter name: gradient}); parameters shared by several
    levels get the sum over them, in level order."""
    names = {id(p): k for k, p in model.named_parameters()}
    feats = {f"feature{l}": d.permute(0, 3, 1, 2).clone() for l, d in enumerate(feature_grads)}
    params = {}

    def add(p, v):
        if id(p) in names:
            params[names[id(p)]] = v if names[id(p)] not in params else params[names[id(p)]] + v

    for lay in layers.values():
        conv = lay.conv
        add(conv.weight, lay.dw.view(lay.Cout, 3, 3, lay.Cin).permute(0, 3, 1, 2).contiguous())
        for l in range(lay.L):
            norm = lay.norms[l]
            bn = getattr(lay, "bn", None)
            if bn is not None:  # batch statistics: d gamma = p, d beta = q of the norm's backward; the GEMM call's own q / r are by-products
                add(norm.weight, bn.qp[l, 1].clone()), add(norm.bias, bn.qp[l, 0].clone())
                if conv.bias is not None:
                    add(conv.bias, lay.q[l].clone())  # (the sum of G_c: zero up to rounding, the norm removes the mean)
                continue
            got = norm_param_grads(conv, norm, lay.keep[2][l], lay.q[l], lay.r[l])
            if "norm.weight" in got:
                add(norm.weight, got["norm.weight"]), add(norm.bias, got["norm.bias"])
            if "bias" in got:
                add(conv.bias, got["bias"])
    return feats, params


class BackwardStages:
    """The backward chain behind a loss plan's own backward call, shared by LossPlan and DenseDepthLossPlan (dense_depth_loss.py): the
    flags with their implications and early refusals, the stage builders from the predictor groups down to the stems, and the read-outs.
    A plan mixes this in beside its forward plan; what it must provide: `tower_info`, `tower_out`, `pred_info`, `tower_bn` / `bn_part` as
    ForwardPlan._heads records them, `_pred_group_table` (what the predictor groups bind), and `grads` handled by its own loss backward."""
    def _chain_flags(self, model, B, Hp, Wp, grads=False, pred_grads=False, tower_grads=False, fpn_grads=False, backbone_grads=False,
                     stem_grads=False, vovnet_grads=False, batch_stats=False, vovnet_stem_grads=False, fpn_batch_stats=False,
                     backbone_batch_stats=False):
        """The flags of the chain, each implying the shallower ones, and what they refuse before anything is built or launched."""
        self.batch_stats = bool(batch_stats)
        self.with_fpn_batch_stats = bool(fpn_batch_stats)  # (`fpn_batch_stats` itself is the read-out method; read by the trunk: _fpn)
        self.with_backbone_batch_stats = covered = bool(backbone_batch_stats)  # (likewise; read by the trunk: _dla)
        if covered:  # before anything is built or launched
            check_backbone_batch_stats(model, B, Hp, Wp, stem_grads=bool(stem_grads))
        if self.batch_stats and not self.with_fpn_batch_stats:
            check_batch_stats(model, B, Hp, Wp, backbone_covered=covered)
        if self.with_fpn_batch_stats:
            check_fpn_batch_stats(model, B, Hp, Wp, backbone_covered=covered)
            if self.batch_stats:  # (FE.FPN.NORM = BN is what the other flag covers)
                check_batch_stats(model, B, Hp, Wp, fpn_covered=True, backbone_covered=covered)
        self.with_vovnet_stem_grads = bool(vovnet_stem_grads)  # (`vovnet_stem_grads` itself is the read-out method)
        self.with_vovnet_grads = bool(vovnet_grads) or self.with_vovnet_stem_grads  # (`vovnet_grads` itself is the read-out method)
        if self.with_vovnet_grads:  # before anything is built or launched
            check_vovnet_backward(model.backbone.bottom_up, model)
        self.with_stem_grads = bool(stem_grads)  # (read by the trunk: the stem keeps its intermediates and the normalised image)
        # (`backbone_grads`, `fpn_grads` and `tower_grads` themselves are the read-out methods)
        self.with_backbone_grads = bool(backbone_grads) or self.with_stem_grads
        if self.with_backbone_grads:  # before anything is built or launched
            check_dla_backward(model.backbone.bottom_up, model)
        if self.with_stem_grads and (int(Hp) % 2 or int(Wp) % 2):
            raise NotImplementedError(f"stem gradients need an even canvas ({Hp} x {Wp}): the stem's lowering sizes level1 as floor(H / 2), the stride-2 "
                                      "backward as ceil(H / 2); canvases padded to the FPN's size divisibility are always even")
        self.with_fpn_grads = bool(fpn_grads) or self.with_backbone_grads or self.with_vovnet_grads
        self.keep_tower_outputs = bool(tower_grads) or self.with_fpn_grads
        self.pred_grads = bool(pred_grads) or self.keep_tower_outputs
        self.grads = bool(grads) or self.pred_grads

    def _check_level_sizes(self):
        """Under batch_stats, behind the trunk: check_batch_stats predicted the level sizes; these are the plan's own."""
        if self.batch_stats:
            small = [(f.H, f.W) for f in self.features if f.B * f.H * f.W < 2]
            if small:
                raise ValueError(f"Expected more than 1 value per channel when training, got a {small[0][0]} x {small[0][1]} level with a batch of {self.B}")

    def _backward_chain(self, model):
        """The stages the flags ask for, behind the plan's loss backward, in their order."""
        if self.pred_grads:
            self._pred_grads(model)
        if self.keep_tower_outputs:
            self._tower_grads(model)
        if self.with_fpn_grads:
            self._fpn_grads(model)
        if self.with_backbone_grads:
            self._backbone_grads(model)
        if self.with_stem_grads:
            self._stem_grads(model)
        if self.with_vovnet_grads:
            self._vovnet_grads(model)
        if self.with_vovnet_stem_grads:
            self._vovnet_stem_grads(model)

    def _built_without(self, flag):
        return RuntimeError(f"this {type(self).__name__} was built without {flag}=True")

    def _pred_grads(self, model):
        """The predictor layer's backward behind the plan's loss backward, one weight-gradient and one input-gradient call per predictor
        group (= per tower) on the main stream -- still one hipGraph.  `_pred_group_table` names the towers and gives per group of
        `pred_info` its slots -- (first channel, channels, slot, Scale list, Offset list) of the per-level scalars --, the gradient buffers
        at its maps and the maps."""
        dev, L = self.device, len(self.features)
        mode = pred_act_mode(self)
        level_hw = [(f.H, f.W) for f in self.features]
        tower_names, slots, grads, maps = self._pred_group_table(model)
        self.pred_groups = {}
        for name, info in self.pred_info.items():
            n, t = info["n"], info["tower"]
            ws, w, bias = {}, [], []
            for l in range(L):
                mods = [c[l if len(c) > 1 else 0] for c in info["convs"]]
                key = tuple(id(m) for m in mods)
                if key not in ws:
                    wt = torch.cat([m.weight.detach().float() for m in mods]).permute(0, 2, 3, 1).contiguous().to(dev)
                    bt = torch.cat([m.bias.detach().float() if m.bias is not None else torch.zeros(m.out_channels, device=m.weight.device) for m in mods])
                    ws[key] = (wt, bt.contiguous().to(dev))
                w.append(ws[key][0])
                bias.append(ws[key][1])
            Cin = int(w[0].shape[-1])
            slot = torch.full((n, ), -1, dtype=torch.int32)
            for c0, cn, j, _, _ in slots[name]:
                slot[c0:c0 + cn] = j
            tv = [self.tower_out[l][t] for l in range(L)]
            act = [(v.ptr if mode == hip.PG_ACT_F32 else v.pptr) for v in tv]
            grp = PredGroupGrads(dev, self.B, level_hw, Cin, n, info["pitch"], act, mode, tv[0].pitch, tv[0].buf.plane_scale,
                                 grads[name], [m.t for m in maps[name]], w, bias, [self._vec(sc) for sc in info["scales"]],
                                 lo=None if info["lo"] is None else self._vec(info["lo"]), slot=slot.to(dev))
            grp.convs, grp.slots, grp.tower = info["convs"], slots[name], tower_names[t]
            self.pred_groups[name] = grp
            self.ops.append(CallOp(lambda lib, st, grp=grp: grp.launch(lib, st), "predictor_grads." + name,
                                   dict(kind="predictor_grads", group=name)))

    def predictor_grads(self):
        """(tower-output gradients, parameter gradients) of the last run, copies: {<tower>_tower_out<l>: (B, Cin, h_l, w_l)} and
        {name in model.named_parameters(): tensor of the parameter's shape}, float32."""
        if not self.pred_grads:
            raise self._built_without("pred_grads")
        names = self._named()
        towers, params = {}, {}
        for grp in self.pred_groups.values():
            for l in range(grp.L):
                towers[f"{grp.tower}_tower_out{l}"] = grp.da[l].permute(0, 3, 1, 2).clone()
            c0 = 0
            for conv in grp.convs:
                oc = conv[0].out_channels
                # a per-level module owns its level's row; a shared one the sum over the rows written (one row when the whole group is shared)
                for m, rows in (zip(conv, [[l] for l in range(grp.L)]) if len(conv) > 1 else [(conv[0], grp.owners)]):
                    dw, db = grp.dw[rows[0], c0:c0 + oc].clone(), grp.db[rows[0], c0:c0 + oc].clone()
                    for l in rows[1:]:
                        dw, db = dw + grp.dw[l, c0:c0 + oc], db + grp.db[l, c0:c0 + oc]
                    params[names[id(m.weight)]] = dw.view(oc, 3, 3, grp.Cin).permute(0, 3, 1, 2).contiguous()
                    if m.bias is not None:
                        params[names[id(m.bias)]] = db
                c0 += oc
            for _, _, j, scales, offsets in grp.slots:
                for l in range(grp.L):
                    params[names[id(scales[l].scale)]] = grp.dscale[l, j:j + 1].clone()
                    if offsets is not None:
                        params[names[id(offsets[l].bias)]] = grp.doffset[l, j:j + 1].clone()
        return towers, params

    def _tower_grads(self, model):
        """The towers' backward behind the predictor groups: one weight-gradient and one input-gradient call per (tower, layer), last
        layer first, on the main stream -- still one hipGraph.  Layer i reads layer i + 1's input gradient (the last layer the predictor
        group's); the first layers of the towers add up, in tower order, to the gradient at the FPN outputs.  One slab of weight-gradient
        partials serves every call: they run in stream order."""
        dev, L = self.device, len(self.features)
        level_hw = [(f.H, f.W) for f in self.features]
        group_of = {grp.tower: grp for grp in self.pred_groups.values()}
        towers = []
        for (tname, i) in self.tower_info:
            if tname not in towers:
                towers.append(tname)
        depth = {t: 1 + max(i for (tn, i) in self.tower_info if tn == t) for t in towers}
        if set(group_of) - set(towers):
            raise NotImplementedError(f"tower gradients need at least one layer in every tower (none in {sorted(set(group_of) - set(towers))})")
        shapes = {(int(v["conv"].weight.shape[1]), int(v["conv"].weight.shape[0])) for v in self.tower_info.values()}
        n_slices = max(hip.tower_grad_slices(self.B, level_hw, ci, co) for ci, co in shapes)
        words = max(ci * co for ci, co in shapes) * 9
        cmax = max(co for _, co in shapes)
        alloc = torch.empty if self.dry_run else torch.zeros  # (a dry-run plan never touches the slab)
        self.tower_slab = (alloc(n_slices * words, dtype=torch.float32, device=dev), alloc(n_slices * cmax, dtype=torch.float32, device=dev))
        self.tower_layers = {}
        feature_da = None
        # Batch-statistics layers: the norm's backward (dd3d_bn_backward_reduce / _apply) turns the gradient at y into the dense
        # gradient G_c at the raw convolution output; the two GEMMs then run on g := G_c with scale ones and, as the stored output
        # whose sign masks g, a plan-owned f32 tensor of ones per level (shared by all layers): the mask passes everything.
        self.tower_ones = None
        if self.tower_bn:
            cmax = max(int(v["conv"].weight.shape[0]) for v in self.tower_bn.values())
            self.tower_ones = [torch.ones((self.B, h, w_, cmax), dtype=torch.float32, device=dev) for h, w_ in level_hw]
            raws = [v for (tname, i), info in self.tower_info.items() if info["raw"] is not None for v in info["raw"]]
            self.tower_bn_reads = self._check_reads("tower norm", list({id(v.buf): v.buf.view() for v in raws}.values()))
        for tname in towers:
            g, g_pitch = group_of[tname].da, group_of[tname].Cin
            for i in reversed(range(depth[tname])):
                info = self.tower_info[(tname, i)]
                conv = info["conv"]
                Cout, Cin = int(conv.weight.shape[0]), int(conv.weight.shape[1])
                y_bind, bn = [act_binding(self, v) for v in info["y"]], None
                if info["raw"] is not None:
                    rec = self.tower_bn[(tname, i)]
                    bn = TowerBnGrads(dev, self.B, level_hw, Cout, [(v.ptr, v.pitch) for v in info["raw"]], y_bind, g, g_pitch,
                                      [rec["stats"][s] for s in rec["segs"]], self.bn_part)
                    self.ops.append(CallOp(lambda lib, st, bn=bn: bn.launch(lib, st), f"tower_bn_grads.{tname}.{i}",
                                           dict(kind="tower_bn_grads", tower=tname, layer=i)))
                    g, g_pitch = bn.gc, Cout
                    y_bind = [(hip.PG_ACT_F32, t.data_ptr(), int(t.shape[-1]), 1.0) for t in self.tower_ones]
                lay = TowerLayerGrads(dev, self.B, level_hw, Cin, Cout, [act_binding(self, v) for v in info["x"]],
                                      y_bind, g, g_pitch, filter_copy(conv, dev), info["scales"],
                                      da_add=feature_da if i == 0 else None, slab=self.tower_slab)
                lay.conv, lay.norms, lay.tower, lay.index, lay.bn = conv, info["norms"], tname, i, bn
                self.tower_layers[(tname, i)] = lay
                self.ops.append(CallOp(lambda lib, st, lay=lay: lay.launch(lib, st), f"tower_grads.{tname}.{i}",
                                       dict(kind="tower_grads", tower=tname, layer=i)))
                g, g_pitch = lay.da, Cin
            feature_da = g
        self.feature_grads = feature_da

    def _grow_slab(self, rows, qrows, budget=True):
        """Make the plan's slab of weight-gradient partials hold `rows` / `qrows` words for the stage about to be built, and re-point
        every layer built so far that has partials at the larger one (their calls take a prefix of it).  `budget`: assert the whole
        slab, whoever sizes it, against DD3D_TG_SLAB_BYTES."""
        dev = self.device
        part, qpart = self.tower_slab
        if budget:
            # a call's slices stay within DD3D_TG_SLAB_BYTES; the towers' rule rounds up once per pyramid level
            # (dd3d_tower_grad_slices: "+ at most one row per level"), so their prefix may pass it by that many tower slices
            slack = 4 * len(self.features) * max(lay.Cout * 9 * lay.Cin for lay in self.tower_layers.values())
            assert 4 * rows <= hip.TG_SLAB_BYTES and 4 * max(rows, part.numel()) <= hip.TG_SLAB_BYTES + slack, \
                f"the backward's slab ({4 * max(rows, part.numel())} bytes) exceeds DD3D_TG_SLAB_BYTES"
        if part.numel() < rows or qpart.numel() < qrows:
            alloc = torch.empty if self.dry_run else torch.zeros
            part = alloc(max(rows, part.numel()), dtype=torch.float32, device=dev)
            qpart = alloc(max(qrows, qpart.numel()), dtype=torch.float32, device=dev)
            for lay in list(self.tower_layers.values()) + [l for l in getattr(self, "fpn_layers", {}).values() if l.with_wgrad]:
                lay.part, lay.qpart = part, qpart
                lay.args.part, lay.args.qpart = part.data_ptr(), qpart.data_ptr()
            self.tower_slab = (part, qpart)

    def _append_calls(self, kind, layers):
        """One CallOp per layer of a backward stage, in the layers' order, on the main stream."""
        for key, lay in layers.items():
            self.ops.append(CallOp(lambda lib, st, lay=lay: lay.launch(lib, st), f"{kind}.{key}", dict(kind=kind, layer=key)))

    def _check_reads(self, what, views, layers=None):
        """Every stored tensor a backward stage reads must still hold the forward's values when the backward runs.  PlanBase.buf gives
        every NAMED buffer a storage of its own for the life of the plan (there is no recycling allocator), so a tensor is intact as long
        as its name still maps to the buffer the view was taken from and no two of them share storage.  `views`: the views read; with
        `layers`, {key: view}, of which the stage reads what its layers' `src` name, in the order of first use.  Returns the buffers'
        names."""
        if layers is not None:
            used = []
            for lay in layers.values():
                for ref in lay.src.values():
                    if ref is not None and ref[0] not in used:
                        used.append(ref[0])
            views = [views[k] for k in used]
        for v in views:
            assert self.bufs.get(v.buf.name) is v.buf, f"the buffer {v.buf.name!r} the {what} backward reads was replaced"
        if not self.dry_run:
            addrs = [(v.pptr or v.ptr) for v in views]
            assert len(set(addrs)) == len(addrs) and all(addrs), f"two tensors the {what} backward reads share storage"
        return [v.buf.name for v in views]

    def _feature_grad_inputs(self):
        """{backbone feature name: the gradient the FPN sends it}, for a bottom-up network whose features have no pad channels."""
        G = {}
        for n, (d, c) in self.backbone_feature_grads.items():
            assert c == d.shape[-1], (n, c, tuple(d.shape))
            G[n] = d
        return G

    def _named(self):
        """{id(parameter): its name in model.named_parameters()}: the read-outs file every gradient under its parameter's name."""
        return {id(p): k for k, p in self.model.named_parameters()}

    def _fpn_grads(self, model):
        """The FPN's backward behind the towers' (include/dd3d_hip.h states it; `fpn_backward` lays out the calls): the top block (P7,
        then P6) down to D of the coarsest stage, the output convolutions, then the laterals -- on the main stream, still one hipGraph.
        Every call shares one slab of weight-gradient partials with the towers', sized for the largest user."""
        dev, B = self.device, self.B
        fpn = model.backbone
        names, stages = list(fpn.in_features), list(fpn.stages)  # finest first
        view = lambda n: self.bufs[n].view()
        selected = list(getattr(model, "in_features", None) or fpn._out_features)
        Cf = view(f"p{stages[0]}").C
        reads = [(n, self.bottom_up[n]) for n in names] + [(f"t{s}", view(f"fpn_lateral{s}")) for s in stages]
        if fpn.top_block is not None:
            reads += [(f"p{stages[-1] + i}", view(f"p{stages[-1] + i}")) for i in range(fpn.top_block.num_levels)]
        acts = {k: (act_binding(self, v), v.H, v.W, v.C) for k, v in reads}
        G = {}  # the gradient at every FPN output: the towers', or zeros for an output the heads do not read
        for name in fpn._out_features:
            v = view(name)
            G[name] = self.feature_grads[selected.index(name)] if name in selected else torch.zeros((B, v.H, v.W, Cf), dtype=torch.float32, device=dev)
            assert tuple(G[name].shape) == (B, v.H, v.W, Cf)
        self._grow_slab(*fpn_slab_words(B, fpn, acts), budget=False)
        bn = None
        if self.with_fpn_batch_stats:  # the norms' backward reads every stage's stored raw convolution outputs and statistics
            bn = {k: dict(raw=[(v.ptr, v.pitch) for v in rec["raw"]], stats=list(rec["stats"]), part=self.fpn_bn_part, ones=rec["ones"])
                  for k, rec in self.fpn_bn.items()}
            self.fpn_bn_reads = self._check_reads("FPN norm", [v for rec in self.fpn_bn.values() for v in rec["raw"]])
        self.fpn_layers, self.backbone_feature_grads = fpn_backward(dev, B, fpn, G, acts, self._vec, slab=self.tower_slab, bn=bn)
        if bn is None:
            self._append_calls("fpn_grads", self.fpn_layers)
        else:  # each norm's call in front of the first convolution call that reads its G_c
            self.fpn_bn_layers = OrderedDict()
            for key, lay in self.fpn_layers.items():
                norm = getattr(lay, "bn", None)
                if norm is not None and all(norm is not b for b in self.fpn_bn_layers.values()):
                    name = "outputs" if key == "outputs" else "laterals"
                    self.fpn_bn_layers[name] = norm
                    self.ops.append(CallOp(lambda lib, st, b=norm: b.launch(lib, st), f"fpn_bn_grads.{name}", dict(kind="fpn_bn_grads", layer=name)))
                self._append_calls("fpn_grads", {key: lay})
        self.fpn_reads, self.fpn_pinned = self._check_reads("FPN", [v for _, v in reads]), []  # (nothing needs pinning beyond the check)

    def fpn_grads(self):
        """(backbone-feature gradients, FPN parameter gradients) of the last run, copies: {backbone_<name>: (B, C_name, h, w)} and {name in
        model.named_parameters(): tensor of the parameter's shape}, float32; the gradients of the buffers' pad channels are dropped."""
        if not self.with_fpn_grads:
            raise self._built_without("fpn_grads")
        feats = {f"backbone_{n}": d[..., :c].permute(0, 3, 1, 2).clone() for n, (d, c) in self.backbone_feature_grads.items()}
        return feats, fpn_param_grads(self._named(), self.fpn_layers)

    def _backbone_grads(self, model):
        """The DLA-34 backbone's backward behind the FPN's (include/dd3d_hip.h states it; `dla_backward` lays out the calls): level5 down
        to level2, one weight-gradient and one input-gradient call per convolution and one launch per 2x2 max-pool, on the main stream --
        still one hipGraph.  The chain ends at the gradient of the tensor level2 reads; LossPlan(stem_grads=True) goes on from
        there (_stem_grads).  Every call shares the one slab of weight-gradient partials, sized for its largest user."""
        dev, B = self.device, self.B
        dla = model.backbone.bottom_up
        l1 = self.bufs[f"level1.{len(dla.level1) - 1}"].view()  # the stem's output, fused or launch by launch
        views = {"level1": l1}
        for name, b in self.bufs.items():
            if name.split(".")[0] in ("level2", "level3", "level4", "level5") and name.rsplit(".", 1)[-1] in ("cat", "mid", "bottom", "out"):
                views[name] = b.view()
        acts = {k: (act_binding(self, v), v.H, v.W, v.C) for k, v in views.items()}
        G = self._feature_grad_inputs()
        self._grow_slab(*dla_slab_words(B, dla, l1.H, l1.W))
        bn = None
        if self.with_backbone_batch_stats:  # the norms' backward reads every layer's stored raw convolution output and statistics
            self.backbone_bn_ones = {c: self._vec(torch.ones(c)) for c in sorted({int(c) for c in dla.channels})}
            bn = dict(layers={k: dict(raw=(rec["raw"].ptr, rec["raw"].pitch), stats=rec["stats"]) for k, rec in self.backbone_bn.items()},
                      part=self.backbone_bn_part, ones=self.backbone_bn_ones)
            self.backbone_bn_reads = self._check_reads("backbone norm", [rec["raw"] for rec in self.backbone_bn.values()])
        self.backbone_layers, self.level1_grad = dla_backward(dev, B, dla, G, acts, self._vec, slab=self.tower_slab, bn=bn)
        self._append_norm_and_conv_calls("backbone", self.backbone_layers)
        self.backbone_reads = self._check_reads("backbone", views, self.backbone_layers)

    def _append_norm_and_conv_calls(self, stage, layers):
        """_append_calls, with each layer's norm backward (backbone_batch_stats: `lay.bn`) in front of the call that reads its G_c."""
        for key, lay in layers.items():
            norm_call = getattr(lay, "bn", None)
            if norm_call is not None:
                self.ops.append(CallOp(lambda lib, st, b=norm_call: b.launch(lib, st), f"{stage}_bn_grads.{key}", dict(kind=f"{stage}_bn_grads", layer=key)))
            self._append_calls(f"{stage}_grads", {key: lay})

    def backbone_grads(self):
        """(the gradient at the stem's stored output, backbone parameter gradients) of the last run, copies: {backbone_level1: (B, C1,
        Hp / 2, Wp / 2)} -- not yet masked by that tensor's own ReLU -- and {name in model.named_parameters(): tensor of the parameter's
        shape} for every parameter of backbone.bottom_up.level2 .. level5, float32."""
        if not self.with_backbone_grads:
            raise self._built_without("backbone_grads")
        return {"backbone_level1": self.level1_grad.permute(0, 3, 1, 2).clone()}, dla_param_grads(self._named(), self.backbone_layers)

    def _stem_grads(self, model):
        """The stem's backward behind the backbone's (csrc/stem_grads.hip; include/dd3d_hip.h states it): level1.0 and level0.0 (weight
        and input gradient), then base_layer (weight gradient; the image has none), on the main stream -- still one hipGraph.  The calls
        read the f32 tensors `img4`, `base` and `level0.0` -- the launch-by-launch stem's own buffers, or what the fused stem's KEEP launch
        and the preprocess launch store for them -- and take the three ReLU masks from `base`, `level0.0` and the stored `level1.0`.  The
        calls share the plan's slab of weight-gradient partials; it never grows for them (a stem slice is at most 32 x 196 words)."""
        from dd3d_amd.layers import fold_norm
        dev, B = self.device, self.B
        dla = model.backbone.bottom_up
        convs = [("base_layer", dla.base_layer, "img4", "base"), ("level0.0", dla.level0[0], "base", "level0.0"), ("level1.0", dla.level1[0], "level0.0", "level1.0")]
        assert len(dla.level0) == 1 and len(dla.level1) == 1, "the stem's backward covers one level0 and one level1 convolution (every DLA)"
        part, qpart = self.tower_slab
        self.stem_layers = OrderedDict()
        g = self.level1_grad
        bbn, ones_y = self.with_backbone_batch_stats, None
        if bbn:  # the convolution calls run on G_c: as the stored output whose sign masks it, a plan-owned f32 tensor of ones (the towers' way)
            self.stem_ones = torch.ones(max(self.bufs[y].t.numel() for _, _, _, y in convs), dtype=torch.float32, device=dev)
            ones_y = lambda c: (hip.PG_ACT_F32, self.stem_ones.data_ptr(), int(c), 1.0)
        for key, conv, xname, yname in reversed(convs):
            xb, yv = self.bufs[xname], self.bufs[yname].view()
            cout, cin, k = int(conv.weight.shape[0]), int(xb.pitch), int(conv.weight.shape[-1])
            assert (k, int(conv.stride), cin, cout) in hip.STEM_GRAD_SHAPES and xb.has_f32 and xb.t is not None, (key, k, conv.stride, cin, cout)
            w = filter_copy(conv, dev, cin)  # (the image's fourth channel: a zero filter)
            n = hip.stem_grad_slices(B, xb.H, xb.W, cin, cout, k, int(conv.stride))
            assert n * cout * k * k * cin <= part.numel() and n * cout <= qpart.numel(), \
                f"stem_grads.{key}: {n} slices of {cout} x {k * k * cin} words do not fit the plan's slab of {part.numel()} words"
            norm_call, yb, scale = None, act_binding(self, yv), None
            if bbn:
                rec = self.backbone_bn[key]
                norm_call = BackboneBnGrads(dev, B, (yv.H, yv.W), cout, (rec["raw"].ptr, rec["raw"].pitch), yb, g, rec["stats"], self.backbone_bn_part)
                g, yb, scale = norm_call.gc[0], ones_y(cout), self.backbone_bn_ones[cout]
            lay = StemConvGrads(dev, B, xb.H, xb.W, cin, cout, k, int(conv.stride), xb.t, yb, g, w,
                                self._vec(fold_norm(conv, None)[0]) if scale is None else scale, slab=self.tower_slab, dgrad=key != "base_layer")
            lay.bn = norm_call
            lay.conv, lay.norm, lay.src = conv, getattr(conv, "norm", None), dict(x=(xname, 0, cin), y=(yname, 0, cout))
            self.stem_layers[key] = lay
            g = lay.da
        self._append_norm_and_conv_calls("stem", self.stem_layers)
        self.stem_reads = self._check_reads("stem", [self.bufs[n].view() for n in ("img4", "base", "level0.0", "level1.0")])

    def stem_grads(self):
        """(the gradients at level0's and base_layer's outputs, the stem's parameter gradients) of the last run, copies:
        {backbone_level0, backbone_base_layer: (B, 16, Hp, Wp)} -- neither masked by its tensor's own ReLU yet -- and {name in
        model.named_parameters(): tensor of the parameter's shape} for backbone.bottom_up.base_layer / level0.0 / level1.0, float32."""
        if not self.with_stem_grads:
            raise self._built_without("stem_grads")
        tens = {"backbone_level0": self.stem_layers["level1.0"].da.permute(0, 3, 1, 2).clone(),
                "backbone_base_layer": self.stem_layers["level0.0"].da.permute(0, 3, 1, 2).clone()}
        return tens, dla_param_grads(self._named(), self.stem_layers)

    def _vovnet_grads(self, model):
        """The VoVNet-V2 backbone's backward behind the FPN's (include/dd3d_hip.h states it; `vovnet_backward` lays out the calls): stage5
        down to stage2, then stem_3 and stem_2 -- per OSA module one eSE call (four launches), one weight-gradient and one input-gradient
        call per convolution, one elementwise sum under `identity`, one launch per 3x3 max-pool -- on the main stream, still one hipGraph.  The chain ends at the gradient of
        stem_1's stored output; LossPlan(vovnet_stem_grads=True) goes on from there (_vovnet_stem_grads).  Every call shares the one slab
        of weight-gradient partials, sized for its largest user."""
        dev, B = self.device, self.B
        vov = model.backbone.bottom_up
        if not self.use_planes:
            raise NotImplementedError("vovnet_grads follows the split-plane data flow; DD3D_PLANES=0 and the f32 arithmetic have no tested backward")
        pred_act_mode(self)  # (names the reduced modes, which have no loader)
        views = {}
        for name, b in self.bufs.items():
            if name in ("stem.0", "stem.1") or (name.split(".")[0] in vov.stage_names and name.rsplit(".", 1)[-1] in ("cat", "xt", "out")):
                views[name] = b.view()
        acts = {k: (act_binding(self, v), v.H, v.W, v.C) for k, v in views.items()}
        G = self._feature_grad_inputs()
        if vov.stage_names[-1] not in G:
            raise NotImplementedError(f"vovnet_grads needs the FPN to read {vov.stage_names[-1]} (FE.FPN.IN_FEATURES = {list(model.backbone.in_features)})")
        s0 = views["stem.0"]
        self._grow_slab(*vovnet_slab_words(B, vov, s0.H, s0.W))
        self.vovnet_layers, self.stem1_grad = vovnet_backward(dev, B, vov, G, acts, self._vec, slab=self.tower_slab)
        self._append_calls("vovnet_grads", self.vovnet_layers)
        self.vovnet_reads = self._check_reads("VoVNet", views, self.vovnet_layers)

    def vovnet_grads(self):
        """(the gradient at stem_1's stored output, VoVNet parameter gradients) of the last run, copies: {backbone_stem_1: (B, 64, Hp / 2,
        Wp / 2)} -- not yet masked by that tensor's own ReLU -- and {name in model.named_parameters(): tensor of the parameter's shape} for
        every parameter of backbone.bottom_up but stem.stem_1/* (those: vovnet_stem_grads), float32."""
        if not self.with_vovnet_grads:
            raise self._built_without("vovnet_grads")
        return {"backbone_stem_1": self.stem1_grad.permute(0, 3, 1, 2).clone()}, vovnet_param_grads(self._named(), self.vovnet_layers)

    def _vovnet_stem_grads(self, model):
        """stem_1's backward behind stem_2's (dd3d_vovnet_stem_wgrad, csrc/stem_grads.hip; include/dd3d_hip.h states it): ONE
        weight-gradient call on the main stream -- still one hipGraph; the image has no gradient.  It reads the f32 normalised image
        `img4` (pitch 4, fourth channel zero), takes the ReLU mask from the stored `stem.0` and the incoming gradient from stem_2's input
        gradient.  The call shares the plan's slab of weight-gradient partials; it never grows for it (a slice is 64 x 36 words)."""
        from dd3d_amd.layers import fold_norm
        dev, B = self.device, self.B
        vov = model.backbone.bottom_up
        cname, nname, _ = vov.stem_seqs[0]
        conv, norm = getattr(vov.stem, cname), getattr(vov.stem, nname)
        xb, yv = self.bufs["img4"], self.bufs["stem.0"].view()
        k, stride, cin, cout = hip.VOVNET_STEM_GRAD_SHAPE
        shape = (int(conv.weight.shape[-1]), int(conv.stride), int(xb.pitch), int(conv.weight.shape[0]))
        assert shape == (k, stride, cin, cout) and xb.has_f32 and xb.t is not None and yv.C == cout, (cname, shape)
        part, qpart = self.tower_slab
        n = hip.vovnet_stem_grad_slices(B, xb.H, xb.W)
        assert n * cout * k * k * cin <= part.numel() and n * cout <= qpart.numel(), \
            f"vovnet_stem_grads.stem_1: {n} slices of {cout} x {k * k * cin} words do not fit the plan's slab of {part.numel()} words"
        w = filter_copy(conv, dev, cin)  # (the image's fourth channel: a zero filter)
        lay = VovnetStemGrads(dev, B, xb.H, xb.W, xb.t, act_binding(self, yv), self.stem1_grad, w, self._vec(fold_norm(conv, norm)[0]), slab=self.tower_slab)
        lay.conv, lay.norm, lay.src = conv, norm, dict(x=("img4", 0, cin), y=("stem.0", 0, cout))
        self.vovnet_stem_layers = OrderedDict(stem_1=lay)
        self._append_calls("vovnet_stem_grads", self.vovnet_stem_layers)
        self.vovnet_stem_reads = self._check_reads("VoVNet stem", [xb.view(), yv])

    def vovnet_stem_grads(self):
        """(nothing, stem_1's parameter gradients) of the last run, copies: {} -- the image has no gradient -- and {name in
        model.named_parameters(): tensor of the parameter's shape} for backbone.bottom_up.stem.stem_1/conv.weight ((64, 3, 3, 3): the pad
        channel's column is dropped) and, for a BN backbone on running statistics, stem.stem_1/norm.weight and .bias; FrozenBN owns
        nothing.  With vovnet_grads' these are the parameters of named_parameters()."""
        if not self.with_vovnet_stem_grads:
            raise self._built_without("vovnet_stem_grads")
        lay = self.vovnet_stem_layers["stem_1"]
        return {}, conv_param_grads(self._named(), lay, lay.conv, lay.norm, lay.dw, lay.scale, lay.q, lay.r)

    def tower_grads(self):
        """(FPN-output gradients, tower parameter gradients) of the last run, copies: {feature<l>: (B, C, h_l, w_l)} and {name in
        model.named_parameters(): tensor of the parameter's shape}, float32.  A filter's gradient is the kernels' dw; the few per-channel
        products of a norm's weight (rstd * (r + (b_conv - mean) * q)) and the sums of q over the levels are torch ops here."""
        if not self.keep_tower_outputs:
            raise self._built_without("tower_grads")
        return assemble_tower_grads(self.model, self.tower_layers, self.feature_grads)

    def tower_batch_stats(self):
        """The batch statistics of the last run, copies keyed by the state-dict names of the towers' norms: under
        `<tower>.<i>.norm.<l>.running_mean` / `.running_var` the values the reference's train() step leaves in those buffers
        ((1 - 0.1) * running + 0.1 * batch, the variance unbiased by N / (N - 1)), under `.batch_mean` / `.batch_var` the batch's mean
        and biased variance.  The model's own buffers are never written."""
        if not self.batch_stats:
            raise self._built_without("batch_stats")
        names = {id(b): k for k, b in self.model.named_buffers()}
        out = {}
        for rec in self.tower_bn.values():
            for l, norm in enumerate(rec["norms"]):
                st = rec["stats"][rec["segs"][l]]
                mean_name, var_name = names[id(norm.running_mean)], names[id(norm.running_var)]
                out[mean_name], out[var_name] = st[hip.BN_ROW_RUN_MEAN].clone(), st[hip.BN_ROW_RUN_VAR].clone()
                stem = mean_name[:-len("running_mean")]
                out[stem + "batch_mean"], out[stem + "batch_var"] = st[hip.BN_ROW_MU].clone(), st[hip.BN_ROW_VAR].clone()
        return out


    def fpn_batch_stats(self):
        """The FPN norms' batch statistics of the last run, copies keyed by the state-dict names of `backbone.fpn_lateral<s>.norm` and
        `backbone.fpn_output<s>.norm`: `.running_mean` / `.running_var` as one training step would leave them, `.batch_mean` /
        `.batch_var` the batch's mean and biased variance (tower_batch_stats' conventions).  The model's own buffers are never written."""
        if not self.with_fpn_batch_stats:
            raise self._built_without("fpn_batch_stats")
        names = {id(b): k for k, b in self.model.named_buffers()}
        out = {}
        for rec in self.fpn_bn.values():
            for norm, st in zip(rec["norms"], rec["stats"]):
                mean_name, var_name = names[id(norm.running_mean)], names[id(norm.running_var)]
                out[mean_name], out[var_name] = st[hip.BN_ROW_RUN_MEAN].clone(), st[hip.BN_ROW_RUN_VAR].clone()
                stem = mean_name[:-len("running_mean")]
                out[stem + "batch_mean"], out[stem + "batch_var"] = st[hip.BN_ROW_MU].clone(), st[hip.BN_ROW_VAR].clone()
        return out


    def backbone_batch_stats(self):
        """The bottom-up network's batch statistics of the last run, copies keyed by the state-dict names of its norms
        (`backbone.bottom_up.base_layer.norm`, `.level0.0.norm`, `.level1.0.norm`, `.level<n>...tree<k>.conv<j>.norm`, `...project.norm`,
        `...root.conv.norm`): `.running_mean` / `.running_var` as one training step would leave them, `.batch_mean` / `.batch_var` the
        batch's mean and biased variance (tower_batch_stats' conventions).  The model's own buffers are never written."""
        if not self.with_backbone_batch_stats:
            raise self._built_without("backbone_batch_stats")
        names = {id(b): k for k, b in self.model.named_buffers()}
        out = {}
        for rec in self.backbone_bn.values():
            norm, st = rec["norm"], rec["stats"]
            mean_name, var_name = names[id(norm.running_mean)], names[id(norm.running_var)]
            out[mean_name], out[var_name] = st[hip.BN_ROW_RUN_MEAN].clone(), st[hip.BN_ROW_RUN_VAR].clone()
            stem = mean_name[:-len("running_mean")]
            out[stem + "batch_mean"], out[stem + "batch_var"] = st[hip.BN_ROW_MU].clone(), st[hip.BN_ROW_VAR].clone()
        return out


class LossPlan(BackwardStages, ForwardPlan):
    """Trunk and heads of the forward plan, then GT assignment, the per-target loss terms and one finalize launch; captured as one
    hipGraph by DD3D.get_loss_plan.  `det_count` (what the read-back record carries beside the status word) holds the positive count."""
    def __init__(self, model, B, Hp, Wp, device=None, max_gt=hip.LOSS_MAX_GT, dry_run=False, grads=False, pred_grads=False, tower_grads=False,
                 fpn_grads=False, backbone_grads=False, stem_grads=False, vovnet_grads=False, batch_stats=False, vovnet_stem_grads=False,
                 fpn_batch_stats=False, backbone_batch_stats=False):
        self._chain_flags(model, B, Hp, Wp, grads=grads, pred_grads=pred_grads, tower_grads=tower_grads, fpn_grads=fpn_grads,
                          backbone_grads=backbone_grads, stem_grads=stem_grads, vovnet_grads=vovnet_grads, batch_stats=batch_stats,
                          vovnet_stem_grads=vovnet_stem_grads, fpn_batch_stats=fpn_batch_stats, backbone_batch_stats=backbone_batch_stats)
        PlanBase.__init__(self, device or model.device, dry_run=dry_run)
        check_loss_config(model.cfg)
        from dd3d_amd.engine.tiling import default_tile_policy
        self.tile_policy = default_tile_policy() or getattr(model, "tile_policy", None) or "latency"  # as ForwardPlan: the forward's own tiles
        self.exchange, self.camera_sharded, self.has_bev_inputs = False, False, False
        self.adopt_weight_store(model)
        self._trunk(model, B, Hp, Wp)
        self._check_level_sizes()
        self._heads(model, self.features, keep_tower_outputs=self.keep_tower_outputs, batch_stats=self.batch_stats)
        self._losses(model, max_gt)

    def _losses(self, model, max_gt):
        cfg, dev, B = model.cfg, self.device, self.B
        feats = self.features
        L = len(feats)
        self.box3d_on, self.nusc = self.b3d_maps is not None, model_is_nusc(model)
        self.max_gt = int(max_gt)
        a = hip.LossArgs()
        level_hw = [(f.H, f.W) for f in feats]
        self.level_sizes = [h * w for h, w in level_hw]
        nloc = _fill_common(a, cfg, model, level_hw, self.strides, B, max_gt)
        off = model.feature_locations_offset
        self.locations = torch.cat([feature_locations(h, w, self.strides[l], off) for l, (h, w) in enumerate(level_hw)]).to(dev)
        for l in range(L):
            a.cls[l] = self.cls_maps[l].t.data_ptr()
            a.box2d[l] = self.b2d_maps[l].t.data_ptr()
            a.box3d[l] = self.b3d_maps[l].t.data_ptr() if self.box3d_on else None
        a.cls_pitch, a.b2d_pitch, a.b3d_pitch = self.cls_pitch, self.b2d_pitch, self.b3d_pitch
        a.attr_off, a.num_attr, a.speed_off = 0, 0, -1
        if self.nusc:  # nuScenes extras ride on the cls map (ForwardPlan._heads)
            a.attr_off, a.num_attr = model.num_classes, num_attributes(model)
            a.speed_off = model.num_classes + a.num_attr
        if self.box3d_on:
            self.canon = torch.tensor([list(r) for r in cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES], dtype=torch.float32, device=dev)
            a.canon_sizes = self.canon.data_ptr()
        a.inv_K = self.inv_K.data_ptr()  # written by the trunk's first launch (K^-1 of the images, core.py:93)
        a.locations = self.locations.data_ptr()
        # GT staging: [offsets B + 1 (int32), padded to 4 words | records B * max_gt * LOSS_GT_FIELDS], pinned mirror + device twin
        self.gt_hdr = (B + 1 + 3) // 4 * 4
        words = self.gt_hdr + B * self.max_gt * hip.LOSS_GT_FIELDS
        self.host_gt = self.host_buf(words, torch.float32)
        self.dev_gt = torch.zeros(words, dtype=torch.float32, device=dev)
        self._gt_words = self.gt_hdr
        a.gt_off, a.gt = self.dev_gt.data_ptr(), self.dev_gt.data_ptr() + 4 * self.gt_hdr
        N = B * nloc
        self.targets = _Targets(a, N, self.box3d_on, self.nusc, dev)
        nblocks = (N + hip.LOSS_BLOCK - 1) // hip.LOSS_BLOCK
        self.partials = torch.zeros((nblocks, hip.LOSS_TERMS), dtype=torch.float32, device=dev)
        self.loss_out = torch.zeros(hip.LOSS_OUT, dtype=torch.float32, device=dev)
        self.det_count = torch.zeros(1, dtype=torch.int32, device=dev)  # the positive count, in the read-back record
        a.partials, a.n_partials, a.out, a.num_pos = self.partials.data_ptr(), nblocks, self.loss_out.data_ptr(), self.det_count.data_ptr()
        self.loss_args = a
        self.ops.append(CallOp(lambda lib, st: hip.check(lib.dd3d_loss_assign(C.byref(a), st), "loss_assign"), "loss_assign",
                               dict(kind="loss_assign")))
        self.ops.append(CallOp(lambda lib, st: hip.check(lib.dd3d_loss_terms(C.byref(a), st), "loss_terms"), "loss_terms",
                               dict(kind="loss_terms")))
        if self.grads:
            self._loss_grads(a)
        self._backward_chain(model)

    def _loss_grads(self, a):
        """Gradient buffers shaped like the head maps, the upstream vector (ones: the gradient of the sum of the dict's values) and one
        more launch, dd3d_loss_backward, behind the loss terms -- still one hipGraph."""
        like = lambda maps: [torch.zeros_like(m.t) for m in maps]
        self.d_cls, self.d_b2d = like(self.cls_maps), like(self.b2d_maps)
        self.d_b3d = like(self.b3d_maps) if self.box3d_on else None
        self.upstream = torch.ones(hip.LOSS_OUT, dtype=torch.float32, device=self.device)
        self.grad_denoms = torch.zeros(hip.LOSS_GRAD_DENOMS, dtype=torch.float32, device=self.device)
        g = fill_grad_args(self.d_cls, self.d_b2d, self.d_b3d, self.upstream, self.grad_denoms)
        self.grad_args = g
        self.ops.append(CallOp(lambda lib, st: hip.check(lib.dd3d_loss_backward(C.byref(a), C.byref(g), st), "loss_backward"), "loss_backward",
                               dict(kind="loss_backward")))

    def _pred_group_table(self, model):
        """The FCOS heads' predictor groups for BackwardStages._pred_grads: (tower names by index, {group: slots}, {group: gradient buffers},
        {group: maps})."""
        h2, h3 = model.fcos2d_head, (None if model.only_box2d else model.fcos3d_head)
        C3 = (1 if h3.class_agnostic else int(model.num_classes)) if h3 is not None else 0
        # (first channel, channels, slot, Scale list, Offset list) of the per-level scalars of a group
        slots = {"cls_map": [], "box2d_map": [(0, 4, 0, h2.scales_box2d_reg, None)] if h2.use_scale else [], "box3d_map": []}
        if h3 is not None and h3.use_scale:
            slots["box3d_map"] = [(4 * C3, 2 * C3, 0, h3.scales_proj_ctr, None), (6 * C3, C3, 1, h3.scales_depth, h3.offsets_depth),
                                  (7 * C3, 3 * C3, 2, h3.scales_size, None), (10 * C3, C3, 3, h3.scales_conf, None)]
        grads = {"cls_map": self.d_cls, "box2d_map": self.d_b2d, "box3d_map": self.d_b3d}
        maps = {"cls_map": self.cls_maps, "box2d_map": self.b2d_maps, "box3d_map": self.b3d_maps}
        return ("cls", "box2d", "box3d"), slots, grads, maps

    def head_grads(self):
        """The gradients of the last run as NCHW per-level tensors (copies) under the keys of the reference's head maps."""
        if not self.grads:
            raise self._built_without("grads")
        return unpack_head_grads(self.d_cls, self.d_b2d, self.d_b3d, int(self.model.num_classes), self.loss_args.num_attr if self.nusc else 0,
                                 bool(self.loss_args.class_agnostic_3d))

    def stage_gt(self, gt_instances):
        """Pack the batch's GT into the pinned mirror (plain host stores); `flush_inputs` ships it."""
        if len(gt_instances) != self.B:
            raise ValueError(f"{len(gt_instances)} GT instances for a plan of {self.B} images")
        off, recs = pack_gt(gt_instances, self.max_gt, self.box3d_on, self.nusc, self.loss_args.num_attr, int(self.model.num_classes))
        self.inputs_writable()
        h = self.host_gt.numpy()
        h[:self.B + 1] = off.view(np.float32)
        h[self.gt_hdr:self.gt_hdr + recs.size] = recs.reshape(-1)
        self._gt_words = self.gt_hdr + recs.size

    def flush_inputs(self):
        """The GT prefix in use goes with the image metadata: one more asynchronous copy per call."""
        n = self._gt_words
        self.dev_gt[:n].copy_(self.host_gt[:n], non_blocking=not self.dry_run)
        super().flush_inputs()

    def loss_dict(self, num_pos):
        """The reference's loss dict: 0-d float32 device tensors, keys in its order (decided by the positive count)."""
        vals = self.loss_out.clone()
        return {k: vals[OUT_INDEX[k]] for k in loss_keys(self.box3d_on, self.nusc, num_pos)}

    def target_dict(self):
        """The targets of the last run, in the form of DD3D.prepare_targets (copies)."""
        d = self.targets.as_dict(self.locations, self.B, len(self.features), self.level_sizes, self.model.num_classes)
        return {k: v.clone() for k, v in d.items()}
