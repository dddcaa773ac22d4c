"""Dense-depth loss engine: the per-level training loss dict of DD3DDenseDepth on the MI355X and, on request, its gradient with respect to
the head's per-level maps and from there, stage by stage, with respect to every parameter of the network: the stages are LossPlan's
(losses.BackwardStages: predictor group, tower, FPN, DLA-34 or VoVNet-V2 with their stems), appended behind the loss backward.

``DenseDepthLossPlan`` has the trunk, tower and predictors of ``DenseDepthPlan`` and, in place of the five up-sampling launches, ONE call of
csrc/dense_depth_loss.hip: a single pass over the ground-truth canvas that evaluates every level's up-sampled prediction in place at the
valid pixels (dense_depth.py:153-171, dense_depth_loss.py:28-36).  The five full-resolution maps are never allocated.  With
``head_grads=True`` one more call follows, csrc/dense_depth_loss_grads.hip: the transposed interpolation without float atomics.
"""
import ctypes as C

import numpy as np
import torch

from dd3d_amd import hip
from dd3d_amd.engine.forward import DenseDepthPlan
from dd3d_amd.engine.losses import BackwardStages
from dd3d_amd.engine.ops import CallOp
from dd3d_amd.engine.plan import PlanBase


def dense_depth_loss_config(cfg):
    """(LOSS_WEIGHT, SMOOTH_L1_BETA, MIN_DEPTH, MAX_DEPTH) of build_dense_depth_loss (dense_depth_loss.py:19-26, :39-43).
    DD3D.FCOS3D.DEPTH_HEAD.{LOSS_TYPE, LOSS_WEIGHT} are in no released config: callers pass them as overrides; a missing one raises a
    ValueError naming it, and so does a LOSS_TYPE other than "L1" (the reference forgets the `raise` and builds None)."""
    c3 = cfg.DD3D.FCOS3D
    head = c3.get("DEPTH_HEAD") if hasattr(c3, "get") else getattr(c3, "DEPTH_HEAD", None)
    if head is None:
        raise ValueError("DD3D.FCOS3D.DEPTH_HEAD is missing from the config: the dense-depth loss needs DD3D.FCOS3D.DEPTH_HEAD.LOSS_TYPE and "
                         "DD3D.FCOS3D.DEPTH_HEAD.LOSS_WEIGHT (pass them as overrides)")
    vals = {}
    for key in ("LOSS_TYPE", "LOSS_WEIGHT"):
        try:
            vals[key] = head[key] if isinstance(head, dict) else getattr(head, key)
        except (KeyError, AttributeError):
            raise ValueError(f"DD3D.FCOS3D.DEPTH_HEAD.{key} is missing from the config (pass it as an override)") from None
    if vals["LOSS_TYPE"] != "L1":
        raise ValueError(f"Not supported depth loss: DD3D.FCOS3D.DEPTH_HEAD.LOSS_TYPE = {vals['LOSS_TYPE']!r} (only 'L1' exists)")
    return float(vals["LOSS_WEIGHT"]), float(c3.LOSS.SMOOTH_L1_BETA), float(c3.MIN_DEPTH), float(c3.MAX_DEPTH)


def level_divisors(num_levels):
    """dense_depth.py:169: np.sqrt(2) ** lvl, the power in float64, then the f32 the division by an f32 tensor sees."""
    return [float(np.float32(np.sqrt(2)**l)) for l in range(num_levels)]


def dense_depth_grad_args(loss_args, d_raw, upstream, slab):
    """A DenseDepthGradArgs over per-level NHWC gradient buffers (the layout of the raw maps), the upstream vector and the slab."""
    g = hip.DenseDepthGradArgs()
    for l, t in enumerate(d_raw):
        g.d_raw[l] = t.data_ptr()
    g.upstream, g.slab, g.n_slab = upstream.data_ptr(), slab.data_ptr(), slab.shape[0]
    assert len(d_raw) == loss_args.num_levels and slab.shape[1] == hip.DDG_ROW
    return g


def check_depth_maps(depths, image_sizes):
    """Every ground-truth map must be a floating tensor (CPU or device, any float dtype) of shape (Hi, Wi) == its image's own size;
    anything else raises a ValueError that names the image."""
    if len(depths) != len(image_sizes):
        raise ValueError(f"{len(depths)} depth maps for {len(image_sizes)} images")
    for i, (d, (hi, wi)) in enumerate(zip(depths, image_sizes)):
        if not isinstance(d, torch.Tensor) or not d.is_floating_point():
            raise ValueError(f"image {i}: 'depth' must be a floating-point tensor, got {type(d).__name__}"
                             + (f" of dtype {d.dtype}" if isinstance(d, torch.Tensor) else ""))
        if tuple(d.shape) != (int(hi), int(wi)):
            raise ValueError(f"image {i}: 'depth' has shape {tuple(d.shape)}, its image is {int(hi)} x {int(wi)}: expected ({int(hi)}, {int(wi)})")


def stage_depth_canvas(canvas, depths, image_sizes, checked=False):
    """ImageList.from_tensors of the ground-truth maps (image_list.py:94-158, pad value 0.0) into `canvas` (B, Hp, Wp) f32, on whatever
    device it lives: every image's map in its top-left corner, ZEROS everywhere else -- whatever an earlier call left there.
    `checked`: the caller has run check_depth_maps on this batch already."""
    if not checked:
        check_depth_maps(depths, image_sizes)
    if len(depths) != canvas.shape[0]:
        raise ValueError(f"{len(depths)} depth maps for a canvas of {canvas.shape[0]} images")
    for i, (hi, wi) in enumerate(image_sizes):
        if hi > canvas.shape[1] or wi > canvas.shape[2]:
            raise ValueError(f"image {i}: {int(hi)} x {int(wi)} does not fit the {canvas.shape[1]} x {canvas.shape[2]} canvas")
    canvas.zero_()
    for i, d in enumerate(depths):
        canvas[i, :d.shape[0], :d.shape[1]].copy_(d.detach(), non_blocking=True)  # (casts to f32)
    return canvas


class DenseDepthLossPlan(BackwardStages, DenseDepthPlan):
    """Trunk, box3d tower and per-level predictors of DenseDepthPlan, then one dd3d_dense_depth_loss call on the raw predictor maps and the
    ground-truth canvas; captured as one hipGraph by DD3DDenseDepth.get_loss_plan.  `head_grads`: one dd3d_dense_depth_loss_backward call
    more, in the same graph, into gradient buffers the plan owns (upstream = 1: the gradient of the sum of the dict's values).  The deeper
    flags append LossPlan's backward stages behind it (losses.BackwardStages; each implies the shallower ones and refuses what LossPlan
    refuses): `pred_grads` the one predictor group (n = 1 at pitch 4, a filter per level, Scale / Offset in slot 0), `tower_grads` the
    box3d tower, `fpn_grads` the FPN, `backbone_grads` / `stem_grads` DLA-34, `vovnet_grads` / `vovnet_stem_grads` the VoVNet-V2
    backbones; `batch_stats` normalises a trainable-BatchNorm2d tower with the batch's statistics, forward and backward, `fpn_batch_stats`
    the FPN's lateral and output norms (FE.FPN.NORM: BN), `backbone_batch_stats` DLA-34's (FE.BACKBONE.NORM: BN).  From
    `tower_grads` on every tower layer keeps its output (5 levels x NUM_CONVS buffers of 256 channels in place of the two ping / pong
    sets); every other plan launches exactly what it launched before these flags existed."""
    def __init__(self, model, B, Hp, Wp, device=None, dry_run=False, head_grads=False, pred_grads=False, tower_grads=False, fpn_grads=False,
                 backbone_grads=False, stem_grads=False, vovnet_grads=False, vovnet_stem_grads=False, batch_stats=False, fpn_batch_stats=False,
                 backbone_batch_stats=False):
        self._chain_flags(model, B, Hp, Wp, grads=head_grads, pred_grads=pred_grads, tower_grads=tower_grads, fpn_grads=fpn_grads,
                          backbone_grads=backbone_grads, stem_grads=stem_grads, vovnet_grads=vovnet_grads, batch_stats=batch_stats,
                          vovnet_stem_grads=vovnet_stem_grads, fpn_batch_stats=fpn_batch_stats, backbone_batch_stats=backbone_batch_stats)
        PlanBase.__init__(self, device or model.device, dry_run=dry_run)
        weight, beta, min_depth, max_depth = dense_depth_loss_config(model.cfg)  # (read here, not in the model's constructor)
        self.adopt_weight_store(model)
        self._trunk(model, B, Hp, Wp)
        self._check_level_sizes()
        self._dense_depth_head(model, keep_tower_outputs=self.keep_tower_outputs, batch_stats=self.batch_stats)
        dev, feats = self.device, self.features
        L = len(feats)
        if L > hip.MAX_LEVELS:
            raise ValueError(f"{L} feature levels exceed {hip.MAX_LEVELS}")
        if Wp % 4:
            raise ValueError(f"canvas width {Wp} is not a multiple of 4")
        self.gt_canvas = torch.zeros((B, Hp, Wp), dtype=torch.float32, device=dev)
        nblocks = hip.dense_depth_loss_blocks(B, Hp, Wp)
        self.partials = torch.zeros((nblocks, hip.DDL_ROW), dtype=torch.float32, device=dev)
        self.loss_out = torch.zeros(L, dtype=torch.float32, device=dev)
        self.valid_count = torch.zeros(1, dtype=torch.int64, device=dev)
        a = hip.DenseDepthLossArgs()
        for l, f in enumerate(feats):
            stride = self.strides[l]
            assert f.H * stride == Hp and f.W * stride == Wp, "pyramid level does not tile the padded input"
            a.raw[l] = self.dd_raw[l].t.data_ptr()
            a.h[l], a.w[l], a.stride[l] = f.H, f.W, stride
        for l, d in enumerate(level_divisors(L)):
            a.divisor[l] = d
        a.gt, a.inv_K = self.gt_canvas.data_ptr(), self.inv_K.data_ptr()  # K^-1: written by the trunk's first launch
        a.partials, a.n_partials = self.partials.data_ptr(), nblocks
        a.out, a.count = self.loss_out.data_ptr(), self.valid_count.data_ptr()
        a.num_levels, a.B, a.Hp, a.Wp, a.pitch = L, B, Hp, Wp, 4
        a.offset_half = int(model.feature_locations_offset == "half")
        a.focal_factor = float(model.scale_depth_by_focal_lengths_factor) if model.scale_depth_by_focal_lengths else 0.0
        a.min_depth, a.max_depth, a.beta, a.loss_weight = min_depth, max_depth, beta, weight
        self.loss_args = a
        self.ops.append(CallOp(lambda lib, st: hip.check(lib.dd3d_dense_depth_loss(C.byref(a), st), "dense_depth_loss"), "dense_depth_loss",
                               dict(kind="dense_depth_loss")))
        if self.grads:
            self._loss_grads(a)
        self._backward_chain(model)

    def _loss_grads(self, a):
        """Gradient buffers shaped like the raw maps (zeros: the kernel writes channel 0 only), the upstream vector and the slab."""
        self.d_raw = [torch.zeros_like(m.t) for m in self.dd_raw]
        self.upstream = torch.ones(a.num_levels, dtype=torch.float32, device=self.device)
        self.grad_slab = torch.zeros((hip.dense_depth_grad_rows(a), hip.DDG_ROW), dtype=torch.float32, device=self.device)
        g = dense_depth_grad_args(a, self.d_raw, self.upstream, self.grad_slab)
        self.grad_args = g
        self.ops.append(CallOp(lambda lib, st: hip.check(lib.dd3d_dense_depth_loss_backward(C.byref(a), C.byref(g), st), "dense_depth_loss_backward"),
                               "dense_depth_loss_backward", dict(kind="dense_depth_loss_backward")))

    def _pred_group_table(self, model):
        """The one predictor group for BackwardStages._pred_grads: g = d_raw, maps = dd_raw, the per-level filters of
        fcos3d_head.dense_depth; with USE_SCALE slot 0 is scales_depth / offsets_depth, else the conv bias takes the gradient."""
        head = model.fcos3d_head
        slots = [(0, 1, 0, head.scales_depth, head.offsets_depth)] if head.use_scale else []
        return ("box3d", ), {"dd_raw": slots}, {"dd_raw": self.d_raw}, {"dd_raw": self.dd_raw}

    def head_grads(self):
        """The gradients of the last run: {"dense_depth<l>": (B, 1, h_l, w_l) float32} (copies), with respect to the head's per-level
        outputs after Scale and Offset."""
        if not self.grads:
            raise RuntimeError("this DenseDepthLossPlan was built without head_grads=True")
        return {f"dense_depth{l}": d[..., 0].unsqueeze(1).clone() for l, d in enumerate(self.d_raw)}

    def stage_depth(self, depths, image_sizes, checked=False):
        """The batch's ground-truth maps into the device canvas, on the current stream (ahead of the run that reads it)."""
        stage_depth_canvas(self.gt_canvas, depths, image_sizes, checked=checked)

    def loss_dict(self):
        """The reference's dict (dense_depth.py:166-171): 0-d float32 device tensors, keys in level order."""
        vals = self.loss_out.clone()
        return {f"loss_dense_depth_lvl_{l}": vals[l] for l in range(vals.shape[0])}
