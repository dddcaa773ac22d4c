"""``DD3DDenseDepth`` meta-architecture (tridet/modeling/dd3d/dense_depth.py:17-163): the depth pre-training network -- the
``box3d_tower`` of the FCOS3D head with one 1-channel ``dense_depth`` predictor PER pyramid level, followed by the aligned
bilinear upsampling of every level to the input resolution and the focal-length scaling.

The reference's ``forward`` only defines the training branch (it ends in ``raise NotImplementedError()`` in eval mode,
dense_depth.py:162-163); everything it computes before the losses is inference math, exposed here as
``predict_dense_depth(batched_inputs)``; ``forward`` keeps the reference's eval-mode behaviour.  What the training branch adds, the
per-level loss dict (dense_depth.py:165-171), is ``compute_losses(batched_inputs)``; with ``head_grads=True`` also the gradient with
respect to the head's per-level maps, and with the deeper flags of ``DD3D.compute_losses`` (``predictor_grads`` .. ``stem_grads``,
``vovnet_grads`` / ``vovnet_stem_grads``) the gradient of every parameter, through the same backward stages as the detector's.
"""
import torch
from torch import nn

from dd3d_amd.layers import Conv2d, Offset, Scale
from dd3d_amd.modeling.dd3d import _deepest, build_feature_extractor
from dd3d_amd.modeling.heads import _init_predictor, _init_tower, _make_tower
from dd3d_amd.registry import META_ARCH_REGISTRY


class DD3DDenseDepthHead(nn.Module):
    """dense_depth.py:17-100."""
    def __init__(self, cfg, input_shape):
        super().__init__()
        c3 = cfg.DD3D.FCOS3D
        self.in_strides = [s.stride for s in input_shape]
        self.num_levels = len(input_shape)
        self.mean_depth_per_level = torch.FloatTensor(list(c3.MEAN_DEPTH_PER_LEVEL))  # plain attributes, as in the reference
        self.std_depth_per_level = torch.FloatTensor(list(c3.STD_DEPTH_PER_LEVEL))
        self.scale_depth_by_focal_lengths_factor = c3.SCALE_DEPTH_BY_FOCAL_LENGTHS_FACTOR
        self.use_scale = c3.USE_SCALE
        self.depth_scale_init_factor = c3.DEPTH_SCALE_INIT_FACTOR
        in_channels = input_shape[0].channels
        if c3.USE_DEFORMABLE:
            raise ValueError("Not supported yet.")
        self.box3d_tower = _make_tower(in_channels, c3.NUM_CONVS, c3.NORM, self.num_levels)
        # each FPN level has its own predictor layer (dense_depth.py:63-67)
        self.dense_depth = nn.ModuleList([Conv2d(in_channels, 1, 3, 1, 1, bias=not self.use_scale) for _ in range(self.num_levels)])
        if self.use_scale:
            self.scales_depth = nn.ModuleList([
                Scale(init_value=float(sigma) * self.depth_scale_init_factor) for sigma in self.std_depth_per_level
            ])
            self.offsets_depth = nn.ModuleList([Offset(init_value=float(b)) for b in self.mean_depth_per_level])
        _init_tower(self.box3d_tower)
        for m in self.dense_depth:
            _init_predictor(m)


@META_ARCH_REGISTRY.register()
class DD3DDenseDepth(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.in_features = cfg.DD3D.IN_FEATURES
        self.feature_locations_offset = cfg.DD3D.FEATURE_LOCATIONS_OFFSET
        self.backbone = build_feature_extractor(cfg)
        shapes = self.backbone.output_shape()
        self.backbone_output_shape = [shapes[f] for f in self.in_features]
        if list(self.in_features) != list(shapes.keys()):
            raise NotImplementedError("DD3D.IN_FEATURES must select every FPN output (all reference configs do)")
        self.fcos3d_head = DD3DDenseDepthHead(cfg, self.backbone_output_shape)
        self.scale_depth_by_focal_lengths = cfg.DD3D.FCOS3D.SCALE_DEPTH_BY_FOCAL_LENGTHS
        self.scale_depth_by_focal_lengths_factor = cfg.DD3D.FCOS3D.SCALE_DEPTH_BY_FOCAL_LENGTHS_FACTOR
        self.register_buffer("pixel_mean", torch.Tensor(list(cfg.MODEL.PIXEL_MEAN)).view(-1, 1, 1))
        self.register_buffer("pixel_std", torch.Tensor(list(cfg.MODEL.PIXEL_STD)).view(-1, 1, 1))
        self._plans = {}
        self.use_graph = True
        self.math = None
        self.training = False

    @property
    def device(self):
        return self.pixel_mean.device

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("dd3d_amd implements the inference math only")
        return super().train(False)

    def invalidate_plans(self):
        """Plans read packed copies of the weights (one store per model, shared by its plans): drop both."""
        self._plans = {}
        self.__dict__.pop("_weight_store", None)

    def load_state_dict(self, *a, **k):
        r = super().load_state_dict(*a, **k)
        self.invalidate_plans()
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self.invalidate_plans()
        return r

    def _cached_plan(self, key, build):
        """The plan under `key` of the bounded cache (most recently used last; bounded like DD3D.get_plan), built and captured on a miss."""
        plan = self._plans.pop(key, None)
        if plan is None:
            plan = build()
            if self.use_graph:
                plan.capture()
        self._plans[key] = plan
        while len(self._plans) > 8:
            if torch.cuda.is_available():
                torch.cuda.synchronize()
            self._plans.pop(next(iter(self._plans)))
        return plan

    def get_plan(self, B, Hp, Wp):
        from dd3d_amd.engine import DenseDepthPlan
        return self._cached_plan((B, Hp, Wp, self.math), lambda: DenseDepthPlan(self, B, Hp, Wp))

    @torch.no_grad()
    def predict_dense_depth(self, batched_inputs):
        """dense_depth.py:121-151 up to (not including) the losses: a list over pyramid levels of (B, Hp, Wp) depth maps at the
        padded input resolution, on the model's device.  The default f16x2 arithmetic is guarded exactly as in DD3D.forward: a kernel
        that met an activation outside the half range trips the plan's status word, the maps are NOT returned, and a model on the
        default arithmetic re-runs (from then on) with the three-term bf16 split."""
        from dd3d_amd.engine import relax_arithmetic
        while True:
            try:
                return self._predict_dense_depth(batched_inputs)
            except FloatingPointError as e:
                if not relax_arithmetic(self, e):  # (plane scale 16 -> 4 -> 1, then bf16x3; an explicitly chosen arithmetic raises)
                    raise

    def _stage(self, batched_inputs, get_plan):
        """Images, sizes and intrinsics of a batch into the plan `get_plan(B, Hp, Wp)` builds for its padded canvas (ImageList.from_tensors'
        geometry).  Returns (plan, image sizes)."""
        images = [x["image"] for x in batched_inputs]
        div = self.backbone.size_divisibility
        H = max(int(im.shape[-2]) for im in images)
        W = max(int(im.shape[-1]) for im in images)
        if div > 1:
            H, W = (H + div - 1) // div * div, (W + div - 1) // div * div
        B = len(images)
        plan = get_plan(B, H, W)
        for i, im in enumerate(images):
            assert im.dtype == torch.uint8 and im.shape[0] == 3
            plan.in_u8[i, :, :im.shape[1], :im.shape[2]].copy_(im, non_blocking=True)
        sizes = [[int(im.shape[-2]), int(im.shape[-1])] for im in images]
        plan.in_sizes.copy_(torch.tensor(sizes, dtype=torch.int32), non_blocking=True)
        if self.scale_depth_by_focal_lengths:
            if "intrinsics" not in batched_inputs[0]:
                raise AssertionError("SCALE_DEPTH_BY_FOCAL_LENGTHS needs 'intrinsics'")  # dense_depth.py:147
            K = torch.stack([x["intrinsics"].float().cpu() for x in batched_inputs], 0)
            if torch.allclose(K[0], torch.eye(3)):
                raise ValueError("Intrinsics is Identity.")  # image_list.py:57-62
            plan.in_K.copy_(K.reshape(B, 9), non_blocking=True)
        return plan, sizes

    def _predict_dense_depth(self, batched_inputs):
        plan, _ = self._stage(batched_inputs, self.get_plan)
        plan.run()
        plan.check_status()  # one 4-byte read behind the forward (the caller is about to consume the maps anyway); raises and clears
        return [m for m in plan.depth_maps]

    def get_loss_plan(self, B, Hp, Wp, head_grads=False, pred_grads=False, tower_grads=False, fpn_grads=False, backbone_grads=False,
                      stem_grads=False, vovnet_grads=False, vovnet_stem_grads=False, **norms):
        """The loss plan (engine.DenseDepthLossPlan) for one geometry, captured as one hipGraph; kept in the same bounded cache as the
        prediction plans, under a key of its own (another one with `head_grads`: the backward call is part of that plan's graph).  The
        deeper flags are DD3D.get_loss_plan's, each implying the shallower ones: one plan, and one cache key, per deepest requested level
        of the backward, and a further key under `batch_stats=True` (the box3d tower's trainable BatchNorm2d on the batch's statistics;
        the keyword is taken from `**norms`, any other extra keyword is a TypeError), and one more under `fpn_batch_stats=True` (the FPN's
        norms under FE.FPN.NORM: BN; taken from `**norms` too) and under `backbone_batch_stats=True` (DLA-34's norms under FE.BACKBONE.NORM: BN)."""
        from dd3d_amd.engine import DenseDepthLossPlan
        batch_stats = bool(norms.pop("batch_stats", False))
        fpn_batch_stats = bool(norms.pop("fpn_batch_stats", False))
        backbone_batch_stats = bool(norms.pop("backbone_batch_stats", False))
        if norms:
            raise TypeError(f"get_loss_plan() got an unexpected keyword argument {next(iter(norms))!r}")
        level = _deepest(vovnet_stem_grads=vovnet_stem_grads, vovnet_grads=vovnet_grads, stem_grads=stem_grads, backbone_grads=backbone_grads,
                         fpn_grads=fpn_grads, tower_grads=tower_grads, pred_grads=pred_grads, head_grads=head_grads)
        if not batch_stats and not fpn_batch_stats and not backbone_batch_stats and not set(level) - {"head_grads"}:  # the two keys from before the deeper levels existed
            return self._cached_plan(("dense_depth_loss_grads" if level else "dense_depth_loss", B, Hp, Wp, self.math),
                                     lambda: DenseDepthLossPlan(self, B, Hp, Wp, **level))
        key = ("dense_depth_loss", B, Hp, Wp, self.math) + tuple(level)
        if batch_stats:
            key, level = key + ("batch_stats", ), dict(level, batch_stats=True)
        if fpn_batch_stats:
            key, level = key + ("fpn_batch_stats", ), dict(level, fpn_batch_stats=True)
        if backbone_batch_stats:
            key, level = key + ("backbone_batch_stats", ), dict(level, backbone_batch_stats=True)
        return self._cached_plan(key, lambda: DenseDepthLossPlan(self, B, Hp, Wp, **level))

    @torch.no_grad()
    def compute_losses(self, batched_inputs, head_grads=False, predictor_grads=False, tower_grads=False, fpn_grads=False, backbone_grads=False,
                       stem_grads=False, **branch):
        """The loss dict of the reference's training forward (dense_depth.py:165-171) for a labelled batch: each item carries `image`,
        `intrinsics` and `depth`, an (Hi, Wi) float map of the image's own size (0 = no return).  Keys `loss_dense_depth_lvl_{l}` in
        level order, values 0-d float32 tensors on the model's device; NaN at every level when no pixel of the batch is valid.  Needs
        DD3D.FCOS3D.DEPTH_HEAD.{LOSS_TYPE, LOSS_WEIGHT} in the config (ValueError otherwise).  By default every norm layer uses its
        running statistics.  The f16x2 range guard acts as in predict_dense_depth.  With `head_grads` the result is (loss dict, grads): the
        gradient of the sum of the dict's values with respect to the head's per-level outputs (the reference's `dense_depth_lvl`, after
        Scale and Offset), {"dense_depth<l>": (B, 1, h_l, w_l) float32 device tensor}; all zeros when no pixel is valid.
        From `predictor_grads` on the result is (loss dict, grads, param_grads) and the backward goes on through the convolutions with the
        flags, implications, keys and shapes of DD3D.compute_losses, every deeper flag returning what the shallower one returns bit for
        bit: `predictor_grads` adds box3d_tower_out<l> to `grads` and to `param_grads` -- keyed by named_parameters() names, float32 of
        the parameter's shape -- fcos3d_head.dense_depth.<l>.weight ((1, 256, 3, 3)), with USE_SCALE fcos3d_head.scales_depth.<l>.scale
        and fcos3d_head.offsets_depth.<l>.bias, without it the predictors' .bias; `tower_grads` adds feature<l> and the parameters of
        fcos3d_head.box3d_tower; `fpn_grads` adds backbone_<name> and the FPN's parameters; `backbone_grads` and `stem_grads` (DLA-34) add
        backbone_level1, then backbone_level0 and backbone_base_layer, and the bottom-up network's parameters; `vovnet_grads` and
        `vovnet_stem_grads` (the four covered VoVNet-V2 specs; taken from `**branch`, as `batch_stats` is; any other extra keyword is a TypeError) add
        backbone_stem_1 and the VoVNet's parameters.  Under `stem_grads` / `vovnet_stem_grads` the keys of `param_grads` are those of
        named_parameters().  `batch_stats` composes with every flag: a box3d tower whose norm is a trainable BatchNorm2d
        (DD3D.FCOS3D.NORM: BN) normalises with the batch's statistics per layer, level and channel, and the backward differentiates
        through them; `get_loss_plan(..., batch_stats=True).tower_batch_stats()` returns them; the model's buffers are never written.
        `fpn_batch_stats` (taken from `**branch` as well; composes with every flag) does the same for the FPN's lateral and output norms
        under FE.FPN.NORM: BN, with the refusals and the `fpn_batch_stats()` read-out of DD3D.compute_losses; `backbone_batch_stats`
        (from `**branch` too) for the DLA-34 bottom-up network's norms under FE.BACKBONE.NORM: BN, read out by `backbone_batch_stats()`.
        What DD3D.compute_losses refuses is refused here in the same words (NotImplementedError: the Bottleneck DLA variants,
        force_generic_dla, the slim / depthwise VoVNet specs, the reduced arithmetic modes, backbone_grads on a VoVNet, vovnet_grads on a
        DLA, FE.BACKBONE.NORM / FE.FPN.NORM = BN under batch_stats).  The filter copies the backward reads are snapshots taken when the
        plan is built; there is no optimiser and no model.train()."""
        from dd3d_amd.engine import relax_arithmetic
        batch_stats = bool(branch.pop("batch_stats", False))
        norms = dict(batch_stats=batch_stats, fpn_batch_stats=True) if branch.pop("fpn_batch_stats", False) else dict(batch_stats=batch_stats)
        if branch.pop("backbone_batch_stats", False):
            norms["backbone_batch_stats"] = True
        vovnet_stem_grads = bool(branch.pop("vovnet_stem_grads", False))
        vovnet_grads = bool(branch.pop("vovnet_grads", False)) or vovnet_stem_grads
        if branch:
            raise TypeError(f"compute_losses() got an unexpected keyword argument {next(iter(branch))!r}")
        for i, x in enumerate(batched_inputs):
            if "depth" not in x:
                raise ValueError(f"image {i}: compute_losses needs a 'depth' map in every item of the batch")
        from dd3d_amd.engine.dense_depth_loss import check_depth_maps, dense_depth_loss_config
        dense_depth_loss_config(self.cfg)  # (config and input errors before a plan is built or an image staged)
        check_depth_maps([x["depth"] for x in batched_inputs], [(int(x["image"].shape[-2]), int(x["image"].shape[-1])) for x in batched_inputs])
        backbone_grads = backbone_grads or stem_grads
        fpn_grads = fpn_grads or backbone_grads or vovnet_grads
        tower_grads = tower_grads or fpn_grads
        flags = dict(vovnet_stem_grads=vovnet_stem_grads, vovnet_grads=vovnet_grads, stem_grads=stem_grads, backbone_grads=backbone_grads,
                     fpn_grads=fpn_grads, tower_grads=tower_grads, pred_grads=predictor_grads, head_grads=head_grads)
        while True:
            try:
                return self._compute_losses(batched_inputs, flags, **norms)
            except FloatingPointError as e:
                if not relax_arithmetic(self, e):
                    raise

    def _compute_losses(self, batched_inputs, flags, **norms):
        """One run of the plan of the deepest flag; results are read only behind a passed status check."""
        plan, sizes = self._stage(batched_inputs, lambda B, H, W: self.get_loss_plan(B, H, W, **norms, **_deepest(**flags)))
        plan.stage_depth([x["depth"] for x in batched_inputs], sizes, checked=True)  # (compute_losses has validated the maps)
        plan.run()
        plan.check_status()
        if not (flags["pred_grads"] or flags["tower_grads"]):
            return (plan.loss_dict(), plan.head_grads()) if flags["head_grads"] else plan.loss_dict()
        tens, params = plan.predictor_grads()
        for name in ("tower_grads", "fpn_grads", "backbone_grads", "stem_grads", "vovnet_grads", "vovnet_stem_grads"):
            if flags[name]:
                more_t, more_p = getattr(plan, name)()
                tens, params = dict(tens, **more_t), dict(params, **more_p)
        return plan.loss_dict(), dict(plan.head_grads(), **tens), params

    def forward(self, batched_inputs):
        raise NotImplementedError()  # the reference's eval-mode forward (dense_depth.py:162-163)
