"""``DD3D`` meta-architecture: the drop-in boundary of the forward path.

Same registered name, constructor signature ``(cfg)``, attributes and call contract as
tridet/modeling/dd3d/core.py:18-175:  ``model(batched_inputs: List[dict]) -> List[{"instances": Instances}]``.
Only the inference branch exists as the forward (training is out of scope); everything from the
uint8 image to the final detections runs in the HIP engine (dd3d_amd.engine) on the model's device.  ``compute_losses`` /
``prepare_targets`` give the training branch's loss dict and targets without gradients (engine.LossPlan).
"""
import numpy as np
import torch
from torch import nn

from dd3d_amd.engine import ForwardPlan
from dd3d_amd.modeling.heads import FCOS2DHead, FCOS3DHead
from dd3d_amd.registry import BACKBONE_REGISTRY, META_ARCH_REGISTRY
from dd3d_amd.structures import Boxes, Boxes3D, Instances, ShapeSpec


_EYE3 = np.eye(3, dtype=np.float32)


def _as_f32_array(t):
    """Host float32 numpy view / copy of a small tensor-like (the per-image intrinsics)."""
    if isinstance(t, torch.Tensor):
        return t.detach().to(device="cpu", dtype=torch.float32).numpy()
    return np.asarray(t, dtype=np.float32)


def _deepest(**flags):
    """{name: True} of the first flag set -- the caller lists the loss plan's levels deepest first, each implying the ones after it --
    or {} when none is: one plan, and one cache key, per deepest requested level of the backward."""
    return next(({name: True} for name, on in flags.items() if on), {})


def build_feature_extractor(cfg, input_shape=None):
    """tridet/modeling/feature_extractor/__init__.py:13-26."""
    if input_shape is None:
        input_shape = ShapeSpec(channels=len(cfg.MODEL.PIXEL_MEAN))
    return BACKBONE_REGISTRY.get(cfg.FE.BUILDER)(cfg, input_shape)


@META_ARCH_REGISTRY.register()
class DD3D(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.backbone = build_feature_extractor(cfg)
        backbone_output_shape = self.backbone.output_shape()
        self.in_features = cfg.DD3D.IN_FEATURES or list(backbone_output_shape.keys())
        self.backbone_output_shape = [backbone_output_shape[f] for f in self.in_features]
        self.feature_locations_offset = cfg.DD3D.FEATURE_LOCATIONS_OFFSET

        self.fcos2d_head = FCOS2DHead(cfg, self.backbone_output_shape)
        if cfg.MODEL.BOX3D_ON:
            self.fcos3d_head = FCOS3DHead(cfg, self.backbone_output_shape)
            self.only_box2d = False
        else:
            self.only_box2d = True

        self.postprocess_in_inference = cfg.DD3D.INFERENCE.DO_POSTPROCESS
        self.do_nms = cfg.DD3D.INFERENCE.DO_NMS
        self.do_bev_nms = cfg.DD3D.INFERENCE.DO_BEV_NMS
        self.bev_nms_iou_thresh = cfg.DD3D.INFERENCE.BEV_NMS_IOU_THRESH
        self.nusc_sample_aggregate_in_inference = cfg.DD3D.INFERENCE.NUSC_SAMPLE_AGGREGATE
        self.num_classes = cfg.DD3D.NUM_CLASSES

        self.register_buffer("pixel_mean", torch.Tensor(list(cfg.MODEL.PIXEL_MEAN)).view(-1, 1, 1))
        self.register_buffer("pixel_std", torch.Tensor(list(cfg.MODEL.PIXEL_STD)).view(-1, 1, 1))
        self._plans = {}
        self.max_cached_plans = 8  # launch plans kept per model (one per (batch, padded size, flags)); least recently used goes first
        self.use_graph = True
        # None: DD3D_MATH / the default ("f16x2", falling back to "bf16x3" for good if an activation ever leaves the half range); or one
        # of "f16x2" / "bf16x3" / "f32" / "bf16x2" / "bf16" (dd3d_amd.engine.default_math), set before the first forward
        self.math = None
        # plane scale of the f16x2 arithmetic (a power of two; None: DD3D_F16_ACT_SCALE / 16).  The range guard's staged fallback lowers it
        # 16 -> 4 -> 1 on an overflow before it gives up the f16x2 speed (dd3d_amd.engine.plan.relax_arithmetic)
        self.act_scale = None
        # None / "latency": launch plans tiled for one forward at a time; "throughput": for plans that share the chip with other plans in
        # flight (dd3d_amd.engine.tiling.THROUGHPUT_TILE_TABLE; PipelinedForward slots covering several requests choose it themselves)
        self.tile_policy = None
        self.training = False

    @property
    def device(self):
        return self.pixel_mean.device

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("dd3d_amd implements the inference forward path only")
        return super().train(False)

    # ------------------------------------------------------------------ plan management
    def invalidate_plans(self):
        """Call after changing weights in place (plans read packed copies of the weights, shared by all plans of the model)."""
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

    def _sync_flags(self):
        """`do_test` / TTA flip these attributes on the instance (scripts/train.py:206-209,268-272); mirror them
        into the config the plan is built from."""
        inf = self.cfg.DD3D.INFERENCE
        inf.DO_POSTPROCESS, inf.DO_NMS = bool(self.postprocess_in_inference), bool(self.do_nms)
        inf.DO_BEV_NMS, inf.BEV_NMS_IOU_THRESH = bool(self.do_bev_nms), float(self.bev_nms_iou_thresh)
        return (bool(self.postprocess_in_inference), bool(self.do_nms), bool(self.do_bev_nms))

    def get_plan(self, B, Hp, Wp, world_size=1, rank=0, exchange=None, camera_sharded=False):
        exchange = world_size > 1 if exchange is None else bool(exchange)
        key = (B, Hp, Wp, world_size, rank, exchange, bool(camera_sharded), self.math, self.act_scale, getattr(self, "tile_policy", None)) + self._sync_flags()
        plan = self._plans.pop(key, None)
        if plan is None:
            plan = ForwardPlan(self, B, Hp, Wp, world_size=world_size, rank=rank, exchange=exchange, camera_sharded=camera_sharded)
            if self.use_graph and not exchange:
                plan.capture()
        self._plans[key] = plan  # (re-)inserted last = most recently used
        self._evict_plans()
        return plan

    def get_loss_plan(self, B, Hp, Wp, grads=False, pred_grads=False, tower_grads=False, fpn_grads=False, backbone_grads=False, stem_grads=False,
                      vovnet_grads=False, batch_stats=False, vovnet_stem_grads=False, fpn_batch_stats=False, backbone_batch_stats=False):
        """The loss plan (engine.LossPlan) for one geometry, captured as one hipGraph; kept in the same bounded cache as the forward plans.
        `grads`: the plan that also runs the loss backward (head-map gradients); `pred_grads`: the plan that runs the predictor layer's
        backward behind it as well (parameter and tower-output gradients; implies `grads`); `tower_grads`: the plan that goes on through
        the head towers (their parameter gradients and the gradient at the FPN outputs; implies `pred_grads`); `fpn_grads`: the plan that
        goes on through the FPN (its parameter gradients and the gradient at the backbone's output features; implies `tower_grads`);
        `backbone_grads`: the plan that goes on through DLA-34's level5 .. level2 (their parameter gradients and the gradient at the stem's
        output; implies `fpn_grads`); `stem_grads`: the plan that goes on through the stem (base_layer, level0, level1: their parameter
        gradients and the gradients at base_layer's and level0's outputs; implies `backbone_grads`); `vovnet_grads`: the plan of a VoVNet-V2
        model that goes on from the FPN through stage5 .. stage2, stem_3 and stem_2 (their parameter gradients and the gradient at stem_1's
        output; implies `fpn_grads`; a DLA model raises NotImplementedError naming `stem_grads`); `vovnet_stem_grads`: the plan that goes on
        through stem_1 (its parameter gradients; the image has no gradient; implies `vovnet_grads`, and raises for whatever that raises for);
        `batch_stats`: the head towers whose norm is
        a trainable BatchNorm2d use the batch's statistics, as the reference's train() does (composes with every level above; a plan of
        its own beside the running-statistics one); `fpn_batch_stats`: the FPN's lateral and output norms (FE.FPN.NORM: BN) use the batch's
        statistics (composes with every level above and with `batch_stats`; one more plan and cache key of its own); `backbone_batch_stats`: the
        norms of a DLA-34 bottom-up network (FE.BACKBONE.NORM: BN) use the batch's statistics (composes with every level above and with
        both other norm flags; one more plan and cache key of its own)."""
        from dd3d_amd.engine.losses import LossPlan
        level = _deepest(vovnet_stem_grads=vovnet_stem_grads, vovnet_grads=vovnet_grads, stem_grads=stem_grads, backbone_grads=backbone_grads,
                         fpn_grads=fpn_grads, tower_grads=tower_grads, pred_grads=pred_grads, grads=grads)
        key = ("losses", B, Hp, Wp, self.math, self.act_scale, getattr(self, "tile_policy", None)) + tuple(level)
        if batch_stats:
            key, level = key + ("batch_stats", ), dict(level, batch_stats=True)
        if fpn_batch_stats:
            key, level = key + ("fpn_batch_stats", ), dict(level, fpn_batch_stats=True)
        if backbone_batch_stats:
            key, level = key + ("backbone_batch_stats", ), dict(level, backbone_batch_stats=True)
        plan = self._plans.pop(key, None)
        if plan is None:
            plan = LossPlan(self, B, Hp, Wp, **level)
            if self.use_graph:
                plan.capture()
        self._plans[key] = plan
        self._evict_plans()
        return plan

    def _evict_plans(self):
        """Inputs of ever-changing size would otherwise pin a buffer set (0.5 - 3 GB) per size for the life of the model."""
        while len(self._plans) > max(1, int(self.max_cached_plans)):
            if torch.cuda.is_available():
                torch.cuda.synchronize()  # its last replay may still be running on the buffers about to be released
            self._plans.pop(next(iter(self._plans)))

    # ------------------------------------------------------------------ host side of forward
    def canvas_size(self, batched_inputs):
        """(B, H, W) of the padded canvas of a batch: ImageList.from_tensors' geometry (image_list.py:120-142), as stage_inputs pads."""
        sizes = [(int(x["image"].shape[-2]), int(x["image"].shape[-1])) for x in batched_inputs]
        div = self.backbone.size_divisibility
        H, W = max(s[0] for s in sizes), max(s[1] for s in sizes)
        if div > 1:
            H, W = (H + div - 1) // div * div, (W + div - 1) // div * div
        return len(sizes), H, W

    def stage_inputs(self, batched_inputs, plan=None, first=0, partial=False, flush=True):
        """core.py:65-72: gather images/intrinsics; the padded canvas geometry is ImageList.from_tensors'
        (image_list.py:120-142).  Returns (plan, image_sizes).  `first` (with a fixed `plan` only): the batch goes to positions
        [first, first + len(batch)) of a plan; `partial` allows a batch shorter than the plan's (PipelinedForward micro-batches, the
        short last batch of a shard): the other positions keep what they held and their outputs are the caller's to ignore.

        Host cost per request (round 6): the image goes by ONE asynchronous copy per image (a pinned source never blocks the host); sizes,
        intrinsics, resize targets (and poses / sample ids of a model with BEV stages) are plain stores into the plan's pinned host mirrors,
        shipped by `plan.flush_inputs()` -- here when `flush`, or once per slot run by a runner that stages several requests into one plan
        (`flush=False`; PipelinedForward._enqueue)."""
        images = [x["image"] for x in batched_inputs]
        image_sizes = [(int(im.shape[-2]), int(im.shape[-1])) for im in images]
        div = self.backbone.size_divisibility
        H = max(s[0] for s in image_sizes)
        W = max(s[1] for s in image_sizes)
        if div > 1:
            H, W = (H + div - 1) // div * div, (W + div - 1) // div * div
        B = len(images)
        if "intrinsics" not in batched_inputs[0]:
            if not self.only_box2d:
                raise ValueError("DD3D with BOX3D_ON needs 'intrinsics' in every input dict")
            K = np.tile(np.eye(3, dtype=np.float32) * 2.0, (B, 1, 1))
        else:
            K = np.stack([_as_f32_array(x["intrinsics"]) for x in batched_inputs], 0)
            if np.allclose(K[0], _EYE3, rtol=1e-5, atol=1e-8):
                raise ValueError("Intrinsics is Identity.")  # image_list.py:57-62
        if plan is None:
            assert first == 0 and not partial
            plan = self.get_plan(B, H, W)
        elif (H, W) != (plan.Hp, plan.Wp) or first < 0 or first + B > plan.B or (B != plan.B and not partial):
            # a fixed plan (DistributedForward / PipelinedForward): a short batch would leave stale images in the other positions (allowed
            # only where the caller says so: `partial`), a smaller canvas would run on a larger padded canvas than the reference's
            # ImageList (other border features)
            raise ValueError(f"batch of {B} images on a {H}x{W} canvas at position {first} does not fit the fixed launch plan "
                             f"(B={plan.B}, {plan.Hp}x{plan.Wp}); pad the batch / canvas or build a plan for this geometry")
        sl = slice(first, first + B)
        for i, im in enumerate(images):
            assert im.dtype == torch.uint8 and im.shape[0] == 3, "expected uint8 (3,H,W) images (dataset_mapper.py:127)"
            if image_sizes[i] == (plan.Hp, plan.Wp):
                plan.in_u8[first + i].copy_(im, non_blocking=True)  # whole canvas: one contiguous copy
            else:
                plan.in_u8[first + i, :, :im.shape[1], :im.shape[2]].copy_(im, non_blocking=True)
        plan.inputs_writable()  # (the previous forward's copy out of the host mirrors has run: normally long ago)
        m = plan.host_np  # numpy views of the pinned mirrors: plain host stores, no tensor is built per request
        m["sizes"][sl] = image_sizes
        m["K"][sl] = K.reshape(B, 9)
        m["outsize"][sl] = [(s[0], s[1], x.get("height", s[0]), x.get("width", s[1])) for s, x in zip(image_sizes, batched_inputs)]
        if plan.has_bev_inputs:  # BEV stages need camera->global poses and sample membership
            m["pose"][sl] = [self._pose_vec(x) for x in batched_inputs]
            if not getattr(plan, "camera_sharded", False):  # (camera-sharded: membership is positional in the global image order)
                # sample ids are per request: offset by the position so that requests sharing a plan never merge their samples
                m["group"][sl] = np.asarray(self._sample_groups(batched_inputs), dtype=np.int32) + first
        if flush:
            plan.flush_inputs()
        return plan, image_sizes

    @staticmethod
    def _pose_vec(x):
        """core.py:138-141: 'pose' if present, else 'extrinsics'; (quat wxyz, tvec) as postprocessing.py:34 reads them."""
        pose = x["pose"] if "pose" in x else x["extrinsics"]
        return [float(v) for v in pose.quat.elements] + [float(v) for v in pose.tvec]

    def _sample_groups(self, batched_inputs):
        return list(range(len(batched_inputs)))

    def _counts(self, plan):
        """Detection counts of the plan's last forward (this is the host's wait for the forward), with the device-side faults checked --
        all out of the forward's read-back record (engine.PlanBase.readback: one asynchronous copy into pinned memory, enqueued behind the
        forward; round 5 read counts, status word and range-guard maxima with one blocking copy each, per request)."""
        rb = plan.readback()
        if not getattr(rb, "checked", False):  # (once per forward: the requests sharing a slot run read the same record)
            plan.check_status(rb)  # a numeric fault flagged by a kernel (half-range overflow of the f16x2 mode) fails the forward loudly
            rb.checked = True
        counts = rb.counts
        if counts.numel() and int(counts.min()) < 0:
            raise RuntimeError("more than 8192 detections met in one BEV NMS problem (the capacity of its LDS sorter): feed fewer images per step")
        n_max = int(counts.max()) if counts.numel() else 0
        if n_max > plan.det_cap:
            raise RuntimeError(f"{n_max} detections exceed the detection buffer ({plan.det_cap}); raise det_cap")
        return counts, n_max

    def _instances(self, plan, d, size, inv_K):
        """Rows of the detection buffer (a PRIVATE copy: the fields below are views of it, no further copies) -> Instances with the
        reference's fields (core.py:153-164)."""
        n = d.shape[0]
        r = Instances(size)
        r.pred_boxes = Boxes(d[:, 0:4])
        r.scores = d[:, 4]
        ints = d[:, 6:8].to(torch.int64)  # [class, level]
        r.pred_classes = ints[:, 0]
        r.locations = d[:, 8:10]
        r.fpn_levels = ints[:, 1]
        if not self.only_box2d:
            r.pred_boxes3d = Boxes3D(d[:, 10:14], d[:, 14:16], d[:, 16:17], d[:, 17:20], inv_K[None].expand(n, 3, 3))
            r.scores_3d = d[:, 5]
        self._collect_extra(r, d, plan)
        return r

    def collect(self, plan, batched_inputs, image_sizes, first=0):
        """Detection buffer -> List[{"instances": Instances}] for the images at positions [first, first + len(batch)) of the plan.  Per image:
        one device copy of its detection rows (the results must not alias a buffer the next forward overwrites) and one integer cast;
        every field is a view of that copy."""
        counts, n_max = self._counts(plan)
        B = len(batched_inputs)
        inv_K = plan.inv_K.view(-1, 3, 3)[first:first + B].clone()
        results = []
        for i, (inp, isz) in enumerate(zip(batched_inputs, image_sizes)):
            g = first + i
            d = plan.det[g, :int(counts[g])].clone()
            size = (int(inp.get("height", isz[0])), int(inp.get("width", isz[1]))) if self.postprocess_in_inference else isz
            results.append({"instances": self._instances(plan, d, size, inv_K[i])})
        return results

    def collect_owned(self, plan):
        """Camera-sharded plans (engine.ForwardPlan(camera_sharded=True)): the detections of the samples THIS rank owns, as
        [(global image index, {"instances": Instances})] -- cameras that other ranks decoded included.  Everything comes from the
        device: counts and detections from the owner's post stages, image sizes and K^-1 from the gathered records."""
        assert plan.camera_sharded
        if plan.G == 0:
            torch.cuda.current_stream().synchronize()
            return []
        counts, n_max = self._counts(plan)
        det = plan.det
        sl = slice(plan.img_first, plan.img_first + plan.G)
        osz = plan.gathered_field("outsize")[sl].cpu()
        inv_K = plan.gathered_field("inv_K")[sl].reshape(-1, 3, 3).clone()
        results = []
        for g in range(plan.G):
            d = det[g, :int(counts[g])].clone()
            size = (int(osz[g, 2]), int(osz[g, 3])) if self.postprocess_in_inference else (int(osz[g, 0]), int(osz[g, 1]))
            results.append((plan.img_first + g, {"instances": self._instances(plan, d, size, inv_K[g])}))
        return results

    def _collect_extra(self, r, d, plan):
        pass

    # ------------------------------------------------------------------ training losses (gradients: head maps and the predictor layer)
    @torch.no_grad()
    def compute_losses(self, batched_inputs, head_grads=False, predictor_grads=False, tower_grads=False, fpn_grads=False, backbone_grads=False,
                       stem_grads=False, batch_stats=False, fpn_batch_stats=False, backbone_batch_stats=False, **branch):
        """The loss dict of the reference's training branch (core.py:95-112; NuscenesDD3D: nuscenes_dd3d.py:376-397) for a labelled batch:
        each item carries `image`, `intrinsics` and `instances` (gt_boxes, gt_classes, gt_boxes3d; nuScenes also gt_attributes,
        gt_speeds).  Values are 0-d float32 tensors on the model's device, keys in the reference's order.  Differences from the
        reference: by default every norm layer uses its running statistics (the head maps are exactly this forward's; `batch_stats`,
        below, gives the reference's train() forward), one process (reduce_sum is the identity).  With `head_grads` the result is (loss dict, grads): the gradient of the sum of the dict's values
        with respect to the head maps the losses read, as NCHW per-level tensors under the reference's names (logits<l>, box2d_reg<l>
        -- post-ReLU --, centerness<l>, quat<l>, ctr<l>, depth<l>, size<l>, conf<l>, attr<l>, speed<l>).  With `predictor_grads` the
        result is (loss dict, grads, param_grads): `grads` holds the same head-map gradients and also the gradient at the tower outputs
        the predictors read (cls_tower_out<l>, box2d_tower_out<l>, box3d_tower_out<l>: (B, 256, h_l, w_l) float32); `param_grads` maps
        the named_parameters() names of the predictor layer (the 3x3 predictors' weight and bias, the per-level Scale.scale and
        Offset.bias) to float32 gradients of the parameter's shape.  With `tower_grads` the result has the same form and the backward
        goes on through the head towers: `grads` also holds the gradient at the FPN outputs the heads read (feature<l>: (B, 256, h_l,
        w_l)), `param_grads` also the tower parameters (every tower filter; a BN tower's per-level norm weight and bias; a norm-less
        tower's conv bias; a FrozenBN tower's norm has no parameters).  With `fpn_grads` the result has the same form again and the
        backward goes on through the FPN: everything `tower_grads` returns, bit for bit, and `grads` also holds the gradient at the
        backbone's output features (backbone_<name>, e.g. backbone_level3 or backbone_stage2: (B, C_name, h, w)), `param_grads` also the
        FPN's parameters (backbone.fpn_lateral<s>.weight, backbone.fpn_output<s>.weight, backbone.top_block.p6 / p7 weight and bias, and
        whatever norm weights or conv biases FE.FPN.NORM owns).  With `backbone_grads` the result has the same form once more and the
        backward goes on through the DLA-34 backbone, level5 down to level2: everything `fpn_grads` returns, bit for bit (backbone_level3..5
        stay the FPN's contribution at those features), `grads` also holds backbone_level1 -- the gradient at the stem's stored output,
        (B, 32, Hp / 2, Wp / 2), not yet masked by that tensor's own ReLU -- and `param_grads` also every parameter of
        backbone.bottom_up.level2 .. level5 (the filters of tree*.conv1 / conv2, project and root.conv; a BN backbone's norm weights and
        biases; a norm-less backbone's conv biases; FrozenBN, the released configs' norm, owns nothing).  With `stem_grads` the result has
        the same form a last time and the backward goes on through the stem: everything `backbone_grads` returns, bit for bit, `grads`
        also holds backbone_level0 and backbone_base_layer -- the gradients at level0's and base_layer's outputs, (B, 16, Hp, Wp), neither
        masked by its tensor's own ReLU yet -- and `param_grads` also backbone.bottom_up.base_layer / level0.0 / level1.0 (.weight; a BN
        backbone's .norm.weight / .norm.bias; a norm-less backbone's .bias): for DLA-34 its keys are then those of named_parameters().
        With `vovnet_grads` (VoVNet-V2 models: V-19-eSE, V-39-eSE, V-57-eSE, V-99-eSE) the result has the form of `fpn_grads` and the
        backward goes on through the bottom-up network, stage5 down to stage2, stem_3 and stem_2: everything `fpn_grads` returns, bit for
        bit (backbone_stage2..5 stay the FPN's contribution at those features), `grads` also holds backbone_stem_1 -- the gradient at
        stem_1's stored output, (B, 64, Hp / 2, Wp / 2), not yet masked by that tensor's own ReLU -- and `param_grads` also every
        parameter of backbone.bottom_up except stem.stem_1/* (each OSA module's layers.<i>.<n>_<i>/conv.weight, concat.<n>_concat/conv.weight,
        ese.fc.weight and ese.fc.bias; stem.stem_2/conv.weight and stem.stem_3/conv.weight; a BN backbone's norm weights and biases).
        With `vovnet_stem_grads` the result has the same form and the backward goes on through stem_1 (3x3 stride 2 on the four-channel
        image; the image itself has no gradient): everything `vovnet_grads` returns, bit for bit (backbone_stem_1 included, still
        unmasked), and `param_grads` also holds backbone.bottom_up.stem.stem_1/conv.weight ((64, 3, 3, 3)) and a BN backbone's
        stem.stem_1/norm.weight / .bias: for the four covered VoVNet specs its keys are then those of named_parameters().  DLA models
        raise NotImplementedError naming `stem_grads`; the slim and depthwise specs, DD3D_PLANES=0 and the reduced arithmetic modes raise
        too.  (`vovnet_grads` and `vovnet_stem_grads` are keywords of their own, not further levels of the chain head_grads .. stem_grads
        above, whose named parameters tests/test_loss_plan_history.py pins: they are taken from `**branch`, and any other extra keyword is
        a TypeError.)
        With `batch_stats` -- it composes with every flag above -- the head towers whose norm is a trainable BatchNorm2d (cls and box2d in
        the released configs, box3d under FCOS3D.NORM: BN) normalise every layer with the batch's mean and biased variance, per pyramid
        level and channel over the B * h_l * w_l pixels of the padded canvas, and the backward differentiates through both, as the
        reference's train() does (csrc/tower_bn.hip); FrozenBN and norm-less towers keep the running-statistics path in the same plan.
        Keys and shapes of every result stay, the values follow the new forward; `plan.tower_batch_stats()` (the plan of
        `get_loss_plan(..., batch_stats=True)`) returns the running statistics the step would leave and the batch's own, and the
        model's buffers are never written.  A level with one value per channel (one 64 x 128 image: P7 is 1 x 1) raises ValueError in
        torch's words; FE.BACKBONE.NORM / FE.FPN.NORM = BN raise NotImplementedError naming the key.
        With `fpn_batch_stats` (it composes with every flag above, `batch_stats` included) the FPN's trainable
        BatchNorm2d norms -- fpn_lateral<s>.norm and fpn_output<s>.norm under FE.FPN.NORM: BN, eps 1e-5 -- normalise with the mean and
        biased variance of their own convolution's output over the B * h_s * w_s pixels of the padded canvas, the top-down sum adds the
        normalised laterals in float32, and the backward goes through both statistics (csrc/fpn_bn.hip); the top block is unchanged.
        Keys and shapes of every result stay; backbone.fpn_lateral<s>.norm.weight / .bias and the fpn_output<s> pair in `param_grads`
        are the norm backward's sums.  `plan.fpn_batch_stats()` (the plan of `get_loss_plan(..., fpn_batch_stats=True)`) returns the
        running statistics the step would leave and the batch's own; the model's buffers are never written.  It is the reference's
        train() forward of an FPN on a frozen bottom-up network: FE.BACKBONE.NORM = BN still raises NotImplementedError naming the key
        (the DLA / VoVNet network would need batch statistics too).  FE.FPN.NORM other than BN raises ValueError naming the key (the
        flag is never a silent no-op), a stage with one value per channel ValueError in torch's words; FE.FPN.OUT_CHANNELS not a
        multiple of 32 or above 256, FUSE_TYPE avg, DD3D_PLANES=0, DD3D_PLANES_ONLY=0, DD3D_MATH=f32 and the reduced arithmetic modes
        raise NotImplementedError.  `batch_stats=True` alone keeps refusing FE.FPN.NORM = BN.
        With `backbone_batch_stats` (it composes with every flag above, `batch_stats` and `fpn_batch_stats` included) every BatchNorm2d of a
        DLA-34 bottom-up network under FE.BACKBONE.NORM: BN -- base_layer, level0, level1 and each tree's conv1 / conv2, project and
        root.conv -- normalises its own convolution's raw output with the mean and biased variance over the B * h * w pixels of the
        padded canvas (relu(n), n for a project, relu(n + residual) for a block's conv2), and the backward goes through both statistics
        (csrc/backbone_bn.hip); the stem runs launch by launch (the fused stem keeps base_layer and level0 in LDS).  Keys and shapes of
        every result stay; the bottom-up norms' .weight / .bias in `param_grads` are the norm backward's sums.
        `plan.backbone_batch_stats()` returns the running statistics the step would leave and the batch's own; the model's buffers are
        never written.  With all three norm flags a DLA-34 model with BN everywhere returns the loss dict and every parameter gradient
        of the reference's train() step.  FE.BACKBONE.NORM other than BN raises ValueError naming the key; a VoVNet, the Bottleneck DLA
        variants, force_generic_dla, DD3D_MATH=f32, DD3D_PLANES=0, DD3D_PLANES_ONLY=0 and the reduced arithmetic modes raise
        NotImplementedError; a level with one value per channel raises ValueError in torch's words.  Without it `batch_stats` and
        `fpn_batch_stats` keep refusing FE.BACKBONE.NORM = BN.
        The filter copies the backward reads are snapshots taken when the plan is built; there is no optimiser and no model.train().  V2-99, the Bottleneck DLA variants, force_generic_dla and the reduced arithmetic modes raise
        NotImplementedError."""
        from dd3d_amd.engine import relax_arithmetic
        vovnet_stem_grads = bool(branch.pop("vovnet_stem_grads", False))
        vovnet_grads = bool(branch.pop("vovnet_grads", False)) or vovnet_stem_grads
        norms = dict(batch_stats=batch_stats, fpn_batch_stats=True) if fpn_batch_stats else dict(batch_stats=batch_stats)
        if backbone_batch_stats:
            norms["backbone_batch_stats"] = True
        if branch:
            raise TypeError(f"compute_losses() got an unexpected keyword argument {next(iter(branch))!r}")
        gt = [x["instances"] for x in batched_inputs]
        while True:
            backbone_grads = backbone_grads or stem_grads
            fpn_grads = fpn_grads or backbone_grads or vovnet_grads
            tower_grads = tower_grads or fpn_grads
            level = _deepest(vovnet_stem_grads=vovnet_stem_grads, vovnet_grads=vovnet_grads, stem_grads=stem_grads, backbone_grads=backbone_grads,
                             fpn_grads=fpn_grads, tower_grads=tower_grads, pred_grads=predictor_grads, grads=head_grads)
            plan = self.get_loss_plan(*self.canvas_size(batched_inputs), **norms, **level)
            plan.stage_gt(gt)
            self.stage_inputs(batched_inputs, plan=plan)  # (its flush ships the GT too)
            plan.run()
            rb = plan.readback()
            try:
                plan.check_status(rb)
            except FloatingPointError as e:  # the f16x2 range guard, as in forward()
                if not relax_arithmetic(self, e):
                    raise
                continue
            losses = plan.loss_dict(int(rb.counts[0]))
            if predictor_grads or tower_grads:
                towers, params = plan.predictor_grads()
                for on, read in ((tower_grads, plan.tower_grads), (fpn_grads, plan.fpn_grads), (backbone_grads, plan.backbone_grads),
                                 (stem_grads, plan.stem_grads), (vovnet_grads, plan.vovnet_grads), (vovnet_stem_grads, plan.vovnet_stem_grads)):
                    if on:
                        tens, more = read()
                        towers, params = dict(towers, **tens), dict(params, **more)
                return losses, dict(plan.head_grads(), **towers), params
            return (losses, plan.head_grads()) if head_grads else losses

    @torch.no_grad()
    def prepare_targets(self, locations, gt_instances, feature_shapes):
        """DD3DTargetPreparer.__call__ (prepare_targets.py:28-91; NuscenesDD3D: nuscenes_dd3d.py:29-99) on the device: `locations` per
        level (H*W, 2), `gt_instances` per image, `feature_shapes` per level (H, W).  Returns the reference's dict of device tensors
        (box3d_targets as a Boxes3D with float32 K^-1)."""
        from dd3d_amd.engine.losses import assign_targets
        return assign_targets(self, locations, gt_instances, feature_shapes)

    @torch.no_grad()
    def forward(self, batched_inputs):
        from dd3d_amd.engine import relax_arithmetic
        while True:
            plan, image_sizes = self.stage_inputs(batched_inputs)
            plan.run()
            try:
                return self.collect(plan, batched_inputs, image_sizes)
            except FloatingPointError as e:
                # The range guard of the f16x2 arithmetic.  A model on the default arithmetic first widens the half range (plane scale 16 -> 4
                # -> 1: activations up to 4094 -> 16376 -> 65504 at the same speed), then runs on the three-term bf16 split from now on (same
                # f32-equivalent products, full f32 exponent range, twice the matrix work); an explicitly chosen arithmetic raises.
                if not relax_arithmetic(self, e):
                    raise
