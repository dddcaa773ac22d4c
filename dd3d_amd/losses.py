"""The fused DD3D training loss as a differentiable torch function of the head maps.

``FusedDD3DLoss(model)(head_maps, inv_K, gt_instances)`` replaces the reference's DD3DTargetPreparer + FCOS2DLoss + FCOS3DLoss (and
NuscenesLoss) on ROCm: one assignment launch and one fused loss launch in forward, one fused launch in backward (csrc/losses.hip,
csrc/loss_grads.hip).  ``head_maps`` holds the reference's per-level NCHW head outputs under the names ``logits<l>``, ``box2d_reg<l>``
(post-ReLU), ``centerness<l>``, ``quat<l>``, ``ctr<l>``, ``depth<l>``, ``size<l>``, ``conf<l>`` and, for NuscenesDD3D, ``attr<l>`` and
``speed<l>``; they may require grad and may be the outputs of further torch ops.  The result is the reference's loss dict, keys in its
order, as 0-d tensors that carry the gradient.  No double backward.

``FusedDenseDepthLoss(model)(dense_depth_maps, intrinsics, depths)`` does the same for the depth pre-training network: it replaces the
aligned_bilinear up-sampling, the focal-length division and DenseDepthL1Loss of the reference's DD3DDenseDepth.forward by one fused
launch in forward and one in backward (csrc/dense_depth_loss.hip, csrc/dense_depth_loss_grads.hip); the up-sampled maps are never stored.
"""
import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from dd3d_amd import hip
from dd3d_amd.engine import losses as E


def _expected_channels(model):
    C_ = int(model.num_classes)
    ch = {"logits": C_, "box2d_reg": 4, "centerness": 1}
    if not model.only_box2d:
        C3 = 1 if bool(model.cfg.DD3D.FCOS3D.CLASS_AGNOSTIC_BOX3D) else C_
        ch.update({k: n * C3 for k, (_, n) in E.BOX3D_COMPONENTS.items()})
    if E.model_is_nusc(model):
        ch.update(attr=E.num_attributes(model), speed=1)
    return ch


def check_head_maps(model, head_maps):
    """Keys, shapes, dtype and device of `head_maps`; returns (families in packing order, per-level (H, W), batch size)."""
    ch = _expected_channels(model)
    L = len(model.backbone_output_shape)
    if not hasattr(head_maps, "keys"):
        raise ValueError("head_maps must be a dict of per-level NCHW tensors")
    missing = [f"{k}{l}" for l in range(L) for k in ch if f"{k}{l}" not in head_maps]
    if missing:
        raise ValueError(f"head_maps lacks {missing}")
    B = None
    level_hw = []
    for l in range(L):
        ref = head_maps[f"logits{l}"]
        for k, n in ch.items():
            t = head_maps[f"{k}{l}"]
            if not isinstance(t, torch.Tensor) or t.dim() != 4:
                raise ValueError(f"{k}{l} must be a 4-d NCHW tensor")
            if t.device.type != "cuda":
                raise ValueError(f"{k}{l} is on {t.device}: the fused loss runs on the HIP device only")
            if t.dtype != torch.float32:
                raise ValueError(f"{k}{l} is {t.dtype}; float32 expected")
            B = int(t.shape[0]) if B is None else B
            want = (B, n, int(ref.shape[2]), int(ref.shape[3]))
            if tuple(t.shape) != want:
                raise ValueError(f"{k}{l} has shape {tuple(t.shape)}; expected {want}")
        level_hw.append((int(ref.shape[2]), int(ref.shape[3])))
    return list(ch), level_hw, B


def _pack_nhwc(parts):
    """cat(parts, 1) as a contiguous NHWC buffer whose channel pitch is a multiple of 4 (the layout of the predictor maps)."""
    t = torch.cat(parts, 1).permute(0, 2, 3, 1)
    n = t.shape[-1]
    pitch = (n + 3) // 4 * 4
    return torch.nn.functional.pad(t, (0, pitch - n)).contiguous(), pitch


class _State:
    """What backward needs of a forward: the argument struct and every buffer it points at."""


class _FusedLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, st, *maps):
        model, fams, level_hw, B = st.model, st.families, st.level_hw, st.B
        dev = maps[0].device
        L, nf = len(level_hw), len(fams)
        m = {f"{k}{l}": maps[l * nf + i].detach() for l in range(L) for i, k in enumerate(fams)}
        box3d, nusc = not model.only_box2d, E.model_is_nusc(model)
        a = hip.LossArgs()
        strides = [s.stride for s in model.backbone_output_shape]
        nloc = E._fill_common(a, model.cfg, model, level_hw, strides, B, st.max_gt)
        keep = []
        for l in range(L):
            cl, a.cls_pitch = _pack_nhwc([m[f"logits{l}"]] + ([m[f"attr{l}"], m[f"speed{l}"]] if nusc else []))
            b2, a.b2d_pitch = _pack_nhwc([m[f"box2d_reg{l}"], m[f"centerness{l}"]])
            a.cls[l], a.box2d[l] = cl.data_ptr(), b2.data_ptr()
            keep += [cl, b2]
            if box3d:
                b3, a.b3d_pitch = _pack_nhwc([m[f"{k}{l}"] for k in E.HEAD_KEYS_3D])
                a.box3d[l] = b3.data_ptr()
                keep.append(b3)
        A = E.num_attributes(model)
        a.attr_off, a.num_attr, a.speed_off = (int(model.num_classes), A, int(model.num_classes) + A) if nusc else (0, 0, -1)
        locs = torch.cat([E.feature_locations(h, w, strides[l], model.feature_locations_offset) for l, (h, w) in enumerate(level_hw)]).to(dev)
        iK = st.inv_K.detach().to(dev, torch.float32).reshape(B, 9).contiguous()
        off, recs = E.pack_gt(st.gt, st.max_gt, box3d, nusc, A, int(model.num_classes))
        g_off = torch.from_numpy(off).to(dev)
        g = torch.from_numpy(recs).to(dev) if recs.shape[0] else torch.zeros((1, hip.LOSS_GT_FIELDS), dtype=torch.float32, device=dev)
        a.locations, a.inv_K, a.gt_off, a.gt = locs.data_ptr(), iK.data_ptr(), g_off.data_ptr(), g.data_ptr()
        if box3d:
            canon = torch.tensor([list(r) for r in model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES], dtype=torch.float32, device=dev)
            a.canon_sizes = canon.data_ptr()
            keep.append(canon)
        targets = E._Targets(a, B * nloc, box3d, nusc, dev)
        nb = (B * nloc + hip.LOSS_BLOCK - 1) // hip.LOSS_BLOCK
        partials = torch.zeros((nb, hip.LOSS_TERMS), dtype=torch.float32, device=dev)
        out = torch.zeros(hip.LOSS_OUT, dtype=torch.float32, device=dev)
        npos = torch.zeros(1, dtype=torch.int32, device=dev)
        a.partials, a.n_partials, a.out, a.num_pos = partials.data_ptr(), nb, out.data_ptr(), npos.data_ptr()
        lib = hip.lib()
        hip.check(lib.dd3d_loss_assign(C.byref(a), hip.current_stream()), "loss_assign")
        hip.check(lib.dd3d_loss_terms(C.byref(a), hip.current_stream()), "loss_terms")
        st.num_pos = int(npos.cpu())  # the one read-back: it decides the key order of the dict
        st.args, st.keep = a, keep + [locs, iK, g_off, g, targets, partials, out, npos]
        st.pitches = (a.cls_pitch, a.b2d_pitch, a.b3d_pitch)
        ctx.st = st
        return out.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        st = ctx.st
        a, model, level_hw, B = st.args, st.model, st.level_hw, st.B
        dev = grad_out.device
        box3d, nusc = not model.only_box2d, E.model_is_nusc(model)
        up = grad_out.detach().to(torch.float32).contiguous()
        # every channel below the pitch is written by the kernel; the pad words are never read back
        mk = lambda pitch: [torch.empty((B, h, w, pitch), dtype=torch.float32, device=dev) for h, w in level_hw]
        d_cls, d_b2d = mk(st.pitches[0]), mk(st.pitches[1])
        d_b3d = mk(st.pitches[2]) if box3d else None
        denoms = torch.empty(hip.LOSS_GRAD_DENOMS, dtype=torch.float32, device=dev)
        g = E.fill_grad_args(d_cls, d_b2d, d_b3d, up, denoms)
        hip.check(hip.lib().dd3d_loss_backward(C.byref(a), C.byref(g), hip.current_stream()), "loss_backward")
        grads = E.unpack_head_grads(d_cls, d_b2d, d_b3d, int(model.num_classes), a.num_attr if nusc else 0, bool(a.class_agnostic_3d))
        return (None, ) + tuple(grads[f"{k}{l}"] for l in range(len(level_hw)) for k in st.families)


class FusedDD3DLoss:
    """`model`: a dd3d_amd DD3D / NuscenesDD3D (its config gives the loss settings, the strides and the class counts; its weights are
    not used).  Call with the head maps, the images' K^-1 (B, 3, 3) and the per-image ground-truth Instances."""
    def __init__(self, model, max_gt=hip.LOSS_MAX_GT):
        E.check_loss_config(model.cfg)
        self.model, self.max_gt = model, int(max_gt)

    def __call__(self, head_maps, inv_K, gt_instances):
        model = self.model
        fams, level_hw, B = check_head_maps(model, head_maps)
        inv_K = torch.as_tensor(inv_K)
        if inv_K.numel() != 9 * B:
            raise ValueError(f"inv_K has {inv_K.numel()} elements for {B} images; expected (B, 3, 3)")
        if len(gt_instances) != B:
            raise ValueError(f"{len(gt_instances)} GT instances for head maps of {B} images")
        st = _State()
        st.model, st.families, st.level_hw, st.B, st.max_gt, st.inv_K, st.gt = model, fams, level_hw, B, self.max_gt, inv_K, list(gt_instances)
        out = _FusedLossFn.apply(st, *[head_maps[f"{k}{l}"] for l in range(len(level_hw)) for k in fams])
        keys = E.loss_keys(not model.only_box2d, E.model_is_nusc(model), st.num_pos)
        return {k: out[E.OUT_INDEX[k]] for k in keys}


def check_dense_depth_maps(model, dense_depth_maps, device_type="cuda"):
    """Level count, device, dtype and shapes of the per-level (B, 1, h, w) maps against the model's strides; returns (B, Hp, Wp).
    `device_type`: where the maps must live (the kernels run on the HIP device only; the tests check the other rules on CPU tensors)."""
    strides = [int(s.stride) for s in model.backbone_output_shape]
    if not isinstance(dense_depth_maps, (list, tuple)):
        raise ValueError("dense_depth_maps must be the per-level list of (B, 1, h, w) tensors")
    if len(dense_depth_maps) != len(strides):
        raise ValueError(f"dense_depth_maps has {len(dense_depth_maps)} levels; the model has {len(strides)} (strides {strides})")
    B = Hp = Wp = None
    for l, (t, s) in enumerate(zip(dense_depth_maps, strides)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4 or t.shape[1] != 1:
            raise ValueError(f"dense_depth_maps[{l}] must be a (B, 1, h, w) tensor" + (f", got shape {tuple(t.shape)}" if isinstance(t, torch.Tensor) else ""))
        if t.device.type != device_type:
            raise ValueError(f"dense_depth_maps[{l}] is on {t.device}: the fused loss runs on the HIP device only")
        if t.dtype != torch.float32:
            raise ValueError(f"dense_depth_maps[{l}] is {t.dtype}; float32 expected")
        if B is None:
            B, Hp, Wp = int(t.shape[0]), int(t.shape[2]) * s, int(t.shape[3]) * s
            if Wp % 4:
                raise ValueError(f"dense_depth_maps[0] gives a canvas {Wp} wide; the width must be a multiple of 4")
        if int(t.shape[0]) != B or int(t.shape[2]) * s != Hp or int(t.shape[3]) * s != Wp:
            raise ValueError(f"dense_depth_maps[{l}] has shape {tuple(t.shape)} at stride {s}: it does not tile the {B} x {Hp} x {Wp} canvas of level 0")
    return B, Hp, Wp


class _FusedDenseDepthLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, st, *maps):
        from dd3d_amd.engine import dense_depth_loss as D
        model, B, Hp, Wp = st.model, st.B, st.Hp, st.Wp
        dev, L = maps[0].device, len(maps)
        weight, beta, min_depth, max_depth = D.dense_depth_loss_config(model.cfg)
        lib = hip.lib()
        raw = [m.detach().contiguous() for m in maps]  # (B, 1, h, w) contiguous IS the kernel's NHWC layout at pitch 1
        a = hip.DenseDepthLossArgs()
        for l, (r, s) in enumerate(zip(raw, model.backbone_output_shape)):
            a.raw[l], a.h[l], a.w[l], a.stride[l] = r.data_ptr(), int(r.shape[2]), int(r.shape[3]), int(s.stride)
        for l, d in enumerate(D.level_divisors(L)):
            a.divisor[l] = d
        canvas = D.stage_depth_canvas(torch.empty((B, Hp, Wp), dtype=torch.float32, device=dev), st.depths, [tuple(d.shape) for d in st.depths], checked=True)
        keep = raw + [canvas]
        if model.scale_depth_by_focal_lengths:
            K = st.intrinsics.detach().to(dev, torch.float32).reshape(B, 9).contiguous()
            inv_K = torch.empty_like(K)
            hip.check(lib.dd3d_invert_intrinsics(K.data_ptr(), inv_K.data_ptr(), B, hip.current_stream()), "invert_intrinsics")
            a.inv_K, a.focal_factor = inv_K.data_ptr(), float(model.scale_depth_by_focal_lengths_factor)
            keep += [K, inv_K]
        nb = hip.dense_depth_loss_blocks(B, Hp, Wp)
        partials = torch.empty((nb, hip.DDL_ROW), dtype=torch.float32, device=dev)
        out = torch.empty(L, dtype=torch.float32, device=dev)
        count = torch.empty(1, dtype=torch.int64, device=dev)
        a.gt, a.partials, a.n_partials, a.out, a.count = canvas.data_ptr(), partials.data_ptr(), nb, out.data_ptr(), count.data_ptr()
        a.num_levels, a.B, a.Hp, a.Wp, a.pitch = L, B, Hp, Wp, 1
        a.offset_half = int(model.feature_locations_offset == "half")
        a.min_depth, a.max_depth, a.beta, a.loss_weight = min_depth, max_depth, beta, weight
        st.grad_rows = hip.dense_depth_grad_rows(a)  # (host only: a geometry the gradient cannot take raises here, before the launch)
        hip.check(lib.dd3d_dense_depth_loss(C.byref(a), hip.current_stream()), "dense_depth_loss")
        st.args, st.keep = a, keep + [partials, out, count]
        ctx.st = st
        return out.clone()

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        from dd3d_amd.engine.dense_depth_loss import dense_depth_grad_args
        st = ctx.st
        a, dev = st.args, grad_out.device
        up = grad_out.detach().to(torch.float32).contiguous()
        # channel 0 of every pixel is written by the kernel, and at pitch 1 there is no other
        d_raw = [torch.empty_like(r) for r in st.keep[:a.num_levels]]
        slab = torch.empty((st.grad_rows, hip.DDG_ROW), dtype=torch.float32, device=dev)
        g = dense_depth_grad_args(a, d_raw, up, slab)
        hip.check(hip.lib().dd3d_dense_depth_loss_backward(C.byref(a), C.byref(g), hip.current_stream()), "dense_depth_loss_backward")
        return (None, ) + tuple(d_raw)


class FusedDenseDepthLoss:
    """`model`: a dd3d_amd DD3DDenseDepth (its config gives the loss settings, the strides, the location offset and the focal scaling; its
    weights are not used).  Call with the head's per-level (B, 1, h, w) float32 maps (the reference's `dense_depth_lvl` list, after Scale
    and Offset), the images' intrinsics (B, 3, 3) -- None when SCALE_DEPTH_BY_FOCAL_LENGTHS is off -- and the per-image ground-truth depth
    maps (Hi, Wi), 0 = no return.  Returns the reference's dict `loss_dense_depth_lvl_<l>` of 0-d tensors that carry the gradient."""
    def __init__(self, model):
        from dd3d_amd.engine.dense_depth_loss import dense_depth_loss_config
        dense_depth_loss_config(model.cfg)
        self.model = model

    def __call__(self, dense_depth_maps, intrinsics, depths):
        from dd3d_amd.engine.dense_depth_loss import check_depth_maps
        model = self.model
        B, Hp, Wp = check_dense_depth_maps(model, dense_depth_maps)
        if model.scale_depth_by_focal_lengths:
            if intrinsics is None:
                raise ValueError("intrinsics is None: SCALE_DEPTH_BY_FOCAL_LENGTHS needs the (B, 3, 3) intrinsics")
            intrinsics = torch.as_tensor(intrinsics)
            if tuple(intrinsics.shape) != (B, 3, 3):
                raise ValueError(f"intrinsics has shape {tuple(intrinsics.shape)} for {B} images; expected ({B}, 3, 3)")
        depths = list(depths)
        if len(depths) != B:
            raise ValueError(f"{len(depths)} depth maps for dense_depth_maps of {B} images")
        for i, d in enumerate(depths):
            if not isinstance(d, torch.Tensor) or d.dim() != 2:
                raise ValueError(f"image {i}: 'depth' must be an (Hi, Wi) floating-point tensor")
            if d.shape[0] > Hp or d.shape[1] > Wp:
                raise ValueError(f"image {i}: its depth map {tuple(d.shape)} does not fit the {Hp} x {Wp} canvas of the maps")
        check_depth_maps(depths, [tuple(d.shape) for d in depths])
        st = _State()
        st.model, st.B, st.Hp, st.Wp, st.intrinsics, st.depths = model, B, Hp, Wp, intrinsics, depths
        out = _FusedDenseDepthLossFn.apply(st, *dense_depth_maps)
        return {f"loss_dense_depth_lvl_{l}": out[l] for l in range(len(dense_depth_maps))}
