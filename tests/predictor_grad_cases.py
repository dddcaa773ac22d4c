"""Seeded inputs of the predictor-backward tests (tests/test_predictor_grads.py, tests/test_predictor_grads_gpu.py): one predictor
group on a list of levels, with clamped channels whose stored maps hold exact zeros, Scale slots, optional per-level filters, a level
whose scale is 0 and dense or sparse head-map gradients; and the split-plane encodings of an activation tensor with the values they
decode to."""
import torch

from tests import predictor_grad_oracle as PO

PYRAMID_64x128 = [(8, 16), (4, 8), (2, 4), (1, 2), (1, 1)]


class GroupCase:
    """act, g, maps: per-level NCHW float32; w: per-level (n, Cin, 3, 3), one object where shared; bias, scale: per-level (n);
    lo: (n) with 0 on the clamped channels and -inf elsewhere, or None; slot: int32 (n)."""
    def __init__(self, level_hw, B, n, Cin, seed=0, per_level=False, zero_scale_level=None, clamp=True, sparse=False, positives=True):
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=gen)
        L = len(level_hw)
        self.level_hw, self.B, self.n, self.Cin, self.L = list(level_hw), B, n, Cin, L
        self.act = [rnd(B, Cin, h, w) for h, w in level_hw]
        shared = rnd(n, Cin, 3, 3) * 0.1
        self.w = [rnd(n, Cin, 3, 3) * 0.1 for _ in range(L)] if per_level else [shared] * L
        sb = rnd(n) * 0.1
        self.bias = [rnd(n) * 0.1 for _ in range(L)] if per_level else [sb] * L
        # channels cycle through: no slot, slot 0, slot 1; each (level, slot) has its own Scale value
        self.slot = (torch.arange(n, dtype=torch.int32) % 3) - 1
        sval = 0.5 + torch.rand(L, 2, generator=gen)
        if zero_scale_level is not None:
            sval[zero_scale_level] = 0.0
        self.scale = [torch.where(self.slot >= 0, sval[l][self.slot.clamp(min=0).long()], torch.ones(n)) for l in range(L)]
        self.offset = [torch.where(self.slot == 1, rnd(1).expand(n), torch.zeros(n)) for _ in range(L)]
        self.lo = torch.where(torch.arange(n) % 4 == 0, torch.zeros(n), torch.full((n, ), -float("inf"))) if clamp else None
        self.maps = PO.forward(self.act, self.w, self.bias, self.scale, self.offset, self.lo)  # stored float32 maps: exact zeros on the clamp
        self.g = [rnd(B, n, h, w) for h, w in level_hw]
        if sparse:  # a few rows only, as the box2d / box3d families are off the positives
            for l, (h, w) in enumerate(level_hw):
                keep = torch.zeros(B, 1, h, w)
                if positives:
                    keep.view(-1)[torch.randint(0, B * h * w, (max(1, B * h * w // 16), ), generator=gen)] = 1.0
                self.g[l] = self.g[l] * keep

    def ref(self, dtype=torch.float64, act=None):
        return PO.group_grads(self.act if act is None else act, self.g, self.maps, self.w, self.bias, self.scale, self.lo, self.slot, dtype)


def encode_f16x2(x, plane_scale):
    """NCHW float32 -> (planes int16 [C/32][B*H*W][2][32] of halves of value * plane_scale, split as csrc/conv_common.h::split_pack
    splits, the float32 NCHW values the planes decode to)."""
    B, C, H, W = x.shape
    y = x.permute(0, 2, 3, 1).reshape(-1, C) * plane_scale
    hi = y.to(torch.float16)
    lo = (y - hi.float()).to(torch.float16)
    dec64 = (hi.double() + lo.double()) / plane_scale
    dec = dec64.float()
    assert torch.equal(dec.double(), dec64)  # the decoded value is a float32
    planes = torch.stack([hi.view(torch.int16), lo.view(torch.int16)], 0).view(2, B * H * W, C // 32, 32).permute(2, 1, 0, 3).contiguous()
    return planes, dec.view(B, H, W, C).permute(0, 3, 1, 2).contiguous()


def encode_bf16x3(x):
    """NCHW float32 -> (planes int16 [C/32][B*H*W][3][32] of the exact three-term bf16 split, the values they decode to: x itself)."""
    from dd3d_amd.engine.packing import split_bf16x3
    B, C, H, W = x.shape
    y = x.permute(0, 2, 3, 1).reshape(-1, C).contiguous()
    planes = split_bf16x3(y).permute(1, 0, 2, 3).contiguous()  # [pixel][C/32][3][32] -> [C/32][pixel][3][32]
    t = (planes.to(torch.int32) << 16).view(torch.float32)
    dec = ((t[:, :, 0] + t[:, :, 1]) + t[:, :, 2]).permute(1, 0, 2).reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous()
    return planes, dec


# ------------------------------------------------------------------ the reference-modules golden (tests/golden/make_predictor_grad_golden.py)
REFERENCE_CASES = {"kitti_b2": ("dd3d_kitti_dla34", "dla34_kitti", 2, "kitti"), "nusc_b2": ("dd3d_nusc_dla34", "dla34_nusc", 2, "nusc")}
REFERENCE_CANVAS = (64, 128)
SAMPLE_CAP = 8192  # stored entries per tensor: keeps a fixture well below the size limit of a committed file


def tower_sample(shape, cap=SAMPLE_CAP):
    """Seeded flat indices into a tensor of `shape` (all of them, in order, when it has at most `cap` entries)."""
    numel = 1
    for s in shape:
        numel *= int(s)
    if numel <= cap:
        return torch.arange(numel)
    return torch.randperm(numel, generator=torch.Generator().manual_seed(numel))[:cap].sort().values


def reference_inputs(name):
    """(synthetic state dict, seeded FPN features per level, batched inputs, ground truth) of a reference case."""
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import META_ARCH_REGISTRY, get_cfg
    from dd3d_amd.synthetic import load_calib, make_gt_instances, make_inputs, make_state_dict
    exp, tag, B, ds = REFERENCE_CASES[name]
    cfg = get_cfg(exp)
    model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
    sd = make_state_dict(model, calib=load_calib(tag))
    gen = torch.Generator().manual_seed(77)
    feats = [torch.randn(B, 256, h, w, generator=gen) for h, w in PYRAMID_64x128]
    inputs = make_inputs(B, *REFERENCE_CANVAS, dataset=ds)
    gt = make_gt_instances(inputs, model.num_classes, cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, n_per_image=8,
                           num_attributes=model.attr_logits.out_channels if hasattr(model, "attr_logits") else None)
    return sd, feats, inputs, gt


def reference_chain(name):
    """The golden's inputs pushed through the project's own CPU statements: the towers and predictors of oracle/dd3d_oracle.py on the
    seeded features, then the loss oracle's head-map gradients.  Returns (cpu model with the state dict loaded, towers {name: per-level
    NCHW}, head maps, the loss_grad_cases.Case that differentiates the losses)."""
    import torch.nn.functional as F
    from oracle import dd3d_oracle as O
    from tests import loss_grad_cases as GC
    exp, tag, B, ds = REFERENCE_CASES[name]
    sd, feats, inputs, gt = reference_inputs(name)
    model = GC.cpu_model(exp)
    model.load_state_dict(sd)
    cfg = model.cfg
    with torch.no_grad():
        c2 = cfg.DD3D.FCOS2D
        logits, reg, ctrn, cls_t = O.fcos2d_head(sd, feats, c2.NUM_CLS_CONVS, num_box_convs=c2.NUM_BOX_CONVS)
        quat, ctr, depth, size, conf = O.fcos3d_head(sd, feats, cfg.DD3D.FCOS3D.NUM_CONVS)
        towers = {"cls": cls_t, "box2d": [O._tower(sd, "fcos2d_head.box2d_tower", f, l, c2.NUM_BOX_CONVS) for l, f in enumerate(feats)],
                  "box3d": [O._tower(sd, "fcos3d_head.box3d_tower", f, l, cfg.DD3D.FCOS3D.NUM_CONVS) for l, f in enumerate(feats)]}
        maps = {}
        for l in range(len(feats)):
            maps.update({f"logits{l}": logits[l], f"box2d_reg{l}": reg[l], f"centerness{l}": ctrn[l], f"quat{l}": quat[l], f"ctr{l}": ctr[l],
                         f"depth{l}": depth[l], f"size{l}": size[l], f"conf{l}": conf[l]})
            if ds == "nusc":
                maps[f"attr{l}"] = O.conv2d(sd, "attr_logits", cls_t[l], padding=1)
                maps[f"speed{l}"] = F.relu(O.conv2d(sd, "speed", cls_t[l], padding=1))
    inv_K = torch.stack([x["intrinsics"] for x in inputs]).float().inverse()
    case = GC.Case(model, maps, gt, PYRAMID_64x128, inv_K)
    return model, towers, maps, case
