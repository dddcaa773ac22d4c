"""CPU oracle of the predictor layer's backward (csrc/predictor_grads.hip, include/dd3d_hip.h::dd3d_pred_grad_args): the forward of one
predictor group as a torch composition,

    map_l = clamp_lo((conv3x3(a_l, W_l) + b_l) * s_l + o_l)

contracted with a constant head-map gradient G_l through the explicit mask [stored map_l > lo] (the stored map decides, not a
recomputation), and differentiated by autograd in float64 or float32.  Everything is NCHW here; `w[l]` is the SAME tensor object on the
levels that share a module.  The acceptance bound of a family is loss_grad_oracle.bar: 8 * max(d32, 2^-23 * max|g64|).
"""
import re

import torch
import torch.nn.functional as F

from tests.loss_grad_oracle import bar  # noqa: F401  (the project's one rule for a gradient's tolerance)

MAX_SLOTS = 8
FAMILIES = ("weight", "bias", "scale", "offset", "da")


def masked(g, maps, lo):
    """g_l: G_l where the channel is not clamped or its stored map lies above the clamp; exact zeros elsewhere."""
    if lo is None:
        return list(g)
    fin = torch.isfinite(lo)[None, :, None, None]
    return [torch.where(fin & ~(m > lo[None, :, None, None].to(m.dtype)), torch.zeros_like(x), x) for x, m in zip(g, maps)]


def forward(act, w, bias, scale, offset, lo):
    """The head maps of a group, per level (what ForwardPlan._heads folds into one launch)."""
    out = []
    for l, a in enumerate(act):
        y = (F.conv2d(a, w[l], padding=1) + bias[l][None, :, None, None]) * scale[l][None, :, None, None] + offset[l][None, :, None, None]
        if lo is not None:
            y = torch.maximum(y, lo[None, :, None, None].to(y.dtype))
        out.append(y)
    return out


def owners(w):
    return [l for l in range(len(w)) if all(w[m] is not w[l] for m in range(l))]


def group_grads(act, g, maps, w, bias, scale, lo=None, slot=None, dtype=torch.float64):
    """Gradients of sum_l <g_l, (conv3x3(a_l, W_l) + b_l) * s_l + o_l> in `dtype`.  Returns a dict:
      dw_level [L] (n, Cin, 3, 3) unscaled per-level partial;  q, r [L] (n);  dw, db {first level of a module: tensor};
      dscale, doffset (L, MAX_SLOTS): sums of r / q over the channels of a slot;  da [L] (B, Cin, H, W)."""
    L = len(act)
    gm = [x.to(dtype) for x in masked(g, maps, lo)]
    own = owners(w)
    owner_of = [next(o for o in own if w[o] is w[l]) for l in range(L)]
    A = [a.detach().to(dtype).requires_grad_(True) for a in act]
    Wm = {o: w[o].detach().to(dtype).requires_grad_(True) for o in own}
    Bm = {o: bias[o].detach().to(dtype).requires_grad_(True) for o in own}
    S = [s.detach().to(dtype).requires_grad_(True) for s in scale]
    O = [torch.zeros_like(s).requires_grad_(True) for s in S]
    total = 0
    for l in range(L):
        y = (F.conv2d(A[l], Wm[owner_of[l]], padding=1) + Bm[owner_of[l]][None, :, None, None]) * S[l][None, :, None, None] + O[l][None, :, None, None]
        total = total + (y * gm[l]).sum()
    total.backward()
    # the unscaled per-level partial: the same contraction with per-level copies of the filter and no scale
    Wl = [w[l].detach().to(dtype).requires_grad_(True) for l in range(L)]
    sum((F.conv2d(act[l].detach().to(dtype), Wl[l], padding=1) * gm[l]).sum() for l in range(L)).backward()
    n = w[0].shape[0]
    res = {"dw_level": [x.grad for x in Wl], "q": [o.grad for o in O], "r": [s.grad for s in S], "dw": {o: Wm[o].grad for o in own},
           "db": {o: Bm[o].grad for o in own}, "da": [a.grad for a in A]}
    ds, do = torch.zeros((L, MAX_SLOTS), dtype=dtype), torch.zeros((L, MAX_SLOTS), dtype=dtype)
    if slot is not None:
        for j in range(MAX_SLOTS):
            sel = slot == j
            if bool(sel.any()):
                for l in range(L):
                    ds[l, j], do[l, j] = S[l].grad[sel].sum(), O[l].grad[sel].sum()
    res["dscale"], res["doffset"] = ds, do
    assert all(x.shape[0] == n for x in res["q"])
    return res


def family_vectors(res, slot=None):
    """The families of the acceptance rule as flat vectors: weight (per-level partials and the module sums), bias (q and db), scale (r
    and the slot sums), offset, and the towers' da."""
    cat = lambda xs: torch.cat([x.reshape(-1) for x in xs]) if len(xs) else torch.zeros(0)
    return {
        "weight": cat(list(res["dw_level"]) + [res["dw"][o] for o in sorted(res["dw"])]),
        "bias": cat(list(res["q"]) + [res["db"][o] for o in sorted(res["db"])]),
        "scale": cat(list(res["r"]) + [res["dscale"]]),
        "offset": cat([res["doffset"]]),
        "da": cat(res["da"]),
    }


# ------------------------------------------------------------------------------------------ the model's own modules, by parameter name
PREDICTOR_PARAM = re.compile(r"^(fcos2d_head\.(cls_logits|box2d_reg|centerness|scales_box2d_reg\.\d+)|"
                             r"fcos3d_head\.(box3d_(quat|ctr|depth|size|conf)\.\d+|scales_(proj_ctr|depth|size|conf)\.\d+|offsets_depth\.\d+)|"
                             r"attr_logits|speed)\.(weight|bias|scale)$")


def predictor_param_names(model):
    """The named_parameters() of the predictor layer: the 3x3 predictors and their per-level Scale / Offset."""
    return sorted(k for k, _ in model.named_parameters() if PREDICTOR_PARAM.match(k))


def model_grads(model, towers, G, maps, dtype=torch.float64):
    """The predictors of `model` applied module by module as the reference's heads apply them (fcos2d.py:143-152, fcos3d.py:175-180,
    nuscenes_dd3d.py:371-374), contracted with the head-map gradients G (keys of DD3D.compute_losses' grads; ReLU outputs through the
    mask of the stored `maps`) and differentiated.  towers: {"cls" | "box2d" | "box3d": per-level NCHW}.  Returns
    ({parameter name: gradient}, {<tower>_tower_out<l>: gradient})."""
    P = {k: p.detach().to(dtype).requires_grad_(True) for k, p in model.named_parameters() if PREDICTOR_PARAM.match(k)}
    T = {t: [a.detach().to(dtype).requires_grad_(True) for a in acts] for t, acts in towers.items()}
    conv = lambda x, name: F.conv2d(x, P[name + ".weight"], P.get(name + ".bias"), padding=1)
    g = lambda k: G[k].to(dtype)
    relu_mask = lambda k: (maps[k] > 0).to(dtype)
    h2 = model.fcos2d_head
    total = 0
    for l in range(len(T["cls"])):
        x = T["cls"][l]
        total = total + (conv(x, "fcos2d_head.cls_logits") * g(f"logits{l}")).sum()
        if hasattr(model, "attr_logits"):
            total = total + (conv(x, "attr_logits") * g(f"attr{l}")).sum() + (conv(x, "speed") * g(f"speed{l}") * relu_mask(f"speed{l}")).sum()
        x = T["box2d"][l]
        reg = conv(x, "fcos2d_head.box2d_reg")
        if h2.use_scale:
            reg = reg * P[f"fcos2d_head.scales_box2d_reg.{l}.scale"]
        total = total + (reg * g(f"box2d_reg{l}") * relu_mask(f"box2d_reg{l}")).sum() + (conv(x, "fcos2d_head.centerness") * g(f"centerness{l}")).sum()
        if not model.only_box2d:
            h3 = model.fcos3d_head
            x, i = T["box3d"][l], (l if h3.use_per_level_predictors else 0)
            sc = (lambda y, name: y * P[f"fcos3d_head.scales_{name}.{l}.scale"]) if h3.use_scale else (lambda y, name: y)
            depth = sc(conv(x, f"fcos3d_head.box3d_depth.{i}"), "depth")
            if h3.use_scale:
                depth = depth + P[f"fcos3d_head.offsets_depth.{l}.bias"]
            total = total + (conv(x, f"fcos3d_head.box3d_quat.{i}") * g(f"quat{l}")).sum() + (sc(conv(x, f"fcos3d_head.box3d_ctr.{i}"), "proj_ctr") * g(f"ctr{l}")).sum() \
                + (depth * g(f"depth{l}")).sum() + (sc(conv(x, f"fcos3d_head.box3d_size.{i}"), "size") * g(f"size{l}")).sum() \
                + (sc(conv(x, f"fcos3d_head.box3d_conf.{i}"), "conf") * g(f"conf{l}")).sum()
    total.backward()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    return {k: zero(p) for k, p in P.items()}, {f"{t}_tower_out{l}": zero(a) for t, acts in T.items() for l, a in enumerate(acts)}
