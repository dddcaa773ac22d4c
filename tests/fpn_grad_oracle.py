"""CPU oracle of the FPN backward (tests/test_fpn_grads.py, tests/test_fpn_grads_gpu.py).

Two statements of the same gradients:
  * `autograd_grads`: torch autograd through oracle.dd3d_oracle.fpn_forward (the forward the goldens pin to the reference) with the
    backbone features and the FPN parameters as leaves.  The only restatement: relu(p6) is p6 * [stored p6 > 0], so that the P7 mask
    comes from a GIVEN stored p6 (`forward`; with no stored p6 it is relu(p6) itself, tested against fpn_forward).
  * `layer_grads` / `chain_grads`: the table of include/dd3d_hip.h layer by layer on STORED activations (what the kernels linearise at),
    in float64 or float32.  With the forward's own activations the two agree to float64 rounding.
The bar is the project's: 8 * max(d32, 2^-23 * max|g64|) (loss_grad_oracle.bar)."""
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from oracle import dd3d_oracle as O
from tests.loss_grad_oracle import bar  # noqa: F401

PREFIX = "backbone"


def spec(model):
    """(in_features, their strides, top block "p6p7" / "p6" / None) of a model's FPN."""
    fpn = model.backbone
    top = None if fpn.top_block is None else ("p6p7" if fpn.top_block.num_levels == 2 else "p6")
    return list(fpn.in_features), [2**s for s in fpn.stages], top


def stages_of(sp):
    return [int(s).bit_length() - 1 for s in sp[1]]


def fpn_param_names(model):
    return sorted(k for k, _ in model.named_parameters() if k.startswith(PREFIX + ".") and not k.startswith(PREFIX + ".bottom_up."))


def family_of(name):
    if ".norm." in name:
        return "norm_weight" if name.endswith(".weight") else "bias"
    return "filter" if name.endswith(".weight") else "bias"


def forward(sd, feats, sp, p6_stored=None):
    """fpn_forward, with the input of P7 stated as p6 * [p6_stored > 0] (p6_stored None: the forward's own p6, i.e. relu(p6))."""
    names, strides, top = sp
    out = O.fpn_forward(sd, feats, names, strides, top_block="p6" if top else None, prefix=PREFIX)
    if top == "p6p7":
        st = stages_of(sp)[-1]
        p6 = out[f"p{st + 1}"]
        m = ((p6 if p6_stored is None else p6_stored) > 0).to(p6.dtype)
        out[f"p{st + 2}"] = O.conv2d(sd, f"{PREFIX}.top_block.p7", p6 * m, stride=2, padding=1)
    return out


def stored_activations(sd, feats, sp):
    """What the plan stores of a forward: {"t": {stage: top-down sum}, "p": {stage: FPN output}} (own statement of the top-down path)."""
    names, _, top = sp
    stages = stages_of(sp)
    norm = lambda c: f"{c}.norm" if f"{c}.norm.weight" in sd else None
    t, p, prev = {}, {}, None
    for idx in reversed(range(len(names))):
        s = stages[idx]
        lat = O.conv2d(sd, f"{PREFIX}.fpn_lateral{s}", feats[names[idx]], norm=norm(f"{PREFIX}.fpn_lateral{s}"))
        if prev is not None:
            lat = lat + prev.repeat_interleave(2, 2).repeat_interleave(2, 3)
        t[s] = prev = lat
        p[s] = O.conv2d(sd, f"{PREFIX}.fpn_output{s}", lat, padding=1, norm=norm(f"{PREFIX}.fpn_output{s}"))
    if top:
        p[stages[-1] + 1] = O.conv2d(sd, f"{PREFIX}.top_block.p6", p[stages[-1]], stride=2, padding=1)
        if top == "p6p7":
            p[stages[-1] + 2] = O.conv2d(sd, f"{PREFIX}.top_block.p7", F.relu(p[stages[-1] + 1]), stride=2, padding=1)
    return {"t": t, "p": p}


def autograd_grads(sd, feats, sp, G, dtype, leaves, p6_stored=None):
    """d sum_k <G[k], p_k> / d (parameters `leaves`, backbone features) by autograd in `dtype`: ({name: grad}, {backbone_<name>: grad})."""
    P = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in sd.items() if k.startswith(PREFIX + ".") and ".bottom_up." not in k}
    for k in leaves:
        P[k].requires_grad_(True)
    X = {n: f.detach().to(dtype).requires_grad_(True) for n, f in feats.items()}
    out = forward(P, X, sp, p6_stored)
    total = sum((out[k] * G[k].to(dtype)).sum() for k in G)
    total.backward()
    return {k: P[k].grad for k in leaves}, {f"backbone_{n}": X[n].grad for n in X}


def pool2x2sum(v, t):
    """v + the four children of each pixel on the finer tensor t, added row by row, left before right (the kernel's order)."""
    return (((v + t[:, :, 0::2, 0::2]) + t[:, :, 0::2, 1::2]) + t[:, :, 1::2, 0::2]) + t[:, :, 1::2, 1::2]


def layer_grads(x, g, w, scale, stride, dtype=torch.float64, in_relu=False, mask=None, add=None, pool=None):
    """One convolution of the table on stored tensors (NCHW): dw_level (P), dw, q, r and da with its epilogue (mask, + add, + pool)."""
    k = w.shape[-1]
    pad = (k - 1) // 2
    X, Gd, W, s = x.to(dtype), g.to(dtype), w.to(dtype), scale.to(dtype)
    Xw = F.relu(X) if in_relu else X
    P = conv2d_weight(Xw, W.shape, Gd, stride=stride, padding=pad)
    da = conv2d_input(X.shape, W, Gd * s[None, :, None, None], stride=stride, padding=pad)
    if mask is not None:
        da = da * (mask > 0).to(dtype)
    if add is not None:
        da = da + add.to(dtype)
    if pool is not None:
        da = pool2x2sum(da, pool.to(dtype))
    return {"dw_level": P, "dw": s[:, None, None, None] * P, "q": Gd.sum((0, 2, 3)), "r": (P * W).sum((1, 2, 3)), "da": da}


def family_vectors(res):
    """Flat vectors per family of one or several layer results: filter (dw and the unscaled P), bias (q), norm_weight (r), input (da)."""
    rs = res if isinstance(res, (list, tuple)) else [res]
    cat = lambda ks: torch.cat([r[k].reshape(-1) for r in rs for k in ks])
    return {"filter": cat(("dw", "dw_level")), "bias": cat(("q", )), "norm_weight": cat(("r", )), "input": cat(("da", ))}


def fold_scale(conv, dtype):
    """a of layers.fold_norm in `dtype`: w * rsqrt(var + eps) of the convolution's norm on running statistics, ones without one."""
    n = getattr(conv, "norm", None)
    if n is None:
        return torch.ones(conv.out_channels, dtype=dtype)
    return n.weight.detach().to(dtype) * torch.rsqrt(n.running_var.to(dtype) + n.eps)


def read_out(conv, scale, q, r, dtype):
    """Gradients of the per-channel parameters from q = sum g and r = sum g * conv: y = (conv + b - mean) * w * rstd + beta."""
    n, out = getattr(conv, "norm", None), {}
    b = conv.bias.detach().to(dtype) if conv.bias is not None else None
    if n is not None and isinstance(n.weight, torch.nn.Parameter):
        centre = (0 if b is None else b) - n.running_mean.to(dtype)
        out["norm.weight"] = torch.rsqrt(n.running_var.to(dtype) + n.eps) * (r + centre * q)
        out["norm.bias"] = q.clone()
    if b is not None:
        out["bias"] = scale * q if n is not None else q.clone()
    return out


def chain_grads(model, stored, feats, G, dtype):
    """The whole table on stored activations: `stored` = {"t": {stage: t_s}, "p": {stage: p_s}} (p of the coarsest stage and p6 are
    read), `feats` {name: f}, `G` {p<s>: gradient; missing = zero}.  Returns ({parameter name: grad}, {backbone_<name>: grad},
    {layer key: layer_grads result}), the read-out (`read_out`) in `dtype` throughout."""
    fpn = model.backbone
    names, stages = list(fpn.in_features), list(fpn.stages)
    pnames = {id(p): k for k, p in model.named_parameters()}
    params, raw = {}, {}

    def run(key, conv, x, g, stride, **kw):
        scale = fold_scale(conv, dtype)
        res = layer_grads(x, g, conv.weight.detach(), scale, stride, dtype, **kw)
        raw[key] = res
        params[pnames[id(conv.weight)]] = res["dw"]
        norm = getattr(conv, "norm", None)
        got = read_out(conv, scale, res["q"], res["r"], dtype)
        for k, p in (("norm.weight", getattr(norm, "weight", None)), ("norm.bias", getattr(norm, "bias", None)), ("bias", conv.bias)):
            if k in got and id(p) in pnames:
                params[pnames[id(p)]] = got[k]
        return res["da"]

    zero = lambda st: torch.zeros_like(stored["p"][st]).to(dtype)
    Gof = lambda st: G[f"p{st}"].to(dtype) if f"p{st}" in G else zero(st)
    s5 = stages[-1]
    D = Gof(s5)
    if fpn.top_block is not None:
        D6 = Gof(s5 + 1)
        if fpn.top_block.num_levels == 2:
            p6 = stored["p"][s5 + 1]
            D6 = run("top_block.p7", fpn.top_block.p7, p6, G[f"p{s5 + 2}"] if f"p{s5 + 2}" in G else torch.zeros_like(stored["p"][s5 + 2]), 2,
                     in_relu=True, mask=p6, add=D6)
        D = run("top_block.p6", fpn.top_block.p6, stored["p"][s5], D6, 2, add=D)
    T = {}
    for i, s in enumerate(stages):
        T[s] = run(f"output{s}", getattr(fpn, f"fpn_output{s}"), stored["t"][s], D if s == s5 else Gof(s), 1, pool=T[stages[i - 1]] if i else None)
    fg = {}
    for i in reversed(range(len(stages))):
        fg[f"backbone_{names[i]}"] = run(f"lateral{stages[i]}", getattr(fpn, f"fpn_lateral{stages[i]}"), feats[names[i]], T[stages[i]], 1)
    return params, fg, raw
