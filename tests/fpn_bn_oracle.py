"""CPU oracle of the FPN's batch-statistics BatchNorm (csrc/fpn_bn.hip, engine.LossPlan(fpn_batch_stats=True)): under FE.FPN.NORM: BN
every lateral and output convolution is followed by F.batch_norm(training=True) -- statistics per channel over the B * h_s * w_s pixels of
its own output, as nn.BatchNorm2d computes them in train() -- and the top-down path adds the normalised laterals.

Forward: the oracle's own FPN (oracle.dd3d_oracle.fpn_forward through fpn_grad_oracle.forward) under
whole_model_grad_oracle.intercepted with the FPN norms' weights as batch-statistics leaves.  Backward: torch autograd, in float64 (the
reference) or float32 (whose deviation sets the bar), either through that forward (`autograd_grads`) or layer by layer at STORED
activations (`chain_grads`, in the style of fpn_grad_oracle.chain_grads: what the kernels linearise at).  The whole model: `norms_on`
widens the set of norms whole_model_grad_oracle.whole_model_grads(batch_stats=True) switches to batch statistics.
The bar of a family is loss_grad_oracle.bar: 8 * max(d32, 2^-23 * max|ref64|)."""
import contextlib

import torch
import torch.nn.functional as F

from oracle import dd3d_oracle as O
from tests import fpn_grad_oracle as FO
from tests import tower_bn_oracle as TB
from tests import whole_model_grad_oracle as WO
from tests.loss_grad_oracle import bar  # noqa: F401

EPS = 1e-5
PREFIX = FO.PREFIX


def norm_prefixes(model):
    """State-dict prefixes of the FPN's trainable BatchNorm2d norms: fpn_lateral<s>.norm and fpn_output<s>.norm of every stage."""
    fpn = model.backbone
    out = []
    for kind in ("fpn_lateral", "fpn_output"):
        for s in fpn.stages:
            assert TB.is_batch_norm(getattr(getattr(fpn, f"{kind}{s}"), "norm", None)), f"{kind}{s} has no trainable BatchNorm2d (FE.FPN.NORM: BN)"
            out.append(f"{PREFIX}.{kind}{s}.norm")
    return out


def batch_stats_names(model):
    """The keys of LossPlan.fpn_batch_stats()."""
    return sorted(p + "." + k for p in norm_prefixes(model) for k in ("running_mean", "running_var", "batch_mean", "batch_var"))


def family_of(name):
    """weight / norm_weight / norm_bias of an FPN parameter name (the top block's conv biases: bias)."""
    if ".norm." in name:
        return "norm_weight" if name.endswith(".weight") else "norm_bias"
    return "weight" if name.endswith(".weight") else "bias"


def forward(sd, feats, sp, p6_stored=None):
    """fpn_grad_oracle.forward with the FPN's norms on batch statistics: {p<s>: tensor}."""
    leaves = [sd[p + ".weight"] for p in sd_norm_prefixes(sd)]
    with WO.intercepted(None, batch_stats=leaves) as rec:
        out = FO.forward(sd, feats, sp, p6_stored)
    assert rec["F"].bn_calls == len(leaves)
    return out


def sd_norm_prefixes(sd):
    return sorted(k[:-len(".weight")] for k in sd if k.startswith(PREFIX + ".fpn_") and k.endswith(".norm.weight"))


def stored_activations(sd, feats, sp):
    """What the plan stores of a forward under the flag: {"t": {stage: top-down sum}, "p": {stage: output}, "c_lat" / "c_out": {stage: raw
    convolution output}, "stats": {norm prefix: (mu, biased variance)}} -- an own statement of the path, norm by norm."""
    names, _, top = sp
    stages = FO.stages_of(sp)
    bn = lambda c, p: F.batch_norm(c, None, None, sd[p + ".weight"], sd[p + ".bias"], training=True, eps=EPS)
    t, p, cl, co, stats, prev = {}, {}, {}, {}, {}, None
    for idx in reversed(range(len(names))):
        s = stages[idx]
        lp, op = f"{PREFIX}.fpn_lateral{s}", f"{PREFIX}.fpn_output{s}"
        cl[s] = F.conv2d(feats[names[idx]], sd[lp + ".weight"])
        lat = bn(cl[s], lp + ".norm")
        if prev is not None:
            lat = lat + prev.repeat_interleave(2, 2).repeat_interleave(2, 3)
        t[s] = prev = lat
        co[s] = F.conv2d(lat, sd[op + ".weight"], padding=1)
        p[s] = bn(co[s], op + ".norm")
        stats[lp + ".norm"], stats[op + ".norm"] = TB.stats(cl[s], cl[s].dtype), TB.stats(co[s], co[s].dtype)
    if top:
        p[stages[-1] + 1] = O.conv2d(sd, f"{PREFIX}.top_block.p6", p[stages[-1]], stride=2, padding=1)
        if top == "p6p7":
            p[stages[-1] + 2] = O.conv2d(sd, f"{PREFIX}.top_block.p7", F.relu(p[stages[-1] + 1]), stride=2, padding=1)
    return {"t": t, "p": p, "c_lat": cl, "c_out": co, "stats": stats}


def autograd_grads(sd, feats, sp, G, dtype, leaves, p6_stored=None):
    """fpn_grad_oracle.autograd_grads through `forward` above."""
    P = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in sd.items() if k.startswith(PREFIX + ".") and ".bottom_up." not in k}
    for k in leaves:
        P[k].requires_grad_(True)
    X = {n: f.detach().to(dtype).requires_grad_(True) for n, f in feats.items()}
    out = forward(P, X, sp, p6_stored)
    sum((out[k] * G[k].to(dtype)).sum() for k in G).backward()
    return {k: P[k].grad for k in leaves}, {f"backbone_{n}": X[n].grad for n in X}


def bn_layer_grads(x, g, conv, dtype, add_pool=None):
    """One convolution + batch-statistics norm of the FPN at a stored input x and the gradient g at the norm's output, by autograd in
    `dtype`: {"dw", "norm.weight", "norm.bias", "da"}; `add_pool`: the finer stage's input gradient, whose 2x2 sums are added to da
    (the transposed top-down path, in the kernel's order)."""
    leaf = lambda v: v.detach().to(dtype).requires_grad_(True)
    X, W, ga, be = leaf(x), leaf(conv.weight), leaf(conv.norm.weight), leaf(conv.norm.bias)
    pad = (conv.weight.shape[-1] - 1) // 2
    (F.batch_norm(F.conv2d(X, W, padding=pad), None, None, ga, be, training=True, eps=conv.norm.eps) * g.to(dtype)).sum().backward()
    da = X.grad if add_pool is None else FO.pool2x2sum(X.grad, add_pool.to(dtype))
    return {"dw": W.grad, "norm.weight": ga.grad, "norm.bias": be.grad, "da": da}


def chain_grads(model, stored, feats, G, dtype):
    """fpn_grad_oracle.chain_grads with the lateral and output norms on batch statistics: the top block by its table
    (fpn_grad_oracle.layer_grads), then every output convolution + norm at the stored t_s, then every lateral + norm at the stored
    backbone feature.  Returns ({parameter name: grad}, {backbone_<name>: grad})."""
    fpn = model.backbone
    names, stages = list(fpn.in_features), list(fpn.stages)
    pnames = {id(p): k for k, p in model.named_parameters()}
    params = {}
    zero = lambda st: torch.zeros_like(stored["p"][st]).to(dtype)
    Gof = lambda st: G[f"p{st}"].to(dtype) if f"p{st}" in G else zero(st)

    def top(conv, x, g, **kw):
        res = FO.layer_grads(x, g, conv.weight.detach(), torch.ones(conv.out_channels, dtype=dtype), 2, dtype, **kw)
        params[pnames[id(conv.weight)]] = res["dw"]
        if conv.bias is not None:
            params[pnames[id(conv.bias)]] = res["q"]
        return res["da"]

    def bn(conv, x, g, add_pool=None):
        res = bn_layer_grads(x, g, conv, dtype, add_pool)
        params[pnames[id(conv.weight)]], params[pnames[id(conv.norm.weight)]], params[pnames[id(conv.norm.bias)]] = res["dw"], res["norm.weight"], res["norm.bias"]
        return res["da"]

    s5 = stages[-1]
    D = Gof(s5)
    if fpn.top_block is not None:
        D6 = Gof(s5 + 1)
        if fpn.top_block.num_levels == 2:
            p6 = stored["p"][s5 + 1]
            D6 = top(fpn.top_block.p7, p6, G[f"p{s5 + 2}"] if f"p{s5 + 2}" in G else torch.zeros_like(stored["p"][s5 + 2]), in_relu=True, mask=p6, add=D6)
        D = top(fpn.top_block.p6, stored["p"][s5], D6, add=D)
    T = {}
    for i, s in enumerate(stages):
        T[s] = bn(getattr(fpn, f"fpn_output{s}"), stored["t"][s], D if s == s5 else Gof(s), add_pool=T[stages[i - 1]] if i else None)
    fg = {}
    for i in reversed(range(len(stages))):
        fg[f"backbone_{names[i]}"] = bn(getattr(fpn, f"fpn_lateral{stages[i]}"), feats[names[i]], T[stages[i]])
    return params, fg


def expected_stats(model, stored, feats, dtype):
    """{key of fpn_batch_stats(): value} from the stored inputs: the batch's mean and biased variance of every norm's convolution output
    and the running statistics one training step leaves."""
    fpn, out = model.backbone, {}
    names, stages = list(fpn.in_features), list(fpn.stages)
    for kind, xs, pad in (("fpn_lateral", {s: feats[names[i]] for i, s in enumerate(stages)}, 0), ("fpn_output", stored["t"], 1)):
        for s in stages:
            conv = getattr(fpn, f"{kind}{s}")
            c = F.conv2d(xs[s].to(dtype), conv.weight.detach().to(dtype), padding=pad)
            mu, v = TB.stats(c, dtype)
            rm, rv = TB.running_update(conv.norm.running_mean.to(dtype), conv.norm.running_var.to(dtype), mu, v, c.shape[0] * c.shape[2] * c.shape[3])
            stem = f"{PREFIX}.{kind}{s}.norm."
            out.update({stem + "batch_mean": mu, stem + "batch_var": v, stem + "running_mean": rm, stem + "running_var": rv})
    return out


def head_maps(model, feats, dtype=torch.float32, tower_batch_stats=False):
    """tower_bn_oracle.head_maps with the towers' norms on the batch's statistics only when `tower_batch_stats`."""
    if tower_batch_stats:
        return TB.head_maps(model, feats, dtype)
    with norms_on(model, towers=False, fpn=False):
        return TB.head_maps(model, feats, dtype)


@contextlib.contextmanager
def norms_on(model, towers=True, fpn=True):
    """Inside, tower_bn_oracle.bn_prefixes -- the set of norms whole_model_grad_oracle.whole_model_grads(batch_stats=True) and
    tower_bn_oracle.head_maps switch to batch statistics -- names the towers' BN norms (`towers`) and the FPN's (`fpn`)."""
    orig = TB.bn_prefixes
    chosen = (orig(model) if towers else set()) | (set(norm_prefixes(model)) if fpn else set())
    TB.bn_prefixes = lambda m: set(chosen)
    try:
        yield chosen
    finally:
        TB.bn_prefixes = orig
