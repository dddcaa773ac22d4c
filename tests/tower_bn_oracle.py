"""CPU oracle of the head towers' batch-statistics BatchNorm (csrc/tower_bn.hip, engine.LossPlan(batch_stats=True)): a tower layer is

    c_l = conv3x3(x_l, W) (+ b)        y_l = relu(F.batch_norm(c_l, ..., weight, bias, training=True))

per pyramid level, statistics per channel over the B * h_l * w_l pixels, as nn.BatchNorm2d computes them in train().  The backward is
taken by autograd in float64 or float32 under the explicit mask [stored y_l > 0], as tests/tower_grad_oracle.py does for the running
statistics; the closed formulas the kernels implement (include/dd3d_hip.h) stand beside it.  Everything is NCHW here.  The acceptance
bound of a family is loss_grad_oracle.bar: 8 * max(d32, 2^-23 * max|ref64|).
"""
import contextlib

import torch
import torch.nn.functional as F

from oracle import dd3d_oracle as O
from tests import tower_grad_oracle as TO
from tests.loss_grad_oracle import bar  # noqa: F401

MOMENTUM = 0.1  # nn.BatchNorm2d's default; get_norm("BN") does not change it
FAMILIES = ("weight", "norm_weight", "norm_bias", "da", "feature")


def is_batch_norm(norm):
    """A trainable BatchNorm2d: what batch_stats=True switches to the batch's statistics (FrozenBN owns buffers only)."""
    return norm is not None and isinstance(getattr(norm, "weight", None), torch.nn.Parameter) and hasattr(norm, "running_mean")


def layer_is_bn(conv, L):
    return all(is_batch_norm(TO.level_norm(conv, l)) for l in range(L))


# ------------------------------------------------------------------------------------------ the closed formulas
def stats(c, dtype=torch.float64):
    """(mu, biased variance) per channel of an NCHW tensor, two passes."""
    c = c.to(dtype)
    mu = c.mean(dim=(0, 2, 3))
    return mu, ((c - mu[None, :, None, None])**2).mean(dim=(0, 2, 3))


def forward_closed(c, gamma, beta, eps, dtype=torch.float64):
    """mu, v, s, t, y of the header's forward in `dtype`."""
    mu, v = stats(c, dtype)
    s = gamma.to(dtype) * torch.rsqrt(v + eps)
    t = beta.to(dtype) - mu * s
    return mu, v, s, t, F.relu(c.to(dtype) * s[None, :, None, None] + t[None, :, None, None])


def backward_closed(c, y, G, gamma, eps, dtype=torch.float64):
    """q, p, G_c of the header's backward in `dtype` (d beta = q, d gamma = p), the mask taken from the stored y."""
    mu, v = stats(c, dtype)
    rstd = torch.rsqrt(v + eps)
    N = c.shape[0] * c.shape[2] * c.shape[3]
    ghat = (G * (y > 0)).to(dtype)
    xhat = (c.to(dtype) - mu[None, :, None, None]) * rstd[None, :, None, None]
    q, p = ghat.sum(dim=(0, 2, 3)), (ghat * xhat).sum(dim=(0, 2, 3))
    s = gamma.to(dtype) * rstd
    return q, p, s[None, :, None, None] * (ghat - q[None, :, None, None] / N - xhat * p[None, :, None, None] / N)


def backward_autograd(c, y, G, gamma, beta, eps, dtype=torch.float64):
    """The same three by autograd through F.batch_norm(training=True): (d beta, d gamma, d c)."""
    cl = c.detach().to(dtype).requires_grad_(True)
    ga, be = gamma.detach().to(dtype).requires_grad_(True), beta.detach().to(dtype).requires_grad_(True)
    (F.batch_norm(cl, None, None, ga, be, training=True, eps=eps) * (G * (y > 0)).to(dtype)).sum().backward()
    return be.grad, ga.grad, cl.grad


def running_update(running_mean, running_var, mu, v, N, momentum=MOMENTUM):
    """What one train() forward leaves in the norm's buffers: the variance unbiased by N / (N - 1)."""
    return (1 - momentum) * running_mean + momentum * mu, (1 - momentum) * running_var + momentum * (v * (N / (N - 1)))


# ------------------------------------------------------------------------------------------ a layer of the model's own modules
def module_layer_grads(conv, x, y, g, dtype=torch.float64):
    """tower_grad_oracle.module_layer_grads with the norm applied as F.batch_norm(..., training=True) on the module's parameters: a layer
    whose norms are not trainable BatchNorm2d falls through to the running-statistics oracle.  Returns ({id(parameter): gradient},
    [d / d x_l])."""
    L = len(x)
    if not layer_is_bn(conv, L):
        return TO.module_layer_grads(conv, x, y, g, dtype)
    leaf = lambda p: p.detach().to(dtype).requires_grad_(True)
    W = leaf(conv.weight)
    leaves = {id(conv.weight): W}
    b = leaves.setdefault(id(conv.bias), leaf(conv.bias)) if conv.bias is not None else None
    X = [a.detach().to(dtype).requires_grad_(True) for a in x]
    total = 0
    for l in range(L):
        norm = TO.level_norm(conv, l)
        nw, nb = leaves.setdefault(id(norm.weight), leaf(norm.weight)), leaves.setdefault(id(norm.bias), leaf(norm.bias))
        c = F.conv2d(X[l], W, b, padding=1)
        total = total + (F.batch_norm(c, None, None, nw, nb, training=True, eps=norm.eps) * (g[l] * (y[l] > 0)).to(dtype)).sum()
    total.backward()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    return {k: zero(p) for k, p in leaves.items()}, [zero(a) for a in X]


def chain_grads(model, stored, g_top, dtype=torch.float64):
    """tower_grad_oracle.chain_grads over `module_layer_grads` above: the towers' backward layer by layer at stored (x_i, y_i)."""
    names = {id(p): k for k, p in model.named_parameters()}
    params, feat, das = {}, None, {}
    for t, convs in TO.tower_modules(model).items():
        g = [v.to(dtype) for v in g_top[t]]
        for i in reversed(range(len(convs))):
            x, y = stored[t][i]
            pg, da = module_layer_grads(convs[i], x, y, g, dtype)
            for k, v in pg.items():
                params[names[k]] = v
            das[(t, i)] = da
            g = da
        feat = g if feat is None else [a + b for a, b in zip(feat, g)]
    return params, {f"feature{l}": v for l, v in enumerate(feat)}, das


def layer_forward(conv, x, dtype):
    """(c_l, y_l, per-level (mu, v)) of one tower module on per-level inputs in `dtype`, batch statistics where the layer is BN."""
    L = len(x)
    W = conv.weight.detach().to(dtype)
    b = conv.bias.detach().to(dtype) if conv.bias is not None else None
    cs, ys, st = [], [], []
    for l in range(L):
        norm = TO.level_norm(conv, l)
        c = F.conv2d(x[l].to(dtype), W, b, padding=1)
        if layer_is_bn(conv, L):
            y = F.relu(F.batch_norm(c, None, None, norm.weight.detach().to(dtype), norm.bias.detach().to(dtype), training=True, eps=norm.eps))
            st.append(stats(c, dtype))
        else:
            sc, sh = TO.fold(conv, norm, dtype)
            y = F.relu((c - (b[None, :, None, None] if b is not None else 0)) * sc[None, :, None, None] + sh[None, :, None, None])
            st.append(None)
        cs.append(c), ys.append(y)
    return cs, ys, st


def batch_stats_names(model):
    """The keys of LossPlan.tower_batch_stats(): the running_* buffers of the BN towers' norms and their batch_* twins."""
    bufs = {id(b): k for k, b in model.named_buffers()}
    out = []
    L = len(model.backbone_output_shape)
    for convs in TO.tower_modules(model).values():
        for conv in convs:
            if layer_is_bn(conv, L):
                for l in range(L):
                    stem = bufs[id(TO.level_norm(conv, l).running_mean)][:-len("running_mean")]
                    out += [stem + k for k in ("running_mean", "running_var", "batch_mean", "batch_var")]
    return sorted(out)


# ------------------------------------------------------------------------------------------ the head maps under batch statistics
@contextlib.contextmanager
def batch_statistics(prefixes):
    """Inside, the oracle's norms whose state-dict prefix is in `prefixes` normalise with the batch's statistics (the running ones in the
    state dict are left alone); every other norm stays in eval mode."""
    eval_norm = O.batch_norm_eval

    def norm(sd, prefix, x, hook=None):
        if prefix not in prefixes:
            return eval_norm(sd, prefix, x, hook)
        return F.batch_norm(x, None, None, sd[prefix + ".weight"], sd[prefix + ".bias"], training=True, eps=1e-5)

    O.batch_norm_eval = norm
    try:
        yield
    finally:
        O.batch_norm_eval = eval_norm


def bn_prefixes(model):
    return {k[:-len(".running_mean")] for k in batch_stats_names(model) if k.endswith(".running_mean")}


def head_maps(model, feats, dtype=torch.float64):
    """The head maps of the reference's training forward on per-level FPN features, NCHW under the loss oracle's keys: the heads of
    oracle/dd3d_oracle.py with the BN towers on batch statistics."""
    sd = {k: (v.detach().to(dtype) if v.is_floating_point() else v.detach()) for k, v in model.state_dict().items()}
    feats = [f.to(dtype) for f in feats]
    out = {}
    with batch_statistics(bn_prefixes(model)):
        logits, reg, ctr, cls_out = O.fcos2d_head(sd, feats, num_convs=len(model.fcos2d_head.cls_tower), num_box_convs=len(model.fcos2d_head.box2d_tower))
        heads = dict(logits=logits, box2d_reg=reg, centerness=ctr)
        if not model.only_box2d:
            heads.update(zip(("quat", "ctr", "depth", "size", "conf"), O.fcos3d_head(sd, feats, num_convs=len(model.fcos3d_head.box3d_tower))))
        if hasattr(model, "attr_logits"):  # nuscenes_dd3d.py:371-374: both read the cls tower's output
            heads["attr"] = [O.conv2d(sd, "attr_logits", t, padding=1) for t in cls_out]
            heads["speed"] = [F.relu(O.conv2d(sd, "speed", t, padding=1)) for t in cls_out]
    for k, levels in heads.items():
        for l, v in enumerate(levels):
            out[f"{k}{l}"] = v
    return out
