"""CPU oracle of a head-tower layer's backward (csrc/tower_grads.hip, include/dd3d_hip.h::dd3d_tower_grad_args): the forward of one tower
layer over the pyramid levels as a torch composition,

    y_l = relu(s_l * conv3x3(x_l, W) + t_l)

contracted with a constant gradient G_l through the explicit mask [stored y_l > 0] (the stored output decides, not a recomputation), and
differentiated by autograd in float64 or float32; and the same applied layer by layer down a tower at given stored (x_i, y_i): the
backward linearised at a plan's activations.  Everything is NCHW here.  The acceptance bound of a family is loss_grad_oracle.bar:
8 * max(d32, 2^-23 * max|g64|).
"""
import re

import torch
import torch.nn.functional as F

from tests.loss_grad_oracle import bar  # noqa: F401  (the project's one rule for a gradient's tolerance)

FAMILIES = ("weight", "norm_weight", "norm_bias", "da")
TOWERS = ("cls", "box2d", "box3d")
TOWER_PREFIX = {"cls": "fcos2d_head.cls_tower", "box2d": "fcos2d_head.box2d_tower", "box3d": "fcos3d_head.box3d_tower"}
TOWER_PARAM = re.compile(r"^(fcos2d_head\.(cls|box2d)_tower|fcos3d_head\.box3d_tower)\.\d+\.(weight|bias|norm\.\d+\.(weight|bias)|norm\.(weight|bias))$")


def forward(x, w, scale, shift):
    """The stored outputs of a layer, per level (what ForwardPlan._heads folds into one launch), in the dtype of its inputs."""
    return [F.relu(F.conv2d(a, w, padding=1) * scale[l][None, :, None, None] + shift[l][None, :, None, None]) for l, a in enumerate(x)]


def layer_grads(x, y, g, w, scale, dtype=torch.float64, da_add=None):
    """Gradients of sum_l <g_l * [y_l > 0], s_l * conv3x3(x_l, W) + t_l> in `dtype`: dw_level [L] (Cout, Cin, 3, 3) unscaled per-level
    partial; dw (Cout, Cin, 3, 3); q, r [L] (Cout): d / d t_l and d / d s_l; da [L] (B, Cin, H, W), plus da_add where given."""
    L = len(x)
    gm = [(g[l] * (y[l] > 0)).to(dtype) for l in range(L)]
    X = [a.detach().to(dtype).requires_grad_(True) for a in x]
    W = w.detach().to(dtype).requires_grad_(True)
    S = [s.detach().to(dtype).requires_grad_(True) for s in scale]
    T = [torch.zeros_like(s).requires_grad_(True) for s in S]
    total = 0
    for l in range(L):
        total = total + ((F.conv2d(X[l], W, padding=1) * S[l][None, :, None, None] + T[l][None, :, None, None]) * gm[l]).sum()
    total.backward()
    Wl = [w.detach().to(dtype).requires_grad_(True) for _ in range(L)]
    sum((F.conv2d(x[l].detach().to(dtype), Wl[l], padding=1) * gm[l]).sum() for l in range(L)).backward()
    da = [a.grad for a in X]
    if da_add is not None:
        da = [da_add[l].to(dtype) + da[l] for l in range(L)]
    return {"dw_level": [v.grad for v in Wl], "dw": W.grad, "q": [t.grad for t in T], "r": [s.grad for s in S], "da": da}


def family_vectors(res):
    cat = lambda xs: torch.cat([v.reshape(-1) for v in xs])
    return {"weight": cat(list(res["dw_level"]) + [res["dw"]]), "norm_weight": cat(res["r"]), "norm_bias": cat(res["q"]), "da": cat(res["da"])}


# ------------------------------------------------------------------------------------------ a layer of the model's own modules, by parameter
def level_norm(conv, l):
    return conv.norm[l] if isinstance(conv.norm, torch.nn.ModuleList) else conv.norm


def module_layer_grads(conv, x, y, g, dtype=torch.float64):
    """One tower module (a Conv2d with its per-level norm) applied as layers.fold_norm states it -- scale = w * rsqrt(var + eps),
    shift = (b - mean) * scale + beta, the reciprocal root evaluated in float32 as fold_norm does -- with the module's PARAMETERS as
    the leaves.  Returns ({id(parameter): gradient}, [d / d x_l])."""
    L = len(x)
    leaf = lambda p: p.detach().to(dtype).requires_grad_(True)
    W = leaf(conv.weight)
    b = leaf(conv.bias) if conv.bias is not None else None
    leaves = {id(conv.weight): W}
    if b is not None:
        leaves[id(conv.bias)] = b
    X = [a.detach().to(dtype).requires_grad_(True) for a in x]
    total = 0
    for l in range(L):
        norm = level_norm(conv, l)
        c = F.conv2d(X[l], W, padding=1)
        shift = b if b is not None else torch.zeros(conv.out_channels, dtype=dtype)
        if norm is not None:
            trainable = isinstance(norm.weight, torch.nn.Parameter)
            nw = leaves.setdefault(id(norm.weight), leaf(norm.weight)) if trainable else norm.weight.detach().to(dtype)
            nb = leaves.setdefault(id(norm.bias), leaf(norm.bias)) if trainable else norm.bias.detach().to(dtype)
            s = nw * torch.rsqrt(norm.running_var.float() + norm.eps).to(dtype)
            shift = (shift - norm.running_mean.to(dtype)) * s + nb
            c = c * s[None, :, None, None]
        total = total + ((c + shift[None, :, None, None]) * (g[l] * (y[l] > 0)).to(dtype)).sum()
    total.backward()
    zero = lambda p: torch.zeros_like(p) if p.grad is None else p.grad
    return {k: zero(p) for k, p in leaves.items()}, [zero(a) for a in X]


def fold(conv, norm, dtype):
    """layers.fold_norm in `dtype` (float32: its very values): the reciprocal root in float32, the products in `dtype`."""
    n = conv.out_channels
    scale, shift = torch.ones(n, dtype=dtype), (conv.bias.detach().to(dtype) if conv.bias is not None else torch.zeros(n, dtype=dtype))
    if norm is not None:
        scale = norm.weight.detach().to(dtype) * torch.rsqrt(norm.running_var.float() + norm.eps).to(dtype)
        shift = (shift - norm.running_mean.to(dtype)) * scale + norm.bias.detach().to(dtype)
    return scale, shift


def tower_modules(model):
    """{tower name: its Conv2d modules in order} of a model (two towers under only_box2d)."""
    out = {"cls": list(model.fcos2d_head.cls_tower), "box2d": list(model.fcos2d_head.box2d_tower)}
    if not model.only_box2d:
        out["box3d"] = list(model.fcos3d_head.box3d_tower)
    return out


def family_of(name):
    """The acceptance rule's family of a tower parameter's name: weight, norm_weight, norm_bias or bias."""
    return "norm_weight" if ".norm." in name and name.endswith(".weight") else "norm_bias" if ".norm." in name else \
        "weight" if name.endswith(".weight") else "bias"


def tower_param_names(model):
    """The named_parameters() of the head towers: the filters, a BN tower's norm weights and biases, a norm-less tower's conv biases."""
    return sorted(k for k, _ in model.named_parameters() if TOWER_PARAM.match(k))


def chain_grads(model, stored, g_top, dtype=torch.float64):
    """The towers' backward layer by layer at stored activations.  stored: {tower: [(x_i levels, y_i levels) for each layer]}; g_top:
    {tower: per-level gradient at the last layer's output}.  Layer i's incoming gradient is layer i + 1's input gradient in `dtype`; the
    towers' first-layer input gradients add up in tower order to the feature gradient.  Returns ({parameter name: gradient},
    {feature<l>: gradient}, {(tower, layer): per-level input gradient})."""
    names = {id(p): k for k, p in model.named_parameters()}
    params, feat, das = {}, None, {}
    for t, convs in tower_modules(model).items():
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


def chain_forward(model, feats):
    """The towers of `model` on per-level features in the features' dtype: {tower: [(x_i levels, y_i levels)]}, the chain's own stored
    activations."""
    stored = {}
    for t, convs in tower_modules(model).items():
        x, stored[t] = list(feats), []
        for conv in convs:
            sc, sh = zip(*[fold(conv, level_norm(conv, l), x[0].dtype) for l in range(len(feats))])
            y = forward(x, conv.weight.detach().to(x[0].dtype), sc, sh)
            stored[t].append((x, y))
            x = y
    return stored
