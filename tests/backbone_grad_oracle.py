"""CPU oracle of the DLA-34 backbone backward (tests/test_backbone_grads.py, tests/test_backbone_grads_gpu.py).

Two statements of the same gradients:
  * `autograd_grads`: torch autograd through oracle.dd3d_oracle._tree (the tree functions of dla_forward, the forward the goldens pin to
    the reference), level2 .. level5, with the level1 tensor and the parameters as leaves.
  * `layer_grads` / `pool_backward` / `chain_grads`: the table of include/dd3d_hip.h call by call on STORED activations (what the kernels
    linearise at), in float64 or float32.  With the forward's own activations the two agree to float64 rounding.
The stored activations carry the names of BackboneLowering._tree's buffers (<tree>.cat, <tree>.tree1.mid, <tree>.tree2.mid, <tree>.bottom,
<tree>.out, and "level1"), NCHW.  The bar is the project's: 8 * max(d32, 2^-23 * max|g64|) (loss_grad_oracle.bar)."""
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from oracle import dd3d_oracle as O
from tests.fpn_grad_oracle import family_of, fold_scale, read_out  # noqa: F401
from tests.loss_grad_oracle import bar  # noqa: F401

LEVELS = (2, 3, 4, 5)


def param_names(dla, prefix="backbone.bottom_up"):
    return sorted(f"{prefix}.{k}" for k, _ in dla.named_parameters() if k.split(".")[0] in [f"level{i}" for i in LEVELS])


def convs_of(dla):
    """{module path below the DLA: Conv2d} of level2 .. level5."""
    return OrderedDict((k, m) for k, m in dla.named_modules() if k.split(".")[0] in [f"level{i}" for i in LEVELS] and getattr(getattr(m, "weight", None), "dim", lambda: 0)() == 4)


def state(dla, dtype):
    """The state dict oracle.dd3d_oracle._tree reads (keys below the DLA).  A convolution without a norm gets an identity one (weight 1,
    bias 0, mean 0, variance 1 - eps), so that the oracle's `norm=` argument applies to every lowering."""
    sd = {k: (v.detach().to(dtype) if v.is_floating_point() else v) for k, v in dla.state_dict().items()}
    for k, m in convs_of(dla).items():
        if getattr(m, "norm", None) is None:
            n = m.weight.shape[0]
            sd.update({f"{k}.norm.weight": torch.ones(n, dtype=dtype), f"{k}.norm.bias": torch.zeros(n, dtype=dtype),
                       f"{k}.norm.running_mean": torch.zeros(n, dtype=dtype), f"{k}.norm.running_var": torch.full((n, ), 1.0 - 1e-5, dtype=dtype)})
    return sd


def forward(dla, sd, level1):
    """{level<n>: output} of level2 .. level5 through the oracle's tree functions."""
    outs, x = OrderedDict(), level1
    ch = dla.channels
    for lvl in LEVELS:
        x = O._tree(sd, f"level{lvl}", x, dla.levels[lvl], ch[lvl - 1], ch[lvl], 2, level_root=(lvl >= 3))
        outs[f"level{lvl}"] = x
    return outs


def autograd_grads(dla, level1, G, dtype, leaves=None):
    """d sum_n <G[level n], level n> / d (parameters, level1) by autograd in `dtype`: ({name below the DLA: grad}, grad at level1).
    `leaves`: parameter names below the DLA (default: every parameter of level2 .. level5)."""
    sd = state(dla, dtype)
    leaves = [k[len("backbone.bottom_up."):] for k in param_names(dla)] if leaves is None else leaves
    for k in leaves:
        sd[k] = sd[k].clone().requires_grad_(True)
    x = level1.detach().to(dtype).requires_grad_(True)
    outs = forward(dla, sd, x)
    sum((outs[k] * G[k].to(dtype)).sum() for k in G).backward()
    return {k: sd[k].grad for k in leaves}, x.grad


def _conv(m, x, relu=False, res=None):
    dtype = x.dtype
    k = m.weight.shape[-1]
    y = F.conv2d(x, m.weight.detach().to(dtype), m.bias.detach().to(dtype) if m.bias is not None else None, stride=m.stride, padding=(k - 1) // 2)
    n = getattr(m, "norm", None)
    if n is not None:
        y = (y - n.running_mean.to(dtype)[None, :, None, None]) * fold_scale(m, dtype)[None, :, None, None] + n.bias.detach().to(dtype)[None, :, None, None]
    if res is not None:
        y = y + res
    return F.relu(y) if relu else y


def stored_activations(dla, level1):
    """What the plan stores of a forward, under the lowering's buffer names (own statement of Tree.forward in the table's restated form:
    bottom, residual, mid1, x1, mid2, x2, root over the concat buffer)."""
    S = {"level1": level1}

    def tree1(m, name, x, cat=None, bottom=None, extra=()):
        oc, s = m.out_channels, m.stride
        if bottom is None:
            bottom = F.max_pool2d(x, 2, 2) if s == 2 else x
            if s == 2 and not m.level_root:
                S[name + ".bottom"] = bottom
        residual = _conv(m.project, bottom) if m.project is not None else bottom
        S[name + ".tree1.mid"] = _conv(m.tree1.conv1, x, relu=True)
        x1 = _conv(m.tree1.conv2, S[name + ".tree1.mid"], relu=True, res=residual)
        S[name + ".tree2.mid"] = _conv(m.tree2.conv1, x1, relu=True)
        x2 = _conv(m.tree2.conv2, S[name + ".tree2.mid"], relu=True, res=x1)
        parts = [x2, x1] + ([bottom] if (m.level_root and cat is None) else []) + list(extra)
        S[cat or name + ".cat"] = torch.cat(parts, 1)
        return _conv(m.root.conv, S[cat or name + ".cat"], relu=True)

    x = level1
    for lvl in LEVELS:
        m, name = getattr(dla, f"level{lvl}"), f"level{lvl}"
        if m.levels == 1:
            x = S[name + ".out"] = tree1(m, name, x)
        else:
            bottom = F.max_pool2d(x, 2, 2) if m.level_root else None
            t1 = tree1(m.tree1, name + ".tree1", x, bottom=bottom)
            x = S[name + ".tree2.out"] = tree1(m.tree2, name + ".tree2", t1, cat=name + ".cat", extra=([bottom] if m.level_root else []) + [t1])
    return S


def layer_grads(x, y, g, w, scale, stride, dtype=torch.float64, add=None, res=None):
    """One convolution of the table on stored tensors (NCHW): gm = g * [y > 0] (y None: g); dw_level (P), dw, q, r and
    da = (add + res_g * [res_y > 0]) + dgrad; `res` = (res_g, res_y)."""
    k = w.shape[-1]
    pad = (k - 1) // 2
    X, W, s = x.to(dtype), w.to(dtype), scale.to(dtype)
    Gm = g.to(dtype) * (y > 0).to(dtype) if y is not None else g.to(dtype)
    P = conv2d_weight(X, W.shape, Gm, stride=stride, padding=pad)
    da = conv2d_input(X.shape, W, Gm * s[None, :, None, None], stride=stride, padding=pad)
    head = None
    if res is not None:
        head = res[0].to(dtype) * (res[1] > 0).to(dtype)
        if add is not None:
            head = add.to(dtype) + head
    elif add is not None:
        head = add.to(dtype)
    if head is not None:
        da = head + da
    return {"dw_level": P, "dw": s[:, None, None, None] * P, "q": Gm.sum((0, 2, 3)), "r": (P * W).sum((1, 2, 3)), "da": da}


def pool_backward(x, g, dtype=torch.float64, add=None, res=None):
    """da[2y+i, 2x+j] = add + (g' if (i, j) is the first maximum of x's window in the order (0,0), (0,1), (1,0), (1,1) else 0), with
    g' = g (+ res_g * [res_y > 0]); own statement (no autograd)."""
    B, C_, H, W = x.shape
    win = torch.stack([x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]], -1)
    best = torch.zeros(win.shape[:-1], dtype=torch.long)
    top = win[..., 0].clone()
    for k in range(1, 4):
        better = win[..., k] > top
        best = torch.where(better, torch.full_like(best, k), best)
        top = torch.where(better, win[..., k], top)
    gp = g.to(dtype) if g is not None else None
    if res is not None:
        rg = res[0].to(dtype) * (res[1] > 0).to(dtype)
        gp = rg if gp is None else gp + rg
    da = torch.zeros(B, C_, H, W, dtype=dtype)
    for k in range(4):
        da[:, :, (k >> 1)::2, (k & 1)::2] = torch.where(best == k, gp, torch.zeros_like(gp))
    return add.to(dtype) + da if add is not None else da


def family_vectors(res):
    """Flat vectors per family of one or several layer results: filter (dw and the unscaled P), bias (q), norm_weight (r), input (da)."""
    rs = res if isinstance(res, (list, tuple)) else [res]
    cat = lambda ks: torch.cat([r[k].reshape(-1) for r in rs for k in ks if k in r] or [torch.zeros(0)])
    return {"filter": cat(("dw", "dw_level")), "bias": cat(("q", )), "norm_weight": cat(("r", )), "input": cat(("da", ))}


def chain_grads(dla, S, G, dtype, prefix="backbone.bottom_up"):
    """The whole table on stored activations `S` (buffer name -> NCHW tensor), `G` {level<n>: the gradient a backbone output feature
    receives from outside}.  Returns ({parameter name: grad}, the gradient at level1, {call key: result}); the read-out in `dtype`."""
    pnames = {id(p): f"{prefix}.{k}" for k, p in dla.named_parameters()}
    params, raw = {}, OrderedDict()
    T = lambda key, c0=0, n=None: S[key][:, c0:(None if n is None else c0 + n)]

    def run(key, conv, x, y, g, stride, **kw):
        scale = fold_scale(conv, dtype)
        res = layer_grads(x, y, g, conv.weight.detach(), scale, stride, dtype, **kw)
        raw[key] = res
        params[pnames[id(conv.weight)]] = res["dw"]
        norm = getattr(conv, "norm", None)
        got = read_out(conv, scale, res["q"], res["r"], dtype)
        for k, p in (("norm.weight", getattr(norm, "weight", None)), ("norm.bias", getattr(norm, "bias", None)), ("bias", conv.bias)):
            if k in got and id(p) in pnames:
                params[pnames[id(p)]] = got[k]
        return res["da"]

    def tree1(m, name, x, dst, G_out, cat=None, bottom=None, bottom_add=None, x_add=None, x_slice=None):
        oc, ic, s = m.out_channels, m.in_channels, m.stride
        own, cat = cat is None, cat or name + ".cat"
        Dcat = run(name + ".root", m.root.conv, S[cat], dst, G_out, 1)
        x2, x1, mid1, mid2 = T(cat, 0, oc), T(cat, oc, oc), S[name + ".tree1.mid"], S[name + ".tree2.mid"]
        if own and m.level_root:
            bottom, bottom_add = T(cat, 2 * oc, ic), Dcat[:, 2 * oc:2 * oc + ic]
        D2, D1 = Dcat[:, :oc], Dcat[:, oc:2 * oc]
        Gmid2 = run(name + ".tree2.conv2", m.tree2.conv2, mid2, x2, D2, 1)
        Gx1 = run(name + ".tree2.conv1", m.tree2.conv1, x1, mid2, Gmid2, 1, add=D1, res=(D2, x2))
        Gmid1 = run(name + ".tree1.conv2", m.tree1.conv2, mid1, x1, Gx1, 1)
        if s == 2:
            Gbottom, res = bottom_add, None
            if m.project is not None:
                Gbottom = run(name + ".project", m.project, bottom if bottom is not None else S[name + ".bottom"], x1, Gx1, 1, add=bottom_add)
            else:
                res = (Gx1, x1)
            Cx = run(name + ".tree1.conv1", m.tree1.conv1, x, mid1, Gmid1, 2, add=x_add)
            raw[name + ".pool"] = {"da": pool_backward(x, Gbottom, dtype, add=Cx, res=res)}
            return raw[name + ".pool"]["da"], Dcat
        A = Dcat[:, x_slice[0]:x_slice[0] + x_slice[1]] if x_slice is not None else x_add
        if m.project is not None:
            A = run(name + ".project", m.project, x, x1, Gx1, 1, add=A)
            return run(name + ".tree1.conv1", m.tree1.conv1, x, mid1, Gmid1, 1, add=A), Dcat
        return run(name + ".tree1.conv1", m.tree1.conv1, x, mid1, Gmid1, 1, add=A, res=(Gx1, x1)), Dcat

    def tree(m, name, x, G_out, x_add):
        if m.levels == 1:
            return tree1(m, name, x, S[name + ".out"], G_out, x_add=x_add)[0]
        oc, ic = m.out_channels, m.in_channels
        cat2, off, bottom = name + ".cat", 2 * oc, None
        if m.level_root:
            bottom, off = T(cat2, off, ic), off + ic
        t1 = T(cat2, off, oc)
        G_t1, Dcat2 = tree1(m.tree2, name + ".tree2", t1, S[name + ".tree2.out"], G_out, cat=cat2, x_slice=(off, oc))
        return tree1(m.tree1, name + ".tree1", x, t1, G_t1, bottom=bottom, bottom_add=Dcat2[:, 2 * oc:2 * oc + ic] if m.level_root else None, x_add=x_add)[0]

    g = G["level5"].to(dtype)
    for lvl in reversed(LEVELS):
        m = getattr(dla, f"level{lvl}")
        if lvl == 2:
            x = S["level1"]
        else:
            p = getattr(dla, f"level{lvl - 1}")
            x = S[f"level{lvl - 1}.out" if p.levels == 1 else f"level{lvl - 1}.tree2.out"]
        xa = G.get(f"level{lvl - 1}")
        g = tree(m, f"level{lvl}", x, g, xa.to(dtype) if xa is not None else None)
    return params, g, raw
