"""CPU oracle of the DLA-34 stem's backward (tests/test_stem_grads.py, tests/test_stem_grads_gpu.py).

Two statements of one stem layer's gradients, y = relu(n(conv_k,s(x))) with n(.) the folded norm (layers.fold_norm, running statistics):
  * `autograd_layer`: torch autograd through F.conv2d + the norm + ReLU, with the filter, the conv bias, the norm's weight and bias and
    the input as leaves.
  * `layer_grads`: the restated form of include/dd3d_hip.h that csrc/stem_grads.hip computes, on the STORED output (gm = g * [y > 0];
    dw_level, dw = scale * dw_level, q = sum gm, r = sum dw_level * w, da = dgrad(scale * gm, w)), and `read_out`, the norm read-out the
    backbone uses (rstd * (r + (b_conv - mean) * q)).
With the forward's own output the two agree to float64 rounding.  The bar is the project's: 8 * max(d32, 2^-23 * max|g64|)
(loss_grad_oracle.bar)."""
import torch
import torch.nn.functional as F

from tests.backbone_grad_oracle import family_vectors, layer_grads  # noqa: F401  (the table's call on stored tensors, any k and Cin)
from tests.loss_grad_oracle import bar  # noqa: F401

SHAPES = {"base_layer": (7, 1, 4, 16), "level0.0": (3, 1, 16, 16), "level1.0": (3, 2, 16, 32)}  # (ksize, stride, Cin, Cout)
EPS = 1e-5


def fold(p, dtype):
    """(scale, rstd) of the folded norm: y = (conv + b - mean) * scale + beta with scale = gamma * rstd; no norm: scale = rstd = 1."""
    if "gamma" not in p:
        one = torch.ones(p["w"].shape[0], dtype=dtype)
        return one, one
    rstd = torch.rsqrt(p["var"].to(dtype) + EPS)
    return p["gamma"].to(dtype) * rstd, rstd


def forward_layer(x, p, stride, dtype):
    """relu(n(conv(x))) in `dtype`; `p`: {"w" [Cout, Cin, k, k], optional "b", optional norm "gamma", "beta", "mean", "var"}."""
    k = p["w"].shape[-1]
    y = F.conv2d(x.to(dtype), p["w"].to(dtype), p["b"].to(dtype) if "b" in p else None, stride=stride, padding=(k - 1) // 2)
    if "gamma" in p:
        scale, _ = fold(p, dtype)
        y = (y - p["mean"].to(dtype)[None, :, None, None]) * scale[None, :, None, None] + p["beta"].to(dtype)[None, :, None, None]
    return F.relu(y)


def autograd_layer(x, p, g, stride, dtype):
    """d <g, relu(n(conv(x)))> / d (w, b, gamma, beta, x) by autograd in `dtype` (the keys the layer has)."""
    leaves = {k: p[k].detach().to(dtype).clone().requires_grad_(True) for k in ("w", "b", "gamma", "beta") if k in p}
    q = dict(p)
    q.update(leaves)
    xx = x.detach().to(dtype).clone().requires_grad_(True)
    (forward_layer(xx, q, stride, dtype) * g.to(dtype)).sum().backward()
    out = {k: v.grad for k, v in leaves.items()}
    out["x"] = xx.grad
    return out


def read_out(p, res, dtype):
    """{w, b, gamma, beta} gradients from one `layer_grads` result: the backbone's norm read-out."""
    scale, rstd = fold(p, dtype)
    out = {"w": res["dw"]}
    if "gamma" in p:
        centre = (p["b"].to(dtype) if "b" in p else 0.0) - p["mean"].to(dtype)
        out["gamma"] = rstd * (res["r"] + centre * res["q"])
        out["beta"] = res["q"]
    if "b" in p:
        out["b"] = scale * res["q"]
    return out


def stem_chain(img4, params, g_level1, dtype, stored=None):
    """The three calls in their order on stored activations: level1.0 (wgrad + dgrad), level0.0 (wgrad + dgrad), base_layer (wgrad).
    `params`: {layer name: p}; `stored`: {"base", "level0.0", "level1.0"} NCHW (default: the forward's own in `dtype`).  Returns
    ({layer: layer_grads result}, {"backbone_level0", "backbone_base_layer"}: the gradients at the two tensors before their own masks)."""
    if stored is None:
        base = forward_layer(img4, params["base_layer"], 1, dtype)
        l0 = forward_layer(base, params["level0.0"], 1, dtype)
        stored = {"base": base, "level0.0": l0, "level1.0": forward_layer(l0, params["level1.0"], 2, dtype)}
    sc = lambda k: fold(params[k], dtype)[0]
    r1 = layer_grads(stored["level0.0"], stored["level1.0"], g_level1, params["level1.0"]["w"], sc("level1.0"), 2, dtype)
    r0 = layer_grads(stored["base"], stored["level0.0"], r1["da"], params["level0.0"]["w"], sc("level0.0"), 1, dtype)
    rb = layer_grads(img4, stored["base"], r0["da"], params["base_layer"]["w"], sc("base_layer"), 1, dtype)
    return {"level1.0": r1, "level0.0": r0, "base_layer": rb}, {"backbone_level0": r1["da"], "backbone_base_layer": r0["da"]}


# ------------------------------------------------------------------------------------------------- the whole model, stem included
def whole_model_grads_with_stem(model_cpu, cfg, inputs, gt, dtype, masks=None, inv_K=None, extras=None):
    """whole_model_grad_oracle.whole_model_grads itself -- ONE autograd pass of the whole model in `dtype`, under `masks` when given --
    with the gradients at the stem's first two ReLU outputs retained as well: that function keeps no handle on the two tensors, so
    its recording ReLU is wrapped for the duration of the call (the forward, the loss and the leaves stay its own).  Returns
    ({parameter: gradient}, its tensor gradients plus backbone_base_layer and backbone_level0, each before the tensor's own mask)."""
    from tests import whole_model_grad_oracle as WO
    outs, orig = [], WO._Functional.relu

    def relu(self, x, inplace=False):
        y = orig(self, x, inplace)
        if len(outs) < 2:  # base_layer's and level0's outputs: the first two ReLU calls of the oracle's DLA forward
            y.retain_grad()
            outs.append(y)
        return y

    WO._Functional.relu = relu
    try:
        params, at, _ = WO.whole_model_grads(model_cpu, cfg, inputs, gt, dtype, masks=masks, inv_K=inv_K, extras=extras)
    finally:
        WO._Functional.relu = orig
    assert WO.stem_relus(model_cpu) == 3 and len(outs) == 2 and outs[0].shape[1] == outs[1].shape[1] == 16
    return params, dict(at, backbone_base_layer=outs[0].grad.detach(), backbone_level0=outs[1].grad.detach())


class WithIdentityNorms:
    """A model whose norm-less DLA convolutions (FE.BACKBONE.NORM "") show an identity norm in state_dict(): oracle.dd3d_oracle's DLA
    forward applies a norm behind every convolution, so such a layer gets weight 1, bias 0, mean 0 and variance 1 - eps, as
    backbone_grad_oracle.state does for level2 .. level5.  named_parameters() and everything else are the model's own."""
    def __init__(self, model):
        self._m = model

    def __getattr__(self, name):
        return getattr(self._m, name)

    def state_dict(self):
        sd = dict(self._m.state_dict())
        for k, m in self._m.backbone.bottom_up.named_modules():
            if getattr(getattr(m, "weight", None), "dim", lambda: 0)() == 4 and getattr(m, "norm", None) is None:
                n, pre = m.weight.shape[0], f"backbone.bottom_up.{k}.norm."
                sd.update({pre + "weight": torch.ones(n), pre + "bias": torch.zeros(n), pre + "running_mean": torch.zeros(n),
                           pre + "running_var": torch.full((n, ), 1.0 - EPS, dtype=torch.float64)})
        return sd


STEM_LAYERS = ("base_layer", "level0.0", "level1.0")
PARAM_NAME = {"w": "weight", "b": "bias", "gamma": "norm.weight", "beta": "norm.bias"}


def model_stem_params(model, dtype=torch.float64):
    """{layer: p} of `forward_layer` / `read_out` from a model's own DLA stem: the filter (base_layer's padded to the image's four
    channels with a zero filter), the conv bias if there is one, the norm's weight, bias and running statistics if there is one."""
    dla, out = model.backbone.bottom_up, {}
    for name in STEM_LAYERS:
        m = dla.get_submodule(name)
        w = m.weight.detach().to(dtype)
        if w.shape[1] == 3:
            w = torch.cat([w, torch.zeros_like(w[:, :1])], 1)
        p = {"w": w}
        if m.bias is not None:
            p["b"] = m.bias.detach().to(dtype)
        if getattr(m, "norm", None) is not None:
            assert m.norm.eps == EPS
            p.update(gamma=m.norm.weight.detach().to(dtype), beta=m.norm.bias.detach().to(dtype), mean=m.norm.running_mean.to(dtype),
                     var=m.norm.running_var.to(dtype))
        out[name] = p
    return out


STEM_BUFFERS = ("base", "level0.0", "level1.0")


def stem_plan_masks(plan, pre64, report=None):
    """whole_model_grad_oracle.plan_masks with the three leading entries -- the oracle's own signs there -- replaced by the signs of the
    plan's decoded stored `base`, `level0.0` and `level1.0`, validated by value as plan_masks validates the rest: the decoded tensor has
    the call's shape and is within STORED_TOL * max(1, max|ref|) of the float64 ReLU output.  `report` receives the three calls first."""
    from tests import whole_model_grad_oracle as WO
    from tests.util import decode
    rest = []
    masks = WO.plan_masks(plan, pre64, rest)
    for k, name in enumerate(STEM_BUFFERS):
        pre = pre64[k]
        got, ref = decode(plan.bufs[name]).double(), pre.double().clamp(min=0)
        if tuple(got.shape) != tuple(ref.shape):
            raise ValueError(f"ReLU call {k} ({name}): stored {tuple(got.shape)}, oracle {tuple(ref.shape)}")
        err, tol = float((got - ref).abs().max()), WO.STORED_TOL * max(1.0, float(ref.abs().max()))
        if not err <= tol:
            raise ValueError(f"ReLU call {k} ({name}): the stored tensor is {err:.3e} from the oracle's (bar {tol:.3e})")
        masks[k] = got > 0
        if report is not None:
            bad = masks[k] != (pre > 0)
            far = bad & (pre.abs() > WO.SIGN_NEAR * float(pre.abs().max()))
            report.append((name, pre.numel(), int(bad.sum()), int(far.sum())))
    if report is not None:
        report.extend(rest)
    return masks


def stem_sign_report(pre_a, pre64):
    """(label, elements, sign disagreements of `pre_a` with the float64 forward, of them beyond SIGN_NEAR of the tensor's maximum) for the
    three stem ReLUs: the two conditions of the whole-model test on another forward's own pre-activations (the float32 oracle's)."""
    from tests import whole_model_grad_oracle as WO
    out = []
    for k, name in enumerate(STEM_BUFFERS):
        bad = (pre_a[k] > 0) != (pre64[k] > 0)
        far = bad & (pre64[k].abs() > WO.SIGN_NEAR * float(pre64[k].abs().max()))
        out.append((name, pre64[k].numel(), int(bad.sum()), int(far.sum())))
    return out
