"""CPU oracle of batch-statistics BN in the DLA-34 bottom-up network (compute_losses(backbone_batch_stats=True), csrc/backbone_bn.hip):
the float64 / float32 torch forward of the bottom-up network with every norm through F.batch_norm(training=True) -- nn.BatchNorm2d in
train() -- and autograd through it under given ReLU signs, by the method of tests/fpn_bn_oracle.py and tests/whole_model_grad_oracle.py:
the oracle forward the goldens pin to the reference (oracle.dd3d_oracle.dla_forward) runs with its functional namespace replaced, so that
the chosen norms normalise with the batch's statistics and every ReLU differentiates through a stored mask.

  forward             {level<n>: tensor} of the bottom-up network on an image batch
  stored_activations  that forward's raw convolution outputs per norm, its batch statistics, every ReLU's input and output (call order)
  chain_grads         d <outputs, G> / d (every bottom-up parameter) and at the stem's tensors, under masks[call] in place of each sign
  expected_stats      the read-out of LossPlan.backbone_batch_stats(): one training step's running statistics and the batch's own
  norms_on            inside, whole_model_grad_oracle.whole_model_grads(batch_stats=True) puts the bottom-up norms (and the towers' / the
                      FPN's) on batch statistics
and for the seam test the closed forms of the three applies and their backward on one segment (apply_closed, backward_closed).
"""
import contextlib
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import dd3d_oracle as O
from tests import fpn_bn_oracle as FN
from tests import loss_grad_oracle as GO
from tests import tower_bn_oracle as TB
from tests import whole_model_grad_oracle as WO

PREFIX = "backbone.bottom_up"
MOMENTUM = TB.MOMENTUM
EPS = 1e-5
RELU, LINEAR, RESIDUAL = range(3)  # hip.BBN_*

bar = GO.bar  # 8 * max(d32, 2^-23 * max|ref64|)


def norm_prefixes(model):
    """State-dict prefixes of the bottom-up network's norms, sorted."""
    return sorted(k[:-len(".running_mean")] for k, _ in model.named_buffers() if k.startswith(PREFIX + ".") and k.endswith(".norm.running_mean"))


def batch_stats_names(model):
    """The keys of LossPlan.backbone_batch_stats()."""
    return sorted(p + "." + k for p in norm_prefixes(model) for k in ("running_mean", "running_var", "batch_mean", "batch_var"))


def family_of(name):
    if ".norm." in name:
        return "norm_weight" if name.endswith(".weight") else "norm_bias"
    return "weight" if name.endswith(".weight") else "bias"


def state(model, dtype, grad=False):
    """The model's state dict in `dtype`; with `grad` the bottom-up parameters are leaves."""
    sd = {k: (v.detach().to(dtype).clone() if v.is_floating_point() else v.detach()) for k, v in model.state_dict().items()}
    if grad:
        for k, _ in model.named_parameters():
            if k.startswith(PREFIX + "."):
                sd[k].requires_grad_(True)
    return sd


class _Recorder(WO._Functional):
    """whole_model_grad_oracle._Functional that also keeps the input of every batch-statistics norm call under the norm's prefix."""
    def __init__(self, masks, leaves):
        super().__init__(masks, list(leaves.values()))
        self.prefix_of, self.raw = {id(w): p for p, w in leaves.items()}, OrderedDict()

    def batch_norm(self, x, running_mean, running_var, weight=None, bias=None, training=False, momentum=0.1, eps=1e-5):
        if id(weight) in self.prefix_of:
            self.raw[self.prefix_of[id(weight)]] = x
        return super().batch_norm(x, running_mean, running_var, weight, bias, training, momentum, eps)


def _run(sd, img, masks=None, out_features=("level3", "level4", "level5")):
    leaves = OrderedDict((k[:-len(".weight")], v) for k, v in sorted(sd.items()) if k.startswith(PREFIX + ".") and k.endswith(".norm.weight"))
    fn = _Recorder(masks, leaves)
    saved = O.F
    O.F = fn
    try:
        outs = O.dla34_forward(sd, img, out_features=out_features)
    finally:
        O.F = saved
    assert fn.bn_calls == len(leaves) == len(fn.raw), (fn.bn_calls, len(leaves))
    if masks is not None and len(masks) != len(fn.pre):
        raise ValueError(f"{len(masks)} masks for {len(fn.pre)} ReLU calls")
    return outs, fn


def forward(sd, img, out_features=("level3", "level4", "level5")):
    """{level<n>: tensor}: the bottom-up network on `img` (B, 3, H, W) with every norm on the batch's statistics."""
    with torch.no_grad():
        return _run(sd, img, None, out_features)[0]


def stats(c):
    """(mean, biased variance) per channel of a raw convolution output (B, C, h, w)."""
    mu = c.mean(dim=(0, 2, 3))
    return mu, ((c - mu.view(1, -1, 1, 1))**2).mean(dim=(0, 2, 3))


def stored_activations(sd, img):
    """dict(out={level<n>}, raw={norm prefix: c}, stats={norm prefix: (mu, v)}, relu_pre=[...], relu_out=[...]) of the forward."""
    with torch.no_grad():
        outs, fn = _run(sd, img)
    return dict(out=outs, raw=OrderedDict(fn.raw), stats=OrderedDict((p, stats(c)) for p, c in fn.raw.items()), relu_pre=list(fn.pre),
                relu_out=list(fn.out))


def chain_grads(model, masks, img, G, dtype=torch.float64):
    """({parameter name: gradient}, {backbone_level1, backbone_level0, backbone_base_layer: gradient at the stem's post-ReLU tensors, not
    masked by the tensor's own ReLU}) of sum_n <level<n>, G[level<n>]> by autograd through the batch-statistics forward in `dtype`;
    `masks`: one boolean tensor per ReLU call (call order) that replaces the derivative's own sign test, or None for the natural signs."""
    sd = state(model, dtype, grad=True)
    outs, fn = _run(sd, img.to(dtype), masks, out_features=tuple(sorted(G)))
    at = {"backbone_base_layer": fn.out[0], "backbone_level0": fn.out[1], "backbone_level1": fn.out[2]}
    for v in at.values():
        v.retain_grad()
    sum((outs[n] * G[n].to(dtype)).sum() for n in sorted(G)).backward()
    names = [k for k, _ in model.named_parameters() if k.startswith(PREFIX + ".")]
    return {k: sd[k].grad.detach() for k in names}, {k: v.grad.detach() for k, v in at.items()}


def expected_stats(model, stored, dtype=torch.float64):
    """The read-out LossPlan.backbone_batch_stats() should return, from stored["raw"] (the raw convolution outputs, NCHW)."""
    sd = model.state_dict()
    out = {}
    for p in norm_prefixes(model):
        c = stored["raw"][p].to(dtype)
        mu, v = stats(c)
        n = c.numel() // c.shape[1]
        out[p + ".batch_mean"], out[p + ".batch_var"] = mu, v
        out[p + ".running_mean"] = (1 - MOMENTUM) * sd[p + ".running_mean"].to(dtype) + MOMENTUM * mu
        out[p + ".running_var"] = (1 - MOMENTUM) * sd[p + ".running_var"].to(dtype) + MOMENTUM * v * (n / (n - 1))
    return out


@contextlib.contextmanager
def norms_on(model, towers=False, fpn=False):
    """Inside, tower_bn_oracle.bn_prefixes -- the norms whole_model_grad_oracle.whole_model_grads(batch_stats=True) switches to batch
    statistics -- names the bottom-up network's norms, and the towers' / the FPN's on request."""
    orig = TB.bn_prefixes
    chosen = set(norm_prefixes(model)) | (orig(model) if towers else set()) | (set(FN.norm_prefixes(model)) if fpn else set())
    TB.bn_prefixes = lambda m: set(chosen)
    try:
        yield chosen
    finally:
        TB.bn_prefixes = orig


# ------------------------------------------------------------------------------------------------- torch's own train() step
class ModuleWalk:
    """DLA.forward / Tree.forward / BasicBlock.forward / Root.forward written out over dd3d_amd.modeling.dla's own module tree (the modules
    are parameter containers without a forward), each Conv2d as F.conv2d followed by a torch.nn.BatchNorm2d in train() that carries the
    module's norm state: torch's own batch norm and its autograd, in `dtype` on `device`.  What tests/test_backbone_bn.py holds the
    oracle to, and what tests/gpu_backbone_bn_time.py times as torch's train()-mode step."""
    def __init__(self, dla, dtype=torch.float64, device="cpu"):
        self.dla, self.norms, self.leaves, self.relus, self.dtype, self.device = dla, {}, {}, [], dtype, device

    def conv(self, m, x, relu=False):
        bn = self.norms.get(id(m))
        if bn is None:
            bn = torch.nn.BatchNorm2d(m.out_channels, eps=m.norm.eps).to(self.dtype).train()
            bn.load_state_dict({k: (v.to(self.dtype) if v.is_floating_point() else v) for k, v in m.norm.state_dict().items()})
            self.norms[id(m)] = bn.to(self.device)
            self.leaves[id(m)] = m.weight.detach().to(self.device, self.dtype).requires_grad_(True)
        y = bn(F.conv2d(x, self.leaves[id(m)], None, stride=m.stride, padding=m.padding))
        return self.relu(y) if relu else y

    def relu(self, x):
        y = F.relu(x)
        self.relus.append(y)
        return y

    def block(self, m, x, residual):
        out = self.conv(m.conv1, x, relu=True)
        return self.relu(self.conv(m.conv2, out) + (x if residual is None else residual))

    def tree(self, m, x, children=None):
        children = [] if children is None else children
        bottom = F.max_pool2d(x, m.stride, stride=m.stride) if m.stride > 1 else x
        residual = self.conv(m.project, bottom) if m.project is not None else bottom
        if m.level_root:
            children.append(bottom)
        if m.levels == 1:
            x1 = self.block(m.tree1, x, residual)
            x2 = self.block(m.tree2, x1, None)
            return self.relu(self.conv(m.root.conv, torch.cat([x2, x1] + children, 1)))
        x1 = self.tree(m.tree1, x)
        children.append(x1)
        return self.tree(m.tree2, x1, children)

    def __call__(self, img):
        d = self.dla
        x = self.conv(d.base_layer, img, relu=True)
        for m in list(d.level0) + list(d.level1):
            x = self.conv(m, x, relu=True)
        outs = {}
        for lvl in range(2, 6):
            x = self.tree(getattr(d, f"level{lvl}"), x)
            outs[f"level{lvl}"] = x
        return outs


# ------------------------------------------------------------------------------------------------- one segment in closed form (the seam)
def apply_closed(c, gamma, beta, act, r=None, eps=EPS, dtype=torch.float64):
    """y of one segment: c, r (N, C); relu(n), n or relu(n + r) with n = (c - mu) * gamma / sqrt(v + eps) + beta.  Returns (y, mu, v)."""
    c = c.to(dtype)
    mu = c.mean(0)
    v = ((c - mu)**2).mean(0)
    n = (c - mu) * (gamma.to(dtype) * torch.rsqrt(v + eps)) + beta.to(dtype)
    if act == RESIDUAL:
        n = n + r.to(dtype)
    return (n if act == LINEAR else n.clamp(min=0)), mu, v


def backward_closed(c, mask, G, gamma, eps=EPS, dtype=torch.float64):
    """(q, p, G_c) of one segment: ghat = G * mask (mask None: G), q = sum ghat, p = sum ghat * xhat, G_c = s (ghat - q / N - xhat p / N)."""
    c, G = c.to(dtype), G.to(dtype)
    N = c.shape[0]
    mu = c.mean(0)
    rstd = torch.rsqrt(((c - mu)**2).mean(0) + eps)
    xh = (c - mu) * rstd
    gh = G if mask is None else G * mask.to(dtype)
    q, p = gh.sum(0), (gh * xh).sum(0)
    return q, p, gamma.to(dtype) * rstd * (gh - q / N - xh * (p / N))
