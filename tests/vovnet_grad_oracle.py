"""CPU oracle of the VoVNet-V2 backward (tests/test_vovnet_grads.py, tests/test_vovnet_grads_gpu.py, tests/test_vovnet_whole_model_gpu.py):
own statements of the 3x3 stride-2 ceil-mode max-pool backward and of the eSE gate backward as include/dd3d_hip.h states them, torch
autograd of oracle.vovnet_oracle._osa under the stored tensors' ReLU masks, a tiny VoVNet spec for the one-stage chain, and the map from
the oracle forward's ReLU calls to a LossPlan's stored VoVNet tensors (every ReLU but stem_1's)."""
from collections import OrderedDict
from types import SimpleNamespace

import torch

from oracle import vovnet_oracle as VO
from tests import whole_model_grad_oracle as WO
from tests.util import decode

MINI = "V-mini-test-eSE"  # two layers per module, 32 / 64 channels; stage2 has two modules, the second with the identity add
MINI_SPEC = dict(stem=[32, 32, 32], stage_conv_ch=[32, 32, 32, 32], stage_out_ch=[64, 64, 64, 64], layer_per_block=2, block_per_stage=[2, 1, 1, 1])


def pool3_out(n):
    """MaxPool2d(3, 2, ceil_mode=True) on n >= 3 rows: ceil((n - 3) / 2) + 1, minus one when the last window would start outside."""
    o = -(-(n - 3) // 2) + 1
    return o - 1 if (o - 1) * 2 >= n else o


def pool3_argmax(x):
    """(by, bx) [B, C, Ho, Wo] of every window's arg-max in x [B, C, H, W]: windows clipped at the border, the first maximum in row-major
    window order wins (a later entry wins only when it is larger)."""
    B, C_, H, W = x.shape
    Ho, Wo = pool3_out(H), pool3_out(W)
    by, bx = torch.zeros(B, C_, Ho, Wo, dtype=torch.long), torch.zeros(B, C_, Ho, Wo, dtype=torch.long)
    for oy in range(Ho):
        for ox in range(Wo):
            top = x[:, :, 2 * oy, 2 * ox].clone()
            iy, ix = torch.full_like(by[:, :, 0, 0], 2 * oy), torch.full_like(by[:, :, 0, 0], 2 * ox)
            for yy in range(2 * oy, min(2 * oy + 3, H)):
                for xx in range(2 * ox, min(2 * ox + 3, W)):
                    better = x[:, :, yy, xx] > top
                    top = torch.where(better, x[:, :, yy, xx], top)
                    iy, ix = torch.where(better, torch.full_like(iy, yy), iy), torch.where(better, torch.full_like(ix, xx), ix)
            by[:, :, oy, ox], bx[:, :, oy, ox] = iy, ix
    return by, bx


def pool3_backward(x, g, dtype=torch.float32, add=None):
    """da = add (or 0), then for the windows in ascending (oy, ox): da[arg-max of the window] += g[oy, ox] -- own statement (no autograd)."""
    B, C_, H, W = x.shape
    by, bx = pool3_argmax(x)
    da = add.to(dtype).clone() if add is not None else torch.zeros(B, C_, H, W, dtype=dtype)
    flat = da.view(B, C_, H * W)
    for oy in range(by.shape[2]):
        for ox in range(by.shape[3]):
            idx = (by[:, :, oy, ox] * W + bx[:, :, oy, ox])[..., None]
            flat.scatter_add_(2, idx, g[:, :, oy, ox, None].to(dtype))  # (one element per (b, c): a single add each, in window order)
    return da


def ese_backward(xt, g, fc_w, fc_b, dtype=torch.float64):
    """The eSE formulas of include/dd3d_hip.h on NCHW tensors: {m, z, s, dz, g_xt, d_fc_w, d_fc_b}; g_xt is not masked by xt's ReLU."""
    X, G, Wf, bf = xt.to(dtype), g.to(dtype), fc_w.to(dtype).reshape(fc_w.shape[0], -1), fc_b.to(dtype)
    HW = X.shape[2] * X.shape[3]
    m = X.sum((2, 3)) / HW
    z = m @ Wf.t() + bf
    s = (z + 3).clamp(0, 6) / 6
    ds = (G * X).sum((2, 3))
    dz = torch.where((z > -3) & (z < 3), ds / 6, torch.zeros_like(ds))
    u = (dz @ Wf) / HW
    return {"m": m, "z": z, "s": s, "dz": dz, "g_xt": G * s[:, :, None, None] + u[:, :, None, None], "d_fc_w": dz.t() @ m, "d_fc_b": dz.sum(0)}


# ------------------------------------------------------------------------------------------------- a tiny VoVNet and its OSA stage
def mini_vovnet(norm="BN", seed=31):
    """A VoVNet of MINI_SPEC (registered at run time) with seeded parameters and norm statistics; eSE weights and biases spread so that the
    gates of a rectified random input fall into all three regions of the hard sigmoid."""
    from dd3d_amd.modeling import vovnet as MV
    MV._STAGE_SPECS[MINI] = MINI_SPEC
    VO.SPECS[MINI] = (MINI_SPEC["stem"], MINI_SPEC["stage_conv_ch"], MINI_SPEC["stage_out_ch"], MINI_SPEC["layer_per_block"], MINI_SPEC["block_per_stage"])
    vov = MV.VoVNet(SimpleNamespace(NAME=MINI, NORM=norm), 3, out_features=["stage2", "stage3", "stage4", "stage5"])
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, mod in vov.named_modules():
            w = getattr(mod, "weight", None)
            if w is not None and w.dim() == 4:
                k = w.shape[-1]
                w.copy_(torch.randn(w.shape, generator=gen) * (1.4 / (k * k * w.shape[1])**0.5))
                if getattr(mod, "bias", None) is not None:  # the eSE fc: biases across the clamp's three regions
                    w.mul_(4.0)
                    mod.bias.copy_(torch.linspace(-5.0, 5.0, w.shape[0])[torch.randperm(w.shape[0], generator=gen)])
            elif hasattr(mod, "running_mean"):
                n = mod.running_mean.shape[0]
                mod.weight.copy_(0.5 + torch.rand(n, generator=gen)), mod.bias.copy_(torch.randn(n, generator=gen) * 0.2)
                mod.running_mean.copy_(torch.randn(n, generator=gen) * 0.2), mod.running_var.copy_(0.5 + torch.rand(n, generator=gen))
    return vov.eval()


def state(vov, dtype, prefix="backbone.bottom_up"):
    """The state dict of `vov` in `dtype` under `prefix`, parameters as autograd leaves."""
    sd = {f"{prefix}.{k}": v.detach().to(dtype).clone() for k, v in vov.state_dict().items() if v.is_floating_point()}
    for k, _ in vov.named_parameters():
        sd[f"{prefix}.{k}"].requires_grad_(True)
    return sd


def stage_forward(vov, sname, x, dtype, masks=None, prefix="backbone.bottom_up"):
    """oracle.vovnet_oracle._osa over the modules of one stage (no pool) on the module input x (NCHW).  Returns (the stage output, the
    autograd leaves {name: tensor} with "x", the ReLU outputs in call order: per module its layers, then xt)."""
    sd = state(vov, dtype, prefix)
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    stage = getattr(vov, sname)
    with WO.intercepted(masks) as rec:
        y = xin
        for mname, m in stage.named_children():
            y = VO._osa(sd, f"{prefix}.{sname}.{mname}", mname, y, len(m.layers), m.identity)
    return y, dict(sd, x=xin), rec["F"].out


def stage_stored(vov, sname, x):
    """The tensors BackboneLowering._vovnet stores for one stage, from a float32 forward on x: {<stage>.<module>.cat, <stage>.<module>.xt,
    <stage>.out} (NCHW), and the ReLU masks in call order."""
    y, _, outs = stage_forward(vov, sname, x, torch.float32)
    S, k, xin = OrderedDict(), 0, x.float()
    mods = list(getattr(vov, sname).named_children())
    with torch.no_grad():
        for j, (mname, m) in enumerate(mods):
            n = len(m.layers)
            S[f"{sname}.{mname}.cat"] = torch.cat([xin] + [outs[k + i].detach() for i in range(n)], 1)
            xt = S[f"{sname}.{mname}.xt"] = outs[k + n].detach()
            k += n + 1
            fc = m.ese.fc
            gate = (torch.nn.functional.conv2d(xt.mean((2, 3), keepdim=True), fc.weight.float(), fc.bias.float()) + 3.0).clamp(0, 6) / 6.0
            xin = xt * gate + (xin if m.identity else 0.0)
        S[f"{sname}.out"] = xin
    assert torch.allclose(xin, y.detach(), rtol=1e-5, atol=1e-6)
    return S, [o.detach() > 0 for o in outs]


def stage_autograd(vov, sname, x, G, dtype, masks, prefix="backbone.bottom_up"):
    """({parameter name: gradient}, the gradient at x) of sum(stage output * G) by autograd in `dtype` under the given ReLU masks."""
    y, leaves, _ = stage_forward(vov, sname, x, dtype, masks, prefix)
    (y * G.to(dtype)).sum().backward()
    params = {k: v.grad for k, v in leaves.items() if k != "x" and v.grad is not None}
    return params, leaves["x"].grad


# ------------------------------------------------------------------------------------------------- the masks of a plan's stored tensors
def vovnet_sites(plan):
    """(label, Buf, first channel, channels, False) per ReLU call of oracle.vovnet_oracle.vovnet_forward, in call order: None for stem_1
    (no compared quantity depends on its sign), stem_2 (`stem.1`), stem_3 (the input slice of stage2's first concat buffer), then per OSA
    module its layers' slices of the concat buffer and the pre-eSE tensor xt."""
    vov = plan.model.backbone.bottom_up
    first = f"stage2.{next(iter(vov.stage2.named_children()))[0]}.cat"
    c3 = int(getattr(vov.stem, vov.stem_seqs[2][0]).weight.shape[0])
    sites = [None, ("stem.1", plan.bufs["stem.1"], 0, None, False), ("stem_3", plan.bufs[first], 0, c3, False)]
    for sname in vov.stage_names:
        for mname, m in getattr(vov, sname).named_children():
            cat = f"{sname}.{mname}.cat"
            sites += [(f"{cat}[{i}]", plan.bufs[cat], m.in_ch + i * m.stage_ch, m.stage_ch, False) for i in range(len(m.layers))]
            sites.append((f"{sname}.{mname}.xt", plan.bufs[f"{sname}.{mname}.xt"], 0, None, False))
    return sites


def relu_sites(plan):
    """whole_model_grad_oracle.relu_sites with the VoVNet's ReLU calls mapped to the plan's stored tensors (all but stem_1's)."""
    sites = WO.relu_sites(plan)
    mine = vovnet_sites(plan)
    assert all(s is None for s in sites[:len(mine)]) and WO.free_relus(plan.model) == len(mine)
    return mine + sites[len(mine):]


def plan_masks(plan, pre64, report=None):
    """whole_model_grad_oracle.plan_masks over `relu_sites` above: one boolean mask per ReLU call from the sign of the plan's decoded
    stored tensor, each validated by value against the float64 forward (STORED_TOL); stem_1 keeps the oracle's own sign."""
    sites = relu_sites(plan)
    if len(sites) != len(pre64):
        raise ValueError(f"{len(sites)} plan tensors for {len(pre64)} ReLU calls of the oracle forward")
    masks = []
    for k, (site, pre) in enumerate(zip(sites, pre64)):
        if site is None:
            masks.append(pre > 0)
            continue
        label, buf, c0, n, stored_is_pre = site
        got = decode(buf, c0, n).double()
        ref = pre.double() if stored_is_pre else pre.double().clamp(min=0)
        if tuple(got.shape) != tuple(ref.shape):
            raise ValueError(f"ReLU call {k} ({label}): stored {tuple(got.shape)}, oracle {tuple(ref.shape)}")
        err, tol = float((got - ref).abs().max()), WO.STORED_TOL * max(1.0, float(ref.abs().max()))
        if not err <= tol:
            raise ValueError(f"ReLU call {k} ({label}): the stored tensor is {err:.3e} from the oracle's (bar {tol:.3e})")
        mask = got > 0
        masks.append(mask)
        if report is not None:
            bad = mask != (pre > 0)
            far = bad & (pre.abs() > WO.SIGN_NEAR * float(pre.abs().max()))
            report.append((label, pre.numel(), int(bad.sum()), int(far.sum())))
    return masks


def whole_model_grads(model_cpu, cfg, inputs, gt, dtype, masks=None, inv_K=None, extras=None):
    """whole_model_grad_oracle.whole_model_grads of a VoVNet model, its tensor gradients extended by backbone_stem_1: the gradient at the
    FIRST ReLU call's output (stem_1's post-ReLU tensor), not masked by that tensor's own ReLU -- the convention of backbone_level1."""
    kept = []

    class _KeepFirst(WO._Functional):
        def relu(self, x, inplace=False):
            y = super().relu(x, inplace)
            if len(self.out) == 1 and y.requires_grad:
                y.retain_grad()
                kept.append(y)
            return y

    saved, WO._Functional = WO._Functional, _KeepFirst
    try:
        params, at, pre = WO.whole_model_grads(model_cpu, cfg, inputs, gt, dtype, masks=masks, inv_K=inv_K, extras=extras)
    finally:
        WO._Functional = saved
    assert len(kept) == 1 and kept[0].grad is not None
    return params, dict(at, backbone_stem_1=kept[0].grad.detach()), pre


def ese_gates64(model_cpu, relu_out):
    """{<stage>.<module>: z [B, C]} of every eSE gate from the float64 forward's ReLU outputs (call order of vovnet_forward)."""
    vov = model_cpu.backbone.bottom_up
    k, out = 3, OrderedDict()
    for sname in vov.stage_names:
        for mname, m in getattr(vov, sname).named_children():
            xt = relu_out[k + len(m.layers)].double()
            k += len(m.layers) + 1
            fc = m.ese.fc
            out[f"{sname}.{mname}"] = xt.mean((2, 3)) @ fc.weight.detach().double().reshape(m.concat_ch, m.concat_ch).t() + fc.bias.detach().double()
    return out


def vovnet_param_names(model):
    """The names vovnet_grads adds to param_grads: every parameter of backbone.bottom_up but stem_1's."""
    return sorted(k for k, _ in model.named_parameters() if k.startswith("backbone.bottom_up.") and ".stem.stem_1/" not in k)


def family_of(name):
    """filter (a convolution's weight), fc_weight / fc_bias (the eSE gate), norm_weight / norm_bias (a BN backbone)."""
    if ".ese.fc." in name:
        return "fc_weight" if name.endswith(".weight") else "fc_bias"
    if "/norm." in name:
        return "norm_weight" if name.endswith(".weight") else "norm_bias"
    return "filter"
