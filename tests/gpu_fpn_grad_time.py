"""Dev tool (GPU): what the FPN's backward adds to the captured loss plan, beside one baseline on the same tensors, on DD3D-DLA34 at
384 x 1280 (B = 1 and 4, KITTI) and one 6-camera 896 x 1600 nuScenes sample, 48 synthetic GT per image:

  (a) the captured plan of compute_losses(tower_grads=True) (the parent commit's largest plan) and of compute_losses(fpn_grads=True),
      replayed on staged inputs; device events around `--iters` replays, `--rounds` rounds, the two plans taken in turn within a round;
      reported: the median over the rounds and their range, and the difference = the added cost
  (b) every FPN layer's weight-gradient call (three launches per level) and input-gradient call (one launch per level) alone, on the
      plan's own buffers, with each GEMM's fraction of the 155 TF f32-matrix peak (2 * output pixels * Cout * k * k * Cin flop per GEMM)
  (c) the baseline: torch autograd in float32 over the same composition (laterals, top-down sum, output convolutions, P6, P7 with their
      folded scales) on decoded f32 NCHW inputs; forward + backward, and an estimate of the backward alone (the difference to a
      forward-only pass)

    python tests/gpu_fpn_grad_time.py > profiles/fpn_grads_time.txt
"""
import ctypes as C
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

g.build()
import dd3d_amd.modeling  # noqa: E402,F401
from dd3d_amd import META_ARCH_REGISTRY, get_cfg, hip  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_gt_instances, make_inputs, make_state_dict  # noqa: E402

CASES = [("dd3d_kitti_dla34", "dla34_kitti", 1, 384, 1280, "kitti"), ("dd3d_kitti_dla34", "dla34_kitti", 4, 384, 1280, "kitti"),
         ("dd3d_nusc_dla34", "dla34_nusc", 6, 896, 1600, "nusc")]
PEAK_TF = 155.0


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def report(name, st, flop=None):
    med = statistics.median(st)
    rate = f", {flop / med * 1e-6:.1f} TF = {flop / med * 1e-6 / PEAK_TF * 100:.0f} % of the {PEAK_TF:.0f} TF f32-matrix peak" if flop else ""
    print(f"  {name}: median {med:.1f} us, range {min(st):.1f} .. {max(st):.1f} us over {len(st)} rounds{rate}")
    return med, min(st), max(st)


def torch_fpn(model, plan):
    """The FPN of `model` as plain float32 torch on the plan's decoded backbone features, with the gradients the plan's backward read."""
    from dd3d_amd.layers import fold_norm
    fpn = model.backbone
    names, stages = list(fpn.in_features), list(fpn.stages)
    X = [plan.bottom_up[n].nchw().float().contiguous().requires_grad_(True) for n in names]
    mods = {}
    for key in [f"fpn_lateral{s}" for s in stages] + [f"fpn_output{s}" for s in stages]:
        mods[key] = getattr(fpn, key)
    if fpn.top_block is not None:
        mods["p6"] = fpn.top_block.p6
        if fpn.top_block.num_levels == 2:
            mods["p7"] = fpn.top_block.p7
    P = {}
    for key, conv in mods.items():
        s, t = fold_norm(conv, None)
        P[key] = (conv.weight.detach().float().clone().requires_grad_(True), s.to(plan.device).clone().requires_grad_(True),
                  t.to(plan.device).clone().requires_grad_(True))
    sel = list(model.in_features)
    G = {n: plan.feature_grads[sel.index(n)].permute(0, 3, 1, 2).contiguous() for n in fpn._out_features if n in sel}

    def conv(key, x, stride=1):
        w, s, t = P[key]
        return F.conv2d(x, w, stride=stride, padding=(w.shape[-1] - 1) // 2) * s[None, :, None, None] + t[None, :, None, None]

    def forward():
        outs, prev = {}, None
        for i in reversed(range(len(stages))):
            lat = conv(f"fpn_lateral{stages[i]}", X[i])
            if prev is not None:
                lat = lat + F.interpolate(prev, scale_factor=2.0, mode="nearest")
            prev = lat
            outs[f"p{stages[i]}"] = conv(f"fpn_output{stages[i]}", lat)
        if "p6" in P:
            outs[f"p{stages[-1] + 1}"] = conv("p6", outs[f"p{stages[-1]}"], 2)
        if "p7" in P:
            outs[f"p{stages[-1] + 2}"] = conv("p7", F.relu(outs[f"p{stages[-1] + 1}"]), 2)
        return sum((outs[k] * G[k]).sum() for k in G)

    leaves = X + [v for tup in P.values() for v in tup]

    def both():
        for t in leaves:
            t.grad = None
        forward().backward()

    def fwd_only():
        with torch.no_grad():
            forward()

    return both, fwd_only


def main():
    iters, rounds = arg("--iters", 10), arg("--rounds", 5)
    for exp, tag, B, H, W, ds in CASES:
        cfg = get_cfg(exp)
        model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
        model.load_state_dict(make_state_dict(model, calib=load_calib(tag)))
        model = model.to("cuda").eval()
        nusc = hasattr(model, "attr_logits")
        inputs = make_inputs(B, H, W, dataset=ds)
        gt = make_gt_instances(inputs, model.num_classes, cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, n_per_image=48,
                               num_attributes=model.attr_logits.out_channels if nusc else None)
        for x, inst in zip(inputs, gt):
            x["instances"] = inst
        for _ in range(3):  # plans, graph capture, staged inputs
            model.compute_losses(inputs, tower_grads=True)
            model.compute_losses(inputs, fpn_grads=True)
        size = model.canvas_size(inputs)
        plan_t, plan_f = model.get_loss_plan(*size, tower_grads=True), model.get_loss_plan(*size, fpn_grads=True)
        out = plan_f.fpn_layers["outputs"]
        print(f"{exp} {B}x{H}x{W}: FPN stages {[tuple(hw) for hw in out.in_hw]}, {int(plan_f.det_count.cpu())} positives, "
              f"activations: {('f32', 'f16x2', 'bf16x3')[out.args.x_mode]}, slab {plan_f.tower_slab[0].numel() * 4 / 2**20:.0f} MiB "
              f"(tower_grads plan: {plan_t.tower_slab[0].numel() * 4 / 2**20:.0f} MiB)")
        tt, tf = [], []
        for _ in range(rounds):
            tt.append(events(plan_t.run, iters))
            tf.append(events(plan_f.run, iters))
        a = report("(a) captured plan, tower_grads (parent)", tt)[0]
        b = report("(a) captured plan, fpn_grads", tf)[0]
        layers = len(plan_t.tower_layers)
        print(f"      added by the FPN's backward: {b - a:.1f} us ({(b - a) / a * 100:.1f} % of the parent's plan)")
        L_, total = hip.lib(), 0.0
        for key, lay in plan_f.fpn_layers.items():
            flop = 2.0 * B * sum(h * w for h, w in lay.out_hw) * lay.Cout * lay.ksize**2 * lay.Cin
            wg = lambda lay=lay: hip.check(L_.dd3d_fpn_wgrad(C.byref(lay.args), hip.current_stream()), "wgrad")
            dg = lambda lay=lay: hip.check(L_.dd3d_fpn_dgrad(C.byref(lay.args), hip.current_stream()), "dgrad")
            w_ = report(f"(b) {key} weight gradient, {3 * lay.L} launches", [events(wg, iters) for _ in range(rounds)], flop)
            d_ = report(f"(b) {key} input gradient, {lay.L} launches", [events(dg, iters) for _ in range(rounds)], flop)
            total += w_[0] + d_[0]
        print(f"      sum of the calls alone: {total:.1f} us ({layers} tower layers in the parent's plan)")
        both, fwd_only = torch_fpn(model, plan_f)
        for _ in range(3):
            both()
            fwd_only()
        torch.cuda.synchronize()
        tb = report("(c) torch autograd over the FPN, forward + backward", [events(both, iters) for _ in range(rounds)])[0]
        tfo = report("(c) torch autograd over the FPN, forward only", [events(fwd_only, iters) for _ in range(rounds)])[0]
        print(f"      torch backward alone (difference): {tb - tfo:.1f} us; new kernels / torch backward = {total / max(tb - tfo, 1e-9):.2f}")
        del model, plan_t, plan_f, both, fwd_only
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
