"""Dev tool (GPU): what the DLA-34 backbone's backward adds to the captured loss plan, beside one baseline on the same tensors, on
DD3D-DLA34 at 384 x 1280 (B = 1 and 4, KITTI) and one 6-camera 896 x 1600 nuScenes sample, 48 synthetic GT per image:

  (a) the captured plan of compute_losses(fpn_grads=True) (the parent commit's largest plan) and of compute_losses(backbone_grads=True),
      replayed on staged inputs; device events around `--iters` replays, `--rounds` rounds, the two plans taken in turn within a round;
      reported: the median over the rounds and their range, and the difference = the added cost
  (b) every call of the backbone backward alone on the plan's own buffers -- weight gradient (three launches), input gradient (one),
      pool backward (one) -- with each GEMM's fraction of the 155 TF f32-matrix peak (2 * output pixels * Cout * k * k * Cin flop per
      GEMM), summed per level and per kernel; one tower layer of the same plan measured the same way as the unit of the work count
  (c) the baseline: torch autograd in float32 over the same composition (level2 .. level5 with their folded scales, max-pools, concats)
      on the decoded level1 tensor; forward + backward, and an estimate of the backward alone (the difference to a forward-only pass)

    python tests/gpu_backbone_grad_time.py > profiles/backbone_grads_time.txt
"""
import ctypes as C
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.gpu_fpn_grad_time import CASES, arg, events, report  # noqa: E402  (builds the library on import)
import dd3d_amd.modeling  # noqa: E402,F401
from dd3d_amd import META_ARCH_REGISTRY, get_cfg, hip  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_gt_instances, make_inputs, make_state_dict  # noqa: E402


def torch_dla(model, plan):
    """level2 .. level5 of `model` as plain float32 torch on the plan's decoded level1 tensor, with the gradients the FPN's backward sends."""
    from dd3d_amd.layers import fold_norm
    dla = model.backbone.bottom_up
    x0 = plan.bufs[f"level1.{len(dla.level1) - 1}"].nchw().float().contiguous().requires_grad_(True)
    P = {}
    for key, m in dla.named_modules():
        if key.split(".")[0] in ("level2", "level3", "level4", "level5") and getattr(getattr(m, "weight", None), "dim", lambda: 0)() == 4:
            s, t = fold_norm(m, None)
            P[id(m)] = (m.weight.detach().float().clone().requires_grad_(True), s.to(plan.device).clone().requires_grad_(True),
                        t.to(plan.device).clone().requires_grad_(True), m.stride)
    G = {n: d[..., :c].permute(0, 3, 1, 2).contiguous() for n, (d, c) in plan.backbone_feature_grads.items()}

    def conv(m, x, relu=False, res=None):
        w, s, t, st = P[id(m)]
        y = F.conv2d(x, w, stride=st, padding=(w.shape[-1] - 1) // 2) * s[None, :, None, None] + t[None, :, None, None]
        y = y if res is None else y + res
        return F.relu(y) if relu else y

    def tree(m, x, children=None):
        children = [] if children is None else children
        bottom = F.max_pool2d(x, 2, 2) if m.stride > 1 else x
        residual = conv(m.project, bottom) if m.project is not None else bottom
        if m.level_root:
            children.append(bottom)
        if m.levels == 1:
            x1 = conv(m.tree1.conv2, conv(m.tree1.conv1, x, True), True, residual)
            x2 = conv(m.tree2.conv2, conv(m.tree2.conv1, x1, True), True, x1)
            return conv(m.root.conv, torch.cat([x2, x1] + children, 1), True)
        x1 = tree(m.tree1, x)
        children.append(x1)
        return tree(m.tree2, x1, children)

    def forward():
        x, total = x0, 0.0
        for lvl in (2, 3, 4, 5):
            x = tree(getattr(dla, f"level{lvl}"), x)
            if f"level{lvl}" in G:
                total = total + (x * G[f"level{lvl}"]).sum()
        return total

    leaves = [x0] + [v for tup in P.values() for v in tup[:3]]

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
    only = arg("--case", -1)
    for ci, (exp, tag, B, H, W, ds) in enumerate(CASES):
        if only >= 0 and ci != only:
            continue
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
            model.compute_losses(inputs, fpn_grads=True)
            model.compute_losses(inputs, backbone_grads=True)
        size = model.canvas_size(inputs)
        plan_f, plan_b = model.get_loss_plan(*size, fpn_grads=True), model.get_loss_plan(*size, backbone_grads=True)
        root = plan_b.backbone_layers["level5.root"]
        words = sum(t.numel() for lay in plan_b.backbone_layers.values() for t, _ in lay._raw)
        filt = sum(lay.keep[1].numel() for k, lay in plan_b.backbone_layers.items() if not k.endswith(".pool"))
        print(f"{exp} {B}x{H}x{W}: level5 {root.H}x{root.W}, {int(plan_b.det_count.cpu())} positives, activations: "
              f"{('f32', 'f16x2', 'bf16x3')[root.args.x_mode]}, slab {plan_b.tower_slab[0].numel() * 4 / 2**20:.0f} MiB (fpn_grads plan: "
              f"{plan_f.tower_slab[0].numel() * 4 / 2**20:.0f} MiB), added memory: outputs {words * 4 / 2**20:.0f} MiB + f32 filters {filt * 4 / 2**20:.0f} MiB")
        tf, tb = [], []
        for _ in range(rounds):
            tf.append(events(plan_f.run, iters))
            tb.append(events(plan_b.run, iters))
        a = report("(a) captured plan, fpn_grads (parent)", tf)[0]
        b = report("(a) captured plan, backbone_grads", tb)[0]
        print(f"      added by the backbone's backward: {b - a:.1f} us ({(b - a) / a * 100:.1f} % of the parent's plan)")
        L_ = hip.lib()
        tl = next(iter(plan_b.tower_layers.values()))
        tflop = 2.0 * B * sum(h * w for h, w in tl.level_hw) * tl.Cout * 9 * tl.Cin
        tw = report("(b) unit: one tower layer, weight gradient", [events(lambda: hip.check(L_.dd3d_tower_wgrad(C.byref(tl.args), hip.current_stream()), "w"), iters)
                                                                   for _ in range(rounds)], tflop)[0]
        td = report("(b) unit: one tower layer, input gradient", [events(lambda: hip.check(L_.dd3d_tower_dgrad(C.byref(tl.args), hip.current_stream()), "d"), iters)
                                                                  for _ in range(rounds)], tflop)[0]
        total, per_level, per_kernel, flops = 0.0, {}, {"wgrad": 0.0, "dgrad": 0.0, "pool": 0.0}, 0.0
        for key, lay in plan_b.backbone_layers.items():
            lvl = key.split(".")[0]
            if key.endswith(".pool"):
                p_ = report(f"(b) {key} pool backward {lay.H}x{lay.W}x{lay.C}", [events(lambda lay=lay: lay.launch(L_, hip.current_stream()), iters) for _ in range(rounds)])[0]
                per_kernel["pool"] += p_
                per_level[lvl] = per_level.get(lvl, 0.0) + p_
                total += p_
                continue
            flop = 2.0 * B * lay.Ho * lay.Wo * lay.Cout * lay.ksize**2 * lay.Cin
            flops += 2 * flop
            wg = lambda lay=lay: hip.check(L_.dd3d_backbone_wgrad(C.byref(lay.args), hip.current_stream()), "wgrad")
            dg = lambda lay=lay: hip.check(L_.dd3d_backbone_dgrad(C.byref(lay.args), hip.current_stream()), "dgrad")
            shape = f"{lay.ksize}x{lay.ksize}s{lay.stride} {lay.Cin}->{lay.Cout} at {lay.H}x{lay.W}"
            w_ = report(f"(b) {key} weight gradient ({shape})", [events(wg, iters) for _ in range(rounds)], flop)[0]
            d_ = report(f"(b) {key} input gradient", [events(dg, iters) for _ in range(rounds)], flop)[0]
            per_kernel["wgrad"] += w_
            per_kernel["dgrad"] += d_
            per_level[lvl] = per_level.get(lvl, 0.0) + w_ + d_
            total += w_ + d_
        print(f"      sum of the calls alone: {total:.1f} us; per level: " + ", ".join(f"{k} {v:.1f}" for k, v in per_level.items()) +
              "; per kernel: " + ", ".join(f"{k} {v:.1f}" for k, v in per_kernel.items()))
        print(f"      work count: {flops / (2 * tflop):.2f} tower layers ({flops * 1e-9:.1f} GF); at the measured tower layer ({tw + td:.1f} us) that is "
              f"{flops / (2 * tflop) * (tw + td):.1f} us expected")
        both, fwd_only = torch_dla(model, plan_b)
        for _ in range(3):
            both()
            fwd_only()
        torch.cuda.synchronize()
        t2 = report("(c) torch autograd over level2 .. level5, forward + backward", [events(both, iters) for _ in range(rounds)])[0]
        t1 = report("(c) torch autograd over level2 .. level5, forward only", [events(fwd_only, iters) for _ in range(rounds)])[0]
        print(f"      torch backward alone (difference): {t2 - t1:.1f} us; new kernels / torch backward = {total / max(t2 - t1, 1e-9):.2f}")
        del model, plan_f, plan_b, both, fwd_only
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
