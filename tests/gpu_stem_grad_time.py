"""Dev tool (GPU): what the DLA-34 stem's backward adds to the captured loss plan, beside one baseline on the same tensors, on DD3D-DLA34
at 384 x 1280 (B = 1 and 4, KITTI) and one 6-camera 896 x 1600 nuScenes sample, 48 synthetic GT per image, all from the same run:

  (a) the captured plan of compute_losses(backbone_grads=True) (the parent commit's largest plan) and of compute_losses(stem_grads=True),
      replayed on staged inputs; device events around `--iters` replays, `--rounds` rounds, the two plans taken in turn within a round;
      reported: the median over the rounds and their range, and the difference = the added cost
  (b) every new call alone on the plan's own buffers -- weight gradient (three launches) and input gradient (one) of level1.0 and level0.0,
      the weight gradient of base_layer -- with the HBM bytes the call must move at least (every operand once: x, g and the stored y read,
      da written; the filter and the slab are small beside them) and the bandwidth that makes of the measured time, next to the GEMM's
      fraction of the 155 TF f32-matrix peak
  (c) the fused stem launch with and without KEEP, and the preprocess launch the stem-gradient plan adds
  (d) the baseline: torch autograd in float32 over the same three layers on the plan's normalised image, with the gradient the plan's
      level1.0 call read; forward + backward, and an estimate of the backward alone (the difference to a forward-only pass)
  (e) at one KITTI image: each family's error against the float64 layer oracle in units of the bar, 8 * max(d32, 2^-23 * max|g64|)

    python tests/gpu_stem_grad_time.py > profiles/stem_grads_time.txt
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

Y_BYTES = {hip.PG_ACT_F32: 4, hip.PG_ACT_F16X2: 4, hip.PG_ACT_BF16X3: 6}  # per channel of the stored output


def call_bytes(lay):
    """(weight gradient, input gradient) HBM bytes of one call, every large operand once."""
    npx, nopx = lay.B * lay.H * lay.W, lay.B * lay.Ho * lay.Wo
    gy = nopx * lay.Cout * (4 + Y_BYTES[lay.args.y_mode])
    return npx * lay.Cin * 4 + gy, gy + npx * lay.Cin * 4


def torch_stem(model, plan):
    from dd3d_amd.layers import fold_norm
    dla = model.backbone.bottom_up
    x0 = plan.bufs["img4"].t[..., :3].permute(0, 3, 1, 2).contiguous()
    P = []
    for m in (dla.base_layer, dla.level0[0], dla.level1[0]):
        s, t = fold_norm(m, None)
        P.append((m.weight.detach().float().clone().requires_grad_(True), s.to(plan.device).clone().requires_grad_(True),
                  t.to(plan.device).clone().requires_grad_(True), m.stride, m.padding))
    g = plan.level1_grad.permute(0, 3, 1, 2).contiguous()

    def forward():
        x = x0
        for w, s, t, st, pd in P:
            x = F.relu(F.conv2d(x, w, stride=st, padding=pd) * s[None, :, None, None] + t[None, :, None, None])
        return (x * g).sum()

    leaves = [v for tup in P for v in tup[:3]]

    def both():
        for t in leaves:
            t.grad = None
        forward().backward()

    def fwd_only():
        with torch.no_grad():
            forward()

    return both, fwd_only


def errors_against_float64(plan):
    from tests import stem_grad_oracle as SO
    from tests.util import decode
    for key, lay in plan.stem_layers.items():
        x, g = lay.keep[0].permute(0, 3, 1, 2).cpu(), lay.keep[1].permute(0, 3, 1, 2).cpu()
        y, w, sc = decode(plan.bufs[lay.src["y"][0]]), lay.keep[2].permute(0, 3, 1, 2).cpu(), lay.scale.cpu()
        r64, r32 = (SO.layer_grads(x, y, g, w, sc, lay.stride, dt) for dt in (torch.float64, torch.float32))
        nchw_w = lambda t: t.view(lay.Cout, lay.ksize, lay.ksize, lay.Cin).permute(0, 3, 1, 2).cpu()
        got = {"dw_level": nchw_w(lay.dw_level), "dw": nchw_w(lay.dw), "q": lay.q.cpu(), "r": lay.r.cpu()}
        if lay.da is not None:
            got["da"] = lay.da.permute(0, 3, 1, 2).cpu()
        else:
            r64, r32 = ({k: v for k, v in r.items() if k != "da"} for r in (r64, r32))
        a, b, k = SO.family_vectors(r64), SO.family_vectors(r32), SO.family_vectors(got)
        for fam in a:
            if a[fam].numel() == 0:
                continue
            bar, d32, gmax = SO.bar(a[fam], b[fam], torch.ones(a[fam].shape[0], dtype=torch.bool))
            dev = float((k[fam].double() - a[fam]).abs().max())
            print(f"  (e) {key} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} = {8 * dev / bar:.2f} of the factor 8")


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
            model.compute_losses(inputs, backbone_grads=True)
            model.compute_losses(inputs, stem_grads=True)
        size = model.canvas_size(inputs)
        plan_b, plan_s = model.get_loss_plan(*size, backbone_grads=True), model.get_loss_plan(*size, stem_grads=True)
        words = sum(t.numel() for lay in plan_s.stem_layers.values() for t, _ in lay._raw)
        kept = sum(plan_s.bufs[n].t.numel() for n in ("img4", "base", "level0.0") if n not in plan_b.bufs)
        print(f"{exp} {B}x{H}x{W}: {int(plan_s.det_count.cpu())} positives, fused stem: {plan_s.fused_stem}, slab {plan_s.tower_slab[0].numel() * 4 / 2**20:.0f} MiB "
              f"(backbone_grads plan: {plan_b.tower_slab[0].numel() * 4 / 2**20:.0f} MiB), added memory: gradients {words * 4 / 2**20:.0f} MiB + kept "
              f"img4 / base / level0.0 {kept * 4 / 2**20:.0f} MiB; slices: " + ", ".join(f"{k} {lay.n_slices}" for k, lay in plan_s.stem_layers.items()))
        tb, ts = [], []
        for _ in range(rounds):
            tb.append(events(plan_b.run, iters))
            ts.append(events(plan_s.run, iters))
        a = report("(a) captured plan, backbone_grads (parent)", tb)[0]
        b = report("(a) captured plan, stem_grads", ts)[0]
        print(f"      added by the stem's backward: {b - a:.1f} us ({(b - a) / a * 100:.1f} % of the parent's plan)")
        L_ = hip.lib()
        total = 0.0
        for key, lay in plan_s.stem_layers.items():
            flop = 2.0 * B * lay.Ho * lay.Wo * lay.Cout * lay.ksize**2 * lay.Cin
            wb, db = call_bytes(lay)
            shape = f"{lay.ksize}x{lay.ksize}s{lay.stride} {lay.Cin}->{lay.Cout} at {lay.H}x{lay.W}"
            wg = lambda lay=lay: hip.check(L_.dd3d_stem_wgrad(C.byref(lay.args), hip.current_stream()), "wgrad")
            w_ = report(f"(b) {key} weight gradient ({shape})", [events(wg, iters) for _ in range(rounds)], flop)[0]
            print(f"      {wb / 2**20:.0f} MiB at least: {wb / w_ * 1e-6:.2f} TB/s")
            total += w_
            if lay.with_dgrad:
                dg = lambda lay=lay: hip.check(L_.dd3d_stem_dgrad(C.byref(lay.args), hip.current_stream()), "dgrad")
                d_ = report(f"(b) {key} input gradient", [events(dg, iters) for _ in range(rounds)], flop)[0]
                print(f"      {db / 2**20:.0f} MiB at least: {db / d_ * 1e-6:.2f} TB/s")
                total += d_
        print(f"      sum of the calls alone: {total:.1f} us")
        stem_s = [op for op in plan_s.ops if (getattr(op, "desc", None) or {}).get("kind") == "fused_stem"]
        stem_b = [op for op in plan_b.ops if (getattr(op, "desc", None) or {}).get("kind") == "fused_stem"]
        if stem_s and stem_b:
            st = hip.current_stream
            k0 = report("(c) fused stem", [events(lambda: stem_b[0](L_, st()), iters) for _ in range(rounds)])[0]
            k1 = report("(c) fused stem with KEEP", [events(lambda: stem_s[0](L_, st()), iters) for _ in range(rounds)])[0]
            pre = [op for op in plan_s.ops if op.name == "preprocess"]
            p_ = report("(c) preprocess into img4", [events(lambda: pre[0](L_, st()), iters) for _ in range(rounds)])[0] if pre else 0.0
            print(f"      KEEP adds {k1 - k0:.1f} us for {2 * B * H * W * 16 * 4 / 2**20:.0f} MiB stored; with the preprocess launch {k1 - k0 + p_:.1f} us")
        both, fwd_only = torch_stem(model, plan_s)
        for _ in range(3):
            both()
            fwd_only()
        torch.cuda.synchronize()
        t2 = report("(d) torch autograd over base_layer, level0, level1, forward + backward", [events(both, iters) for _ in range(rounds)])[0]
        t1 = report("(d) torch autograd over base_layer, level0, level1, forward only", [events(fwd_only, iters) for _ in range(rounds)])[0]
        print(f"      torch backward alone (difference): {t2 - t1:.1f} us; new kernels / torch backward = {total / max(t2 - t1, 1e-9):.2f}")
        if ci == 0:
            errors_against_float64(plan_s)
        del model, plan_b, plan_s, both, fwd_only
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
