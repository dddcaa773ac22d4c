"""Dev tool (GPU): what the predictor layer's backward adds to the captured loss plan, beside the same gradients from a torch
composition, on DD3D-DLA34 at 384 x 1280 (B = 1 and 4, KITTI) and one 6-camera 896 x 1600 nuScenes sample, 48 synthetic GT per image:

  (a) the captured plan of compute_losses(head_grads=True) (the parent commit's largest plan) and of compute_losses(predictor_grads=True),
      replayed on staged inputs; device events around `--iters` replays, `--rounds` rounds, the two plans taken in turn within a round;
      reported: the median over the rounds and their range, and the difference = the added cost
  (b) each group's weight-gradient call (four launches) and input-gradient call (one launch) alone, on the plan's own buffers
  (c) the same gradients by torch autograd on the same device: (F.conv2d(a_l, W) + b) * s_l contracted with the masked head-map gradient,
      backward to W, b, s_l and a_l, over the decoded tower outputs (float32 NCHW, made once outside the timed region), all levels and
      the three groups; forward + backward, and an estimate of the backward alone (the difference to a forward-only pass)

    python tests/gpu_predictor_grad_time.py > profiles/predictor_grads_time.txt
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


def report(name, st):
    print(f"  {name}: median {statistics.median(st):.1f} us, range {min(st):.1f} .. {max(st):.1f} us over {len(st)} rounds")
    return statistics.median(st)


def torch_composition(plan):
    """(forward + backward, forward only) closures of the torch composition on the plan's decoded tower outputs."""
    groups = []
    for grp in plan.pred_groups.values():
        gr, maps, w, bias, scale, lo, _ = grp.keep
        t = {"cls": 0, "box2d": 1, "box3d": 2}[grp.tower]
        n = grp.n
        lvls = []
        for l in range(grp.L):
            a = plan.tower_out[l][t].nchw().float().contiguous().requires_grad_(True)
            gm = gr[l][..., :n].permute(0, 3, 1, 2)
            if lo is not None:
                m = maps[l][..., :n].permute(0, 3, 1, 2)
                gm = torch.where(torch.isfinite(lo)[None, :, None, None] & ~(m > lo[None, :, None, None]), torch.zeros_like(gm), gm)
            lvls.append((a, gm.contiguous(), scale[l].clone().requires_grad_(True)))
        W = w[0].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        groups.append((lvls, W, bias[0].clone().requires_grad_(True)))

    def forward():
        total = 0
        for lvls, W, b in groups:
            for a, gm, s in lvls:
                total = total + ((F.conv2d(a, W, b, padding=1) * s[None, :, None, None]) * gm).sum()
        return total

    def both():
        for lvls, W, b in groups:
            W.grad = b.grad = None
            for a, _, s in lvls:
                a.grad = s.grad = None
        forward().backward()

    def fwd_only():
        with torch.no_grad():
            forward()

    return both, fwd_only


def main():
    iters, rounds = arg("--iters", 20), arg("--rounds", 7)
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
            model.compute_losses(inputs, head_grads=True)
            model.compute_losses(inputs, predictor_grads=True)
        size = model.canvas_size(inputs)
        plan_g, plan_p = model.get_loss_plan(*size, grads=True), model.get_loss_plan(*size, pred_grads=True)
        pixels = B * sum(f.H * f.W for f in plan_p.features)
        print(f"{exp} {B}x{H}x{W}: {pixels} pixels over {len(plan_p.features)} levels, {int(plan_p.det_count.cpu())} positives, "
              f"activations: {('f32', 'f16x2', 'bf16x3')[plan_p.pred_groups['cls_map'].args.act_mode]}")
        tg, tp = [], []
        for _ in range(rounds):
            tg.append(events(plan_g.run, iters))
            tp.append(events(plan_p.run, iters))
        a = report("(a) captured plan, head_grads (parent)", tg)
        b = report("(a) captured plan, predictor_grads", tp)
        print(f"      added by the predictor backward: {b - a:.1f} us ({(b - a) / a * 100:.1f} % of the parent's plan)")
        L_, total = hip.lib(), 0.0
        for name, grp in plan_p.pred_groups.items():
            wg = lambda grp=grp: hip.check(L_.dd3d_predictor_wgrad(C.byref(grp.args), hip.current_stream()), "wgrad")
            dg = lambda grp=grp: hip.check(L_.dd3d_predictor_dgrad(C.byref(grp.args), hip.current_stream()), "dgrad")
            total += report(f"(b) {name} (n = {grp.n}, {grp.n_slices} slices) weight gradient, 4 launches", [events(wg, iters) for _ in range(rounds)])
            total += report(f"(b) {name} input gradient, 1 launch", [events(dg, iters) for _ in range(rounds)])
        print(f"      sum of the calls alone: {total:.1f} us")
        both, fwd_only = torch_composition(plan_p)
        for _ in range(5):
            both()
            fwd_only()
        torch.cuda.synchronize()
        tb = report("(c) torch composition, forward + backward", [events(both, iters) for _ in range(rounds)])
        tf = report("(c) torch composition, forward only", [events(fwd_only, iters) for _ in range(rounds)])
        print(f"      torch backward alone (difference): {tb - tf:.1f} us; fused added cost / torch backward = {(b - a) / max(tb - tf, 1e-9):.2f}, "
              f"fused added cost / torch forward + backward = {(b - a) / tb:.2f}")
        del model, plan_g, plan_p, both, fwd_only
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
