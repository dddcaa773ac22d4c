"""Dev tool (GPU): DD3D.compute_losses with and without head-map gradients, in one process and alternating, on a 4 x 384 x 1280 KITTI
batch (DD3D-DLA34) and one 6-camera 896 x 1600 nuScenes sample (NuscenesDD3D-DLA34), 48 synthetic GT per image:

  (a) compute_losses(inputs)                    the loss plan of the parent commit: trunk, heads, assign, terms
  (b) compute_losses(inputs, head_grads=True)   the same plan plus the dd3d_loss_backward launch, and the gradient maps cloned to NCHW
  (c) the loss stages alone (assign + terms + finalize) and the backward launch alone (denominators + per-target rows), on the plan's
      own buffers, device events

(a) and (b) are timed from the host call to a device synchronise, `--rounds` rounds of `--iters` calls each, taken in turn within a round;
reported: the median over all calls and the spread of the per-round medians (the method of tests/gpu_dense_depth_loss_time.py).

    python tests/gpu_loss_grad_time.py > profiles/loss_grads_time.txt
"""
import ctypes as C
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

g.build()
import dd3d_amd.modeling  # noqa: E402,F401
from dd3d_amd import META_ARCH_REGISTRY, get_cfg, hip  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_gt_instances, make_inputs, make_state_dict  # noqa: E402

CASES = [("dd3d_kitti_dla34", "dla34_kitti", 4, 384, 1280, "kitti"), ("dd3d_nusc_dla34", "dla34_nusc", 6, 896, 1600, "nusc")]


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def events(fn, rounds, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st = []
    for _ in range(rounds):
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        st.append(e0.elapsed_time(e1) / reps * 1e3)
    return st


def main():
    iters, rounds = arg("--iters", 20), arg("--rounds", 5)
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
        paths = [("(a) compute_losses", lambda: model.compute_losses(inputs)),
                 ("(b) compute_losses(head_grads=True)", lambda: model.compute_losses(inputs, head_grads=True))]
        for _, fn in paths:  # warm-up: plans, graph capture
            for _ in range(3):
                fn()
        times = {name: [] for name, _ in paths}
        for _ in range(rounds):
            for name, fn in paths:
                ts = []
                for _ in range(iters):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    ts.append((time.perf_counter() - t0) * 1e3)
                times[name].append(ts)
        plan = model.get_loss_plan(*model.canvas_size(inputs), grads=True)
        N = B * sum(f.H * f.W for f in plan.features)
        print(f"{exp} {B}x{H}x{W}: {N} targets, {int(plan.det_count.cpu())} positives, {sum(len(x) for x in gt)} GT")
        for name, _ in paths:
            allt = [t for r in times[name] for t in r]
            meds = [statistics.median(r) for r in times[name]]
            print(f"  {name}: median {statistics.median(allt):.3f} ms over {len(allt)} calls; per-round medians {min(meds):.3f} .. {max(meds):.3f} ms")
        a, ga, L_ = plan.loss_args, plan.grad_args, hip.lib()

        def fwd():
            hip.check(L_.dd3d_loss_assign(C.byref(a), hip.current_stream()), "assign")
            hip.check(L_.dd3d_loss_terms(C.byref(a), hip.current_stream()), "terms")

        bwd = lambda: hip.check(L_.dd3d_loss_backward(C.byref(a), C.byref(ga), hip.current_stream()), "backward")
        for what, fn in (("loss stages alone (assign + terms + finalize)", fwd), ("backward alone (denominators + per-target rows)", bwd)):
            st = events(fn, max(rounds, 5), 20)
            print(f"  (c) {what}, device events, 20 back-to-back calls per sample: median {statistics.median(st):.1f} us, "
                  f"range {min(st):.1f} .. {max(st):.1f} us")
        words = sum(t.numel() for t in plan.d_cls + plan.d_b2d + (plan.d_b3d or []))
        print(f"      gradient maps: {words * 4 / 1e6:.2f} MB written per backward (rows of {plan.cls_pitch} + {plan.b2d_pitch} + {plan.b3d_pitch} words)")
        del model, plan
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
