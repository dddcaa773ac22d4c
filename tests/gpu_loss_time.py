"""Dev tool (GPU): DD3D.compute_losses per call next to the inference forward alone, in the same run, on a 4 x 384 x 1280 KITTI batch
(DD3D-DLA34) and one 6-camera 896 x 1600 nuScenes sample (NuscenesDD3D-DLA34), 48 synthetic GT per image.  Both are timed from the host
call to its result (the forward: model(inputs) -> Instances; the losses: the dict, whose positive count is read back), device-synchronised,
median of `--iters`.  The loss stages alone (assignment, terms, finalize) are device events around the two launches on the plan's own
buffers.  Kernel times per launch come from a separate run under rocprofv3:

    python tests/gpu_loss_time.py > profiles/losses_time.txt
    rocprofv3 --kernel-trace --stats -d <dir> -- python tests/gpu_loss_time.py --iters 3
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


def timed(fn, iters):
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
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
        with torch.no_grad():
            model(inputs)
            losses = model.compute_losses(inputs)
        t_fwd = timed(lambda: model(inputs), iters)
        t_loss = timed(lambda: model.compute_losses(inputs), iters)
        plan = model.get_loss_plan(*model.canvas_size(inputs))
        a, L_ = plan.loss_args, hip.lib()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st = []
        for _ in range(iters):
            e0.record()
            hip.check(L_.dd3d_loss_assign(C.byref(a), hip.current_stream()), "assign")
            hip.check(L_.dd3d_loss_terms(C.byref(a), hip.current_stream()), "terms")
            e1.record()
            torch.cuda.synchronize()
            st.append(e0.elapsed_time(e1))
        N = B * sum(f.H * f.W for f in plan.features)
        print(f"{exp} {B}x{H}x{W}: {N} targets, {int(plan.det_count.cpu())} positives, {sum(len(x) for x in gt)} GT | forward alone "
              f"{t_fwd:.3f} ms | compute_losses {t_loss:.3f} ms (x{t_loss / t_fwd:.2f}) | loss stages alone (assign + terms + finalize, "
              f"device events) {statistics.median(st):.3f} ms | median of {iters}")
        print("  losses:", {k: round(float(v), 5) for k, v in losses.items()})
        del model, plan
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
