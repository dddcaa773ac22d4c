"""Dev tool (GPU): DD3DDenseDepth.compute_losses next to the alternatives, in one process and alternating, on a 4 x 384 x 1280 KITTI batch
(DLA-34) with the sparse ground truth of dd3d_amd.synthetic.make_depth_maps:

  (a) compute_losses                       the fused plan: trunk, head, ONE loss call; no full-resolution map is stored
  (b) predict_dense_depth                  trunk, head, five up-sampling launches (five B x Hp x Wp f32 maps written)
  (c) predict_dense_depth + masked loss in torch on the device: the unfused composition
  (d) the loss launch alone (dd3d_dense_depth_loss on the plan's own buffers), device events

(a) - (c) are timed from the host call to a device synchronise, `--rounds` rounds of `--iters` calls each, the three taken in turn within a
round; reported: the median over all calls and the spread of the per-round medians.  From (d): achieved bytes/s against the algorithmic
bytes (the ground truth read once + the raw maps read once) and the bound that applies.

    python tests/gpu_dense_depth_loss_time.py > profiles/dense_depth_loss_time.txt
"""
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

g.build()
import dd3d_amd.modeling  # noqa: E402,F401
from dd3d_amd import META_ARCH_REGISTRY, get_cfg, hip  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_depth_maps, make_inputs, make_state_dict  # noqa: E402

OVER = {"MODEL": {"META_ARCHITECTURE": "DD3DDenseDepth"},
        "DD3D": {"IN_FEATURES": ["p3", "p4", "p5", "p6", "p7"], "FCOS3D": {"DEPTH_HEAD": {"LOSS_TYPE": "L1", "LOSS_WEIGHT": 1.0}}}}
HBM_PEAK = 8.0e12  # bytes/s, MI355X


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def torch_loss(maps, gt, min_depth, max_depth, beta, weight):
    """The unfused composition's second half: the masked smooth-L1 mean per level, in torch on the device."""
    M = ((gt < min_depth).to(torch.float32) + (gt > max_depth).to(torch.float32)) == 0.
    tgt = gt[M]
    out = {}
    for l, m in enumerate(maps):
        n = torch.abs(m[M] - tgt)
        t = n if beta < 1e-5 else torch.where(n < beta, 0.5 * n**2, n - 0.5 * beta)
        out[f"loss_dense_depth_lvl_{l}"] = (weight * t.mean()) / (np.sqrt(2)**l)
    return out


def main():
    iters, rounds = arg("--iters", 40), arg("--rounds", 5)
    B, H, W = arg("--batch", 4), arg("--height", 384), arg("--width", 1280)
    cfg = get_cfg("dd3d_kitti_dla34", OVER)
    model = META_ARCH_REGISTRY.get("DD3DDenseDepth")(cfg)
    model.load_state_dict(make_state_dict(model, calib=load_calib("dla34_kitti")))
    model = model.to("cuda").eval()
    c3 = cfg.DD3D.FCOS3D
    mn, mx, beta, weight = float(c3.MIN_DEPTH), float(c3.MAX_DEPTH), float(c3.LOSS.SMOOTH_L1_BETA), float(c3.DEPTH_HEAD.LOSS_WEIGHT)
    inputs = make_inputs(B, H, W)
    base = model.predict_dense_depth(inputs)[2].cpu()  # level 2 lies inside the depth range almost everywhere
    for x, d in zip(inputs, make_depth_maps(inputs, base=[base[i] for i in range(B)], min_depth=mn, max_depth=mx, beta=beta)):
        x["depth"] = d.cuda()
    gt = torch.stack([x["depth"] for x in inputs])

    fused = lambda: model.compute_losses(inputs)
    predict = lambda: model.predict_dense_depth(inputs)
    unfused = lambda: torch_loss(model.predict_dense_depth(inputs), gt, mn, mx, beta, weight)
    paths = [("(a) compute_losses", fused), ("(b) predict_dense_depth", predict), ("(c) predict_dense_depth + torch loss", unfused)]
    for _, fn in paths:  # warm-up: plans, graph capture, torch's kernels
        for _ in range(3):
            fn()
    la, lc = fused(), unfused()
    print(f"DD3DDenseDepth DLA-34 {B}x{H}x{W}, valid pixels {int(model.get_loss_plan(B, H, W).valid_count.cpu())} of {B * H * W}")
    print("  fused  :", {k: round(float(v), 6) for k, v in la.items()})
    print("  unfused:", {k: round(float(v), 6) for k, v in lc.items()})
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
    for name, _ in paths:
        allt = [t for r in times[name] for t in r]
        meds = [statistics.median(r) for r in times[name]]
        print(f"{name}: median {statistics.median(allt):.3f} ms over {len(allt)} calls ({sum(allt) / 1e3:.2f} s in all); per-round medians "
              f"{min(meds):.3f} .. {max(meds):.3f} ms")

    plan = model.get_loss_plan(B, H, W)
    a, L_ = plan.loss_args, hip.lib()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, st = 50, []
    for _ in range(max(rounds, 5)):
        e0.record()
        for _ in range(reps):
            hip.check(L_.dd3d_dense_depth_loss(C.byref(a), hip.current_stream()), "dense_depth_loss")
        e1.record()
        torch.cuda.synchronize()
        st.append(e0.elapsed_time(e1) / reps)
    t_d = statistics.median(st)
    raw_bytes = sum(f.B * f.H * f.W * 4 * 4 for f in plan.features)  # NHWC pitch 4: the lines are read whole
    algo = B * H * W * 4 + raw_bytes
    print(f"(d) loss launch alone (main pass + finalize, device events, {reps} back-to-back launches per sample): median {t_d * 1e3:.1f} us, "
          f"range {min(st) * 1e3:.1f} .. {max(st) * 1e3:.1f} us")
    frac = algo / (t_d * 1e-3) / HBM_PEAK
    # per valid pixel and level: ~40 f32 / integer operations and 4 taps; far below the vector rate, so of the two roofline bounds memory is
    # the larger one -- whether the launch is NEAR it is what the achieved fraction says
    t_mem = algo / HBM_PEAK * 1e6
    verdict = ("close to the memory bound" if frac >= 0.5 else
               "the memory bound is the larger of the two roofline bounds, but the launch is far from it: launch overhead of two short kernels "
               "and the latency of the dependent taps dominate, not bandwidth")
    print(f"    algorithmic bytes {algo / 1e6:.2f} MB (ground truth {B * H * W * 4 / 1e6:.2f} MB + raw maps {raw_bytes / 1e6:.2f} MB) -> "
          f"{algo / (t_d * 1e-3) / 1e12:.2f} TB/s achieved, {100 * frac:.0f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak ({t_mem:.1f} us at peak): "
          f"{verdict}.  Back-to-back launches re-read a ground truth that fits the 256 MB Infinity Cache: a cache-warm figure.")

if __name__ == "__main__":
    main()
