"""Dev tool (GPU): the dense-depth loss with its gradient next to the alternatives, in one process and alternating, on 2 x 384 x 1280 and
4 x 384 x 1280 KITTI batches (DLA-34) with the sparse ground truth of dd3d_amd.synthetic.make_depth_maps.  At the seam -- from the
head's raw per-level maps to the loss values and the gradient at those maps -- on the plan's own buffers:

  (a) dd3d_dense_depth_loss alone                                   the fused forward: what the library had before the gradient
  (b) dd3d_dense_depth_loss + dd3d_dense_depth_loss_backward         forward and the new backward (two launches each)
  (c) the unfused composition in torch on the device, autograd on:  aligned_bilinear of every level (replicate-pad, bilinear resize,
      crop), the focal-length division, the masked smooth-L1 mean per level, then .backward() to the raw maps; its backward also alone

(a) and (b) by device events over `reps` back-to-back launches, (c) by device events around single calls (it launches dozens of
kernels; the host enqueue is part of what a user of it pays), `--rounds` rounds, the three taken in turn within a round; reported: the
median over the rounds and their range.  Then, end to end from the host call to a device synchronise, DD3DDenseDepth.compute_losses
with and without head_grads.

    python tests/gpu_dense_depth_loss_grad_time.py > profiles/dense_depth_loss_grad_time.txt
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
import dd3d_amd.modeling  # noqa: E402,F401  (registers the meta-architectures)
from dd3d_amd import META_ARCH_REGISTRY, get_cfg, hip  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_depth_maps, make_inputs, make_state_dict  # noqa: E402
from oracle.dense_depth_oracle import aligned_bilinear  # noqa: E402

OVER = {"MODEL": {"META_ARCHITECTURE": "DD3DDenseDepth"},
        "DD3D": {"IN_FEATURES": ["p3", "p4", "p5", "p6", "p7"], "FCOS3D": {"DEPTH_HEAD": {"LOSS_TYPE": "L1", "LOSS_WEIGHT": 1.0}}}}


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def torch_losses(raw, gt, strides, offset, pixel_size, min_depth, max_depth, beta, weight):
    """The unfused composition: per-level values as a differentiable function of the raw maps, on the device."""
    M = ((gt < min_depth).to(torch.float32) + (gt > max_depth).to(torch.float32)) == 0.
    tgt = gt[M]
    out = []
    for l, (r, s) in enumerate(zip(raw, strides)):
        m = aligned_bilinear(r, s, offset).squeeze(1)
        if pixel_size is not None:
            m = m / pixel_size
        n = torch.abs(m[M] - tgt)
        t = n if beta < 1e-5 else torch.where(n < beta, 0.5 * n**2, n - 0.5 * beta)
        out.append((weight * t.mean()) / (np.sqrt(2)**l))
    return out


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps  # us


def line(name, xs, unit="us"):
    d = 3 if unit == "ms" else 1
    print(f"{name}: median {statistics.median(xs):.{d}f} {unit}, range {min(xs):.{d}f} .. {max(xs):.{d}f} {unit} over {len(xs)} rounds")
    return statistics.median(xs)


def measure(model, cfg, B, H, W, rounds, reps, iters):
    c3 = cfg.DD3D.FCOS3D
    mn, mx, beta, weight = float(c3.MIN_DEPTH), float(c3.MAX_DEPTH), float(c3.LOSS.SMOOTH_L1_BETA), float(c3.DEPTH_HEAD.LOSS_WEIGHT)
    inputs = make_inputs(B, H, W)
    base = model.predict_dense_depth(inputs)[2].cpu()  # level 2 lies inside the depth range almost everywhere
    for x, d in zip(inputs, make_depth_maps(inputs, base=[base[i] for i in range(B)], min_depth=mn, max_depth=mx, beta=beta)):
        x["depth"] = d.cuda()
    losses, grads = model.compute_losses(inputs, head_grads=True)
    plan = model.get_loss_plan(B, H, W, head_grads=True)
    a, ga, L_ = plan.loss_args, plan.grad_args, hip.lib()
    print(f"DD3DDenseDepth DLA-34 {B}x{H}x{W}, valid pixels {int(plan.valid_count.cpu())} of {B * H * W}, slab {plan.grad_slab.shape[0]} rows "
          f"({plan.grad_slab.numel() * 4 / 1e6:.2f} MB)")

    # the unfused composition on the plan's own raw maps
    strides = [int(s.stride) for s in model.backbone_output_shape]
    raw = [m.t[..., 0].unsqueeze(1).clone().requires_grad_(True) for m in plan.dd_raw]
    gt = plan.gt_canvas
    pixel = None
    if model.scale_depth_by_focal_lengths:
        iK = plan.inv_K.reshape(B, 3, 3)
        pixel = (torch.sqrt(iK[:, 0, 0]**2 + iK[:, 1, 1]**2) * float(model.scale_depth_by_focal_lengths_factor)).reshape(-1, 1, 1)
    ref = torch_losses(raw, gt, strides, model.feature_locations_offset, pixel, mn, mx, beta, weight)
    sum(ref).backward()
    for l in range(len(raw)):
        gk, gr = grads[f"dense_depth{l}"], raw[l].grad
        print(f"  level {l}: loss fused {float(losses[f'loss_dense_depth_lvl_{l}']):.6f} torch {float(ref[l].detach()):.6f}; "
              f"max|grad fused - torch| {float((gk - gr).abs().max()):.3e} of max|grad| {float(gr.abs().max()):.3e}")

    fwd = lambda: hip.check(L_.dd3d_dense_depth_loss(C.byref(a), hip.current_stream()), "dense_depth_loss")

    def fwd_bwd():
        fwd()
        hip.check(L_.dd3d_dense_depth_loss_backward(C.byref(a), C.byref(ga), hip.current_stream()), "dense_depth_loss_backward")

    def unfused(parts):
        for r in raw:
            r.grad = None
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        total = sum(torch_losses(raw, gt, strides, model.feature_locations_offset, pixel, mn, mx, beta, weight))
        e[1].record()
        total.backward()
        e[2].record()
        torch.cuda.synchronize()
        parts.append((e[0].elapsed_time(e[2]) * 1e3, e[1].elapsed_time(e[2]) * 1e3))

    for _ in range(3):  # warm-up
        fwd(), fwd_bwd(), unfused([])
    ta, tb, tc, tcb = [], [], [], []
    for _ in range(rounds):
        ta.append(events(fwd, reps))
        tb.append(events(fwd_bwd, reps))
        parts = []
        for _ in range(iters):
            unfused(parts)
        tc.append(statistics.median(p[0] for p in parts))
        tcb.append(statistics.median(p[1] for p in parts))
    ma = line(f"(a) fused forward alone ({reps} back-to-back launches per round)", ta)
    mb = line(f"(b) fused forward + backward ({reps} back-to-back per round)", tb)
    mc = line(f"(c) unfused torch forward + backward ({iters} calls per round, median)", tc)
    mcb = line("    of which its backward", tcb)
    print(f"    (b) - (a) = {mb - ma:.1f} us = {(mb - ma) / ma:.2f} x (a);  (b) / (c) = {mb / mc:.3f};  fused backward / torch backward = {(mb - ma) / mcb:.3f}")

    # end to end
    paths = [("compute_losses", lambda: model.compute_losses(inputs)), ("compute_losses(head_grads=True)", lambda: model.compute_losses(inputs, head_grads=True))]
    for _, fn in paths:
        for _ in range(3):
            fn()
    times = {n: [] for n, _ in paths}
    for _ in range(rounds):
        for n, fn in paths:
            ts = []
            for _ in range(iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            times[n].append(statistics.median(ts))
    for n, _ in paths:
        line(f"end to end {n} ({iters} calls per round, median)", times[n], unit="ms")
    print()


def main():
    rounds, reps, iters = arg("--rounds", 5), arg("--reps", 50), arg("--iters", 20)
    H, W = arg("--height", 384), arg("--width", 1280)
    cfg = get_cfg("dd3d_kitti_dla34", OVER)
    model = META_ARCH_REGISTRY.get("DD3DDenseDepth")(cfg)
    model.load_state_dict(make_state_dict(model, calib=load_calib("dla34_kitti")))
    model = model.to("cuda").eval()
    for B in (2, 4):
        measure(model, cfg, B, H, W, rounds, reps, iters)


if __name__ == "__main__":
    main()
