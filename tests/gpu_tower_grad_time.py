"""Dev tool (GPU): what the towers' backward adds to the captured loss plan, beside two baselines on the same tensors, on DD3D-DLA34 at
384 x 1280 (B = 1 and 4, KITTI) and one 6-camera 896 x 1600 nuScenes sample, 48 synthetic GT per image:

  (a) the captured plan of compute_losses(predictor_grads=True) (the parent commit's largest plan) and of compute_losses(tower_grads=True),
      replayed on staged inputs; device events around `--iters` replays, `--rounds` rounds, the two plans taken in turn within a round;
      reported: the median over the rounds and their range, and the difference = the added cost
  (b) every (tower, layer)'s weight-gradient call (three launches) and input-gradient call (one launch) alone, on the plan's own
      buffers, with each GEMM's fraction of the 155 TF f32-matrix peak (2 * pixels * Cout * 9 * Cin flop per GEMM)
  (c) baseline 1 on the layers of BASELINE_LAYERS: the predictor layer's own dd3d_predictor_wgrad / dd3d_predictor_dgrad called with
      n = 256 (lo = 0, map = the decoded stored output as f32 NHWC, made outside the timed region) on the same input, gradient and filter
  (d) baseline 2 on the same layers: torch autograd over relu(F.conv2d(x_l, W) * s_l + t_l) on decoded f32 NCHW inputs, all levels;
      forward + backward, and an estimate of the backward alone (the difference to a forward-only pass)

    python tests/gpu_tower_grad_time.py > profiles/tower_grads_time.txt
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
from dd3d_amd.engine.losses import PredGroupGrads  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_gt_instances, make_inputs, make_state_dict  # noqa: E402

CASES = [("dd3d_kitti_dla34", "dla34_kitti", 1, 384, 1280, "kitti"), ("dd3d_kitti_dla34", "dla34_kitti", 4, 384, 1280, "kitti"),
         ("dd3d_nusc_dla34", "dla34_nusc", 6, 896, 1600, "nusc")]
BASELINE_LAYERS = [("cls", 3), ("box3d", 1)]
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


def predictor_baseline(plan, key):
    """The layer `key` as a predictor group of n = Cout channels: every channel clamped at 0, the stored output decoded to f32 NHWC."""
    lay, info = plan.tower_layers[key], plan.tower_info[key]
    gr, w, scale, _, _ = lay.keep
    dev = plan.device
    maps = [v.nchw().float().permute(0, 2, 3, 1).contiguous() for v in info["y"]]
    xb = [(lay.args.x_mode, lay.args.x[l], lay.args.x_pitch, lay.args.x_plane_scale) for l in range(lay.L)]
    zeros = torch.zeros(lay.Cout, dtype=torch.float32, device=dev)
    return PredGroupGrads(dev, lay.B, lay.level_hw, lay.Cin, lay.Cout, lay.args.g_pitch, [b[1] for b in xb], xb[0][0], xb[0][2], xb[0][3], gr, maps,
                          [w] * lay.L, [zeros] * lay.L, scale, lo=zeros.clone())


def torch_layer(plan, key):
    lay, info = plan.tower_layers[key], plan.tower_info[key]
    gr, w, scale, _, _ = lay.keep
    xs = [v.nchw().float().contiguous().requires_grad_(True) for v in info["x"]]
    gm = [gr[l][..., :lay.Cout].permute(0, 3, 1, 2).contiguous() for l in range(lay.L)]
    W = w.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    S = [s.clone().requires_grad_(True) for s in scale]
    T = [torch.zeros_like(s).requires_grad_(True) for s in scale]

    def forward():
        total = 0
        for l in range(lay.L):
            total = total + (F.relu(F.conv2d(xs[l], W, padding=1) * S[l][None, :, None, None] + T[l][None, :, None, None]) * gm[l]).sum()
        return total

    def both():
        W.grad = None
        for t in xs + S + T:
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
            model.compute_losses(inputs, predictor_grads=True)
            model.compute_losses(inputs, tower_grads=True)
        size = model.canvas_size(inputs)
        plan_p, plan_t = model.get_loss_plan(*size, pred_grads=True), model.get_loss_plan(*size, tower_grads=True)
        pixels = B * sum(f.H * f.W for f in plan_t.features)
        first = plan_t.tower_layers[("cls", 3)]
        print(f"{exp} {B}x{H}x{W}: {pixels} pixels over {len(plan_t.features)} levels, {int(plan_t.det_count.cpu())} positives, "
              f"activations: {('f32', 'f16x2', 'bf16x3')[first.args.y_mode]}, {first.n_slices} slices of the partial slab "
              f"({first.n_slices * first.Cout * 9 * first.Cin * 4 / 2**20:.0f} MiB)")
        tp, tt = [], []
        for _ in range(rounds):
            tp.append(events(plan_p.run, iters))
            tt.append(events(plan_t.run, iters))
        a = report("(a) captured plan, predictor_grads (parent)", tp)[0]
        b = report("(a) captured plan, tower_grads", tt)[0]
        print(f"      added by the towers' backward: {b - a:.1f} us ({(b - a) / a * 100:.1f} % of the parent's plan)")
        L_, total, alone = hip.lib(), 0.0, {}
        for key, lay in plan_t.tower_layers.items():
            flop = 2.0 * pixels * lay.Cout * 9 * lay.Cin
            wg = lambda lay=lay: hip.check(L_.dd3d_tower_wgrad(C.byref(lay.args), hip.current_stream()), "wgrad")
            dg = lambda lay=lay: hip.check(L_.dd3d_tower_dgrad(C.byref(lay.args), hip.current_stream()), "dgrad")
            alone[key] = (report(f"(b) {key[0]}.{key[1]} weight gradient, 3 launches", [events(wg, iters) for _ in range(rounds)], flop),
                          report(f"(b) {key[0]}.{key[1]} input gradient, 1 launch", [events(dg, iters) for _ in range(rounds)], flop))
            total += alone[key][0][0] + alone[key][1][0]
        print(f"      sum of the calls alone: {total:.1f} us")
        for key in BASELINE_LAYERS:
            grp = predictor_baseline(plan_t, key)
            wg = lambda: hip.check(L_.dd3d_predictor_wgrad(C.byref(grp.args), hip.current_stream()), "wgrad")
            dg = lambda: hip.check(L_.dd3d_predictor_dgrad(C.byref(grp.args), hip.current_stream()), "dgrad")
            for _ in range(2):
                wg(), dg()
            torch.cuda.synchronize()
            bw = report(f"(c) {key[0]}.{key[1]} dd3d_predictor_wgrad at n = 256 ({grp.n_slices} slices)", [events(wg, iters) for _ in range(rounds)])
            bd = report(f"(c) {key[0]}.{key[1]} dd3d_predictor_dgrad at n = 256", [events(dg, iters) for _ in range(rounds)])
            for what, base, new in (("weight", bw, alone[key][0]), ("input", bd, alone[key][1])):
                # (median, fastest, slowest round) of each: the ranges are disjoint when one side's fastest round is slower than the other's slowest
                verdict = "the new kernels win beyond both ranges" if base[1] > new[2] else \
                    "the new kernels LOSE beyond both ranges" if new[1] > base[2] else "the ranges overlap"
                print(f"      {what} gradient: baseline / new = {base[0] / new[0]:.2f} (medians); {verdict}")
            del grp
            both, fwd_only = torch_layer(plan_t, key)
            for _ in range(3):
                both()
                fwd_only()
            torch.cuda.synchronize()
            tb = report(f"(d) {key[0]}.{key[1]} torch autograd, forward + backward", [events(both, iters) for _ in range(rounds)])[0]
            tf = report(f"(d) {key[0]}.{key[1]} torch autograd, forward only", [events(fwd_only, iters) for _ in range(rounds)])[0]
            new = alone[key][0][0] + alone[key][1][0]
            print(f"      torch backward alone (difference): {tb - tf:.1f} us; new kernels / torch backward = {new / max(tb - tf, 1e-9):.2f}")
            del both, fwd_only
            torch.cuda.empty_cache()
        del model, plan_p, plan_t
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
