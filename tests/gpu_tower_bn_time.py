"""Dev tool (GPU): what batch-statistics BN in the head towers costs.  The captured loss plan (graph replay, device events, median of
`--iters`, the two plans alternating inside one loop) with and without batch_stats -- the plan without the flag is the parent commit's
plan: same ops, same buffers, same bits -- for plain losses and for tower_grads=True, at three sizes: one KITTI image, four KITTI images
(384 x 1280) and the six-camera nuScenes sample (896 x 1600).  Then the new launches of the batch-statistics plan one by one (device
events around `--reps` back-to-back calls on the plan's own buffers) with the bytes each moves and the bandwidth that gives, against the
MI355X's measured float4-copy bandwidth (6.29 TB/s; 8.0 TB/s spec).

    python tests/gpu_tower_bn_time.py > profiles/tower_bn_time.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

g.build()
import dd3d_amd.modeling  # noqa: E402,F401
from dd3d_amd import META_ARCH_REGISTRY, get_cfg, hip  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_gt_instances, make_inputs, make_state_dict  # noqa: E402

CASES = [("dd3d_kitti_dla34", "dla34_kitti", 1, 384, 1280, "kitti"), ("dd3d_kitti_dla34", "dla34_kitti", 4, 384, 1280, "kitti"),
         ("dd3d_nusc_dla34", "dla34_nusc", 6, 896, 1600, "nusc")]
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def replay_ms(plans, iters):
    """Median device time of one graph replay of each plan, the plans alternating."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in plans]
    ts = [[] for _ in plans]
    for _ in range(iters):
        for i, p in enumerate(plans):
            ev[i][0].record()
            p.graph.replay()
            ev[i][1].record()
        torch.cuda.synchronize()
        for i in range(len(plans)):
            ts[i].append(ev[i][0].elapsed_time(ev[i][1]))
    return [statistics.median(t) for t in ts]


def op_ms(plan, op, iters, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st, ts = hip.current_stream(), []
    op(plan.lib, st)
    for _ in range(iters):
        e0.record()
        for _ in range(reps):
            op(plan.lib, st)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / reps)
    return statistics.median(ts)


def op_bytes(plan, op):
    """Bytes the algorithm moves in one call of a new op (every tensor once per pass that touches it; the per-channel vectors are noise)."""
    kind = op.desc["kind"]
    npl = hip.MATH_PLANES[plan.math] if plan.use_planes else 0
    if kind in ("bn_batch_stats", "bn_apply_relu_split"):
        px = sum(s["raw"].B * s["raw"].H * s["raw"].W for s in op.desc["segs"])
        Cn = op.desc["segs"][0]["raw"].C
        return px * Cn * (8 if kind == "bn_batch_stats" else 4 + (2 * npl if npl else 4))  # two read passes | one read, one plane / f32 write
    lay = plan.tower_layers[(op.desc["tower"], op.desc["layer"])].bn
    px = sum(lay.B * h * w for h, w in lay.level_hw)
    ybytes = 2 * npl if npl else 4
    return px * lay.C * ((4 + 4 + ybytes) + (4 + 4 + ybytes + 4))  # reduce: c, g, y | apply: c, g, y read, G_c written


def main():
    iters, reps = arg("--iters", 30), arg("--reps", 10)
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
        print(f"== {exp} {B} x {H} x {W}")
        for flags in ({}, {"tower_grads": True}):
            with torch.no_grad():
                model.compute_losses(inputs, **flags)
                model.compute_losses(inputs, batch_stats=True, **flags)
            canvas = model.canvas_size(inputs)
            off, on = model.get_loss_plan(*canvas, **flags), model.get_loss_plan(*canvas, batch_stats=True, **flags)
            replay_ms([off, on], 3)
            t_off, t_on = replay_ms([off, on], iters)
            what = "tower_grads=True" if flags else "plain losses"
            print(f"{what}: running statistics (the parent's plan) {t_off:.3f} ms | batch_stats {t_on:.3f} ms (+{t_on - t_off:.3f} ms, x{t_on / t_off:.3f}) | "
                  f"{len(off.ops)} -> {len(on.ops)} ops | graph replay, device events, median of {iters}")
            if not flags:
                continue
            rows = {}
            for op in on.ops:
                if getattr(op, "desc", None) and op.desc.get("kind") in ("bn_batch_stats", "bn_apply_relu_split", "tower_bn_grads"):
                    t, nb = op_ms(on, op, max(5, iters // 3), reps), op_bytes(on, op)
                    key = op.desc["kind"]
                    r = rows.setdefault(key, [0, 0.0, 0])
                    r[0], r[1], r[2] = r[0] + 1, r[1] + t, r[2] + nb
                    if op.name.endswith((".0.bn_stats", ".0.bn_apply")) or op.name == "tower_bn_grads.cls.0":
                        print(f"  {op.name}: {t * 1e3:.1f} us, {nb / 1e6:.1f} MB -> {nb / t / 1e9:.2f} TB/s ({100 * nb / t * 1e3 / HBM_MEASURED:.0f} % of the measured "
                              f"{HBM_MEASURED / 1e12:.2f} TB/s, {100 * nb / t * 1e3 / HBM_SPEC:.0f} % of spec)")
            for key, (n, t, nb) in rows.items():
                print(f"  all {n} {key} calls: {t:.3f} ms, {nb / 1e6:.1f} MB -> {nb / t / 1e9:.2f} TB/s ({100 * nb / t * 1e3 / HBM_MEASURED:.0f} % of measured HBM copy bandwidth)")
            raw = [op for op in on.ops if op.name.endswith(".raw")]
            fused_off = [op for op in off.ops if op.name in ("towers.0", "towers.1", "towers.2", "towers.3")]
            fused_on = [op for op in on.ops if op.name in ("towers.0", "towers.1", "towers.2", "towers.3")]
            t_raw, t_fon = sum(op_ms(on, op, 5, reps) for op in raw), sum(op_ms(on, op, 5, reps) for op in fused_on)
            t_foff = sum(op_ms(off, op, 5, reps) for op in fused_off)
            print(f"  tower convolutions: one fused launch per depth {t_foff:.3f} ms (parent) | split into running-statistics segments {t_fon:.3f} ms + "
                  f"raw segments {t_raw:.3f} ms")
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
