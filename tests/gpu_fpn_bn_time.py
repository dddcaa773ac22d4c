"""Dev tool (GPU): what batch-statistics BN in the FPN costs.  The captured loss plan of the FE.FPN.NORM: BN model (graph replay, device
events, median of `--iters`, the two plans alternating inside one loop) with and without fpn_batch_stats -- the plan without the flag is
the parent commit's plan: same ops, same buffers, same bits -- for plain losses and for fpn_grads=True, at three sizes: one KITTI image,
four KITTI images (384 x 1280) and the six-camera nuScenes sample (896 x 1600).  Then the new launches of the flagged plan one by one
(device events around `--reps` back-to-back calls on the plan's own buffers) with the bytes the algorithm moves and the bandwidth that
gives, against the MI355X's measured float4-copy bandwidth (6.29 TB/s; 8.0 TB/s spec), and the FPN's convolutions in both plans.

    python tests/gpu_fpn_bn_time.py > profiles/fpn_bn_time.txt
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.gpu_tower_bn_time import CASES, HBM_MEASURED, HBM_SPEC, arg, op_ms, replay_ms  # noqa: E402  (builds the library on import)

import dd3d_amd.modeling  # noqa: E402,F401
from dd3d_amd import META_ARCH_REGISTRY, get_cfg, hip  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_gt_instances, make_inputs, make_state_dict  # noqa: E402

FPN_BN = {"FE": {"FPN": {"NORM": "BN"}}}
NEW_KINDS = ("bn_batch_stats", "bn_apply_topdown_split", "fpn_bn_grads")


def op_bytes(plan, op):
    """Bytes the algorithm moves in one call of a new op: every tensor once per pass that touches it (a coarser stage's raw tensor that
    the top-down sum re-reads for its finer stages is counted once, in its own segment; the per-channel vectors are noise)."""
    kind = op.desc["kind"]
    npl = hip.MATH_PLANES[plan.math]
    if kind in ("bn_batch_stats", "bn_apply_topdown_split"):
        px = sum(s["raw"].B * s["raw"].H * s["raw"].W for s in op.desc["segs"])
        Cn = op.desc["segs"][0]["raw"].C
        copy = 4 if (kind != "bn_batch_stats" and op.desc["segs"][0]["out"].has_f32) else 0
        return px * Cn * (8 if kind == "bn_batch_stats" else 4 + 2 * npl + copy)  # two read passes | one read, one plane write
    lay = plan.fpn_bn_layers[op.desc["layer"]]
    px = sum(lay.B * h * w for h, w in lay.level_hw)
    return px * lay.C * ((4 + 4) + (4 + 4 + 4))  # reduce: c, g | apply: c, g read, G_c written


def main():
    iters, reps = arg("--iters", 20), arg("--reps", 10)
    only = arg("--case", -1)
    for ci, (exp, tag, B, H, W, ds) in enumerate(CASES):
        if only >= 0 and ci != only:
            continue
        cfg = get_cfg(exp, FPN_BN)
        model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
        model.load_state_dict(make_state_dict(model, calib=load_calib(tag)))
        model = model.to("cuda").eval()
        nusc = hasattr(model, "attr_logits")
        inputs = make_inputs(B, H, W, dataset=ds)
        gt = make_gt_instances(inputs, model.num_classes, cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, n_per_image=48,
                               num_attributes=model.attr_logits.out_channels if nusc else None)
        for x, inst in zip(inputs, gt):
            x["instances"] = inst
        print(f"== {exp} (FE.FPN.NORM: BN) {B} x {H} x {W}")
        for flags in ({}, {"fpn_grads": True}):
            with torch.no_grad():
                model.compute_losses(inputs, **flags)
                model.compute_losses(inputs, fpn_batch_stats=True, **flags)
            canvas = model.canvas_size(inputs)
            off, on = model.get_loss_plan(*canvas, **flags), model.get_loss_plan(*canvas, fpn_batch_stats=True, **flags)
            replay_ms([off, on], 3)
            t_off, t_on = replay_ms([off, on], iters)
            what = "fpn_grads=True" if flags else "plain losses"
            print(f"{what}: running statistics (the parent's plan) {t_off:.3f} ms | fpn_batch_stats {t_on:.3f} ms (+{t_on - t_off:.3f} ms, x{t_on / t_off:.3f}) | "
                  f"{len(off.ops)} -> {len(on.ops)} ops | graph replay, device events, median of {iters}")
            if not flags:
                continue
            total = 0.0
            for op in on.ops:
                if getattr(op, "desc", None) and op.desc.get("kind") in NEW_KINDS and op.name.startswith("fpn_"):
                    t, nb = op_ms(on, op, max(5, iters // 3), reps), op_bytes(on, op)
                    total += t
                    print(f"  {op.name}: {t * 1e3:.1f} us, {nb / 1e6:.1f} MB -> {nb / t / 1e9:.2f} TB/s ({100 * nb / t * 1e3 / HBM_MEASURED:.0f} % of the measured "
                          f"{HBM_MEASURED / 1e12:.2f} TB/s float4 copy, {100 * nb / t * 1e3 / HBM_SPEC:.0f} % of spec)")
            is_conv = lambda op: op.name.startswith(("fpn_lateral", "fpn_outputs")) and (getattr(op, "desc", None) or {}).get("kind") == "conv"
            t_conv_off = sum(op_ms(off, op, 5, reps) for op in off.ops if is_conv(op))
            t_conv_on = sum(op_ms(on, op, 5, reps) for op in on.ops if is_conv(op))
            back = lambda p: sum(op_ms(p, op, 5, reps) for op in p.ops if op.name.startswith("fpn_grads.") and not op.name.startswith("fpn_grads.top_block"))
            print(f"  the six norm launches' calls: {total:.3f} ms back to back | FPN convolutions: fused epilogues {t_conv_off:.3f} ms (parent) -> raw f32 outputs "
                  f"{t_conv_on:.3f} ms | the lateral / output convolutions' backward {back(off):.3f} ms (parent) -> {back(on):.3f} ms on g := G_c")
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
