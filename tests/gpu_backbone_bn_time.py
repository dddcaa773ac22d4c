"""Dev tool (GPU): what batch-statistics BN in the DLA-34 bottom-up network costs.  The captured stem_grads loss plan of the
FE.BACKBONE.NORM: BN model (graph replay, device events, median of `--iters`, the two plans alternating inside one loop) with and
without backbone_batch_stats -- the plan without the flag is the parent commit's plan, the fused stem included: same ops, same buffers,
same bits -- at three sizes: one KITTI image, four KITTI images (384 x 1280) and the six-camera nuScenes sample (896 x 1600).  Then where
the flagged plan's time goes: its new launches by kind (device events around `--reps` back-to-back calls on the plan's own buffers) with
the bytes the algorithm moves, and the stem and the trees' convolutions in both plans.  Last, torch's own train()-mode step of the
bottom-up network alone (F.conv2d + nn.BatchNorm2d in train(), forward plus backward from random gradients at level3..5, float32; the
package's modules have no forward: tests/backbone_bn_oracle.ModuleWalk writes it out).

    python tests/gpu_backbone_bn_time.py > profiles/backbone_bn_time.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.gpu_tower_bn_time import CASES, HBM_MEASURED, arg, op_ms, replay_ms  # noqa: E402  (builds the library on import)

import dd3d_amd.modeling  # noqa: E402,F401
from dd3d_amd import META_ARCH_REGISTRY, get_cfg, hip  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_gt_instances, make_inputs, make_state_dict  # noqa: E402

BB_BN = {"FE": {"BACKBONE": {"NORM": "BN"}}}
KINDS = ("backbone_bn_batch_stats", "backbone_bn_apply", "backbone_bn_grads", "stem_bn_grads")


def op_bytes(plan, op):
    """Bytes the algorithm moves in one call of a new op: every tensor once per pass that touches it (the per-channel vectors are noise)."""
    kind = op.desc["kind"]
    if kind in KINDS[:2]:
        raw, out = op.desc["raw"], op.desc["out"]
        px = raw.B * raw.H * raw.W
        if kind == KINDS[0]:
            return px * raw.C * 8  # two read passes
        res = 0 if op.desc["res"] is None else (2 * hip.MATH_PLANES[plan.math] if op.desc["res"].np else 4)
        return px * raw.C * (4 + res + (2 * hip.MATH_PLANES[plan.math] if out.np else 0) + (4 if out.has_f32 else 0))
    lay = (plan.stem_layers if kind == KINDS[3] else plan.backbone_layers)[op.desc["layer"]].bn
    h, w = lay.level_hw[0]
    ybytes = 4 if lay.args.y_mode == hip.PG_ACT_F32 else 2 * hip.MATH_PLANES[plan.math]
    return lay.B * h * w * lay.C * ((4 + 4 + ybytes) + (4 + 4 + ybytes + 4))  # reduce: c, g, y | apply: c, g, y read, G_c written


def torch_step_ms(model, inputs, plan, iters):
    """Median device time of torch's train()-mode forward plus backward of the bottom-up network on the plan's normalised canvas."""
    from tests.backbone_bn_oracle import ModuleWalk
    img = plan.normalized_image().float().contiguous()
    walk = ModuleWalk(model.backbone.bottom_up, torch.float32, "cuda")
    gen = torch.Generator(device="cuda").manual_seed(0)
    G, ts = None, []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for it in range(iters + 2):
        walk.relus = []
        e0.record()
        with torch.enable_grad():
            outs = walk(img)
            if G is None:
                G = {k: torch.randn(outs[k].shape, generator=gen, device="cuda") for k in ("level3", "level4", "level5")}
            sum((outs[k] * G[k]).sum() for k in G).backward()
        e1.record()
        torch.cuda.synchronize()
        if it >= 2:
            ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def main():
    iters, reps = arg("--iters", 10), arg("--reps", 5)
    only = arg("--case", -1)
    for ci, (exp, tag, B, H, W, ds) in enumerate(CASES):
        if only >= 0 and ci != only:
            continue
        cfg = get_cfg(exp, BB_BN)
        model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
        model.load_state_dict(make_state_dict(model, calib=load_calib(tag)))
        model = model.to("cuda").eval()
        nusc = hasattr(model, "attr_logits")
        inputs = make_inputs(B, H, W, dataset=ds)
        gt = make_gt_instances(inputs, model.num_classes, cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, n_per_image=48,
                               num_attributes=model.attr_logits.out_channels if nusc else None)
        for x, inst in zip(inputs, gt):
            x["instances"] = inst
        print(f"== {exp} (FE.BACKBONE.NORM: BN) {B} x {H} x {W}")
        with torch.no_grad():
            model.compute_losses(inputs, stem_grads=True)
            model.compute_losses(inputs, stem_grads=True, backbone_batch_stats=True)
        canvas = model.canvas_size(inputs)
        off, on = model.get_loss_plan(*canvas, stem_grads=True), model.get_loss_plan(*canvas, stem_grads=True, backbone_batch_stats=True)
        replay_ms([off, on], 2)
        t_off, t_on = replay_ms([off, on], iters)
        print(f"stem_grads=True: running statistics (the parent's plan, fused stem {bool(off.fused_stem)}) {t_off:.3f} ms | backbone_batch_stats {t_on:.3f} ms "
              f"(+{t_on - t_off:.3f} ms, x{t_on / t_off:.3f}) | {len(off.ops)} -> {len(on.ops)} ops | graph replay, device events, median of {iters}")
        by_kind = {}
        for op in on.ops:
            kind = (getattr(op, "desc", None) or {}).get("kind")
            if kind in KINDS:
                t, nb = op_ms(on, op, 3, reps), op_bytes(on, op)
                rec = by_kind.setdefault(kind, [0, 0.0, 0])
                rec[0], rec[1], rec[2] = rec[0] + 1, rec[1] + t, rec[2] + nb
                if op.name.split(".")[0] in ("base_layer", "stem_bn_grads") or "level5.root" in op.name:
                    print(f"  {op.name}: {t * 1e3:.1f} us, {nb / 1e6:.1f} MB -> {nb / t / 1e9:.2f} TB/s")
        for kind, (n, t, nb) in by_kind.items():
            print(f"  all {n} {kind} calls: {t:.3f} ms back to back, {nb / 1e6:.0f} MB -> {nb / t / 1e9:.2f} TB/s ({100 * nb / t * 1e3 / HBM_MEASURED:.0f} % of the "
                  f"measured {HBM_MEASURED / 1e12:.2f} TB/s float4 copy)")
        fwd = lambda p: sum(op_ms(p, op, 3, reps) for op in p.ops if (op.name == "stem" or op.name.split(".")[0] in ("base_layer", "level0", "level1", "level2",
                            "level3", "level4", "level5")) and (getattr(op, "desc", None) or {}).get("kind") not in KINDS)
        back = lambda p: sum(op_ms(p, op, 3, reps) for op in p.ops if op.name.startswith(("backbone_grads.", "stem_grads.")))
        print(f"  bottom-up forward without the norm launches: {fwd(off):.3f} ms (parent: fused stem, fused epilogues) -> {fwd(on):.3f} ms (launch-by-launch stem, raw "
              f"f32 outputs) | its convolutions' and pools' backward {back(off):.3f} ms (parent) -> {back(on):.3f} ms on g := G_c")
        t_torch = torch_step_ms(model, inputs, on, max(3, iters // 2))
        print(f"  torch, bottom-up network alone, train()-mode forward + backward, float32: {t_torch:.3f} ms")
        del model, off, on
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
