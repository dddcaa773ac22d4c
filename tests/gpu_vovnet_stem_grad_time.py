"""Dev tool (GPU): what stem_1's weight gradient adds to the captured loss plan of DD3D-V2-99 at 384 x 1280 (B = 1 and 4, KITTI) and one
6-camera 896 x 1600 nuScenes sample, 48 synthetic GT per image:

  (a) the captured plan of compute_losses(vovnet_grads=True) (the parent commit's largest V2-99 plan) and of
      compute_losses(vovnet_stem_grads=True), replayed on staged inputs; device events around `--iters` replays, `--rounds` rounds, the two
      plans taken in turn within a round; reported: the median over the rounds and their range, and the difference = the added cost
  (b) the call alone on the plan's own buffers (three launches: the slices, the reduce, the per-channel sums) with its fraction of the
      155 TF f32-matrix peak (2 * output pixels * 64 * 36 flop) and the bytes it has to read at least (the image, the gradient, the mask)
  (c) the memory the call adds

    python tests/gpu_vovnet_stem_grad_time.py > profiles/vovnet_stem_grads_time.txt

`--errors` instead runs tests/test_vovnet_stem_whole_model_gpu.py and tests/test_vovnet_stem_grads_gpu.py with their printed ratios and
writes them to profiles/vovnet_stem_grads_errors.txt.  No time bar is set: the numbers are a record beside the parent's plan."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.gpu_fpn_grad_time import arg, events, report  # noqa: E402  (builds the library on import)
import dd3d_amd.modeling  # noqa: E402,F401
from dd3d_amd import META_ARCH_REGISTRY, get_cfg, hip  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_gt_instances, make_inputs, make_state_dict  # noqa: E402
from tests.gpu_vovnet_grad_time import CASES  # noqa: E402


def main():
    iters, rounds = arg("--iters", 5), arg("--rounds", 3)
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
            model.compute_losses(inputs, vovnet_grads=True)
            model.compute_losses(inputs, vovnet_stem_grads=True)
        size = model.canvas_size(inputs)
        plan_v, plan_s = model.get_loss_plan(*size, vovnet_grads=True), model.get_loss_plan(*size, vovnet_stem_grads=True)
        lay = plan_s.vovnet_stem_layers["stem_1"]
        added = sum(t.numel() for t, _ in lay._raw) * 4 + lay.keep[2].numel() * 4
        print(f"{exp} {B}x{size[1]}x{size[2]}: stem_1 output {lay.Ho}x{lay.Wo}, {int(plan_s.det_count.cpu())} positives, mask storage: "
              f"{('f32', 'f16x2', 'bf16x3')[lay.args.y_mode]}, {lay.n_slices} slices, slab {plan_s.tower_slab[0].numel() * 4 / 2**20:.0f} MiB (vovnet_grads plan: "
              f"{plan_v.tower_slab[0].numel() * 4 / 2**20:.0f} MiB)")
        print(f"  (c) added memory: dw_level, dw, q, r and the f32 filter copy {added / 2**10:.1f} KiB; no new activation buffer")
        tv, ts = [], []
        for _ in range(rounds):
            tv.append(events(plan_v.run, iters))
            ts.append(events(plan_s.run, iters))
        a = report("(a) captured plan, vovnet_grads (parent)", tv)[0]
        b = report("(a) captured plan, vovnet_stem_grads", ts)[0]
        print(f"      added by stem_1's weight gradient: {b - a:.1f} us ({(b - a) / a * 100:.2f} % of the parent's plan)")
        L_ = hip.lib()
        flop = 2.0 * B * lay.Ho * lay.Wo * 64 * 36
        t = report("(b) the call alone (three launches)", [events(lambda: lay.launch(L_, hip.current_stream()), iters) for _ in range(rounds)], flop)[0]
        mask_bytes = {hip.PG_ACT_F32: 4, hip.PG_ACT_F16X2: 4, hip.PG_ACT_BF16X3: 6}[lay.args.y_mode]
        least = B * lay.H * lay.W * 16 + B * lay.Ho * lay.Wo * 64 * (4 + mask_bytes)
        print(f"      at least {least / 2**20:.1f} MiB to read: {least / t * 1e-6:.2f} TB/s", flush=True)
        del model, plan_v, plan_s, lay
        torch.cuda.empty_cache()


def errors():
    import subprocess
    out = os.path.join(ROOT, "profiles", "vovnet_stem_grads_errors.txt")
    tmp = out + ".rows"
    if os.path.exists(tmp):
        os.remove(tmp)
    env = dict(os.environ, DD3D_VOVNET_STEM_ERRORS_FILE=tmp)
    files = [os.path.join(ROOT, "tests", n) for n in ("test_vovnet_stem_whole_model_gpu.py", "test_vovnet_stem_grads_gpu.py")]
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider"] + files, env=env, capture_output=True, text=True, cwd=ROOT)
    rows = open(tmp).read().splitlines() if os.path.exists(tmp) else []
    whole = [l for l in rows if l.startswith("kitti_v99")]
    seam = [l for l in rows if not l.startswith("kitti_v99")]
    signs = [l[l.index("[vovnet_stem_whole_model] signs"):] for l in r.stdout.splitlines() if "[vovnet_stem_whole_model] signs" in l]
    with open(out, "w") as f:
        f.write("Measured deviation from float64 autograd over the bar 8 * max(d32, 2^-23 * max|g64|), per family (MI355X).\n\n")
        f.write("DD3D.compute_losses(vovnet_stem_grads=True), V2-99, 1 x 128 x 256 (tests/test_vovnet_stem_whole_model_gpu.py):\n")
        f.write("\n".join(whole + signs) + "\n")
        f.write("\nThe seam, dd3d_vovnet_stem_wgrad (tests/test_vovnet_stem_grads_gpu.py):\n" + "\n".join(seam) + "\n")
    if os.path.exists(tmp):
        os.remove(tmp)
    print(r.stdout[-3000:])
    sys.exit(r.returncode)


if __name__ == "__main__":
    errors() if "--errors" in sys.argv else main()
