"""Dev tool (GPU): what the VoVNet-V2 backbone's backward adds to the captured loss plan, beside one baseline on the same tensors, on
DD3D-V2-99 at 384 x 1280 (B = 1 and 4, KITTI) and one 6-camera 896 x 1600 nuScenes sample, 48 synthetic GT per image:

  (a) the captured plan of compute_losses(fpn_grads=True) (the parent commit's largest V2-99 plan) and of compute_losses(vovnet_grads=True),
      replayed on staged inputs; device events around `--iters` replays, `--rounds` rounds, the two plans taken in turn within a round;
      reported: the median over the rounds and their range, and the difference = the added cost
  (b) every call of the VoVNet backward alone on the plan's own buffers -- eSE (four launches), weight gradient (three), input gradient
      (one), the module-input sum (one), pool backward (one) -- summed per kernel family and per stage, each GEMM family with its
      fraction of the 155 TF f32-matrix peak (2 * output pixels * Cout * k * k * Cin flop per GEMM), and the five slowest calls
  (c) the baseline: torch autograd in float32 over the same composition (stem_2, stem_3, the OSA stages with their folded scales, eSE
      gates, 3x3 ceil-mode pools) on the decoded stem_1 output; forward + backward, and an estimate of the backward alone
  (d) the memory the per-call da, dw_level / dw and eSE buffers take

    python tests/gpu_vovnet_grad_time.py > profiles/vovnet_grads_time.txt

`--errors` instead runs tests/test_vovnet_whole_model_gpu.py and tests/test_vovnet_grads_gpu.py with their printed ratios and writes
the whole-model ratios to profiles/vovnet_grads_errors.txt."""
import ctypes as C
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.gpu_fpn_grad_time import arg, events, report  # noqa: E402  (builds the library on import)
import dd3d_amd.modeling  # noqa: E402,F401
from dd3d_amd import META_ARCH_REGISTRY, get_cfg, hip  # noqa: E402
from dd3d_amd.synthetic import load_calib, make_gt_instances, make_inputs, make_state_dict  # noqa: E402

CASES = [("dd3d_kitti_v99", "v99_kitti", 1, 384, 1280, "kitti"), ("dd3d_kitti_v99", "v99_kitti", 4, 384, 1280, "kitti"),
         ("dd3d_nusc_v99", "v99_nusc", 6, 896, 1600, "nusc")]


def torch_vovnet(model, plan):
    """stem_2 .. stage5 of `model` as plain float32 torch on the plan's decoded stem_1 output, with the gradients the FPN's backward sends."""
    from dd3d_amd.layers import fold_norm
    from dd3d_amd.modeling.vovnet import seq_conv, seq_norm
    vov = model.backbone.bottom_up
    x0 = plan.bufs["stem.0"].nchw().float().contiguous().requires_grad_(True)
    P = {}

    def reg(conv, norm):
        s, t = fold_norm(conv, norm)
        P[id(conv)] = (conv.weight.detach().float().clone().requires_grad_(True), s.to(plan.device).clone().requires_grad_(True),
                       t.to(plan.device).clone().requires_grad_(True), conv.stride)

    for c, n, _ in vov.stem_seqs[1:]:
        reg(getattr(vov.stem, c), getattr(vov.stem, n))
    fcs = {}
    for sname in vov.stage_names:
        for _, m in getattr(vov, sname).named_children():
            for seq in list(m.layers) + [m.concat]:
                reg(seq_conv(seq), seq_norm(seq))
            fcs[id(m)] = (m.ese.fc.weight.detach().float().clone().requires_grad_(True), m.ese.fc.bias.detach().float().clone().requires_grad_(True))
    G = {n: d[..., :c].permute(0, 3, 1, 2).contiguous() for n, (d, c) in plan.backbone_feature_grads.items()}

    def conv(m, x):
        w, s, t, st = P[id(m)]
        return F.relu(F.conv2d(x, w, stride=st, padding=(w.shape[-1] - 1) // 2) * s[None, :, None, None] + t[None, :, None, None])

    def forward():
        x = x0
        for c, _, _ in vov.stem_seqs[1:]:
            x = conv(getattr(vov.stem, c), x)
        total = 0.0
        for sname in vov.stage_names:
            stage = getattr(vov, sname)
            if stage.has_pool:
                x = F.max_pool2d(x, 3, 2, ceil_mode=True)
            for _, m in stage.named_children():
                outs, y = [x], x
                for seq in m.layers:
                    y = conv(seq_conv(seq), y)
                    outs.append(y)
                xt = conv(seq_conv(m.concat), torch.cat(outs, 1))
                fw, fb = fcs[id(m)]
                xt = xt * (F.relu6(F.conv2d(F.adaptive_avg_pool2d(xt, 1), fw, fb) + 3.0) / 6.0)
                x = xt + x if m.identity else xt
            if sname in G:
                total = total + (x * G[sname]).sum()
        return total

    leaves = [x0] + [v for tup in P.values() for v in tup[:3]] + [v for tup in fcs.values() for v in tup]

    def both():
        for t in leaves:
            t.grad = None
        forward().backward()

    def fwd_only():
        with torch.no_grad():
            forward()

    return both, fwd_only


def family(key, lay):
    if key.endswith(".ese"):
        return "ese"
    if key.endswith(".sum"):
        return "module-input sum"
    if key.endswith(".pool"):
        return "pool"
    if key.startswith("stem"):
        return "stem 3x3"
    return "concat 1x1" if key.endswith(".concat") else "layer 3x3"


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
            model.compute_losses(inputs, fpn_grads=True)
            model.compute_losses(inputs, vovnet_grads=True)
        size = model.canvas_size(inputs)
        plan_f, plan_v = model.get_loss_plan(*size, fpn_grads=True), model.get_loss_plan(*size, vovnet_grads=True)
        L = plan_v.vovnet_layers
        convs = {k: lay for k, lay in L.items() if hasattr(lay, "conv")}
        da = sum(lay.da.numel() for lay in L.values()) * 4 / 2**20
        dw = sum(lay.dw.numel() + lay.dw_level.numel() for lay in convs.values()) * 4 / 2**20
        filt = sum(lay.keep[1].numel() for lay in convs.values()) * 4 / 2**20
        rest = sum(t.numel() for lay in L.values() for t, _ in lay._raw) * 4 / 2**20 - da - dw
        top = L[f"stage5.{list(model.backbone.bottom_up.stage5.named_children())[-1][0]}.concat"]
        print(f"{exp} {B}x{H}x{W}: stage5 {top.H}x{top.W}, {int(plan_v.det_count.cpu())} positives, activations: "
              f"{('f32', 'f16x2', 'bf16x3')[top.args.x_mode]}, slab {plan_v.tower_slab[0].numel() * 4 / 2**20:.0f} MiB (fpn_grads plan: "
              f"{plan_f.tower_slab[0].numel() * 4 / 2**20:.0f} MiB)")
        print(f"  (d) added memory: da / g_xt {da:.0f} MiB, dw_level + dw {dw:.0f} MiB, f32 filter copies {filt:.0f} MiB, q / r / eSE vectors and fc gradients {rest:.0f} MiB")
        tf, tv = [], []
        for _ in range(rounds):
            tf.append(events(plan_f.run, iters))
            tv.append(events(plan_v.run, iters))
        a = report("(a) captured plan, fpn_grads (parent)", tf)[0]
        b = report("(a) captured plan, vovnet_grads", tv)[0]
        print(f"      added by the VoVNet backward: {b - a:.1f} us ({(b - a) / a * 100:.1f} % of the parent's plan)")
        L_ = hip.lib()
        fam_t, fam_f, stage_t, calls = {}, {}, {}, []

        def note(key, what, us, flop=0.0):
            f = family(key, None) + (" " + what if what else "")
            fam_t[f], fam_f[f] = fam_t.get(f, 0.0) + us, fam_f.get(f, 0.0) + flop
            stage_t[key.split(".")[0]] = stage_t.get(key.split(".")[0], 0.0) + us
            calls.append((us, f"{key} {what}".strip(), flop))

        med = lambda fn: sorted(events(fn, iters) for _ in range(rounds))[rounds // 2]
        for key, lay in L.items():
            if key not in convs:
                note(key, "", med(lambda lay=lay: lay.launch(L_, hip.current_stream())))
                continue
            flop = 2.0 * B * lay.Ho * lay.Wo * lay.Cout * lay.ksize**2 * lay.Cin
            note(key, "weight gradient", med(lambda lay=lay: hip.check(L_.dd3d_vovnet_conv_wgrad(C.byref(lay.args), hip.current_stream()), "wgrad")), flop)
            note(key, "input gradient", med(lambda lay=lay: hip.check(L_.dd3d_vovnet_conv_dgrad(C.byref(lay.args), hip.current_stream()), "dgrad")), flop)
        total = sum(fam_t.values())
        print(f"  (b) sum of the calls alone: {total:.1f} us")
        for f in sorted(fam_t, key=lambda f: -fam_t[f]):
            rate = f", {fam_f[f] / fam_t[f] * 1e-6:.1f} TF = {fam_f[f] / fam_t[f] * 1e-6 / 155.0 * 100:.0f} % of the 155 TF f32-matrix peak" if fam_f[f] else ""
            print(f"      {f}: {fam_t[f]:.1f} us ({fam_t[f] / total * 100:.0f} %){rate}")
        print("      per stage: " + ", ".join(f"{k} {v:.1f}" for k, v in stage_t.items()))
        for us, name, flop in sorted(calls, reverse=True)[:5]:
            lay = L[name.split(" ")[0]]
            shape = f" ({lay.ksize}x{lay.ksize} {lay.Cin}->{lay.Cout} at {lay.H}x{lay.W}, {flop / us * 1e-6:.1f} TF)" if flop else ""
            print(f"      slowest: {name}{shape}: {us:.1f} us")
        both, fwd_only = torch_vovnet(model, plan_v)
        for _ in range(2):
            both()
            fwd_only()
        torch.cuda.synchronize()
        t2 = report("(c) torch autograd over stem_2 .. stage5, forward + backward", [events(both, iters) for _ in range(rounds)])[0]
        t1 = report("(c) torch autograd over stem_2 .. stage5, forward only", [events(fwd_only, iters) for _ in range(rounds)])[0]
        print(f"      torch backward alone (difference): {t2 - t1:.1f} us; new kernels / torch backward = {total / max(t2 - t1, 1e-9):.2f}", flush=True)
        del model, plan_f, plan_v, both, fwd_only, L, convs
        torch.cuda.empty_cache()


def errors():
    import subprocess
    out = os.path.join(ROOT, "profiles", "vovnet_grads_errors.txt")
    env = dict(os.environ, DD3D_VOVNET_ERRORS_FILE=out + ".whole")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-s", "-p", "no:cacheprovider", os.path.join(ROOT, "tests", "test_vovnet_whole_model_gpu.py"),
                        os.path.join(ROOT, "tests", "test_vovnet_grads_gpu.py")], env=env, capture_output=True, text=True, cwd=ROOT)
    seam = [l[l.index("[vovnet_grads]"):] for l in r.stdout.splitlines() if "[vovnet_grads]" in l]
    with open(out, "w") as f:
        f.write("Measured deviation from float64 autograd over the bar 8 * max(d32, 2^-23 * max|g64|), per family (MI355X).\n\n")
        f.write("DD3D.compute_losses(vovnet_grads=True), V2-99, 1 x 128 x 256 (tests/test_vovnet_whole_model_gpu.py):\n")
        if os.path.exists(out + ".whole"):
            f.write(open(out + ".whole").read())
            os.remove(out + ".whole")
        f.write("\nThe seams (tests/test_vovnet_grads_gpu.py):\n" + "\n".join(seam) + "\n")
    print(r.stdout[-3000:])
    sys.exit(r.returncode)


if __name__ == "__main__":
    errors() if "--errors" in sys.argv else main()
