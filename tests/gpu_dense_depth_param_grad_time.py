"""Dev tool (GPU): what each depth of DD3DDenseDepth's backward chain adds to the captured loss plan, beside torch autograd over the same
composition, with make_depth_maps ground truth: DLA-34 at 1 and 4 x 384 x 1280, V2-99 at 1 x 384 x 1280.

  (a) the captured plan of compute_losses at every depth -- no flag, head_grads, predictor_grads, tower_grads, fpn_grads, then
      backbone_grads and stem_grads (DLA-34) or vovnet_grads and vovnet_stem_grads (V2-99) -- replayed on staged inputs; device events
      around `--iters` replays, `--rounds` rounds, the plans taken in turn within a round; reported: the median over the rounds, their
      range, and the difference to the parent depth = what the stage adds
  (b) torch autograd on the device over the same composition in float32: the oracle's forward (oracle/dense_depth_oracle.py) from the
      normalised image to the raw maps, the up-sampling and the masked smooth-L1 means, backward to every parameter; forward + backward,
      and an estimate of the backward alone (the difference to a forward-only pass)

    python tests/gpu_dense_depth_param_grad_time.py > profiles/dense_depth_param_grads_time.txt

With `--errors` it runs tests/test_dense_depth_param_grads_gpu.py instead, in a child process, with DD3D_DENSE_DEPTH_ERRORS_FILE pointing
at profiles/dense_depth_param_grads_errors.txt: the measured use of the bar per (case, stage, family)."""
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

DLA_LADDER = [None, "head_grads", "predictor_grads", "tower_grads", "fpn_grads", "backbone_grads", "stem_grads"]
V99_LADDER = DLA_LADDER[:5] + ["vovnet_grads", "vovnet_stem_grads"]
PLAN_FLAG = {"predictor_grads": "pred_grads"}
HEAD = {"MODEL": {"META_ARCHITECTURE": "DD3DDenseDepth"}, "DD3D": {"FCOS3D": {"DEPTH_HEAD": {"LOSS_TYPE": "L1", "LOSS_WEIGHT": 1.0}}}}
CASES = [("dd3d_kitti_dla34", "dla34_kitti", ["p3", "p4", "p5", "p6", "p7"], 1, DLA_LADDER), ("dd3d_kitti_dla34", "dla34_kitti", ["p3", "p4", "p5", "p6", "p7"], 4, DLA_LADDER),
         ("dd3d_kitti_v99", "v99_kitti", ["p2", "p3", "p4", "p5", "p6"], 1, V99_LADDER)]
H, W = 384, 1280


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


def report(name, st):
    med = statistics.median(st)
    print(f"  {name}: median {med:.1f} us, range {min(st):.1f} .. {max(st):.1f} us over {len(st)} rounds")
    return med


def torch_composition(model, cfg, inputs, depths):
    """(forward + backward, forward only) of the same composition in torch on the device, float32."""
    from oracle import dense_depth_oracle as DDO
    sd = {k: (v.detach().float().cuda().clone() if v.is_floating_point() else v.detach().cuda()) for k, v in model.state_dict().items()}
    leaves = [sd[k].requires_grad_(True) for k, _ in model.named_parameters()]
    batch = [dict(x, image=x["image"].cuda().float(), intrinsics=x["intrinsics"].cuda()) for x in inputs]
    c3 = cfg.DD3D.FCOS3D
    gt = torch.stack([d.cuda() for d in depths])  # (every image has the canvas' size)
    M = (gt >= float(c3.MIN_DEPTH)) & (gt <= float(c3.MAX_DEPTH))
    beta, weight = float(c3.LOSS.SMOOTH_L1_BETA), float(c3.DEPTH_HEAD.LOSS_WEIGHT)

    def forward():
        with torch.device("cuda"):  # (the oracle makes its constants on the default device)
            maps, _ = DDO.dense_depth_forward(sd, cfg, batch)
        total = 0
        for l, m in enumerate(maps):
            n = (m[M] - gt[M]).abs()
            total = total + weight * torch.where(n < beta, 0.5 * n * n / beta, n - 0.5 * beta).mean() / (2.0**0.5)**l
        return total

    def both():
        for t in leaves:
            t.grad = None
        forward().backward()

    def fwd_only():
        with torch.no_grad():
            forward()

    return both, fwd_only


def main():
    g.build()
    import dd3d_amd.modeling  # noqa: F401
    from dd3d_amd import META_ARCH_REGISTRY, get_cfg
    from dd3d_amd.synthetic import load_calib, make_depth_maps, make_inputs, make_state_dict
    from tests.golden.make_dense_depth_loss_golden import _merge
    iters, rounds = arg("--iters", 10), arg("--rounds", 5)
    for exp, tag, feats, B, ladder in CASES:
        cfg = get_cfg(exp, _merge(HEAD, {"DD3D": {"IN_FEATURES": feats}}))
        model = META_ARCH_REGISTRY.get(cfg.MODEL.META_ARCHITECTURE)(cfg)
        model.load_state_dict(make_state_dict(model, calib=load_calib(tag)))
        model = model.to("cuda").eval()
        inputs = make_inputs(B, H, W)
        depths = make_depth_maps(inputs, seed=3000)
        for x, d in zip(inputs, depths):
            x["depth"] = d
        plans = []
        for flag in ladder:
            kw = {flag: True} if flag else {}
            for _ in range(3):  # plans, graph capture, staged inputs
                model.compute_losses(inputs, **kw)
            plans.append(model.get_loss_plan(B, H, W, **({PLAN_FLAG.get(flag, flag): True} if flag else {})))
        assert len({id(p) for p in plans}) == len(plans) and all(p.graph is not None for p in plans)
        deep = plans[-1]
        print(f"{exp} DD3DDenseDepth {B}x{H}x{W}: {len(deep.features)} levels at strides {deep.strides}, {int(deep.valid_count.cpu())} valid pixels, "
              f"FCOS3D.NORM {cfg.DD3D.FCOS3D.NORM!r}, {len(deep.ops)} ops at the deepest plan, slab of partials "
              f"{deep.tower_slab[0].numel() * 4 / 2**20:.0f} MiB")
        times = [[] for _ in plans]
        for _ in range(rounds):
            for t, p in zip(times, plans):
                t.append(events(p.run, iters))
        meds = [report(f"(a) captured plan, {flag or 'losses only'}", t) for flag, t in zip(ladder, times)]
        added = {flag: b - a for flag, a, b in zip(ladder[1:], meds[:-1], meds[1:])}
        for flag, d in added.items():
            print(f"      added by {flag}: {d:.1f} us ({d / meds[0] * 100:.1f} % of the forward-and-loss plan)")
        top = max(added, key=added.get)
        print(f"      the whole backward adds {meds[-1] - meds[0]:.1f} us to {meds[0]:.1f} us; the dominating stage is {top} ({added[top] / (meds[-1] - meds[0]) * 100:.0f} % of it)")
        both, fwd_only = torch_composition(model, cfg, inputs, depths)
        for _ in range(3):
            both()
            fwd_only()
        torch.cuda.synchronize()
        tb = report("(b) torch autograd, forward + backward", [events(both, max(1, iters // 2)) for _ in range(rounds)])
        tf = report("(b) torch autograd, forward only", [events(fwd_only, max(1, iters // 2)) for _ in range(rounds)])
        print(f"      torch backward alone (difference): {tb - tf:.1f} us; captured backward / torch backward = {(meds[-1] - meds[0]) / max(tb - tf, 1e-9):.2f}; "
              f"captured plan / torch forward + backward = {meds[-1] / tb:.2f}")
        del model, plans, deep, both, fwd_only
        torch.cuda.empty_cache()


def errors():
    out = os.path.join(ROOT, "profiles", "dense_depth_param_grads_errors.txt")
    if os.path.exists(out):
        os.remove(out)
    env = dict(os.environ, DD3D_DENSE_DEPTH_ERRORS_FILE=out)
    return subprocess.run([sys.executable, "-m", "pytest", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_dense_depth_param_grads_gpu.py")], env=env, cwd=ROOT).returncode


if __name__ == "__main__":
    sys.exit(errors() if "--errors" in sys.argv else main())
