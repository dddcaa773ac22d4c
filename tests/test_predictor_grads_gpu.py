"""Predictor-layer backward on the MI355X (csrc/predictor_grads.hip, engine.LossPlan(pred_grads=True)): dd3d_predictor_wgrad and
dd3d_predictor_dgrad at their C-ABI seam on seeded groups (tests/predictor_grad_cases.py) against the float64 autograd of the CPU oracle
(tests/predictor_grad_oracle.py), in the three activation storages; sentinel-framed outputs, clamped channels, a zero Scale, batches
without positives, shared against per-level filters, determinism; and DD3D.compute_losses(predictor_grads=True) end to end.

The bar of a family (weight, bias, scale, offset, a tower's da) in a case is 8 * max(d32, 2^-23 * max|g64|): d32 is the deviation of the
oracle's float32 autograd from its float64 autograd, computed here on the CPU (loss_grad_oracle.bar).
"""
import pytest
import torch

from tests import loss_grad_cases as GC
from tests import predictor_grad_cases as PC
from tests import predictor_grad_oracle as PO

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
POISON = 3.0e30  # pad words of the inputs: a kernel that read them would not stay finite


def nhwc(x, pitch, pad=POISON):
    B, C, H, W = x.shape
    t = torch.full((B, H, W, pitch), pad, dtype=torch.float32)
    t[..., :C] = x.permute(0, 2, 3, 1)
    return t.contiguous().cuda()


def run_seam(case, storage="f32", plane_scale=1.0, act_pad=0):
    """One weight-gradient and one input-gradient call on a GroupCase.  Returns (results shaped like PO.group_grads, on the CPU; the
    PredGroupGrads; the float32 activations the storage decodes to)."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import PredGroupGrads
    n, Cin = case.n, case.Cin
    pitch = (n + 3) // 4 * 4
    keep = []
    if storage == "f32":
        bufs = [nhwc(a, Cin + act_pad) for a in case.act]
        act, dec, mode, apitch = [b.data_ptr() for b in bufs], case.act, hip.PG_ACT_F32, Cin + act_pad
    else:
        enc = [PC.encode_f16x2(a, plane_scale) if storage == "f16x2" else PC.encode_bf16x3(a) for a in case.act]
        bufs = [p.cuda() for p, _ in enc]
        act, dec, mode, apitch = [b.data_ptr() for b in bufs], [d for _, d in enc], (hip.PG_ACT_F16X2 if storage == "f16x2" else hip.PG_ACT_BF16X3), 0
    keep.append(bufs)
    g, maps = [nhwc(x, pitch) for x in case.g], [nhwc(x, pitch) for x in case.maps]
    uniq = {}
    w = [uniq.setdefault(id(x), x.permute(0, 2, 3, 1).contiguous().cuda()) for x in case.w]
    bias = [uniq.setdefault(id(x), x.contiguous().cuda()) for x in case.bias]
    scale = [s.contiguous().cuda() for s in case.scale]
    grp = PredGroupGrads("cuda", case.B, case.level_hw, Cin, n, pitch, act, mode, apitch, plane_scale, g, maps, w, bias, scale,
                         lo=None if case.lo is None else case.lo.cuda(), slot=case.slot.cuda(), fill=SENTINEL, guard=64)
    grp.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    grp.keep_alive = keep
    return collect(grp), grp, dec


def collect(grp):
    nchw_w = lambda t: t.view(grp.n, 3, 3, grp.Cin).permute(0, 3, 1, 2).cpu()
    return {"dw_level": [nchw_w(grp.dw_level[l]) for l in range(grp.L)], "q": [grp.q[l].cpu() for l in range(grp.L)],
            "r": [grp.r[l].cpu() for l in range(grp.L)], "dw": {o: nchw_w(grp.dw[o]) for o in grp.owners},
            "db": {o: grp.db[o].cpu() for o in grp.owners}, "dscale": grp.dscale.cpu(), "doffset": grp.doffset.cpu(),
            "da": [d.permute(0, 3, 1, 2).cpu() for d in grp.da]}


def check(got, ref64, ref32, what):
    a, b, k = PO.family_vectors(ref64), PO.family_vectors(ref32), PO.family_vectors(got)
    for fam in PO.FAMILIES:
        assert bool(torch.isfinite(k[fam]).all()), (what, fam)
        keep = torch.ones(a[fam].shape[0], dtype=torch.bool)
        bar, d32, gmax = PO.bar(a[fam], b[fam], keep)
        dev = float((k[fam].double() - a[fam]).abs().max())
        print(f"[predictor_grads] {what} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e}")
        assert dev <= bar, (what, fam, dev, bar, d32, gmax)


def frame_ok(grp):
    """Guard words and the rows of dw / db that belong to no first level keep the sentinel; every other output word is written."""
    assert grp.guards_intact(SENTINEL)
    for l in range(grp.L):
        for t in (grp.dw[l], grp.db[l]):
            assert bool((t == SENTINEL).all()) if l not in grp.owners else not bool((t == SENTINEL).any())
    for t in [grp.part, grp.qpart, grp.dw_level, grp.q, grp.r, grp.dscale, grp.doffset] + grp.da:
        assert not bool((t == SENTINEL).any())


# level shapes: 1x1 (only the centre tap lands), 1x257 (a row longer than four units, the last one pixel long), 3x10 and 5x7 (odd, no
# multiple of any block), 30x70 (more units than slices: several units per slice), the pyramid of a 64x128 canvas
SEAM_CASES = {
    "1x1_n1_c32_f32": (dict(level_hw=[(1, 1)], B=1, n=1, Cin=32, seed=1), "f32", 1.0),
    "1x257_n5_c64_f16s16": (dict(level_hw=[(1, 257)], B=1, n=5, Cin=64, seed=2), "f16x2", 16.0),
    "3x10_5x7_n14_c32_bf16x3": (dict(level_hw=[(3, 10), (5, 7)], B=2, n=14, Cin=32, seed=3, zero_scale_level=1), "bf16x3", 1.0),
    "30x70_n5_c32_f32": (dict(level_hw=[(30, 70)], B=1, n=5, Cin=32, seed=4), "f32", 1.0),
    "pyramid_n55_c256_f16s1": (dict(level_hw=PC.PYRAMID_64x128, B=2, n=55, Cin=256, seed=5, zero_scale_level=2), "f16x2", 1.0),
    "pyramid_n110_c256_f32_per_level": (dict(level_hw=PC.PYRAMID_64x128, B=2, n=110, Cin=256, seed=6, per_level=True), "f32", 1.0),
    "pyramid_n14_c64_bf16x3_sparse": (dict(level_hw=PC.PYRAMID_64x128, B=2, n=14, Cin=64, seed=7, sparse=True), "bf16x3", 1.0),
}


@pytest.mark.parametrize("name", list(SEAM_CASES))
def test_seam_against_oracle(hiplib, name):
    kw, storage, ps = SEAM_CASES[name]
    case = PC.GroupCase(**kw)
    got, grp, dec = run_seam(case, storage, ps, act_pad=4 if storage == "f32" else 0)
    frame_ok(grp)
    check(got, case.ref(torch.float64, dec), case.ref(torch.float32, dec), name)
    if kw.get("zero_scale_level") is not None:  # s_l = 0: finite, and the Scale gradients of that level are the oracle's (checked above), not 0
        l = kw["zero_scale_level"]
        assert float(got["dscale"][l, :2].abs().max()) > 0.0 and float(got["da"][l].abs().max()) > 0.0  # (the slot-less channels still reach da)
    again, _, _ = run_seam(case, storage, ps, act_pad=4 if storage == "f32" else 0)
    for fam, v in PO.family_vectors(again).items():
        assert torch.equal(v, PO.family_vectors(got)[fam]), (name, fam)  # the same call twice: the same bits


@pytest.mark.parametrize("storage,ps", [("f16x2", 16.0), ("f16x2", 1.0), ("bf16x3", 1.0)])
def test_plane_and_f32_paths_agree_on_the_same_values(hiplib, storage, ps):
    case = PC.GroupCase(level_hw=[(5, 7), (3, 10)], B=2, n=14, Cin=64, seed=11)
    got, _, dec = run_seam(case, storage, ps)
    twin = PC.GroupCase(level_hw=[(5, 7), (3, 10)], B=2, n=14, Cin=64, seed=11)
    twin.act = dec  # the f32 loader on the values the planes decode to (the stored maps stay the case's)
    twin.maps = case.maps
    f32, _, _ = run_seam(twin, "f32")
    for fam in PO.FAMILIES:
        assert torch.equal(PO.family_vectors(got)[fam], PO.family_vectors(f32)[fam]), fam  # the loaders hand over the same float32 values
    check(got, case.ref(torch.float64, dec), case.ref(torch.float32, dec), f"{storage}@{ps}")


def test_clamped_channels_give_exact_zeros(hiplib):
    """Stored maps with exact zeros on the clamped channels: those entries contribute exact zeros; a Scale whose channels are all
    clamped away gets an exact 0."""
    case = PC.GroupCase(level_hw=[(3, 10), (5, 7)], B=2, n=14, Cin=32, seed=21)
    clamped = torch.isfinite(case.lo)
    assert all(bool((m[:, clamped] == 0).any()) for m in case.maps)
    for m in case.maps:
        m[:, clamped] = 0.0  # every clamped channel sits on its clamp everywhere
    case.slot = torch.where(clamped, torch.tensor(2, dtype=torch.int32), case.slot)  # slot 2 = exactly the clamped channels
    got, grp, _ = run_seam(case)
    for l in range(case.L):
        assert float(got["dw_level"][l][clamped].abs().max()) == 0.0 and float(got["q"][l][clamped].abs().max()) == 0.0
        assert float(got["r"][l][clamped].abs().max()) == 0.0 and float(got["dscale"][l, 2]) == 0.0 and float(got["doffset"][l, 2]) == 0.0
    assert float(got["dw"][0][clamped].abs().max()) == 0.0 and float(got["dw"][0][~clamped].abs().min()) > 0.0
    check(got, case.ref(torch.float64), case.ref(torch.float32), "all-clamped")
    # the same gradient with those channels' G zeroed gives the same da: nothing of a clamped entry reaches the tower
    twin = PC.GroupCase(level_hw=[(3, 10), (5, 7)], B=2, n=14, Cin=32, seed=21)
    twin.maps, twin.slot = case.maps, case.slot
    for g in twin.g:
        g[:, clamped] = 0.0
    tw, _, _ = run_seam(twin)
    assert all(torch.equal(x, y) for x, y in zip(tw["da"], got["da"]))


def test_no_positives_gives_exact_zeros(hiplib):
    """A sparse family on a batch without positives: every output is an exact zero (and written)."""
    case = PC.GroupCase(level_hw=PC.PYRAMID_64x128, B=2, n=14, Cin=64, seed=31, sparse=True, positives=False)
    got, grp, _ = run_seam(case)
    frame_ok(grp)
    for fam, v in PO.family_vectors(got).items():
        assert float(v.abs().max()) == 0.0, fam


def test_shared_sum_equals_scaled_per_level_partials(hiplib):
    """PER_LEVEL_PREDICTORS on and off: with the same filter values on every level the per-level partials are the same bits, the shared
    module's gradient is their scaled sum in level order, the per-level modules' gradients are the scaled partials themselves."""
    kw = dict(level_hw=PC.PYRAMID_64x128, B=2, n=5, Cin=32, seed=41)
    shared = PC.GroupCase(**kw)
    split = PC.GroupCase(**kw)
    split.w, split.bias = [x.clone() for x in shared.w], [x.clone() for x in shared.bias]  # equal values, distinct modules
    a, ga, _ = run_seam(shared)
    b, gb, _ = run_seam(split)
    assert ga.owners == [0] and gb.owners == list(range(shared.L))
    assert all(torch.equal(x, y) for x, y in zip(a["dw_level"], b["dw_level"])) and all(torch.equal(x, y) for x, y in zip(a["da"], b["da"]))
    total, mag = torch.zeros_like(a["dw"][0], dtype=torch.float64), torch.zeros_like(a["dw"][0], dtype=torch.float64)
    for l in range(shared.L):
        s = shared.scale[l][:, None, None, None]
        assert torch.equal(b["dw"][l], s * b["dw_level"][l])
        total, mag = total + s.double() * b["dw_level"][l].double(), mag + (s.double() * b["dw_level"][l].double()).abs()
    # the kernel's sum is one fmaf per level: at most one float32 rounding of a partial sum per level
    assert bool(((total - a["dw"][0].double()).abs() <= shared.L * 2.0**-24 * mag).all())
    check(b, split.ref(torch.float64), split.ref(torch.float32), "per-level")


def test_bad_arguments_are_rejected(hiplib):
    import ctypes as C
    from dd3d_amd import hip
    case = PC.GroupCase(level_hw=[(3, 10)], B=1, n=5, Cin=32, seed=51)
    _, grp, _ = run_seam(case)
    lib, st = hip.lib(), hip.current_stream()
    for field, value in (("Cin", 48), ("g_pitch", 6), ("act_pitch", 34), ("n", 0), ("n", hip.PG_MAX_N + 1), ("act_mode", 7), ("n_slices", 0)):
        old = getattr(grp.args, field)
        setattr(grp.args, field, value)
        assert lib.dd3d_predictor_wgrad(C.byref(grp.args), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_predictor_wgrad"), field
        setattr(grp.args, field, old)
    old = grp.args.g[0]
    grp.args.g[0] = None
    assert lib.dd3d_predictor_wgrad(C.byref(grp.args), st) == -1 and lib.dd3d_predictor_dgrad(C.byref(grp.args), st) == -1
    grp.args.g[0] = old
    assert lib.dd3d_predictor_grad_slices(C.byref(grp.args)) == grp.n_slices == hip.pred_grad_slices(1, [(3, 10)])
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------- end to end
def _group_inputs(plan, name):
    """A captured group's inputs as the oracle takes them: the plan's own tower outputs (the values its storage decodes to), stored maps
    and head-map gradients, NCHW on the CPU."""
    grp = plan.pred_groups[name]
    g, maps, w, bias, scale, lo, slot = grp.keep
    t = {"cls": 0, "box2d": 1, "box3d": 2}[grp.tower]
    n = grp.n
    case = PC.GroupCase.__new__(PC.GroupCase)
    case.act = [plan.tower_out[l][t].nchw().float().cpu().contiguous() for l in range(grp.L)]
    case.g = [x[..., :n].permute(0, 3, 1, 2).cpu().contiguous() for x in g]
    case.maps = [x[..., :n].permute(0, 3, 1, 2).cpu().contiguous() for x in maps]
    uniq = {}
    case.w = [uniq.setdefault(x.data_ptr(), x.permute(0, 3, 1, 2).cpu().contiguous()) for x in w]
    case.bias = [uniq.setdefault(x.data_ptr(), x.cpu()) for x in bias]
    case.scale, case.lo, case.slot = [x.cpu() for x in scale], (None if lo is None else lo.cpu()), slot.cpu()
    return case, grp


def _end_to_end(exp, weights, B, H, W, ds, math=None, act_scale=None):
    from dd3d_amd.synthetic import make_gt_instances, make_inputs
    from tests.test_loss_grads_gpu import _model
    from tests.test_losses_gpu import _maps_nchw
    model = _model(exp, weights)
    model.math, model.act_scale = math, act_scale
    nusc = hasattr(model, "attr_logits")
    inputs = make_inputs(B, H, W, dataset=ds)
    gt = make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES,
                           num_attributes=model.attr_logits.out_channels if nusc else None, empty_images=(1, ))
    for x, g in zip(inputs, gt):
        x["instances"] = g
    ref_losses, ref_grads = model.compute_losses(inputs, head_grads=True)
    losses, grads, params = model.compute_losses(inputs, predictor_grads=True)
    # the loss dict and the head-map gradients are those of head_grads=True, bit for bit
    assert list(losses) == list(ref_losses) and all(torch.equal(losses[k], ref_losses[k]) for k in losses)
    assert all(torch.equal(grads[k], ref_grads[k]) for k in ref_grads)
    plan = model.get_loss_plan(*model.canvas_size(inputs), pred_grads=True)
    names = [op.name for op in plan.ops]
    assert names[-4:] == ["loss_backward", "predictor_grads.cls_map", "predictor_grads.box2d_map", "predictor_grads.box3d_map"]
    towers = sorted(set(grads) - set(ref_grads))
    L = len(plan.features)
    assert towers == sorted(f"{t}_tower_out{l}" for t in ("cls", "box2d", "box3d") for l in range(L))
    assert all(grads[k].shape == (B, 256, plan.features[int(k[-1])].H, plan.features[int(k[-1])].W) and grads[k].dtype == torch.float32 for k in towers)
    cpu = GC.cpu_model(exp)
    assert sorted(params) == PO.predictor_param_names(cpu)
    assert all(params[k].shape == p.shape and params[k].dtype == torch.float32 for k, p in cpu.named_parameters() if k in params)
    # each group's raw outputs against the group oracle on the plan's own inputs
    for name in plan.pred_groups:
        case, grp = _group_inputs(plan, name)
        check(collect(grp), case.ref(torch.float64), case.ref(torch.float32), f"e2e:{ds}:{name}")
    # the named parameter gradients and the tower gradients against the model's modules applied one by one (float64 / float32 autograd)
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    tw = {t: [plan.tower_out[l][i].nchw().float().cpu() for l in range(L)] for i, t in enumerate(("cls", "box2d", "box3d"))}
    hg, hm = {k: v.cpu() for k, v in ref_grads.items()}, _maps_nchw(plan)
    p64, t64 = PO.model_grads(cpu, tw, hg, hm, torch.float64)
    p32, t32 = PO.model_grads(cpu, tw, hg, hm, torch.float32)
    fam_of = lambda k: "weight" if k.endswith(".weight") else "scale" if k.endswith(".scale") else "offset" if "offsets_" in k else "bias"
    for fam in ("weight", "bias", "scale", "offset"):
        ks = [k for k in sorted(params) if fam_of(k) == fam]
        a, b, c = (torch.cat([d[k].reshape(-1).cpu() for k in ks]) for d in (p64, p32, params))
        bar, d32, gmax = PO.bar(a, b, torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((c.double() - a).abs().max())
        print(f"[predictor_grads] e2e:{ds} named {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e}")
        assert dev <= bar and gmax > 0.0, (fam, dev, bar)
    for t in ("cls", "box2d", "box3d"):
        ks = [f"{t}_tower_out{l}" for l in range(L)]
        a, b, c = (torch.cat([d[k].reshape(-1).cpu() for k in ks]) for d in (t64, t32, grads))
        bar, d32, gmax = PO.bar(a, b, torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((c.double() - a).abs().max())
        print(f"[predictor_grads] e2e:{ds} {t} tower da: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e}")
        assert dev <= bar and gmax > 0.0, (t, dev, bar)
    # a second call is bit-equal; the captured graph equals launch-by-launch execution
    _, g2, p2 = model.compute_losses(inputs, predictor_grads=True)
    assert all(torch.equal(g2[k], grads[k]) for k in grads) and all(torch.equal(p2[k], params[k]) for k in params)
    model.use_graph = False
    model.invalidate_plans()
    l3, g3, p3 = model.compute_losses(inputs, predictor_grads=True)
    assert all(torch.equal(l3[k], losses[k]) for k in losses)
    assert all(torch.equal(g3[k], grads[k]) for k in grads) and all(torch.equal(p3[k], params[k]) for k in params)
    return model, plan


@pytest.mark.parametrize("exp,weights,B,H,W,ds", [("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti"),
                                                   ("dd3d_nusc_dla34", "dla34_nusc", 6, 128, 224, "nusc")])
def test_compute_losses_predictor_grads_end_to_end(hiplib, exp, weights, B, H, W, ds):
    model, plan = _end_to_end(exp, weights, B, H, W, ds)
    from dd3d_amd import hip
    assert plan.pred_groups["cls_map"].args.act_mode == hip.PG_ACT_F16X2 and plan.pred_groups["cls_map"].args.plane_scale == 16.0


def test_compute_losses_predictor_grads_bf16x3(hiplib):
    from dd3d_amd import hip
    _, plan = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti", math="bf16x3")
    assert plan.pred_groups["cls_map"].args.act_mode == hip.PG_ACT_BF16X3


def test_compute_losses_predictor_grads_plane_scale_1(hiplib):
    _, plan = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti", act_scale=1.0)
    assert plan.pred_groups["cls_map"].args.plane_scale == 1.0


def test_reduced_modes_name_themselves(hiplib):
    from tests.test_loss_grads_gpu import _model
    model = _model("dd3d_kitti_dla34", "dla34_kitti")
    model.math = "bf16x2"
    with pytest.raises(NotImplementedError, match="bf16x2"):
        model.get_loss_plan(1, 128, 128, pred_grads=True)


# --------------------------------------------------------------------------------------------------- the reference-modules golden
def _run_reference_groups(model, towers, maps, case):
    """dd3d_loss_backward on a reference chain's head maps, then the predictor backward of every group on its gradient maps and the f32
    tower outputs.  Returns a dry-run LossPlan (the groups' folding, no device work of its own) whose groups hold the device results, so
    that LossPlan.predictor_grads assembles them under the parameters' names."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import LossPlan, PredGroupGrads
    from tests.test_loss_grads_gpu import run_seam as loss_seam
    B = towers["cls"][0].shape[0]
    lg = loss_seam(case)
    assert lg["num_pos"] == case.num_pos and lg["primal_mismatch"] == 0
    plan = LossPlan(model, B, *PC.REFERENCE_CANVAS, device="cpu", dry_run=True, pred_grads=True)
    raw = {"cls_map": ("cls", ["logits", "attr", "speed"]), "box2d_map": ("b2d", ["box2d_reg", "centerness"]),
           "box3d_map": ("b3d", ["quat", "ctr", "depth", "size", "conf"])}
    for gname, dry in list(plan.pred_groups.items()):
        _, _, w, bias, scale, lo, slot = dry.keep
        kind, keys = raw[gname]
        stored = [torch.cat([maps[f"{k}{l}"] for k in keys if f"{k}{l}" in maps], 1) for l in range(dry.L)]
        assert all(s.shape[1] == dry.n for s in stored)
        pitch = (dry.n + 3) // 4 * 4
        acts = [nhwc(a, 256) for a in towers[dry.tower]]
        uniq = {}
        grp = PredGroupGrads("cuda", B, PC.PYRAMID_64x128, 256, dry.n, pitch, [a.data_ptr() for a in acts], hip.PG_ACT_F32, 256, 1.0,
                             [g.cuda() for g in lg["raw"][kind]], [nhwc(s, pitch) for s in stored],
                             [uniq.setdefault(x.data_ptr(), x.cuda()) for x in w], [uniq.setdefault(x.data_ptr(), x.cuda()) for x in bias],
                             [x.cuda() for x in scale], lo=None if lo is None else lo.cuda(), slot=slot.cuda(), fill=SENTINEL, guard=64)
        assert grp.owners == dry.owners and lg["raw"][kind][0].shape[-1] == pitch
        grp.launch(hip.lib(), hip.current_stream())
        torch.cuda.synchronize()
        frame_ok(grp)
        grp.convs, grp.slots, grp.tower, grp.acts = dry.convs, dry.slots, dry.tower, acts
        plan.pred_groups[gname] = grp
    return plan


def test_batch_without_positives_reaches_the_cls_group_only(hiplib):
    """dd3d_loss_backward on a batch without ground truth: the logits carry the focal loss's gradient, every other family is zero -- so
    the cls group's gradients are non-zero and the box2d and box3d groups' parameter gradients and their towers' da are exact zeros."""
    from dd3d_amd.structures import Boxes, Boxes3D, Instances
    model, towers, maps, case = PC.reference_chain("kitti_b2")

    def empty():
        inst = Instances((1, 1))
        inst.gt_boxes, inst.gt_classes = Boxes(torch.zeros((0, 4))), torch.zeros(0, dtype=torch.long)
        inst.gt_boxes3d = Boxes3D(torch.zeros((0, 4)), torch.zeros((0, 2)), torch.zeros((0, 1)), torch.zeros((0, 3)), torch.zeros((0, 3, 3)))
        return inst

    none = GC.Case(model, maps, [empty(), empty()], PC.PYRAMID_64x128, case.inv_K)
    assert none.num_pos == 0
    tw, params = _run_reference_groups(model, towers, maps, none).predictor_grads()
    for k, v in list(params.items()) + list(tw.items()):
        cls_side = k.startswith("fcos2d_head.cls_logits") or k.startswith("cls_tower_out")
        assert (float(v.abs().max()) > 0.0) if cls_side else (float(v.abs().max()) == 0.0), k


@pytest.mark.parametrize("name", list(PC.REFERENCE_CASES))
def test_kernels_match_the_reference_modules_golden(hiplib, name):
    """The reference's own heads and loss modules under torch autograd (tests/golden/predictor_grads_*.npz) against the kernels: the
    golden's seeded features through the CPU towers and predictors, dd3d_loss_backward on those head maps, then the predictor backward
    on its gradient maps and the f32 tower outputs, assembled under the parameters' names by LossPlan.predictor_grads.  Within 2 * bar:
    the golden is a float32 autograd, within one bar of the float64 gradient like the kernels."""
    import os
    import numpy as np
    from tests.test_predictor_grads import ROOT, golden_families
    z = np.load(os.path.join(ROOT, "tests", "golden", f"predictor_grads_{name}.npz"))
    model, towers, maps, case = PC.reference_chain(name)
    plan = _run_reference_groups(model, towers, maps, case)
    tw, params = plan.predictor_grads()
    params, tw = {k: v.cpu() for k, v in params.items()}, {k: v.cpu() for k, v in tw.items()}
    p64, t64 = PO.model_grads(model, towers, case.ref(torch.float64), maps, torch.float64)
    p32, t32 = PO.model_grads(model, towers, case.ref(torch.float32), maps, torch.float32)
    f64, f32, got = golden_families(z, p64, t64), golden_families(z, p32, t32), golden_families(z, params, tw)
    for fam, (gold, a) in f64.items():
        bar, d32, gmax = PO.bar(a, f32[fam][1], torch.ones(a.shape[0], dtype=torch.bool))
        dev, dev64 = float((got[fam][1].double() - gold.double()).abs().max()), float((got[fam][1].double() - a).abs().max())
        print(f"[predictor_grads] ref:{name} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernels against the golden {dev:.3e} (bar {2 * bar:.3e}), "
              f"against float64 {dev64:.3e} (bar {bar:.3e})")
        assert dev <= 2 * bar and dev64 <= bar, (name, fam, dev, dev64, bar)
