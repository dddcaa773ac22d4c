"""Loss backward on the MI355X (csrc/loss_grads.hip, engine.LossPlan(grads=True), dd3d_amd.losses.FusedDD3DLoss): dd3d_loss_backward at
its C-ABI seam on the committed reference head maps and on hand-built non-smooth points, against the float64 autograd of the CPU oracle
(tests/loss_grad_oracle.py) and the reference's own loss modules (tests/golden/loss_grads_*.npz); sentinel-framed buffers, upstream
weights, batches without positives, determinism, DD3D.compute_losses(head_grads=True) end to end and the autograd entry point; the same
seam at every row of loss_grad_cases.SETTINGS (each loss setting away from its released value), on saturated logits and on the
renormalised decode path.

The bar of a family in a case is 8 * max(d32, 2^-23 * max|g64|): d32 is the deviation of the oracle's float32 autograd from its float64
autograd, computed here on the CPU (tests/loss_grad_oracle.bar).  Positives within 1e-4 of a non-smooth point (loss_grad_oracle.near_kink)
are compared for finiteness only.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import loss_grad_cases as GC
from tests import loss_grad_oracle as GO
from tests import loss_oracle as LO
from tests.test_losses_gpu import GOLDEN_CASES

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def run_seam(case, upstream=None, backward=True, maps=None):
    """dd3d_loss_assign + dd3d_loss_terms (+ dd3d_loss_backward) on a case's head maps, laid out as ForwardPlan._heads writes them; the
    gradient buffers are filled with SENTINEL before the call.  Returns a dict: losses, num_pos, grads (NCHW per level, on the CPU), raw
    (the NHWC buffers, on the CPU), channel counts, denoms and the flags word."""
    from dd3d_amd import hip
    from dd3d_amd.engine import losses as E
    model, level_hw, gt = case.model, case.level_hw, case.gt
    maps = case.maps if maps is None else maps
    dev = "cuda"
    B, L, C_ = maps["logits0"].shape[0], len(level_hw), int(model.num_classes)
    nusc, box3d = hasattr(model, "attr_logits"), not model.only_box2d
    strides = [s.stride for s in model.backbone_output_shape]
    a = hip.LossArgs()
    nloc = E._fill_common(a, model.cfg, model, level_hw, strides, B, hip.LOSS_MAX_GT)
    keep = []

    def nhwc(parts):
        t = torch.cat(parts, 1).permute(0, 2, 3, 1)
        pitch = (t.shape[-1] + 3) // 4 * 4
        buf = torch.zeros(t.shape[:-1] + (pitch, ), dtype=torch.float32)
        buf[..., :t.shape[-1]] = t
        buf = buf.contiguous().to(dev)
        keep.append(buf)
        return buf, pitch, t.shape[-1]

    A = model.attr_logits.out_channels if nusc else 0
    bufs = {"cls": [], "b2d": [], "b3d": []}
    nch = {}
    for l in range(L):
        b, a.cls_pitch, nch["cls"] = nhwc([maps[f"logits{l}"]] + ([maps[f"attr{l}"], maps[f"speed{l}"]] if nusc else []))
        bufs["cls"].append(b)
        b, a.b2d_pitch, nch["b2d"] = nhwc([maps[f"box2d_reg{l}"], maps[f"centerness{l}"]])
        bufs["b2d"].append(b)
        if box3d:
            b, a.b3d_pitch, nch["b3d"] = nhwc([maps[f"{k}{l}"] for k in ("quat", "ctr", "depth", "size", "conf")])
            bufs["b3d"].append(b)
        a.cls[l], a.box2d[l] = bufs["cls"][l].data_ptr(), bufs["b2d"][l].data_ptr()
        a.box3d[l] = bufs["b3d"][l].data_ptr() if box3d else None
    a.attr_off, a.num_attr, a.speed_off = (C_, A, C_ + A) if nusc else (0, 0, -1)
    locs = torch.cat([E.feature_locations(h, w, strides[l], model.feature_locations_offset) for l, (h, w) in enumerate(level_hw)]).to(dev)
    canon = torch.tensor([list(r) for r in model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES], dtype=torch.float32, device=dev)
    iK = case.inv_K.float().reshape(B, 9).contiguous().to(dev)
    off, recs = E.pack_gt(gt, hip.LOSS_MAX_GT, box3d, nusc, A, C_)
    g_off = torch.from_numpy(off).to(dev)
    g = torch.from_numpy(recs if recs.shape[0] else np.zeros((1, hip.LOSS_GT_FIELDS), np.float32)).to(dev)
    a.locations, a.canon_sizes, a.inv_K, a.gt_off, a.gt = locs.data_ptr(), canon.data_ptr(), iK.data_ptr(), g_off.data_ptr(), g.data_ptr()
    t = E._Targets(a, B * nloc, box3d, nusc, dev)
    nb = (B * nloc + hip.LOSS_BLOCK - 1) // hip.LOSS_BLOCK
    partials = torch.zeros((nb, hip.LOSS_TERMS), device=dev)
    out = torch.zeros(hip.LOSS_OUT, device=dev)
    npos = torch.zeros(1, dtype=torch.int32, device=dev)
    a.partials, a.n_partials, a.out, a.num_pos = partials.data_ptr(), nb, out.data_ptr(), npos.data_ptr()
    lib, st = hip.lib(), hip.current_stream()
    hip.check(lib.dd3d_loss_assign(C.byref(a), st), "assign")
    hip.check(lib.dd3d_loss_terms(C.byref(a), st), "terms")
    res = {"nch": nch, "targets": t}
    if backward:
        sent = lambda bs: [torch.full_like(b, SENTINEL) for b in bs]
        d_cls, d_b2d, d_b3d = sent(bufs["cls"]), sent(bufs["b2d"]), (sent(bufs["b3d"]) if box3d else None)
        up = torch.ones(hip.LOSS_OUT, device=dev) if upstream is None else torch.zeros(hip.LOSS_OUT, device=dev)
        if upstream is not None:
            up[:10] = torch.as_tensor(upstream, dtype=torch.float32).to(dev)
        denoms = torch.full((hip.LOSS_GRAD_DENOMS, ), 7.0, device=dev)
        ga = E.fill_grad_args(d_cls, d_b2d, d_b3d, up, denoms)
        hip.check(lib.dd3d_loss_backward(C.byref(a), C.byref(ga), st), "backward")
        torch.cuda.synchronize()
        res["grads"] = {k: v.cpu() for k, v in E.unpack_head_grads(d_cls, d_b2d, d_b3d, C_, A, bool(a.class_agnostic_3d)).items()}
        res["raw"] = {"cls": [b.cpu() for b in d_cls], "b2d": [b.cpu() for b in d_b2d], "b3d": [b.cpu() for b in d_b3d] if box3d else []}
        res["primal_mismatch"] = int(denoms.cpu().view(torch.int32)[3])
    torch.cuda.synchronize()
    n = int(npos.cpu())
    o = out.cpu()
    res["losses"] = {k: o[E.OUT_INDEX[k]] for k in E.loss_keys(box3d, nusc, n)}
    res["num_pos"], res["renorm"] = n, int(t.flags.cpu())
    return res


def check_against_oracle(case, got, upstream=None, what="", report=None, nan_row=None):
    """Every family within its bar of the float64 autograd off the kink mask; masked rows finite.  `nan_row`: a target whose rows must
    be NaN exactly where the float64 autograd's are; it is left out of the bar (d32 and max|g64| over the other rows)."""
    g64, g32 = case.ref(torch.float64, upstream), case.ref(torch.float32, upstream)
    keep = case.keep_rows()
    for fam in GO.families(case.p):
        a, b, k = GO.flat_family(g64, fam, case.p), GO.flat_family(g32, fam, case.p), GO.flat_family(got, fam, case.p)
        if nan_row is not None:
            assert torch.equal(torch.isnan(k[nan_row]), torch.isnan(a[nan_row])) and bool(torch.isfinite(k[nan_row][~torch.isnan(a[nan_row])]).all()), (what, fam)
            rest = torch.ones(a.shape[0], dtype=torch.bool)
            rest[nan_row] = False
            keep = keep & rest
            a, b, k = (torch.where(rest[:, None], x, torch.zeros_like(x)) for x in (a, b, k))
        assert bool(torch.isfinite(k).all()), (what, fam)
        bar, d32, gmax = GO.bar(a, b, keep)
        dev = float((k.double() - a)[keep].abs().max())
        print(f"[loss_grads] {what} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (dev/max {dev / max(gmax, 1e-30):.2e})")
        if report is not None:
            report[fam] = (dev, bar, gmax)
        assert dev <= bar, (what, fam, dev, bar, d32, gmax)


@pytest.fixture(scope="module")
def seam_runs(hiplib):
    """One seam run per committed head-map case, shared by the tests below."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = run_seam(GC.golden_case(name))
        return cache[name]

    return get


@pytest.mark.parametrize("name", list(GOLDEN_CASES))
def test_backward_at_seam_on_reference_head_maps(seam_runs, name):
    case, got = GC.golden_case(name), seam_runs(name)
    assert got["num_pos"] == case.num_pos > 20 and int(case.kink.sum()) <= GC.KINK_CAP * case.num_pos
    assert got["primal_mismatch"] == 0  # the dual decode's value part gives the forward's entangled error, bit for bit, in every positive
    check_against_oracle(case, got["grads"], what=name)


@pytest.mark.parametrize("name", list(GC.REFERENCE_CASES))
def test_backward_matches_reference_modules_golden(hiplib, name):
    """The gradients torch autograd gives the reference's own FCOS2DLoss / FCOS3DLoss / NuscenesLoss (make_loss_grad_golden.py)."""
    case = GC.reference_case(name)
    got = run_seam(case)
    assert got["primal_mismatch"] == 0
    check_against_oracle(case, got["grads"], what="ref:" + name)
    z, keep = case.golden, case.keep_rows()
    pos = torch.from_numpy(z["pos_inds"])
    assert torch.equal(pos, case.targets["pos_inds"])
    g32 = case.ref(torch.float32)
    for fam in GO.families(case.p):
        k = GO.flat_family(got["grads"], fam, case.p)
        ref = torch.from_numpy(z["dense_logits"]) if fam == "logits" else torch.from_numpy(z["pos_" + fam])
        mine = k if fam == "logits" else k[pos]
        kp = keep if fam == "logits" else keep[pos]
        # the golden is a float32 autograd: its own distance from the float64 gradient is the d32 of the bar
        bar, _, _ = GO.bar(GO.flat_family(case.ref(), fam, case.p), GO.flat_family(g32, fam, case.p), keep)
        dev = float((mine.double() - ref.double())[kp].abs().max()) if mine.numel() else 0.0
        print(f"[loss_grads] ref:{name} {fam}: against the reference modules {dev:.3e}, bar {2 * bar:.3e}")
        assert dev <= 2 * bar, (name, fam, dev, bar)  # both sides are within one bar of the float64 gradient


@pytest.mark.parametrize("H,W,agnostic", [(4, 4, False), (4, 4, True), (1, 257, False), (1, 257, True)])
def test_backward_on_handmade_nonsmooth_points(hiplib, H, W, agnostic):
    case = GC.handmade_case(H, W, class_agnostic=agnostic)
    got = run_seam(case)
    assert got["num_pos"] == len(case.specs) == case.num_pos and got["primal_mismatch"] == 0
    check_against_oracle(case, got["grads"], what=f"hand{H}x{W}{'a' if agnostic else ''}")
    g64 = case.ref()
    pos = case.targets["pos_inds"]
    C3 = 1 if agnostic else case.p["num_classes"]
    lab = case.targets["labels"][pos]
    row = lambda grads, fam, j: GO.flat_family(grads, fam, case.p)[pos[j]]
    for j, sp in enumerate(case.specs):
        c = 0 if agnostic else int(lab[j])
        if "depth" in sp:  # clamped away: no gradient into the depth channel, exactly
            assert float(row(got["grads"], "depth", j)[c]) == 0.0 and float(row(g64, "depth", j)[c]) == 0.0
        if "depth_exact" in sp:  # on the bound the clamp passes the gradient (torch's clamp backward is inclusive)
            assert float(row(got["grads"], "depth", j)[c]) != 0.0
        if "size" in sp:  # saturated tanh: 1 - tanh^2 == 0 in float32
            assert float(row(got["grads"], "size", j)[c]) == 0.0
        if sp.get("reg") == "tie":  # exact in both precisions: the tie splits in halves, as torch.min / torch.max do
            a, k = row(g64, "box2d_reg", j), row(got["grads"], "box2d_reg", j).double()
            assert float((a - k).abs().max()) <= 8 * 2.0**-23 * float(GO.flat_family(g64, "box2d_reg", case.p).abs().max())
        if "attr" in sp:
            assert float(row(got["grads"], "attr", j).abs().max()) == 0.0 and float(row(got["grads"], "speed", j).abs().max()) == 0.0
    # every candidate of matrix_to_quaternion was taken: the egocentric quaternion's largest component sits at 0, 1, 2, 3
    from oracle import dd3d_oracle as O
    for j in range(4):
        c = 0 if agnostic else int(lab[j])
        y, x = int(pos[j]) // W, int(pos[j]) % W
        q = torch.stack([case.maps["quat0"][0, k * C3 + c, y, x] for k in range(4)])[None].double()
        ctr = torch.stack([case.maps["ctr0"][0, k * C3 + c, y, x] for k in range(2)])[None].double() + case.targets["locations"][pos[j]][None].double()
        qn = q / q.norm()
        ego, _ = O.allocentric_to_egocentric(qn, ctr, case.inv_K.double())
        assert int(ego.abs().argmax()) == j, (j, ego)
        assert float(row(got["grads"], "quat", j).abs().max()) > 0.0


def test_sentinel_frame_and_exact_zeros(seam_runs):
    """Pad words up to the pitch keep the sentinel; background rows and the 3D channels of the other classes are exact zeros; every
    channel below the pitch is written."""
    for name in ("dla34_kitti_128x384_b2_ragged", "dla34_nusc_128x224_b6"):
        case, got = GC.golden_case(name), seam_runs(name)
        C_ = case.p["num_classes"]
        for kind, bufs in got["raw"].items():
            n = got["nch"][kind]
            for b in bufs:
                assert bool((b[..., n:] == SENTINEL).all()) and not bool((b[..., :n] == SENTINEL).any()), (name, kind)
        labels, pos = case.targets["labels"], case.targets["pos_inds"]
        bg = labels == C_
        for fam in GO.families(case.p):
            if fam != "logits":
                assert float(GO.flat_family(got["grads"], fam, case.p)[bg].abs().max()) == 0.0, (name, fam)
        for fam, k in (("quat", 4), ("ctr", 2), ("depth", 1), ("size", 3), ("conf", 1)):
            g = GO.flat_family(got["grads"], fam, case.p)[pos].reshape(-1, k, C_)
            other = torch.ones(len(pos), k, C_, dtype=torch.bool)
            other[torch.arange(len(pos)), :, labels[pos]] = False
            assert float(g[other].abs().max()) == 0.0 and float(g[~other].abs().max()) > 0.0, (name, fam)


def test_upstream_weights(hiplib, seam_runs):
    name = "dla34_nusc_128x224_b6"
    case = GC.golden_case(name)
    w = (torch.rand(10, generator=torch.Generator().manual_seed(3)) + 0.5).tolist()
    weighted = run_seam(case, upstream=w)["grads"]
    check_against_oracle(case, weighted, upstream=w, what="weighted")
    onehot = [run_seam(case, upstream=[1.0 if i == k else 0.0 for i in range(10)])["grads"] for k in range(10)]
    keep = case.keep_rows()
    for fam in GO.families(case.p):
        s = sum(w[k] * GO.flat_family(onehot[k], fam, case.p).double() for k in range(10))
        a = GO.flat_family(case.ref(torch.float64, w), fam, case.p)
        bar, _, _ = GO.bar(a, GO.flat_family(case.ref(torch.float32, w), fam, case.p), keep)
        assert float((s - GO.flat_family(weighted, fam, case.p).double()).abs().max()) <= bar, fam
    touched = lambda grads: {fam for fam in GO.families(case.p) if float(GO.flat_family(grads, fam, case.p).abs().max()) > 0.0}
    assert touched(onehot[GO.OUT_INDEX["loss_box3d_depth"]]) == {"depth"}
    assert touched(onehot[GO.OUT_INDEX["loss_box3d_quat"]]) == {"quat", "ctr"}  # allocentric: through the viewing ray
    assert touched(onehot[GO.OUT_INDEX["loss_conf3d"]]) == {"conf"} and touched(onehot[GO.OUT_INDEX["loss_cls"]]) == {"logits"}
    ego = GC.golden_case("dla34_kitti_variant_egocentric_agnostic")
    g = run_seam(ego, upstream=[1.0 if i == GO.OUT_INDEX["loss_box3d_quat"] else 0.0 for i in range(10)])["grads"]
    assert {fam for fam in GO.families(ego.p) if float(GO.flat_family(g, fam, ego.p).abs().max()) > 0.0} == {"quat"}


def test_no_positives_and_an_image_without_gt(hiplib):
    from dd3d_amd.structures import Boxes, Boxes3D, Instances
    case = GC.golden_case("dla34_kitti_128x384_b2_ragged")

    def empty():
        inst = Instances((1, 1))
        inst.gt_boxes, inst.gt_classes = Boxes(torch.zeros((0, 4))), torch.zeros(0, dtype=torch.long)
        inst.gt_boxes3d = Boxes3D(torch.zeros((0, 4)), torch.zeros((0, 2)), torch.zeros((0, 1)), torch.zeros((0, 3)), torch.zeros((0, 3, 3)))
        return inst

    none = GC.Case(case.model, case.maps, [empty(), empty()], case.level_hw, case.inv_K)
    got = run_seam(none)
    assert got["num_pos"] == 0
    check_against_oracle(none, got["grads"], what="nopos")
    for fam in GO.families(none.p):
        m = float(GO.flat_family(got["grads"], fam, none.p).abs().max())
        assert (m > 0.0) if fam == "logits" else (m == 0.0), fam
    one = GC.Case(case.model, case.maps, [case.gt[0], empty()], case.level_hw, case.inv_K)
    got = run_seam(one)
    assert got["num_pos"] > 0
    check_against_oracle(one, got["grads"], what="one-empty")
    second = one.targets["im_inds"] == 1
    for fam in GO.families(one.p):
        if fam != "logits":
            assert float(GO.flat_family(got["grads"], fam, one.p)[second].abs().max()) == 0.0, fam


def _model(exp, weights, overrides=None):
    from dd3d_amd.synthetic import load_calib, make_state_dict
    m = GC.cpu_model(exp, overrides)
    m.load_state_dict(make_state_dict(m, calib=load_calib(weights)))
    return m.to("cuda").eval()


@pytest.mark.parametrize("exp,weights,B,H,W,ds", [("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti"),
                                                   ("dd3d_nusc_dla34", "dla34_nusc", 6, 128, 224, "nusc")])
def test_compute_losses_head_grads_end_to_end_and_determinism(hiplib, exp, weights, B, H, W, ds):
    _end_to_end(exp, weights, B, H, W, ds)


def test_compute_losses_head_grads_end_to_end_away_from_the_released_settings(hiplib):
    """The captured graph carries non-default settings: the powf branch without alpha, beta 0.5, temperature 3 and other weights."""
    over = GC.merged(GC.SETTINGS["gamma1.5_alpha_off"], GC.SETTINGS["beta0.5_T3_weights"])
    _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti", over)


def _end_to_end(exp, weights, B, H, W, ds, overrides=None):
    from dd3d_amd.synthetic import make_gt_instances, make_inputs
    from tests.test_losses_gpu import _maps_nchw
    model = _model(exp, weights, overrides)
    nusc = hasattr(model, "attr_logits")
    inputs = make_inputs(B, H, W, dataset=ds)
    gt = make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES,
                           num_attributes=model.attr_logits.out_channels if nusc else None, empty_images=(1, ))
    for x, g in zip(inputs, gt):
        x["instances"] = g
    plain = model.compute_losses(inputs)
    losses, grads = model.compute_losses(inputs, head_grads=True)
    assert list(losses) == list(plain) and all(torch.equal(losses[k], plain[k]) for k in plain)  # the default path's values, bit for bit
    plan = model.get_loss_plan(*model.canvas_size(inputs), grads=True)
    assert [op.name for op in plan.ops][-2:] == ["loss_terms", "loss_backward"]
    assert int(plan.grad_denoms.cpu().view(torch.int32)[3]) == 0
    case = GC.Case(GC.cpu_model(exp, overrides), _maps_nchw(plan), gt, [(f.H, f.W) for f in plan.features], plan.inv_K.view(-1, 3, 3).cpu())
    assert int(case.kink.sum()) <= GC.KINK_CAP * case.num_pos and case.num_pos > 20
    check_against_oracle(case, {k: v.cpu() for k, v in grads.items()}, what="e2e:" + ds + (":settings" if overrides else ""))
    if overrides:  # the settings reached the loss values as well
        from tests.test_losses_gpu import _close
        _close({k: v.cpu() for k, v in losses.items()}, case.losses(), 5e-6)
        assert (case.p["gamma"], case.p["alpha"], case.p["beta"], case.p["temperature"]) == (1.5, -1.0, 0.5, 3.0)
    # two calls agree bit for bit; the captured graph equals launch-by-launch execution
    _, again = model.compute_losses(inputs, head_grads=True)
    assert all(torch.equal(again[k], grads[k]) for k in grads)
    model.use_graph = False
    model.invalidate_plans()
    l2, eager = model.compute_losses(inputs, head_grads=True)
    assert all(torch.equal(eager[k], grads[k]) for k in grads) and all(torch.equal(l2[k], plain[k]) for k in plain)


# ---------------------------------------------------------------------------------------------- away from the released settings
@pytest.mark.parametrize("name,key", GC.SETTINGS_ROWS)
def test_backward_at_seam_away_from_the_released_settings(hiplib, name, key):
    case = GC.settings_case(name, key)
    got = run_seam(case)
    assert got["num_pos"] == case.num_pos > 20 and int(case.kink.sum()) <= GC.KINK_CAP * case.num_pos and got["renorm"] == 0
    assert got["primal_mismatch"] == 0
    check_against_oracle(case, got["grads"], what=f"{name}:{key}")


@pytest.mark.parametrize("gamma", GC.SATURATED_GAMMAS)
@pytest.mark.parametrize("H,W", [(4, 4), (1, 257)])
def test_backward_on_saturated_logits(hiplib, H, W, gamma):
    """Logits of +-60 (1 - p_t exactly 0 or 1 in float32) on positives and on whole background rows: every gradient word finite and
    within the bar.  At gamma 0 the derivative of m^0 is 0, as torch's pow gives it, not 0 * 0^-1."""
    case = GC.handmade_case(H, W, gamma=gamma)
    got = run_seam(case)
    assert got["num_pos"] == len(case.specs) == case.num_pos and got["primal_mismatch"] == 0
    assert all(bool(torch.isfinite(v).all()) for v in got["grads"].values())
    check_against_oracle(case, got["grads"], what=f"saturated{H}x{W}:gamma{gamma}")
    lg, g64 = GO.flat_family(got["grads"], "logits", case.p), GO.flat_family(case.ref(), "logits", case.p)
    sat = LO.flat(case.maps, "logits", 1, case.p["num_classes"]).abs() == 60.0
    assert int(sat.sum()) == 3 + 2 * case.p["num_classes"]
    # the confidently wrong logits carry a gradient of the order of 1 / num_pos, the confidently right ones next to none
    assert float(lg[sat].abs().max()) > 0.1 and float(g64[sat].abs().max()) > 0.1 and float(lg[sat].abs().min()) <= 1e-20


@pytest.mark.parametrize("name", GC.POISONED_CASES)
def test_backward_on_the_renormalised_path(hiplib, name):
    """The batch-wide renormalisation of the allocentric decode (geometry.py:48-53; loss_assign_kernel's flags word, the `*flags`
    branch of loss_common.h::decoded_quat on floats in the forward and on dual numbers here), reached with finite numbers: one
    positive's quaternion is all zeros (loss_grad_cases.poisoned_case), that box decodes to NaN and sets the trigger, and every other
    positive of the batch is divided by its clamped norm.

    Proves: the trigger fires (flags 1; 0 on the clean case) and is batch-wide; the float and the dual instantiation agree bit for bit
    under it (primal_mismatch 0, NaN counted equal to NaN); the poisoned target's rows are NaN exactly where the float64 autograd's
    are (quat, ctr, conf), and every other row is finite and within the usual bar of the float64 autograd, which takes its own
    renormalisation branch (allclose on a NaN norm is false).
    Does not prove: that the derivative of the division is right in detail.  A proper rotation's quaternion has norm 1 whatever the
    inputs, so dividing by the norm moves the float64 gradient by about 1e-17 of its size (measured on the CPU); a subtly wrong
    derivative of that division cannot be told from a correct one here."""
    case, clean = GC.poisoned_case(name), GC.golden_case(name)
    got = run_seam(case)
    assert got["renorm"] == 1 and got["num_pos"] == case.num_pos and got["primal_mismatch"] == 0
    n = int(case.targets["pos_inds"][case.poisoned])
    nan_fams = {fam for fam in GO.families(case.p) if bool(torch.isnan(GO.flat_family(got["grads"], fam, case.p)[n]).any())}
    assert nan_fams == {"quat", "ctr", "conf"}
    check_against_oracle(case, got["grads"], what="poisoned:" + name, nan_row=n)
    assert run_seam(clean, backward=False)["renorm"] == 0


def test_poisoned_quaternion_leaves_the_egocentric_flag_clear(hiplib):
    """Without PREDICT_ALLOCENTRIC_ROT there is no renormalisation: the same poison (class-agnostic: channel 0) makes its own box NaN
    and leaves the flags word at 0."""
    name = "dla34_kitti_variant_egocentric_agnostic"
    case = GC.poisoned_case(name)
    got = run_seam(case)
    assert got["renorm"] == 0 and got["primal_mismatch"] == 0
    n = int(case.targets["pos_inds"][case.poisoned])
    assert bool(torch.isnan(GO.flat_family(got["grads"], "quat", case.p)[n]).all())
    check_against_oracle(case, got["grads"], what="poisoned:" + name, nan_row=n)


def test_seam_determinism(hiplib, seam_runs):
    name = "dla34_kitti_128x384_b2_ragged"
    a, b = seam_runs(name), run_seam(GC.golden_case(name))
    assert all(torch.equal(a["grads"][k], b["grads"][k]) for k in a["grads"])


def test_fused_loss_autograd(hiplib, seam_runs):
    from dd3d_amd.losses import FusedDD3DLoss
    name = "dla34_nusc_128x224_b6"
    case = GC.golden_case(name)
    model = case.model
    w = (torch.rand(10, generator=torch.Generator().manual_seed(5)) + 0.5).tolist()
    seam = run_seam(case, upstream=w)
    leaf = {k: v.cuda().requires_grad_(True) for k, v in case.maps.items()}
    out = FusedDD3DLoss(model)(leaf, case.inv_K.cuda(), case.gt)
    assert list(out) == list(seam["losses"]) and all(torch.equal(out[k].detach().cpu(), seam["losses"][k]) for k in out)
    assert all(v.dim() == 0 and v.requires_grad for v in out.values())
    sum(w[GO.OUT_INDEX[k]] * v for k, v in out.items()).backward()
    for k, v in leaf.items():
        assert torch.equal(v.grad.cpu(), seam["grads"][k]), k  # the same kernel on the same bytes
    # through further torch ops: maps = relu(raw * s) -- the gradient reaches raw and s
    raw = {k: v.cuda().requires_grad_(True) for k, v in case.maps.items()}
    s = torch.tensor(1.0, device="cuda", requires_grad=True)
    maps = {k: (torch.relu(v * s) if k.startswith("box2d_reg") else v * s) for k, v in raw.items()}
    total = sum(FusedDD3DLoss(model)(maps, case.inv_K.cuda(), case.gt).values())
    total.backward()
    ones = run_seam(case)["grads"]
    for k, v in raw.items():  # s == 1 and the committed box2d_reg maps are post-ReLU: d total / d raw = the seam's gradient where raw > 0
        ref = ones[k] * (case.maps[k] > 0) if k.startswith("box2d_reg") else ones[k]
        assert torch.equal(v.grad.cpu(), ref), k
    ds = sum(float((ones[k].double() * case.maps[k].double()).sum()) for k in ones)
    assert abs(float(s.grad) - ds) <= 1e-4 * abs(ds) and ds != 0.0
