"""FPN backward on the MI355X (csrc/fpn_grads.hip, engine.LossPlan(fpn_grads=True)): dd3d_fpn_wgrad and dd3d_fpn_dgrad at their C-ABI
seam on seeded convolutions of the FPN family (tests/fpn_grad_cases.py) against the float64 oracle (tests/fpn_grad_oracle.py) -- stride-2
3x3 (P6 / P7: input ReLU, mask, add), stride-1 3x3 with a filter per level and the pool add, 1x1 laterals up to Cin 1024 in the three
storages -- sentinel-framed outputs, poisoned pads, every case twice with equal bits; the transposed top-down sum bit for bit; a mini
pyramid through engine.losses.fpn_backward; rejected arguments; the slice count; DD3D.compute_losses(fpn_grads=True) end to end.

The bar of a family (filter, bias / q, norm weight / r, input gradient) in a case is 8 * max(d32, 2^-23 * max|g64|): d32 is the deviation
of the oracle's float32 run from its float64 run on the same case, computed here on the CPU (loss_grad_oracle.bar).
"""
import ctypes as C

import pytest
import torch

from tests import fpn_grad_cases as FC
from tests import fpn_grad_oracle as FO
from tests import loss_grad_cases as GC

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
POISON = 3.0e30  # pad words of the inputs: a kernel that read them would not stay finite


def nhwc(x, pitch, pad=POISON):
    B, C_, H, W = x.shape
    t = torch.full((B, H, W, pitch), pad, dtype=torch.float32)
    t[..., :C_] = x.permute(0, 2, 3, 1)
    return t.contiguous().cuda()


def store(tensors, storage, plane_scale=1.0, pad=4):
    """Per-level NCHW float32 -> (device buffers, bindings (mode, address, pitch, plane scale), the float32 values the storage decodes to)."""
    from dd3d_amd import hip
    C_ = tensors[0].shape[1]
    if storage == "f32":
        bufs = [nhwc(a, C_ + pad) for a in tensors]
        return bufs, [(hip.PG_ACT_F32, b.data_ptr(), C_ + pad, 1.0) for b in bufs], list(tensors)
    enc = [FC.encode_f16x2(a, plane_scale) if storage == "f16x2" else FC.encode_bf16x3(a) for a in tensors]
    bufs = [p.cuda() for p, _ in enc]
    mode = hip.PG_ACT_F16X2 if storage == "f16x2" else hip.PG_ACT_BF16X3
    return bufs, [(mode, b.data_ptr(), 0, float(plane_scale)) for b in bufs], [d for _, d in enc]


def run_seam(case, storage="f32", plane_scale=1.0, mask_storage=None, mask_scale=16.0, dgrad_rows=0, fill=SENTINEL, add=True, pool=True):
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import FpnConvGrads
    xb, xbind, xdec = store(case.x, storage, plane_scale)
    mb, mbind, mdec = store(case.mask, mask_storage or storage, mask_scale if mask_storage else plane_scale) if case.mask is not None else (None, None, None)
    gpitch = case.Cout + 4
    g = [nhwc(v, gpitch) for v in case.g]
    w = [v.permute(0, 2, 3, 1).contiguous().cuda() for v in case.w]
    scale = [s.contiguous().cuda() for s in case.scale]
    addt = [nhwc(v, case.Cin) for v in case.add] if (case.add is not None and add) else None
    lay = FpnConvGrads("cuda", case.B, case.in_hw, case.Cin, case.Cout, case.ksize, case.stride, xbind, g, gpitch, w, scale, mask=mbind, add=addt,
                       pool=([None] + ["prev"] * (case.L - 1)) if (case.chain and pool) else None, in_relu=case.in_relu, fill=fill, guard=64,
                       dgrad_rows=dgrad_rows)
    lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    lay.keep_alive = (xb, mb)
    return collect(lay), lay, xdec, mdec


def collect(lay):
    nchw_w = lambda t: t.view(lay.Cout, lay.ksize, lay.ksize, lay.Cin).permute(0, 3, 1, 2).cpu()
    return [{"dw_level": nchw_w(lay.dw_level[l]), "dw": nchw_w(lay.dw[l]), "q": lay.q[l].cpu(), "r": lay.r[l].cpu(), "da": lay.da[l].permute(0, 3, 1, 2).cpu()}
            for l in range(lay.L)]


WORST = {}


def check(got, ref64, ref32, what, families=("filter", "bias", "norm_weight", "input")):
    a, b, k = FO.family_vectors(ref64), FO.family_vectors(ref32), FO.family_vectors(got)
    for fam in families:
        assert bool(torch.isfinite(k[fam]).all()), (what, fam)
        bar, d32, gmax = FO.bar(a[fam], b[fam], torch.ones(a[fam].shape[0], dtype=torch.bool))
        dev = float((k[fam].double() - a[fam]).abs().max())
        use = 8 * dev / bar if bar > 0 else 0.0
        WORST[fam] = max(WORST.get(fam, 0.0), use)
        print(f"[fpn_grads] {what} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8; "
              f"worst so far {WORST[fam]:.2f})")
        assert dev <= bar, (what, fam, dev, bar, d32, gmax)


def frame_ok(lay, fill=SENTINEL):
    """Guard words keep the sentinel; every output word is written (the scratch rows in use included)."""
    assert lay.guards_intact(fill)
    for t in [lay.part, lay.qpart, lay.dw_level, lay.dw, lay.q, lay.r] + lay.da:
        assert not bool((t == fill).any())


def same_bits(a, b):
    va, vb = FO.family_vectors(a), FO.family_vectors(b)
    return all(torch.equal(va[f], vb[f]) for f in va)


# stride-2 3x3 (the top block): 1x1 and 2x2 -> 1x1 (one output pixel; in 2x2 only parity-matched taps land), 3x5 -> 2x3 and 5x7 -> 3x4
# (odd sizes: the ceil output), 12x40 -> 6x20 with B = 2 (several tiles); with and without the input ReLU, mask and add.
# stride-1 3x3, a filter per level: 1x1, 1x257 (five units, the last one pixel long), 6x20 + 3x10 chained through the pool add, 30x70.
# 1x1 laterals: Cin 32 .. 1024 (four blocks of 256 input channels in the input gradient), Cout 32 and 256, 1 / 63 / 65 pixels (around a
# unit) and 30x70, the three storages.
SEAM_CASES = {
    "s2_1x1_plain": (dict(in_hw=[(1, 1)], B=1, Cin=32, Cout=32, ksize=3, stride=2, seed=1), dict()),
    "s2_2x2_relu_mask_add": (dict(in_hw=[(2, 2)], B=1, Cin=32, Cout=32, ksize=3, stride=2, seed=2, in_relu=True, with_mask=True, with_add=True), dict()),
    "s2_3x5_relu_mask_add_f16": (dict(in_hw=[(3, 5)], B=2, Cin=64, Cout=64, ksize=3, stride=2, seed=3, in_relu=True, with_mask=True, with_add=True),
                                 dict(storage="f16x2", plane_scale=16.0)),
    "s2_5x7_add_bf16x3": (dict(in_hw=[(5, 7)], B=2, Cin=64, Cout=32, ksize=3, stride=2, seed=4, with_add=True), dict(storage="bf16x3")),
    "s2_5x7_plain": (dict(in_hw=[(5, 7)], B=1, Cin=32, Cout=64, ksize=3, stride=2, seed=5), dict()),
    "s2_12x40_b2_relu_mask_add_x_f32_mask_f16": (dict(in_hw=[(12, 40)], B=2, Cin=64, Cout=64, ksize=3, stride=2, seed=6, in_relu=True, with_mask=True,
                                                      with_add=True), dict(storage="f32", mask_storage="f16x2", mask_scale=16.0, dgrad_rows=4)),
    "s2_12x40_b2_plain_f16s1": (dict(in_hw=[(12, 40)], B=2, Cin=32, Cout=32, ksize=3, stride=2, seed=7), dict(storage="f16x2", plane_scale=1.0)),
    "s1_1x1": (dict(in_hw=[(1, 1)], B=1, Cin=32, Cout=32, ksize=3, stride=1, seed=11), dict()),
    "s1_1x257_f16": (dict(in_hw=[(1, 257)], B=1, Cin=64, Cout=64, ksize=3, stride=1, seed=12), dict(storage="f16x2", plane_scale=16.0)),
    "s1_6x20_3x10_chain": (dict(in_hw=[(6, 20), (3, 10)], B=2, Cin=64, Cout=64, ksize=3, stride=1, seed=13, chain=True), dict(dgrad_rows=2)),
    "s1_30x70_bf16x3": (dict(in_hw=[(30, 70)], B=1, Cin=32, Cout=32, ksize=3, stride=1, seed=14), dict(storage="bf16x3", dgrad_rows=8)),
    "lat_c32_o32_1px": (dict(in_hw=[(1, 1)], B=1, Cin=32, Cout=32, ksize=1, stride=1, seed=21), dict()),
    "lat_c128_o256_63px_f16s16": (dict(in_hw=[(1, 63)], B=1, Cin=128, Cout=256, ksize=1, stride=1, seed=22), dict(storage="f16x2", plane_scale=16.0)),
    "lat_c512_o32_65px_f16s1": (dict(in_hw=[(1, 65)], B=2, Cin=512, Cout=32, ksize=1, stride=1, seed=23), dict(storage="f16x2", plane_scale=1.0)),
    "lat_c1024_o256_65px_bf16x3": (dict(in_hw=[(5, 13)], B=1, Cin=1024, Cout=256, ksize=1, stride=1, seed=24), dict(storage="bf16x3")),
    "lat_c128_o256_30x70_f32": (dict(in_hw=[(30, 70)], B=1, Cin=128, Cout=256, ksize=1, stride=1, seed=25), dict(dgrad_rows=4)),
    "lat_zero_scale_stage": (dict(in_hw=[(3, 10), (5, 7)], B=2, Cin=64, Cout=32, ksize=1, stride=1, seed=26, zero_scale_level=1), dict()),
}


@pytest.mark.parametrize("name", list(SEAM_CASES))
def test_seam_against_oracle(hiplib, name):
    kw, run = SEAM_CASES[name]
    case = FC.ConvCase(**kw)
    got, lay, xdec, mdec = run_seam(case, **run)
    frame_ok(lay)
    check(got, case.ref(torch.float64, xdec, mdec), case.ref(torch.float32, xdec, mdec), name)
    again, _, _, _ = run_seam(case, **run)
    assert same_bits(again, got), name  # the same call twice: the same bits
    if kw.get("zero_scale_level") is not None:
        l = kw["zero_scale_level"]
        assert float(got[l]["da"].abs().max()) == 0.0 and float(got[l]["dw"].abs().max()) == 0.0 and float(got[l]["r"].abs().max()) > 0.0


def test_all_negative_p6_masks_to_exact_zeros_and_leaves_g6_alone(hiplib):
    case = FC.ConvCase(in_hw=[(3, 5)], B=2, Cin=32, Cout=32, ksize=3, stride=2, seed=31, in_relu=True, with_mask=True, with_add=True, negative_mask=True)
    case.x = [m.clone() for m in case.mask]  # P7: its input IS the stored p6
    got, lay, _, _ = run_seam(case)
    frame_ok(lay)
    assert torch.equal(got[0]["da"], case.add[0])  # D6 = G6 + 0, bit for bit
    assert float(got[0]["dw"].abs().max()) == 0.0 and float(got[0]["r"].abs().max()) == 0.0  # relu(p6) = 0: no filter gradient
    assert float(got[0]["q"].abs().max()) > 0.0  # the bias still sees G7
    without, _, _, _ = run_seam(case, add=False)
    assert float(without[0]["da"].abs().max()) == 0.0


def test_tile_choice_and_previous_contents_do_not_change_the_bits(hiplib):
    case = FC.ConvCase(in_hw=[(12, 40)], B=2, Cin=32, Cout=32, ksize=3, stride=2, seed=33, with_add=True)
    auto, _, _, _ = run_seam(case)
    for rows in (2, 4, 8):
        forced, lay, _, _ = run_seam(case, dgrad_rows=rows, fill=7.5)
        frame_ok(lay, 7.5)
        assert same_bits(forced, auto), rows


@pytest.mark.parametrize("hw", [(1, 1), (3, 5)])
def test_transposed_top_down_is_bit_exact(hiplib, hw):
    """T_coarse = dgrad + pool2x2sum(T_fine): ((((v + t00) + t01) + t10) + t11), one float32 rounding per add, in this order."""
    fine = (2 * hw[0], 2 * hw[1])
    case = FC.ConvCase(in_hw=[fine, hw], B=2, Cin=32, Cout=32, ksize=1, stride=1, seed=41, chain=True)
    with_pool, lay, _, _ = run_seam(case)
    frame_ok(lay)
    without, _, _, _ = run_seam(case, pool=False)
    assert torch.equal(with_pool[0]["da"], without[0]["da"])
    assert torch.equal(with_pool[1]["da"], FO.pool2x2sum(without[1]["da"], with_pool[0]["da"]))


def _mini_chain(model, feats, G, stored, fill=SENTINEL):
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import fpn_backward, fpn_param_grads
    fpn = model.backbone
    B = next(iter(feats.values())).shape[0]
    keep, acts = [], {}
    tensors = dict(feats)
    tensors.update({f"t{s}": v for s, v in stored["t"].items()})
    tensors.update({f"p{s}": v for s, v in stored["p"].items()})
    for k, v in tensors.items():
        bufs, bind, _ = store([v], "f32")
        keep.append(bufs)
        acts[k] = (bind[0], v.shape[2], v.shape[3], v.shape[1])
    Gd = {k: nhwc(v, v.shape[1]) for k, v in G.items()}
    layers, backbone = fpn_backward("cuda", B, fpn, Gd, acts, lambda t: t.detach().float().contiguous().cuda(), fill=fill, guard=64)
    for lay in layers.values():
        lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    for lay in layers.values():
        frame_ok(lay, fill)
    params = {k: v.cpu() for k, v in fpn_param_grads({id(p): k for k, p in model.named_parameters()}, layers).items()}
    fg = {f"backbone_{n}": d[..., :c].permute(0, 3, 1, 2).cpu() for n, (d, c) in backbone.items()}
    return params, fg, layers, keep


def check_named(params, fg, ref64, ref32, what):
    fams = {}
    for k in sorted(params):
        fams.setdefault(FO.family_of(k), []).append(k)
    rows = [(fam, [params[k] for k in ks], [ref64[0][k] for k in ks], [ref32[0][k] for k in ks]) for fam, ks in fams.items()]
    rows.append(("input", [fg[k] for k in sorted(fg)], [ref64[1][k] for k in sorted(fg)], [ref32[1][k] for k in sorted(fg)]))
    for fam, c, a, b in rows:
        c, a, b = (torch.cat([v.reshape(-1).cpu() for v in vs]) for vs in (c, a, b))
        bar, d32, gmax = FO.bar(a.double(), b, torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((c.double() - a.double()).abs().max())
        use = 8 * dev / bar if bar > 0 else 0.0
        WORST[fam] = max(WORST.get(fam, 0.0), use)
        print(f"[fpn_grads] {what} named {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8; "
              f"worst so far {WORST[fam]:.2f})")
        assert dev <= bar and gmax > 0.0, (what, fam, dev, bar)


@pytest.mark.parametrize("norm,top", [("BN", "p6p7"), ("", "p6")])
def test_mini_pyramid_chain(hiplib, norm, top):
    """t3 12x20, t4 6x10, t5 3x5, p6 2x3, p7 1x2, 64 channels, B = 2: the whole chain through engine.losses.fpn_backward."""
    model = FC.MiniModel(norm=norm, top=top)
    feats, G, sd = FC.mini_inputs(model, 2, (12, 20))
    stored = FO.stored_activations(sd, feats, FO.spec(model))
    params, fg, _, _ = _mini_chain(model, feats, G, stored)
    assert sorted(params) == FO.fpn_param_names(model) and all(params[k].shape == p.shape for k, p in model.named_parameters())
    r64, r32 = FO.chain_grads(model, stored, feats, G, torch.float64), FO.chain_grads(model, stored, feats, G, torch.float32)
    check_named(params, fg, r64, r32, f"mini:{norm or 'none'}:{top}")
    again, fg2, _, _ = _mini_chain(model, feats, G, stored, fill=7.5)
    assert all(torch.equal(again[k], params[k]) for k in params) and all(torch.equal(fg2[k], fg[k]) for k in fg)


def test_bad_arguments_are_rejected(hiplib):
    from dd3d_amd import hip
    case = FC.ConvCase(in_hw=[(6, 20), (3, 10)], B=1, Cin=32, Cout=32, ksize=3, stride=1, seed=51, chain=True, with_mask=True, with_add=True)
    _, lay, _, _ = run_seam(case)
    lib, st = hip.lib(), hip.current_stream()
    a = lay.args
    both = (("dd3d_fpn_wgrad", lib.dd3d_fpn_wgrad), ("dd3d_fpn_dgrad", lib.dd3d_fpn_dgrad))
    for field, value, entries in (("Cin", 48, both), ("Cin", 1056, both), ("Cout", 16, both), ("Cout", 288, both), ("stride", 3, both), ("stride", 0, both),
                                  ("ksize", 2, both), ("ksize", 5, both), ("g_pitch", 34, both), ("g_pitch", 28, both), ("x_pitch", 34, both[:1]),
                                  ("x_pitch", 28, both[:1]), ("mask_pitch", 28, both[1:]), ("x_mode", 7, both[:1]), ("mask_mode", 7, both[1:]),
                                  ("n_slices", 0, both[:1]), ("dgrad_rows", 3, both), ("num_levels", 0, both), ("B", 0, both)):
        old = getattr(a, field)
        setattr(a, field, value)
        for name, fn in entries:
            assert fn(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(name), (field, name)
        setattr(a, field, old)
    for field, entries in (("g", both), ("w", both), ("scale", both), ("x", both[:1]), ("da", both[1:])):
        arr = getattr(a, field)
        old = arr[0]
        arr[0] = None
        for name, fn in entries:
            assert fn(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(name), (field, name)
        arr[0] = old
    for field in ("part", "qpart", "dw_level", "dw", "q", "r"):
        old = getattr(a, field)
        setattr(a, field, None)
        assert lib.dd3d_fpn_wgrad(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_fpn_wgrad"), field
        setattr(a, field, old)
    a.pool_H[1] += 1  # non-halving levels for the pool add
    assert lib.dd3d_fpn_dgrad(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_fpn_dgrad")
    a.pool_H[1] -= 1
    a.H[1] += 1
    assert lib.dd3d_fpn_dgrad(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_fpn_dgrad")
    a.H[1] -= 1
    assert lib.dd3d_fpn_grad_slices(None) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_fpn_grad_slices")
    assert lib.dd3d_fpn_wgrad(None, st) == -1 and lib.dd3d_fpn_dgrad(None, st) == -1
    assert lib.dd3d_fpn_wgrad(C.byref(a), st) == 0 and lib.dd3d_fpn_dgrad(C.byref(a), st) == 0  # the restored arguments still run
    torch.cuda.synchronize()
    frame_ok(lay)


def test_slice_count_is_a_pure_shape_query(hiplib):
    from dd3d_amd import hip
    bare = hip.FpnGradArgs()  # the geometry, the channel counts and the convolution's form alone: no pointer is set
    for (B, hw, ci, co, k, s) in ((1, [(1, 1)], 32, 32, 3, 2), (2, [(12, 40)], 64, 64, 3, 2), (1, [(30, 70)], 128, 256, 1, 1), (1, [(1, 257)], 64, 64, 3, 1),
                                  (2, [(48, 160), (24, 80), (12, 40)], 256, 256, 3, 1), (6, [(112, 200)], 1024, 256, 1, 1), (3, [(100, 64)], 256, 256, 3, 1)):
        bare.num_levels, bare.B, bare.Cin, bare.Cout, bare.ksize, bare.stride = len(hw), B, ci, co, k, s
        for l, (h, w) in enumerate(hw):
            bare.H[l], bare.W[l] = h, w
        assert hiplib.dd3d_fpn_grad_slices(C.byref(bare)) == hip.fpn_grad_slices(B, hw, ci, co, k, s), (B, hw, ci, co, k, s)
    assert hip.fpn_grad_slices(1, [(1, 1)], 32, 32, 3, 2) == 1 and hip.fpn_grad_slices(1, [(30, 70)], 128, 256, 1, 1) == 15
    assert hip.fpn_grad_slices(2, [(12, 40)], 64, 64, 3, 2) == 3  # 2 x 6 rows of 20 output pixels: 12 units of 32, four per slice
    assert hip.fpn_grad_slices(3, [(100, 64)], 256, 256, 3, 1) == 60  # the slab's byte budget decides: five units per slice
    bare.ksize = 2
    assert hiplib.dd3d_fpn_grad_slices(C.byref(bare)) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_fpn_grad_slices")


# ---------------------------------------------------------------------------------------------------------------------- end to end
def _plan_tensors(model, plan):
    fpn = model.backbone
    nchw = lambda v: v.nchw().float().cpu().contiguous()
    feats = {n: nchw(plan.bottom_up[n])[:, :fpn.bottom_up.output_shape()[n].channels] for n in fpn.in_features}
    stored = {"t": {s: nchw(plan.bufs[f"fpn_lateral{s}"].view()) for s in fpn.stages}, "p": {}}
    top = 0 if fpn.top_block is None else fpn.top_block.num_levels
    for i in range(top + 1):
        stored["p"][fpn.stages[-1] + i] = nchw(plan.bufs[f"p{fpn.stages[-1] + i}"].view())
    return feats, stored


def _end_to_end(exp, weights, B, H, W, ds, math=None, act_scale=None, empty=(1, )):
    from dd3d_amd.synthetic import make_gt_instances, make_inputs
    from tests.test_loss_grads_gpu import _model
    model = _model(exp, weights)
    model.math, model.act_scale = math, act_scale
    nusc = hasattr(model, "attr_logits")
    inputs = make_inputs(B, H, W, dataset=ds)
    gt = make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES,
                           num_attributes=model.attr_logits.out_channels if nusc else None, empty_images=empty)
    for x, g in zip(inputs, gt):
        x["instances"] = g
    ref_losses, ref_grads, ref_params = model.compute_losses(inputs, tower_grads=True)
    losses, grads, params = model.compute_losses(inputs, fpn_grads=True)
    # the loss dict and everything the tower backward returns are those of tower_grads=True, bit for bit
    assert list(losses) == list(ref_losses) and all(torch.equal(losses[k], ref_losses[k]) for k in losses)
    assert all(torch.equal(grads[k], ref_grads[k]) for k in ref_grads) and all(torch.equal(params[k], ref_params[k]) for k in ref_params)
    plan = model.get_loss_plan(*model.canvas_size(inputs), fpn_grads=True)
    fpn = model.backbone
    cpu = GC.cpu_model(exp)
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    shapes = fpn.bottom_up.output_shape()
    new_g, new_p = {k: v for k, v in grads.items() if k not in ref_grads}, {k: v.cpu() for k, v in params.items() if k not in ref_params}
    assert sorted(new_g) == sorted(f"backbone_{n}" for n in fpn.in_features) and sorted(new_p) == FO.fpn_param_names(cpu)
    assert all(new_g[f"backbone_{n}"].shape == (B, shapes[n].channels, plan.bottom_up[n].H, plan.bottom_up[n].W) and new_g[f"backbone_{n}"].dtype == torch.float32
               for n in fpn.in_features)
    named = dict(cpu.named_parameters())
    assert all(v.shape == named[k].shape and v.dtype == torch.float32 for k, v in new_p.items())
    feats, stored = _plan_tensors(model, plan)
    sel = list(model.in_features)
    G = {n: grads[f"feature{sel.index(n)}"].cpu() for n in fpn._out_features if n in sel}
    # every layer: the raw outputs against the layer oracle fed the plan's own stored input and the gradient the layer itself read
    for key, lay in plan.fpn_layers.items():
        assert lay.guards_intact(0.0)
        g, w, scale, add, pool, _ = lay.keep
        xs = {"top_block.p7": [stored["p"].get(fpn.stages[-1] + 1)], "top_block.p6": [stored["p"][fpn.stages[-1]]],
              "outputs": [stored["t"][s] for s in fpn.stages]}.get(key) or [feats[fpn.in_features[fpn.stages.index(int(key[7:]))]]]
        ref = {}
        for dtype in (torch.float64, torch.float32):
            res = []
            for l in range(lay.L):
                res.append(FO.layer_grads(xs[l], g[l].permute(0, 3, 1, 2).cpu(), w[l].permute(0, 3, 1, 2).cpu(), scale[l].cpu(), lay.stride, dtype,
                                          in_relu=key == "top_block.p7", mask=xs[l] if key == "top_block.p7" else None,
                                          add=add[l].permute(0, 3, 1, 2).cpu() if add is not None and add[l] is not None else None,
                                          pool=res[l - 1]["da"] if (pool is not None and pool[l] is not None) else None))
            ref[dtype] = res
        check(collect(lay), ref[torch.float64], ref[torch.float32], f"e2e:{ds}:{key}")
    # the named parameters and the backbone-feature gradients against the chain oracle on the plan's stored activations
    r64, r32 = FO.chain_grads(cpu, stored, feats, G, torch.float64), FO.chain_grads(cpu, stored, feats, G, torch.float32)
    check_named(new_p, {k: v.cpu() for k, v in new_g.items()}, r64, r32, f"e2e:{ds}")
    # a second call is bit-equal; the captured graph equals launch-by-launch execution
    _, g2, p2 = model.compute_losses(inputs, fpn_grads=True)
    assert all(torch.equal(g2[k], grads[k]) for k in grads) and all(torch.equal(p2[k], params[k]) for k in params)
    names = [op.name for op in plan.ops]
    model.use_graph = False
    model.invalidate_plans()
    l3, g3, p3 = model.compute_losses(inputs, fpn_grads=True)
    assert all(torch.equal(l3[k], losses[k]) for k in losses)
    assert all(torch.equal(g3[k], grads[k]) for k in grads) and all(torch.equal(p3[k], params[k]) for k in params)
    return model, plan, names


def test_compute_losses_fpn_grads_kitti_dla34(hiplib):
    from dd3d_amd import hip
    model, plan, names = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti")
    assert names[-6:] == ["fpn_grads.top_block.p7", "fpn_grads.top_block.p6", "fpn_grads.outputs", "fpn_grads.lateral5", "fpn_grads.lateral4",
                          "fpn_grads.lateral3"] and names[-7] == "tower_grads.box3d.0"
    a = plan.fpn_layers["outputs"].args
    assert a.x_mode == hip.PG_ACT_F16X2 and a.x_plane_scale == 16.0 and plan.fpn_layers["top_block.p7"].args.mask_mode == hip.PG_ACT_F16X2


def test_compute_losses_fpn_grads_bf16x3(hiplib):
    from dd3d_amd import hip
    _, plan, _ = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti", math="bf16x3")
    assert plan.fpn_layers["lateral3"].args.x_mode == hip.PG_ACT_BF16X3


def test_compute_losses_fpn_grads_plane_scale_1(hiplib):
    _, plan, _ = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti", act_scale=1.0)
    assert plan.fpn_layers["outputs"].args.x_plane_scale == 1.0


def test_compute_losses_fpn_grads_nusc_dla34(hiplib):
    _end_to_end("dd3d_nusc_dla34", "dla34_nusc", 6, 128, 224, "nusc")


def test_compute_losses_fpn_grads_kitti_v99(hiplib):
    """LastLevelP6, four stages, the Cin 1024 lateral."""
    _, plan, names = _end_to_end("dd3d_kitti_v99", "v99_kitti", 1, 128, 256, "kitti", empty=())
    assert "fpn_grads.top_block.p7" not in names and names[-4:] == [f"fpn_grads.lateral{s}" for s in (5, 4, 3, 2)]
    assert plan.fpn_layers["lateral5"].Cin == 1024


def test_no_positives_gives_finite_results_and_exact_zeros(hiplib):
    from dd3d_amd.synthetic import make_gt_instances, make_inputs
    from tests.test_loss_grads_gpu import _model
    model = _model("dd3d_kitti_dla34", "dla34_kitti")
    inputs = make_inputs(2, 128, 384, dataset="kitti")
    for x, g in zip(inputs, make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, empty_images=(0, 1))):
        x["instances"] = g
    _, tg, tp = model.compute_losses(inputs, tower_grads=True)
    _, grads, params = model.compute_losses(inputs, fpn_grads=True)
    assert all(bool(torch.isfinite(v).all()) for v in list(grads.values()) + list(params.values()))
    assert all(torch.equal(grads[k], tg[k]) for k in tg) and all(torch.equal(params[k], tp[k]) for k in tp)
    if all(float(tg[f"feature{l}"].abs().max()) == 0.0 for l in range(5)):  # (the classification loss has a gradient without positives too)
        assert all(float(v.abs().max()) == 0.0 for k, v in grads.items() if k.startswith("backbone_"))


def test_reduced_modes_name_themselves(hiplib):
    from tests.test_loss_grads_gpu import _model
    model = _model("dd3d_kitti_dla34", "dla34_kitti")
    model.math = "bf16x2"
    with pytest.raises(NotImplementedError, match="bf16x2"):
        model.get_loss_plan(1, 128, 128, fpn_grads=True)
