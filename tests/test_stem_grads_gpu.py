"""DLA-34 stem backward on the MI355X (csrc/stem_grads.hip): dd3d_stem_wgrad and dd3d_stem_dgrad at their C-ABI seam on seeded
convolutions of the three stem shapes (tests/stem_grad_cases.py) against the float64 oracle (tests/stem_grad_oracle.py) -- several units,
slices and tiles with a partial last one in each direction, inputs smaller than a tile, odd sizes at stride 2, the three storages of the
stored output with poisoned neighbours, operands as channel slices of wider buffers, an all-zero gradient, wgrad_blocks, every rejected
argument; sentinel-framed outputs, every case twice with equal bits.  Then the fused stem's KEEP launch (dd3d_stem_fused_keep_f16x2)
at its seam, and DD3D.compute_losses(stem_grads=True) end to end on the whole-model cases (tests/whole_model_grad_oracle.py).

The bar of a family (filter, bias / q, norm weight / r, input gradient) in a case is 8 * max(d32, 2^-23 * max|g64|): d32 is the deviation
of the oracle's float32 run from its float64 run on the same case, computed here on the CPU (loss_grad_oracle.bar).

The weight gradient runs one wave per unit of up to 64 output pixels of a row, four pixels a step, slices of 8 to 64 units; the input
gradient runs one wave per 16 (stride 2: 32) input pixels of a row.
"""
import ctypes as C

import pytest
import torch

from tests import stem_grad_cases as SC
from tests import stem_grad_oracle as SO
from tests.predictor_grad_cases import encode_bf16x3, encode_f16x2

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
POISON = 3.0e30  # neighbour channels of the inputs: a kernel that read them would not stay finite
KEEP = 7.25      # what the words of a wider output buffer outside the slice hold before the call, and must hold after it


def wide(x, c0=0, tail=4, pad=POISON):
    """NCHW -> device [B, H, W, c0 + C + tail] with x in channels c0 .. c0 + C and `pad` elsewhere; returns (buffer, the slice view)."""
    B, C_, H, W = x.shape
    t = torch.full((B, H, W, c0 + C_ + tail), pad, dtype=torch.float32)
    t[..., c0:c0 + C_] = x.permute(0, 2, 3, 1)
    t = t.cuda()
    return t, t[..., c0:c0 + C_]


def store_y(y, storage, plane_scale=16.0, c0=0):
    """NCHW float32 stored output -> (device buffer, binding (mode, address, pitch, plane scale), the float32 values it decodes to).  Split
    planes hold 32 channels a chunk: the channels above Cout carry a positive value that would unmask what it must not, and a chunk of
    junk follows."""
    from dd3d_amd import hip
    if storage == "f32":
        buf, _ = wide(y, c0)
        return buf, (hip.PG_ACT_F32, buf.data_ptr() + 4 * c0, buf.shape[-1], 1.0), y
    cout = y.shape[1]
    padded = torch.cat([y, torch.full((y.shape[0], 32 - cout) + tuple(y.shape[2:]), 1000.0)], 1) if cout < 32 else y
    planes, dec = encode_f16x2(padded, plane_scale) if storage == "f16x2" else encode_bf16x3(padded)
    junk = torch.full((1, ) + tuple(planes.shape[1:]), 0x7BFF if storage == "f16x2" else 0x7F00, dtype=torch.int16)
    buf = torch.cat([planes, junk], 0).contiguous().cuda()
    return buf, (hip.PG_ACT_F16X2 if storage == "f16x2" else hip.PG_ACT_BF16X3, buf.data_ptr(), 0, float(plane_scale)), dec[:, :cout].contiguous()


def run_seam(case, y_storage="f32", x_c0=0, g_c0=0, da_c0=None, wgrad_blocks=0, fill=SENTINEL, g=None):
    """One stem convolution through StemConvGrads; the 7 x 7 runs the weight gradient alone.  `da_c0`: write the input gradient into
    channels da_c0 .. of a wider buffer."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import StemConvGrads
    xbuf, x = wide(case.x, x_c0)
    ybuf, ybind, ydec = store_y(case.y, y_storage)
    gbuf, gv = wide(case.g if g is None else g, g_c0)
    dgrad = case.ksize == 3
    dabuf = da = None
    if da_c0 is not None and dgrad:
        dabuf = torch.full((case.B, case.hw[0], case.hw[1], da_c0 + case.Cin + 8), KEEP, dtype=torch.float32, device="cuda")
        da = dabuf[..., da_c0:da_c0 + case.Cin]
    lay = StemConvGrads("cuda", case.B, case.hw[0], case.hw[1], case.Cin, case.Cout, case.ksize, case.stride, x, ybind, gv,
                        case.w.permute(0, 2, 3, 1).contiguous().cuda(), case.scale.contiguous().cuda(), da=da, fill=fill, guard=64,
                        wgrad_blocks=wgrad_blocks, dgrad=dgrad)
    lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    lay.keep_alive = (xbuf, ybuf, gbuf, dabuf)
    if dabuf is not None:  # the words outside the slice keep what they held
        outside = torch.ones(dabuf.shape[-1], dtype=torch.bool)
        outside[da_c0:da_c0 + case.Cin] = False
        assert bool((dabuf[..., outside.cuda()] == KEEP).all()) and not bool((da == KEEP).any())
    return collect(lay), lay, ydec


def collect(lay):
    nchw_w = lambda t: t.view(lay.Cout, lay.ksize, lay.ksize, lay.Cin).permute(0, 3, 1, 2).cpu()
    out = {"dw_level": nchw_w(lay.dw_level), "dw": nchw_w(lay.dw), "q": lay.q.cpu(), "r": lay.r.cpu()}
    if lay.da is not None:
        out["da"] = lay.da.permute(0, 3, 1, 2).cpu()
    return out


WORST = {}


def check(got, ref64, ref32, what):
    if "da" not in got:
        ref64, ref32 = ({k: v for k, v in r.items() if k != "da"} for r in (ref64, ref32))
    a, b, k = SO.family_vectors(ref64), SO.family_vectors(ref32), SO.family_vectors(got)
    for fam in a:
        if a[fam].numel() == 0:
            continue
        assert k[fam].numel() == a[fam].numel() and bool(torch.isfinite(k[fam]).all()), (what, fam)
        bar, d32, gmax = SO.bar(a[fam], b[fam], torch.ones(a[fam].shape[0], dtype=torch.bool))
        dev = float((k[fam].double() - a[fam]).abs().max())
        use = 8 * dev / bar if bar > 0 else 0.0
        WORST[fam] = max(WORST.get(fam, 0.0), use)
        print(f"[stem_grads] {what} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8; "
              f"worst so far {WORST[fam]:.2f})")
        assert gmax > 0.0 and dev <= bar, (what, fam, dev, bar, d32, gmax)


def frame_ok(lay, fill=SENTINEL, own_da=True):
    """Guard words keep the sentinel; every output word is written (the scratch rows in use included)."""
    assert lay.guards_intact(fill)
    n = lay.n_slices * lay.Cout
    for t in [lay.part.reshape(-1)[:n * lay.ksize**2 * lay.Cin], lay.qpart.reshape(-1)[:n], lay.dw_level, lay.dw, lay.q, lay.r] + (
            [lay.da] if own_da and lay.da is not None else []):
        assert not bool((t == fill).any())


def same_bits(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


def refs(case, ydec):
    return case.ref(torch.float64, y=ydec), case.ref(torch.float32, y=ydec)


# "big": four slices of the weight gradient (30 units of up to 64 output pixels, 8 a slice, the last slice 6; three units a row, the last
# 37 or 38 pixels long and its last four-pixel step partial), eleven tiles a row in the input gradient with a partial last one (5 of 16,
# 11 of 32 pixels); the stride-2 input is odd in both directions (9 x 331 -> 5 x 166): the last row and column have taps past the output.
# "tiny": smaller than a unit, a step and a tile in both directions.  "one": a single pixel, every tap but the centre in the padding.
SEAM_CASES = {
    "base_big": ("base_layer", dict(hw=(5, 165), B=2, seed=1)), "base_tiny": ("base_layer", dict(hw=(3, 5), B=1, seed=2)),
    "base_one": ("base_layer", dict(hw=(1, 1), B=1, seed=3)),
    "level0_big": ("level0.0", dict(hw=(5, 165), B=2, seed=4)), "level0_tiny": ("level0.0", dict(hw=(3, 5), B=1, seed=5)),
    "level0_one": ("level0.0", dict(hw=(1, 1), B=1, seed=6)),
    "level1_big_odd": ("level1.0", dict(hw=(9, 331), B=2, seed=7)), "level1_tiny_odd": ("level1.0", dict(hw=(3, 5), B=1, seed=8)),
    "level1_even": ("level1.0", dict(hw=(4, 66), B=1, seed=9)), "level1_2x2": ("level1.0", dict(hw=(2, 2), B=1, seed=10)),
    "level1_one": ("level1.0", dict(hw=(1, 1), B=1, seed=11)),
}
_CASES = {}


def seam_case(name):
    if name not in _CASES:
        layer, kw = SEAM_CASES[name]
        _CASES[name] = SC.stem_case(layer, **kw)
    return _CASES[name]


@pytest.mark.parametrize("name", list(SEAM_CASES))
def test_layer_at_the_seam(hiplib, name):
    """Against the float64 oracle at the bar; framed outputs; two runs with equal bits."""
    case = seam_case(name)
    got, lay, ydec = run_seam(case)
    frame_ok(lay)
    assert ("da" in got) == (case.ksize == 3)
    check(got, *refs(case, ydec), name)
    again, lay2, _ = run_seam(case)
    assert same_bits(got, again)
    if name.endswith("_big") or name == "level1_big_odd":
        assert lay.n_slices == 4


@pytest.mark.parametrize("storage", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("name", ["base_big", "level0_tiny", "level1_big_odd"])
def test_stored_output_as_split_planes(hiplib, name, storage):
    """The mask from f16x2 and bf16x3 planes: the channels above Cout of a chunk and the chunk behind it hold values that would unmask."""
    case = seam_case(name)
    got, lay, ydec = run_seam(case, y_storage=storage)
    frame_ok(lay)
    check(got, *refs(case, ydec), f"{name} {storage}")
    assert same_bits(got, run_seam(case, y_storage=storage)[0])
    if storage == "bf16x3":  # an exact split: the same masks as the f32 storage, so the same bits
        assert same_bits(got, run_seam(case)[0])


@pytest.mark.parametrize("name", ["base_big", "level0_big", "level1_big_odd"])
def test_operands_as_slices_of_wider_buffers(hiplib, name):
    """x, y, g and da at nonzero channel offsets of wider buffers with poisoned neighbours: the same bits as the plain call, and the words
    outside da's slice keep what they held."""
    case = seam_case(name)
    plain, _, _ = run_seam(case)
    got, lay, ydec = run_seam(case, x_c0=8, g_c0=4, da_c0=12)
    frame_ok(lay, own_da=False)
    assert same_bits(plain, got)


@pytest.mark.parametrize("name", ["base_big", "level0_big", "level1_big_odd"])
def test_result_does_not_depend_on_wgrad_blocks(hiplib, name):
    """Two blocks walking the four slices, one block walking all of them, more blocks than slices: the bits of one block per slice."""
    case = seam_case(name)
    auto, _, _ = run_seam(case)
    for blocks in (1, 2, 3, 1000):
        forced, lay, _ = run_seam(case, wgrad_blocks=blocks, fill=7.5)
        frame_ok(lay, 7.5)
        assert same_bits(forced, auto), blocks


@pytest.mark.parametrize("name", ["base_big", "level0_big", "level1_big_odd", "level1_tiny_odd"])
def test_zero_gradient_gives_exact_zeros(hiplib, name):
    case = seam_case(name)
    got, lay, _ = run_seam(case, g=torch.zeros_like(case.g))
    frame_ok(lay)
    for k, v in got.items():
        assert bool((v == 0).all()), k


def test_fully_masked_layer_gives_exact_zeros(hiplib):
    case = SC.stem_case("level1.0", (5, 7), B=1, seed=12, negative_y=True)
    got, lay, _ = run_seam(case)
    frame_ok(lay)
    assert all(bool((v == 0).all()) for v in got.values())


def test_rejected_arguments(hiplib):
    from dd3d_amd import hip
    lib = hip.lib()
    st = hip.current_stream()
    for name in ("base_tiny", "level0_tiny", "level1_tiny_odd"):
        case = seam_case(name)
        _, lay, _ = run_seam(case)
        both = ("dd3d_stem_wgrad", "dd3d_stem_dgrad")
        w_only, d_only = both[:1], both[1:]
        bad = [("B", 0, both), ("H", 0, both), ("W", 0, both), ("Cin", 32, both), ("Cout", 64, both), ("ksize", 5, both), ("stride", 3, both),
               ("g", None, both), ("w", None, both), ("scale", None, both), ("y", None, both), ("g_pitch", lay.args.g_pitch + 2, both),
               ("g_pitch", case.Cout - 4, both), ("y_mode", 3, both), ("y_pitch", 2, both), ("x", None, w_only), ("x_pitch", case.Cin + 1, w_only),
               ("x_pitch", case.Cin - 4, w_only), ("part", None, w_only), ("qpart", None, w_only), ("dw_level", None, w_only), ("dw", None, w_only),
               ("q", None, w_only), ("r", None, w_only), ("n_slices", 0, w_only), ("wgrad_blocks", -1, w_only), ("da", None, d_only),
               ("da_pitch", case.Cin - 4, d_only), ("da_pitch", case.Cin + 3, d_only), ("g", lay.args.g + 4, d_only), ("H", 1 << 14, both)]
        for field, value, who in bad:
            for entry in who:
                if entry == "dd3d_stem_dgrad" and case.ksize == 7:
                    continue
                a = hip.StemGradArgs.from_buffer_copy(lay.args)
                if field == "H" and value == 1 << 14:
                    a.W = 1 << 13  # 2^27 pixels
                setattr(a, field, value)
                assert getattr(lib, entry)(C.byref(a), st) == -1, (name, entry, field, value)
                assert lib.dd3d_last_error().decode().startswith(entry), (name, entry, field, lib.dd3d_last_error())
        if case.ksize == 7:  # the image has no gradient
            a = hip.StemGradArgs.from_buffer_copy(lay.args)
            a.da, a.da_pitch = lay.dw.data_ptr(), 4
            assert lib.dd3d_stem_dgrad(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_stem_dgrad")
        a = hip.StemGradArgs.from_buffer_copy(lay.args)
        a.y_mode, a.y_plane_scale = hip.PG_ACT_F16X2, 0.0
        assert lib.dd3d_stem_wgrad(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_stem_wgrad")
        assert lib.dd3d_stem_wgrad(None, st) == -1 and lib.dd3d_stem_dgrad(None, st) == -1
        torch.cuda.synchronize()
        frame_ok(lay)  # no rejected call wrote anything


# ------------------------------------------------------------------------------------------------ the KEEP stem at its seam
def _keep_case(B, Hp, Wp, sizes, keep, seed=0):
    """The fused stem on seeded uint8 images, with (`keep`) or without the two stored intermediates; every output a channel slice of a
    wider, sentinel-filled buffer.  Returns (plan, op, buffers, float64 references of base, level0, level1, the convolutions)."""
    import torch.nn.functional as F
    from dd3d_amd import hip
    from dd3d_amd.engine import FusedStemOp, PlanBase
    from dd3d_amd.layers import fold_norm
    from tests.util import bundle, gpu_model
    cfg, sd = bundle("dd3d_kitti_dla34", "dla34_kitti")
    model = gpu_model(cfg, sd, use_graph=False)
    dla = model.backbone.bottom_up
    plan = PlanBase("cuda")
    plan.math = hip.MATH_F16X2
    plan.B, plan.Hp, plan.Wp = B, Hp, Wp
    u8 = torch.randint(0, 256, (B, 3, Hp, Wp), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))
    plan.in_u8 = u8.cuda()
    plan.in_sizes = torch.tensor(sizes, dtype=torch.int32).cuda()
    guards = {}

    def framed(b):  # the buffer's f32 storage between two runs of GUARD sentinel words
        raw = torch.full((b.t.numel() + 2 * GUARD, ), SENTINEL, dtype=torch.float32, device="cuda")
        b.t = raw[GUARD:GUARD + b.t.numel()].view(b.t.shape)
        guards[b.name] = raw
        return b

    out = framed(plan.buf("level1", B, Hp // 2, Wp // 2, 64, kind="both"))
    out.p.fill_(0x1234)
    bufs = {"out": out}
    kv = None
    if keep:
        for n in ("base", "level0"):
            bufs[n] = framed(plan.buf(n, B, Hp, Wp, 4 + 16 + 4))
        kv = (bufs["base"].view(4, 16), bufs["level0"].view(4, 16))
    convs = [dla.base_layer, dla.level0[0], dla.level1[0]]
    op = FusedStemOp(plan, model, convs, out.view(32, 32), keep=kv)
    mean, std = model.pixel_mean.cpu().view(3, 1, 1), model.pixel_std.cpu().view(3, 1, 1)
    x = torch.zeros(B, 3, Hp, Wp)
    for b, (h, w) in enumerate(sizes):
        x[b, :, :h, :w] = (u8[b, :, :h, :w].float() - mean) / std
    refs, ref = [], x.double()

    def layer(cv, t):
        sc, sh = fold_norm(cv, None)
        return F.relu(F.conv2d(t, cv.weight.detach().cpu().double(), None, stride=cv.stride, padding=cv.padding) * sc.cpu().double().view(1, -1, 1, 1)
                      + sh.cpu().double().view(1, -1, 1, 1))

    for cv in convs:
        ref = layer(cv, ref)
        refs.append(ref)
    plan.guards = guards
    return plan, op, bufs, refs, lambda t: layer(convs[2], t)


GUARD = 256  # sentinel words in front of and behind every f32 buffer of the KEEP tests


def guards_intact(plan):
    return all(bool((raw[:GUARD] == SENTINEL).all()) and bool((raw[-GUARD:] == SENTINEL).all()) for raw in plan.guards.values())


# 38 x 140: a 19 x 70 level1 map -- three rows and three columns of 8 x 32 tiles, the last of each partial (3 of 8, 6 of 32); the second
# image is smaller than the canvas.  32 x 128: whole tiles only.
@pytest.mark.parametrize("B,Hp,Wp,sizes", [(2, 38, 140, [(38, 140), (29, 101)]), (1, 32, 128, [(32, 128)])], ids=["partial_tiles_b2", "aligned"])
def test_keep_stem_at_the_seam(hiplib, B, Hp, Wp, sizes):
    plain_plan, plain_op, plain, _, _ = _keep_case(B, Hp, Wp, sizes, keep=False)
    plain_plan.ops.append(plain_op)
    plain_plan.launch()
    plan, op, bufs, refs, level1_of = _keep_case(B, Hp, Wp, sizes, keep=True)
    plan.ops.append(op)
    plan.launch()
    torch.cuda.synchronize()
    # out and out_planes: the bits of dd3d_stem_fused_f16x2 on the same inputs
    assert torch.equal(bufs["out"].t, plain["out"].t) and torch.equal(bufs["out"].p, plain["out"].p)
    assert bool((bufs["out"].t[..., :32] == SENTINEL).all()) and bool((bufs["out"].p[0] == 0x1234).all()) and not bool((bufs["out"].t[..., 32:] == SENTINEL).any())
    got = {}
    for n, ref in (("base", refs[0]), ("level0", refs[1])):
        t = bufs[n].t
        assert bool((t[..., :4] == SENTINEL).all()) and bool((t[..., 20:] == SENTINEL).all()) and not bool((t[..., 4:20] == SENTINEL).any()), n
        got[n] = t[..., 4:20].permute(0, 3, 1, 2).cpu()
        tol = 2e-5 * max(1.0, float(ref.abs().max()))
        dev = float((got[n].double() - ref).abs().max())
        print(f"[stem_grads] keep {n} {B}x{Hp}x{Wp}: deviation {dev:.3e} bar {tol:.3e}")
        assert dev <= tol, (n, dev, tol)
    # level1 from the kept level0 in float64: the stored tensor is what the next layer consumed
    l1 = bufs["out"].t[..., 32:].permute(0, 3, 1, 2).cpu().double()
    re = level1_of(got["level0"].double())
    assert float((l1 - re).abs().max()) <= 2e-5 * max(1.0, float(re.abs().max()))
    assert int(plan.status.cpu()) == 0
    # the guard words in front of and behind out, keep_base and keep_level0: nothing is stored before the first or past the last pixel
    assert sorted(plan.guards) == ["base", "level0", "level1"] and guards_intact(plan) and guards_intact(plain_plan)
    first = {n: bufs[n].t.clone() for n in bufs}
    plan.launch()
    torch.cuda.synchronize()
    assert all(torch.equal(first[n], bufs[n].t) for n in bufs) and guards_intact(plan)


def test_keep_stem_rejected_arguments(hiplib):
    from dd3d_amd import hip
    plan, op, bufs, _, _ = _keep_case(1, 16, 64, [(16, 64)], keep=True)
    lib, st = hip.lib(), hip.current_stream()
    for field, value in (("keep_base", None), ("keep_level0", None), ("keep_base_pitch", 12), ("keep_level0_pitch", 18), ("keep_base", op.keep_args.keep_base + 4)):
        a = hip.StemKeepArgs.from_buffer_copy(op.keep_args)
        setattr(a, field, value)
        assert lib.dd3d_stem_fused_keep_f16x2(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_stem_fused_keep_f16x2"), field
    a = hip.StemKeepArgs.from_buffer_copy(op.keep_args)
    a.stem.Hp = 15
    assert lib.dd3d_stem_fused_keep_f16x2(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_stem_fused_keep_f16x2")
    torch.cuda.synchronize()
    assert all(bool((b.t == SENTINEL).all()) for b in bufs.values()) and guards_intact(plan)


# ------------------------------------------------------------------------------------------------ end to end
E2E_CASES = ["kitti_dla34", "kitti_dla34_bf16x3", "kitti_dla34_plane_scale_1", "kitti_dla34_bn", "nusc_dla34"]
_NATURAL = {}
FAMILY = {"weight": "filter", "norm.weight": "norm_weight", "norm.bias": "bias", "bias": "bias"}


@pytest.mark.parametrize("name", E2E_CASES)
def test_compute_losses_with_stem_grads(hiplib, name):
    """DD3D.compute_losses(stem_grads=True) on the whole-model cases: everything backbone_grads returns bit for bit; each stem call against
    the layer oracle on the plan's own stored input and the gradient the call read; the stem's parameters and the two new tensor gradients
    against ONE autograd pass of the whole model under the stored signs of ALL ReLUs; exact key sets; a second call and launch-by-launch
    execution with the same bits."""
    from tests import loss_grad_cases as GC
    from tests import whole_model_grad_oracle as WO
    from tests.test_loss_grads_gpu import _model
    from tests.util import decode
    F64, F32 = torch.float64, torch.float32
    case = WO.CASES[name]
    model = _model(case["exp"], case["weights"], case["overrides"])
    model.math, model.act_scale = case["math"], case["act_scale"]
    cpu = GC.cpu_model(case["exp"], case["overrides"])
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    inputs, gt = WO.case_inputs(case, cpu)
    for x, g in zip(inputs, gt):
        x["instances"] = g
    lb, gb, pb = model.compute_losses(inputs, backbone_grads=True)
    losses, grads, params = model.compute_losses(inputs, stem_grads=True)
    plan = model.get_loss_plan(*model.canvas_size(inputs), stem_grads=True)
    assert plan.fused_stem == (case["math"] is None)  # the default arithmetic runs the fused stem with KEEP, bf16x3 launch by launch
    # the loss dict and every key backbone_grads returns: the same bits; the key sets: exact
    assert list(lb) == list(losses) and all(torch.equal(lb[k], losses[k]) for k in lb)
    assert all(torch.equal(gb[k], grads[k]) for k in gb) and all(torch.equal(pb[k], params[k]) for k in pb)
    assert sorted(set(grads) - set(gb)) == ["backbone_base_layer", "backbone_level0"]
    named = dict(cpu.named_parameters())
    assert sorted(params) == sorted(named) and all(params[k].shape == named[k].shape and params[k].dtype == F32 for k in params)
    pfx = "backbone.bottom_up."
    stem_keys = sorted(set(params) - set(pb))
    assert stem_keys == sorted(k for k in named if k.startswith((pfx + "base_layer.", pfx + "level0.", pfx + "level1.")))

    # each call against the layer oracle, fed what the call itself read
    for key, lay in plan.stem_layers.items():
        x = lay.keep[0].permute(0, 3, 1, 2).cpu()
        y = decode(plan.bufs[lay.src["y"][0]])
        g = lay.keep[1].permute(0, 3, 1, 2).cpu()
        w, sc = lay.keep[2].permute(0, 3, 1, 2).cpu(), lay.scale.cpu()
        r64, r32 = (SO.layer_grads(x, y, g, w, sc, lay.stride, dt) for dt in (F64, F32))
        check(collect(lay), r64, r32, f"{name} call {key}")

    # the stored signs of all ReLUs, the stem's three included, and the two conditions on them
    inv_K = plan.inv_K.view(-1, 3, 3).cpu()
    if case["ref"] not in _NATURAL:
        _NATURAL[case["ref"]] = WO.whole_model_grads(cpu, cpu.cfg, inputs, gt, F64, inv_K=inv_K, backward=False)[2]
    pre64 = _NATURAL[case["ref"]]
    report = []
    masks = SO.stem_plan_masks(plan, pre64, report)
    total, bad, far = sum(v.numel() for v in pre64), sum(r[2] for r in report), sum(r[3] for r in report)
    for label, n, b, f in report[:3]:
        print(f"[stem_grads] {name} signs {label}: {b} of {n} differ from the float64 forward's, {f} of them beyond 2^-16 of the tensor's maximum")
    print(f"[stem_grads] {name} signs: {bad} of {total} ReLU elements differ ({bad / total:.1e}; cap 1e-4), {far} beyond 2^-16 (cap 0)")
    assert far == 0 and bad <= WO.SIGN_CAP * total, (name, bad, far, total)

    # ONE autograd pass of the whole model per precision
    p64, a64 = SO.whole_model_grads_with_stem(cpu, cpu.cfg, inputs, gt, F64, masks, inv_K)
    p32, a32 = SO.whole_model_grads_with_stem(cpu, cpu.cfg, inputs, gt, F32, masks, inv_K)
    fams = {}
    for k in stem_keys:
        fams.setdefault(FAMILY[k.split(".", 4)[-1] if ".norm." in k else k.rsplit(".", 1)[-1]], []).append(k)
    rows = [(fam, [params[k] for k in ks], [p64[k] for k in ks], [p32[k] for k in ks]) for fam, ks in sorted(fams.items())]
    rows += [(k, [grads[k]], [a64[k]], [a32[k]]) for k in ("backbone_level0", "backbone_base_layer")]
    for fam, c, a, b in rows:
        c, a, b = (torch.cat([v.reshape(-1).cpu() for v in vs]) for vs in (c, a, b))
        assert bool(torch.isfinite(c).all()), (name, fam)
        bar, d32, gmax = SO.bar(a.double(), b, torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((c.double() - a.double()).abs().max())
        print(f"[stem_grads] {name} whole model {fam}: n {a.numel()} max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} "
              f"(uses {8 * dev / bar if bar > 0 else 0.0:.2f} of the factor 8)")
        assert gmax > 0.0 and dev <= bar, (name, fam, dev, bar, d32, gmax)

    # a second call is bit-equal; the captured graph equals launch-by-launch execution
    same = lambda r: all(torch.equal(r[0][k], losses[k]) for k in losses) and all(torch.equal(r[1][k], grads[k]) for k in grads) and \
        all(torch.equal(r[2][k], params[k]) for k in params)
    assert same(model.compute_losses(inputs, stem_grads=True))
    model.use_graph = False
    model.invalidate_plans()
    assert same(model.compute_losses(inputs, stem_grads=True))
