"""VoVNet-V2 backbone backward on the MI355X at its C-ABI seams (csrc/vovnet_grads.hip, the wide entry points of csrc/backbone_grads.hip):
dd3d_ese_backward against the float64 statement of the eSE formulas with gates in all three regions of the hard sigmoid;
dd3d_maxpool3x3s2_ceil_backward bit for bit against the restatement that equals torch's CPU autograd (tests/test_vovnet_grads.py);
dd3d_vovnet_conv_wgrad / dd3d_vovnet_conv_dgrad at the smallest shapes that cross the DLA entry points' limits, with slices, `add`, the
third term (summed beforehand by dd3d_vovnet_add), the mask, equal bits across tile choices and runs, and their rejections; one
two-module OSA stage through engine.losses.vovnet_backward against float64 autograd of oracle.vovnet_oracle._osa under the stored tensors' masks.

The bar of a family is the project's, 8 * max(d32, 2^-23 * max|g64|): d32 is the deviation of the reference's float32 run from its float64
run on the same case (loss_grad_oracle.bar).  The pool backward is a selection and at most four float32 adds in a stated order: equality."""
import ctypes as C

import pytest
import torch

from tests import backbone_grad_cases as BC
from tests import backbone_grad_oracle as BO
from tests import loss_grad_oracle as GO
from tests import vovnet_grad_oracle as VG
from tests.test_backbone_grads_gpu import KEEP, SENTINEL, collect, same_bits, store, wide
from tests.test_vovnet_grads import pool_input

pytestmark = pytest.mark.gpu

WORST = {}


def within_bar(what, fam, got, ref64, ref32):
    got, ref64, ref32 = (torch.cat([v.reshape(-1).cpu() for v in (vs if isinstance(vs, (list, tuple)) else [vs])]) for vs in (got, ref64, ref32))
    assert bool(torch.isfinite(got).all()), (what, fam)
    bar, d32, gmax = GO.bar(ref64.double(), ref32, torch.ones(ref64.shape[0], dtype=torch.bool))
    dev = float((got.double() - ref64.double()).abs().max())
    use = 8 * dev / bar if bar > 0 else 0.0
    WORST[fam] = max(WORST.get(fam, 0.0), use)
    print(f"[vovnet_grads] {what} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8; "
          f"worst so far {WORST[fam]:.2f})")
    assert dev <= bar, (what, fam, dev, bar, d32, gmax)
    return gmax


# ------------------------------------------------------------------------------------------------------------------- eSE backward
def ese_case(Cc, hw, seed):
    """B = 2: a rectified xt, a gradient, fc weights and biases spread so that the gates fall below, inside and above the clamp."""
    gen = torch.Generator().manual_seed(seed)
    xt = torch.relu(torch.randn(2, Cc, hw[0], hw[1], generator=gen))
    g = torch.randn(2, Cc, hw[0], hw[1], generator=gen)
    fc_w = torch.randn(Cc, Cc, generator=gen) * (2.0 / Cc**0.5)
    fc_b = torch.linspace(-5.0, 5.0, Cc)[torch.randperm(Cc, generator=gen)]
    return xt, g, fc_w, fc_b


def run_ese(xt, g, fc_w, fc_b, storage, scale=16.0, rsplit=None, fill=SENTINEL):
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import EseGrads
    B, Cc, H, W = xt.shape
    xb, xbind, xdec = store(xt, storage, scale, 32 if storage != "f32" else 0)
    gb, gv = wide(g, 32)
    lay = EseGrads("cuda", B, H, W, Cc, xbind, gv, fc_w.contiguous().cuda(), fc_b.contiguous().cuda(), rsplit=rsplit, fill=fill, guard=64)
    lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    assert lay.guards_intact(fill)
    for t in (lay.part, lay.m, lay.z, lay.s, lay.dz, lay.u, lay.g_xt, lay.d_fc_w, lay.d_fc_b):
        assert not bool((t == fill).any())
    lay.keep_alive = (xb, gb)
    got = {"g_xt": lay.g_xt.permute(0, 3, 1, 2).cpu(), "d_fc_w": lay.d_fc_w.cpu(), "d_fc_b": lay.d_fc_b.cpu(), "z": lay.z.cpu(), "s": lay.s.cpu()}
    return got, lay, xdec


@pytest.mark.parametrize("storage", ["f32", "f16x2"])
@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (20, 30)])  # HW = 1, 15, 600 (600: two row splits)
@pytest.mark.parametrize("Cc", [32, 96])
def test_ese_backward_against_the_formulas(hiplib, Cc, hw, storage):
    """The call has no identity operand: under `identity` the module's G_out reaches the module input as the third term of layer 0's
    input gradient (test_wide_convolution_against_oracle, test_one_stage_chain); G_xt is the same with and without it."""
    xt, g, fc_w, fc_b = ese_case(Cc, hw, seed=100 + Cc + hw[0])
    got, lay, xdec = run_ese(xt, g, fc_w, fc_b, storage)
    assert lay.rsplit == (2 if hw == (20, 30) else 1)
    r64, r32 = VG.ese_backward(xdec, g, fc_w, fc_b, torch.float64), VG.ese_backward(xdec, g, fc_w, fc_b, torch.float32)
    z = r64["z"]
    assert float((z.abs() - 3).abs().min()) > 1e-3  # no gate within 1e-3 of a clamp edge: rounding cannot move one across it
    assert bool((z <= -3).any()) and bool((z >= 3).any()) and bool(((z > -3) & (z < 3)).any())
    assert float((got["z"].double() - z).abs().max()) < 1e-4 and torch.equal(got["z"] > -3, z > -3) and torch.equal(got["z"] < 3, z < 3)
    what = f"ese:{Cc}:{hw[0]}x{hw[1]}:{storage}"
    for fam in ("g_xt", "d_fc_w", "d_fc_b"):
        assert within_bar(what, fam, got[fam], r64[fam], r32[fam]) > 0.0
    again, _, _ = run_ese(xt, g, fc_w, fc_b, storage, fill=7.5)
    assert same_bits(again, got)


def test_ese_backward_rejects_bad_arguments(hiplib):
    from dd3d_amd import hip
    xt, g, fc_w, fc_b = ese_case(32, (3, 5), seed=1)
    _, lay, _ = run_ese(xt, g, fc_w, fc_b, "f32")
    a, lib, st = lay.args, hip.lib(), hip.current_stream()
    for field, value in (("C", 48), ("C", 1056), ("rsplit", 0), ("rsplit", 65), ("xt_mode", 5), ("xt_pitch", 30), ("g_pitch", 30), ("gxt_pitch", 28), ("B", 0),
                         ("HW", 0), ("xt", None), ("g", None), ("fc_w", None), ("part", None), ("g_xt", None), ("d_fc_b", None)):
        old = getattr(a, field)
        setattr(a, field, value)
        assert lib.dd3d_ese_backward(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_ese_backward"), field
        setattr(a, field, old)
    assert lib.dd3d_ese_backward(None, st) == -1
    assert lib.dd3d_ese_backward(C.byref(a), st) == 0
    torch.cuda.synchronize()
    assert lay.guards_intact(SENTINEL)


# ------------------------------------------------------------------------------------------------------------------- pool backward
def run_pool3(x, g, storage="f32", plane_scale=1.0, add=None, fill=SENTINEL):
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import Pool3Grads
    B, C_, H, W = x.shape
    c0 = 32 if storage != "f32" else 0
    xb, xbind, xdec = store(x, storage, plane_scale, c0)
    gb, gv = wide(g, 32)
    ab, av = wide(add, 0) if add is not None else (None, None)
    lay = Pool3Grads("cuda", B, H, W, C_, xbind, gv, add=av, fill=fill, guard=64)
    lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    assert lay.guards_intact(fill) and not bool((lay.da == fill).any())
    lay.keep_alive = (xb, gb, ab)
    return lay.da.permute(0, 3, 1, 2).cpu(), xdec, lay


POOL3_CASES = {
    "3x3_random_f32": ((3, 3), "random", "f32", 1.0, False),
    "3x3_equal_f16_add": ((3, 3), "equal", "f16x2", 16.0, True),
    "4x5_ties_f32_add": ((4, 5), "ties", "f32", 1.0, True),
    "4x5_negative_bf16x3": ((4, 5), "negative", "bf16x3", 1.0, False),
    "7x8_relu_f16s1_add": ((7, 8), "relu", "f16x2", 1.0, True),
    "7x8_equal_f32": ((7, 8), "equal", "f32", 1.0, False),
    "7x8_ties_bf16x3_add": ((7, 8), "ties", "bf16x3", 1.0, True),
    "9x9_negative_f32_add": ((9, 9), "negative", "f32", 1.0, True),
    "9x9_relu_f16": ((9, 9), "relu", "f16x2", 16.0, False),
    "9x9_random_bf16x3": ((9, 9), "random", "bf16x3", 1.0, False),
}


@pytest.mark.parametrize("name", list(POOL3_CASES))
def test_pool3_backward_is_bit_exact(hiplib, name):
    hw, kind, storage, scale, with_add = POOL3_CASES[name]
    gen = torch.Generator().manual_seed(91)
    x = pool_input(kind, 2, 32, hw, seed=90)
    g = torch.randn(2, 32, VG.pool3_out(hw[0]), VG.pool3_out(hw[1]), generator=gen)
    add = torch.randn(2, 32, hw[0], hw[1], generator=gen) if with_add else None
    got, xdec, lay = run_pool3(x, g, storage, scale, add=add)
    assert (lay.Ho, lay.Wo) == tuple(g.shape[2:])
    assert torch.equal(got, VG.pool3_backward(xdec, g, torch.float32, add=add)), name
    if kind == "equal":  # the top-left corner of every window takes it all
        base = add if add is not None else torch.zeros_like(got)
        want = base.clone()
        want[:, :, 0:2 * g.shape[2]:2, 0:2 * g.shape[3]:2] += g
        assert torch.equal(got, want)
    again, _, _ = run_pool3(x, g, storage, scale, add=add, fill=7.5)
    assert torch.equal(again, got)


def test_pool3_backward_rejects_bad_arguments(hiplib):
    from dd3d_amd import hip
    x = pool_input("random", 1, 32, (4, 5))
    _, _, lay = run_pool3(x, torch.zeros(1, 32, 2, 2))
    a, lib, st = lay.args, hip.lib(), hip.current_stream()
    for field, value in (("H", 2), ("W", 2), ("C", 48), ("C", 1056), ("x_mode", 9), ("x_pitch", 28), ("g_pitch", 30), ("da_pitch", 16), ("B", 0), ("x", None),
                         ("g", None), ("da", None)):
        old = getattr(a, field)
        setattr(a, field, value)
        assert lib.dd3d_maxpool3x3s2_ceil_backward(C.byref(a), st) == -1 and \
            lib.dd3d_last_error().decode().startswith("dd3d_maxpool3x3s2_ceil_backward"), field
        setattr(a, field, old)
    assert lib.dd3d_maxpool3x3s2_ceil_backward(None, st) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------- wide convolution entry points
def run_wide(case, add2=None, x_storage="f32", y_storage=None, x_scale=1.0, y_scale=16.0, x_c0=0, y_c0=0, g_c0=0, da_c0=None, dgrad_rows=0, dgrad_group=0,
             fill=SENTINEL):
    """One convolution through VovnetConvGrads (run_seam of tests/test_backbone_grads_gpu.py); with `add2` the head term is summed
    beforehand by one SumGrads launch, T = add + add2 (or add2 alone stands in for `add`), as engine.losses.vovnet_backward does."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import SumGrads, VovnetConvGrads
    y_storage = y_storage or x_storage
    ys = y_scale if y_storage != x_storage else x_scale
    xb, xbind, xdec = store(case.x, x_storage, x_scale, x_c0)
    yb, ybind, ydec = store(case.y, y_storage, ys, y_c0)
    rb, rbind, rdec = store(case.res_y, y_storage, ys, x_c0) if case.res_y is not None else (None, None, None)
    gbuf, g = wide(case.g, g_c0)
    abuf, addt = wide(case.add, 32 if x_c0 else 0) if case.add is not None else (None, None)
    a2buf, add2t = wide(add2, 64) if add2 is not None else (None, None)
    rgbuf, rg = wide(case.res_g, x_c0) if case.res_g is not None else (None, None)
    dabuf = da = None
    if da_c0 is not None:
        dabuf = torch.full((case.B, case.hw[0], case.hw[1], da_c0 + case.Cin + 32), KEEP, dtype=torch.float32, device="cuda")
        da = dabuf[..., da_c0:da_c0 + case.Cin]
    head = None
    if addt is not None and add2t is not None:
        head = SumGrads("cuda", addt, add2t, fill=fill, guard=64)
        head.launch(hip.lib(), hip.current_stream())
        addt = head.da
    elif add2t is not None:
        addt = add2t
    lay = VovnetConvGrads("cuda", case.B, case.hw[0], case.hw[1], case.Cin, case.Cout, case.ksize, case.stride, xbind, ybind, g,
                          case.w.permute(0, 2, 3, 1).contiguous().cuda(), case.scale.contiguous().cuda(), add=addt,
                          res=(rg, rbind) if rg is not None else None, da=da, fill=fill, guard=64, dgrad_rows=dgrad_rows, dgrad_group=dgrad_group)
    lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    lay.keep_alive = (xb, yb, rb, gbuf, abuf, a2buf, rgbuf, dabuf, head)
    assert lay.guards_intact(fill) and (head is None or (head.guards_intact(fill) and not bool((head.da == fill).any())))
    n = lay.n_slices * lay.Cout
    for t in [lay.part.reshape(-1)[:n * lay.ksize**2 * lay.Cin], lay.qpart.reshape(-1)[:n], lay.dw_level, lay.dw, lay.q, lay.r] + ([lay.da] if da is None else []):
        assert not bool((t == fill).any())
    if dabuf is not None:  # the words outside the slice keep what they held
        outside = torch.ones(dabuf.shape[-1], dtype=torch.bool)
        outside[da_c0:da_c0 + case.Cin] = False
        assert bool((dabuf[..., outside.cuda()] == KEEP).all()) and not bool((da == KEEP).any())
    return collect(lay), lay, dict(x=xdec, y=ydec, res_y=rdec)


def wide_ref(case, dec, add2, dtype):
    head = None  # (add + add2) in the kernel's order; the residual pair follows inside layer_grads
    for t in (case.add, add2):
        if t is not None:
            head = t.to(dtype) if head is None else head + t.to(dtype)
    res = (case.res_g, dec["res_y"]) if case.res_g is not None else None
    return BO.layer_grads(dec["x"], dec["y"], case.g, case.w, case.scale, case.stride, dtype, add=head, res=res)


# the smallest shapes past dd3d_backbone_wgrad's limits (Cin 1280, Cout 512): Cin 1312 (41 chunks: 11 input-channel groups of 128, the last
# one chunk wide), Cout 544 (five row tiles of the weight gradient, the last one wave wide; 17 chunks in the input gradient's chain), and a
# 3x3 with Cin 1024 -> Cout 160 (the stage3 layer-0 shape of an identity module) on 1 x 4 x 6 with all three head terms.
WIDE_CASES = {
    "1x1_c1312_o32_slices_f16": (dict(hw=(3, 5), B=2, Cin=1312, Cout=32, ksize=1, stride=1, seed=61, with_add=True), True,
                                 dict(x_storage="f16x2", x_scale=16.0, x_c0=32, y_c0=64, g_c0=32, da_c0=64)),
    "1x1_c32_o544_add2_only": (dict(hw=(3, 5), B=2, Cin=32, Cout=544, ksize=1, stride=1, seed=62), True, dict()),
    "3x3_c1024_o160_4x6_three_terms": (dict(hw=(4, 6), B=1, Cin=1024, Cout=160, ksize=3, stride=1, seed=63, with_add=True, with_res=True), True,
                                       dict(x_storage="bf16x3")),
    "1x1_c1312_o544_no_head": (dict(hw=(1, 7), B=1, Cin=1312, Cout=544, ksize=1, stride=1, seed=64), False, dict()),
}


@pytest.mark.parametrize("name", list(WIDE_CASES))
def test_wide_convolution_against_oracle(hiplib, name):
    kw, with_add2, run = WIDE_CASES[name]
    case = BC.ConvCase(**kw)
    add2 = torch.randn(case.B, case.Cin, *case.hw, generator=torch.Generator().manual_seed(kw["seed"] + 1000)) if with_add2 else None
    got, lay, dec = run_wide(case, add2, **run)
    r64, r32 = wide_ref(case, dec, add2, torch.float64), wide_ref(case, dec, add2, torch.float32)
    a, b, k = BO.family_vectors(r64), BO.family_vectors(r32), BO.family_vectors(got)
    for fam in ("filter", "bias", "norm_weight", "input"):
        assert within_bar("wide:" + name, fam, k[fam], a[fam], b[fam]) > 0.0
    again, _, _ = run_wide(case, add2, **run)
    assert same_bits(again, got), name


def test_wide_third_term_alone_is_added_bit_for_bit(hiplib):
    """An all-non-positive stored output masks every gradient: da = add + add2 in float32, bit for bit; without both an exact zero."""
    case = BC.ConvCase(hw=(3, 5), B=2, Cin=1312, Cout=32, ksize=1, stride=1, seed=65, with_add=True, negative_y=True)
    add2 = torch.randn(2, 1312, 3, 5, generator=torch.Generator().manual_seed(66))
    got, _, _ = run_wide(case, add2)
    assert torch.equal(got["da"], case.add + add2) and all(float(got[k].abs().max()) == 0.0 for k in ("dw", "dw_level", "q", "r"))
    case.add = None
    got, _, _ = run_wide(case, add2)
    assert torch.equal(got["da"], add2)
    got, _, _ = run_wide(case, None)
    assert float(got["da"].abs().max()) == 0.0


def test_wide_tile_choice_does_not_change_the_bits(hiplib):
    case = BC.ConvCase(hw=(6, 20), B=2, Cin=1312, Cout=64, ksize=1, stride=1, seed=67, with_add=True)
    add2 = torch.randn(2, 1312, 6, 20, generator=torch.Generator().manual_seed(68))
    auto, _, _ = run_wide(case, add2)
    for rows, group in ((2, 128), (2, 256), (4, 256), (8, 128), (8, 256)):
        forced, _, _ = run_wide(case, add2, dgrad_rows=rows, dgrad_group=group, fill=7.5)
        assert same_bits(forced, auto), (rows, group)


def test_wide_entry_points_reject_bad_arguments(hiplib):
    from dd3d_amd import hip
    case = BC.ConvCase(hw=(3, 5), B=1, Cin=32, Cout=32, ksize=3, stride=1, seed=69, with_add=True, with_res=True)
    add2 = torch.randn(1, 32, 3, 5, generator=torch.Generator().manual_seed(70))
    _, lay, _ = run_wide(case, add2)
    lib, st, a = hip.lib(), hip.current_stream(), lay.args
    both = (("dd3d_vovnet_conv_wgrad", lib.dd3d_vovnet_conv_wgrad), ("dd3d_vovnet_conv_dgrad", lib.dd3d_vovnet_conv_dgrad))
    for field, value, entries in (("Cin", 48, both), ("Cin", 2176, both), ("Cout", 16, both), ("Cout", 1056, both), ("stride", 3, both), ("ksize", 2, both),
                                  ("g_pitch", 34, both), ("x_pitch", 28, both[:1]), ("y_mode", 7, both), ("add_pitch", 28, both[1:]), ("da_pitch", 28, both[1:]),
                                  ("n_slices", 0, both[:1]), ("dgrad_rows", 3, both), ("dgrad_group", 64, both), ("B", 0, both), ("g", None, both),
                                  ("x", None, both[:1]), ("da", None, both[1:]), ("dw", None, both[:1])):
        old = getattr(a, field)
        setattr(a, field, value)
        for name, fn in entries:
            assert fn(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(name), (field, name)
        setattr(a, field, old)
    assert lib.dd3d_vovnet_conv_wgrad(None, st) == -1 and lib.dd3d_vovnet_conv_dgrad(None, st) == -1
    # the DLA entry points keep their limits: the same arguments past them are refused there and accepted here
    a.Cin = 1312
    assert lib.dd3d_backbone_grad_slices(C.byref(a)) == -1 and lib.dd3d_vovnet_conv_grad_slices(C.byref(a)) >= 1
    a.Cin = 32
    assert lib.dd3d_vovnet_conv_wgrad(C.byref(a), st) == 0 and lib.dd3d_vovnet_conv_dgrad(C.byref(a), st) == 0
    torch.cuda.synchronize()
    assert lay.guards_intact(SENTINEL)
    # the elementwise sum
    x, y, out = (torch.zeros(1, 3, 5, 36, device="cuda") for _ in range(3))
    good = [x.data_ptr(), y.data_ptr(), out.data_ptr(), 15, 32, 36, 36, 36]
    assert lib.dd3d_vovnet_add(*good, st) == 0
    for i, value in ((0, None), (1, None), (2, None), (3, 0), (4, 30), (4, 0), (4, 2176), (5, 28), (6, 34), (7, 16), (0, x.data_ptr() + 4)):
        bad = list(good)
        bad[i] = value
        assert lib.dd3d_vovnet_add(*bad, st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_vovnet_add"), (i, value)
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------------------- one-stage chain
def _stage_chain(vov, S, G, storage, fill=SENTINEL):
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import vovnet_backward, vovnet_param_grads
    B = G.shape[0]
    keep, acts = [], {}
    for k, v in S.items():
        buf, bind, dec = store(v, storage)
        assert torch.equal(dec, v)  # (f32 and bf16x3 decode exactly: the oracle's stored activations are the kernels')
        keep.append(buf)
        acts[k] = (bind, v.shape[2], v.shape[3], v.shape[1])
    layers, gin = vovnet_backward("cuda", B, vov, {"stage2": wide(G, 0, 0)[0]}, acts, lambda t: t.detach().float().contiguous().cuda(), fill=fill, guard=64,
                                  stages=["stage2"], stem=False)
    for lay in layers.values():
        lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    for lay in layers.values():
        assert lay.guards_intact(fill) and not bool((lay.da == fill).any())
    named = {id(p): f"backbone.bottom_up.{k}" for k, p in vov.named_parameters()}
    return {k: v.cpu() for k, v in vovnet_param_grads(named, layers).items()}, gin.permute(0, 3, 1, 2).cpu(), layers, keep


@pytest.mark.parametrize("norm,storage", [("BN", "f32"), ("FrozenBN", "bf16x3")])
def test_one_stage_chain(hiplib, norm, storage):
    """stage2 of the tiny spec: two OSA modules of two layers, 32 -> 32, 32 | concat 96 -> 64, then 64 -> 32, 32 | concat 128 -> 64 with the
    identity add; B = 2 on 6 x 10 -- eSE, concat, layers 1 and 0 and the module input's three terms, through engine.losses.vovnet_backward."""
    vov = VG.mini_vovnet(norm)
    gen = torch.Generator().manual_seed(41)
    x = torch.relu(torch.randn(2, 32, 6, 10, generator=gen))
    S, masks = VG.stage_stored(vov, "stage2", x)
    G = torch.randn(S["stage2.out"].shape, generator=gen)
    params, gin, layers, _ = _stage_chain(vov, S, G, storage)
    assert list(layers) == [f"stage2.OSA2_2.{c}" for c in ("ese", "concat", "1", "sum", "0")] + [f"stage2.OSA2_1.{c}" for c in ("ese", "concat", "1", "0")]
    assert layers["stage2.OSA2_2.0"].args.add == layers["stage2.OSA2_2.sum"].da.data_ptr()
    head = layers["stage2.OSA2_2.sum"]  # the module input's head term: D_cat[x] + G_out in float32, bit for bit
    assert torch.equal(head.da.cpu(), (head.keep[0] + head.keep[1]).cpu())
    for key in ("stage2.OSA2_1.ese", "stage2.OSA2_2.ese"):  # gates on all sides of the clamp, none on an edge
        z = layers[key].z.cpu()
        assert float((z.abs() - 3).abs().min()) > 1e-3 and bool((z <= -3).any()) and bool((z >= 3).any()) and bool(((z > -3) & (z < 3)).any()), key
    p64, x64 = VG.stage_autograd(vov, "stage2", x, G, torch.float64, masks)
    p32, x32 = VG.stage_autograd(vov, "stage2", x, G, torch.float32, masks)
    named = dict(vov.named_parameters())
    want = sorted(k for k in p64 if ".stage2." in k)
    assert sorted(params) == want and all(params[k].shape == named[k[len("backbone.bottom_up."):]].shape for k in params)
    fams = {}
    for k in want:
        fams.setdefault(VG.family_of(k), []).append(k)
    assert set(fams) == {"filter", "fc_weight", "fc_bias"} | ({"norm_weight", "norm_bias"} if norm == "BN" else set())
    what = f"chain:{norm}:{storage}"
    for fam, ks in sorted(fams.items()):
        assert within_bar(what, fam, [params[k] for k in ks], [p64[k] for k in ks], [p32[k] for k in ks]) > 0.0
    assert within_bar(what, "input", gin, x64, x32) > 0.0
    again, gin2, _, _ = _stage_chain(vov, S, G, storage, fill=7.5)
    assert all(torch.equal(again[k], params[k]) for k in params) and torch.equal(gin2, gin)
