"""DLA-34 backbone backward on the MI355X (csrc/backbone_grads.hip, engine.LossPlan(backbone_grads=True)): dd3d_backbone_wgrad,
dd3d_backbone_dgrad and dd3d_maxpool2x2_backward at their C-ABI seam on seeded convolutions of the backbone family
(tests/backbone_grad_cases.py) against the float64 oracle (tests/backbone_grad_oracle.py) -- 3x3 stride 1 and 2, 1x1 up to Cin 1280 and
Cout 512, operands as channel slices of wider buffers, the three storages -- sentinel-framed outputs, poisoned neighbours, every case
twice with equal bits; the pool backward bit for bit; a mini DLA through engine.losses.dla_backward; rejected arguments; the slice count;
DD3D.compute_losses(backbone_grads=True) end to end.

The bar of a family (filter, bias / q, norm weight / r, input gradient) in a case is 8 * max(d32, 2^-23 * max|g64|): d32 is the deviation
of the oracle's float32 run from its float64 run on the same case, computed here on the CPU (loss_grad_oracle.bar).  The pool backward
is a selection and at most two float32 adds in a stated order: it is held to equality with the float32 oracle.
"""
import ctypes as C

import pytest
import torch

from tests import backbone_grad_cases as BC
from tests import backbone_grad_oracle as BO
from tests import loss_grad_cases as GC
from tests.util import decode

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
POISON = 3.0e30  # neighbour channels and pad words of the inputs: a kernel that read them would not stay finite
KEEP = 7.25      # what the words of a wider output buffer outside the slice hold before the call, and must hold after it


def wide(x, c0=0, tail=4, pad=POISON):
    """NCHW -> device [B, H, W, c0 + C + tail] with x in channels c0 .. c0 + C and `pad` elsewhere; returns (buffer, the slice view)."""
    B, C_, H, W = x.shape
    t = torch.full((B, H, W, c0 + C_ + tail), pad, dtype=torch.float32)
    t[..., c0:c0 + C_] = x.permute(0, 2, 3, 1)
    t = t.cuda()
    return t, t[..., c0:c0 + C_]


def store(x, storage, plane_scale=1.0, c0=0):
    """NCHW float32 -> (device buffer, binding (mode, address, pitch, plane scale) of the slice that holds x at channel c0 of a wider
    buffer with poisoned neighbours, the float32 values the storage decodes to)."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import slice_binding
    if storage == "f32":
        buf, _ = wide(x, c0)
        return buf, (hip.PG_ACT_F32, buf.data_ptr() + 4 * c0, buf.shape[-1], 1.0), x
    planes, dec = BC.encode_f16x2(x, plane_scale) if storage == "f16x2" else BC.encode_bf16x3(x)
    junk = lambda n: torch.full((n, ) + tuple(planes.shape[1:]), 0x7BFF if storage == "f16x2" else 0x7F00, dtype=torch.int16)
    buf = torch.cat([junk(c0 // 32), planes, junk(1)], 0).contiguous().cuda()
    mode = hip.PG_ACT_F16X2 if storage == "f16x2" else hip.PG_ACT_BF16X3
    npix = x.shape[0] * x.shape[2] * x.shape[3]
    return buf, slice_binding((mode, buf.data_ptr(), 0, float(plane_scale)), c0, npix), dec


def run_seam(case, x_storage="f32", y_storage=None, x_scale=1.0, y_scale=16.0, x_c0=0, y_c0=0, g_c0=0, da_c0=None, dgrad_rows=0, dgrad_group=0,
             fill=SENTINEL, add=True):
    """One convolution through BackboneConvGrads.  `da_c0`: write the input gradient into channels da_c0 .. of a wider buffer."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import BackboneConvGrads
    y_storage = y_storage or x_storage
    ys = y_scale if y_storage != x_storage else x_scale
    xb, xbind, xdec = store(case.x, x_storage, x_scale, x_c0)
    yb, ybind, ydec = store(case.y, y_storage, ys, y_c0) if case.y is not None else (None, None, None)
    rb, rbind, rdec = store(case.res_y, y_storage, ys, x_c0) if case.res_y is not None else (None, None, None)
    gbuf, g = wide(case.g, g_c0)
    abuf, addt = wide(case.add, 32 if x_c0 else 0) if (case.add is not None and add) else (None, None)
    rgbuf, rg = wide(case.res_g, x_c0) if case.res_g is not None else (None, None)
    dabuf = da = None
    if da_c0 is not None:
        dabuf = torch.full((case.B, case.hw[0], case.hw[1], da_c0 + case.Cin + 32), KEEP, dtype=torch.float32, device="cuda")
        da = dabuf[..., da_c0:da_c0 + case.Cin]
    lay = BackboneConvGrads("cuda", case.B, case.hw[0], case.hw[1], case.Cin, case.Cout, case.ksize, case.stride, xbind, ybind, g,
                            case.w.permute(0, 2, 3, 1).contiguous().cuda(), case.scale.contiguous().cuda(), add=addt,
                            res=(rg, rbind) if rg is not None else None, da=da, fill=fill, guard=64, dgrad_rows=dgrad_rows, dgrad_group=dgrad_group)
    lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    lay.keep_alive = (xb, yb, rb, gbuf, abuf, rgbuf, dabuf)
    if dabuf is not None:  # the words outside the slice keep what they held
        outside = torch.ones(dabuf.shape[-1], dtype=torch.bool)
        outside[da_c0:da_c0 + case.Cin] = False
        assert bool((dabuf[..., outside.cuda()] == KEEP).all()) and not bool((da == KEEP).any())
    return collect(lay), lay, dict(x=xdec, y=ydec, res_y=rdec)


def collect(lay):
    nchw_w = lambda t: t.view(lay.Cout, lay.ksize, lay.ksize, lay.Cin).permute(0, 3, 1, 2).cpu()
    return {"dw_level": nchw_w(lay.dw_level), "dw": nchw_w(lay.dw), "q": lay.q.cpu(), "r": lay.r.cpu(), "da": lay.da.permute(0, 3, 1, 2).cpu()}


WORST = {}


def check(got, ref64, ref32, what, families=("filter", "bias", "norm_weight", "input")):
    a, b, k = BO.family_vectors(ref64), BO.family_vectors(ref32), BO.family_vectors(got)
    for fam in families:
        if a[fam].numel() == 0:
            continue
        assert bool(torch.isfinite(k[fam]).all()), (what, fam)
        bar, d32, gmax = BO.bar(a[fam], b[fam], torch.ones(a[fam].shape[0], dtype=torch.bool))
        dev = float((k[fam].double() - a[fam]).abs().max())
        use = 8 * dev / bar if bar > 0 else 0.0
        WORST[fam] = max(WORST.get(fam, 0.0), use)
        print(f"[backbone_grads] {what} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8; "
              f"worst so far {WORST[fam]:.2f})")
        assert dev <= bar, (what, fam, dev, bar, d32, gmax)


def frame_ok(lay, fill=SENTINEL, own_da=True):
    """Guard words keep the sentinel; every output word is written (the scratch rows in use included)."""
    assert lay.guards_intact(fill)
    n = lay.n_slices * lay.Cout
    for t in [lay.part.reshape(-1)[:n * lay.ksize**2 * lay.Cin], lay.qpart.reshape(-1)[:n], lay.dw_level, lay.dw, lay.q, lay.r] + ([lay.da] if own_da else []):
        assert not bool((t == fill).any())


def same_bits(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


# 3x3 stride 1: one pixel (every tap but the centre in the padding) with mask, add and the residual pair; 1x257 (five units, the last one
# pixel long); 512 -> 512 at 3x5 with B = 2 (K = 4608 in the input gradient, the widest Cout: four row tiles in the weight gradient).
# 3x3 stride 2: 2x2 -> 1x1 (only parity-matched taps land), 6x10 -> 3x5 with B = 2, 5x7 -> 3x4 (the ceil output).
# 1x1: the level5 root 1280 -> 512 (ten groups of 128 input channels), the level3 root 448 -> 128, a project (no mask) 256 -> 512.
# Slices: x, y, g and da each at a nonzero 32-channel offset of a wider buffer with poisoned neighbours, f32 with a pitch and as planes.
SEAM_CASES = {
    "s1_1x1_mask_add_res": (dict(hw=(1, 1), B=1, Cin=64, Cout=64, ksize=3, stride=1, seed=1, with_add=True, with_res=True), dict()),
    "s1_1x257_f16": (dict(hw=(1, 257), B=1, Cin=64, Cout=64, ksize=3, stride=1, seed=2), dict(x_storage="f16x2", x_scale=16.0)),
    "s1_3x5_b2_c512": (dict(hw=(3, 5), B=2, Cin=512, Cout=512, ksize=3, stride=1, seed=3, with_add=True), dict(x_storage="bf16x3")),
    "s2_2x2": (dict(hw=(2, 2), B=1, Cin=32, Cout=64, ksize=3, stride=2, seed=4), dict()),
    "s2_6x10_b2_x_f32_y_f16": (dict(hw=(6, 10), B=2, Cin=64, Cout=128, ksize=3, stride=2, seed=5, with_add=True),
                               dict(x_storage="f32", y_storage="f16x2", y_scale=16.0)),
    "s2_5x7_f16s1": (dict(hw=(5, 7), B=1, Cin=32, Cout=32, ksize=3, stride=2, seed=6), dict(x_storage="f16x2", x_scale=1.0)),
    "root5_c1280_o512_65px": (dict(hw=(1, 65), B=1, Cin=1280, Cout=512, ksize=1, stride=1, seed=7), dict(x_storage="f16x2", x_scale=16.0)),
    "root3_c448_o128_5x13": (dict(hw=(5, 13), B=1, Cin=448, Cout=128, ksize=1, stride=1, seed=8), dict()),
    "project_c256_o512_63px": (dict(hw=(1, 63), B=1, Cin=256, Cout=512, ksize=1, stride=1, seed=9, with_y=False, with_add=True), dict(x_storage="bf16x3")),
    "slices_f32": (dict(hw=(4, 6), B=2, Cin=64, Cout=32, ksize=3, stride=1, seed=10, with_add=True, with_res=True),
                   dict(x_c0=32, y_c0=64, g_c0=32, da_c0=96)),
    "slices_f16": (dict(hw=(4, 6), B=2, Cin=64, Cout=32, ksize=3, stride=1, seed=11, with_res=True),
                   dict(x_storage="f16x2", x_scale=16.0, x_c0=64, y_c0=32, g_c0=64, da_c0=32)),
    "slices_bf16x3_s2": (dict(hw=(6, 10), B=1, Cin=32, Cout=64, ksize=3, stride=2, seed=12, with_add=True),
                         dict(x_storage="bf16x3", x_c0=32, y_c0=96, g_c0=32, da_c0=64)),
}


@pytest.mark.parametrize("name", list(SEAM_CASES))
def test_seam_against_oracle(hiplib, name):
    kw, run = SEAM_CASES[name]
    case = BC.ConvCase(**kw)
    got, lay, dec = run_seam(case, **run)
    frame_ok(lay, own_da=run.get("da_c0") is None)
    check(got, case.ref(torch.float64, **dec), case.ref(torch.float32, **dec), name)
    again, _, _ = run_seam(case, **run)
    assert same_bits(again, got), name  # the same call twice: the same bits


def test_root_gradient_written_whole_is_read_back_by_slices(hiplib):
    """level3.tree2.root: the input gradient over [x2 | x1 | bottom | t1] (128 + 128 + 64 + 128 channels) is written once; each consumer
    reads its slice through the pointer of the slice's first channel and the buffer's pitch."""
    case = BC.ConvCase(hw=(5, 13), B=1, Cin=448, Cout=128, ksize=1, stride=1, seed=8)
    got, lay, dec = run_seam(case)
    ref = case.ref(torch.float64, **dec)["da"]
    ref32 = case.ref(torch.float32, **dec)["da"]
    for c0, n in ((0, 128), (128, 128), (256, 64), (320, 128)):
        sl = lay.da[..., c0:c0 + n]
        assert sl.data_ptr() == lay.da.data_ptr() + 4 * c0 and sl.stride(-2) == 448
        check({"da": sl.permute(0, 3, 1, 2).cpu()}, {"da": ref[:, c0:c0 + n]}, {"da": ref32[:, c0:c0 + n]}, f"root3 slice {c0}", families=("input", ))


def test_all_non_positive_output_gives_exact_zeros(hiplib):
    case = BC.ConvCase(hw=(3, 5), B=2, Cin=32, Cout=64, ksize=3, stride=1, seed=21, with_add=True, negative_y=True)
    case.y[0, 0, 0, 0] = 0.0  # an entry ON the clamp is masked too
    got, lay, _ = run_seam(case)
    frame_ok(lay)
    assert all(float(got[k].abs().max()) == 0.0 for k in ("dw", "dw_level", "q", "r"))
    assert torch.equal(got["da"], case.add)  # da = add + 0, bit for bit
    without, _, _ = run_seam(case, add=False)
    assert float(without["da"].abs().max()) == 0.0


def test_zero_scale_gives_exact_zero_filter_and_input_gradients(hiplib):
    case = BC.ConvCase(hw=(3, 5), B=2, Cin=32, Cout=64, ksize=3, stride=1, seed=22, zero_scale=True)
    got, lay, _ = run_seam(case)
    frame_ok(lay)
    assert float(got["dw"].abs().max()) == 0.0 and float(got["da"].abs().max()) == 0.0 and float(got["r"].abs().max()) > 0.0


def test_tile_choice_and_previous_contents_do_not_change_the_bits(hiplib):
    case = BC.ConvCase(hw=(12, 40), B=2, Cin=288, Cout=64, ksize=3, stride=2, seed=23, with_add=True, with_res=True)
    auto, _, _ = run_seam(case)
    for rows, group in ((2, 128), (2, 256), (4, 256), (8, 128), (8, 256)):
        forced, lay, _ = run_seam(case, dgrad_rows=rows, dgrad_group=group, fill=7.5)
        frame_ok(lay, 7.5)
        assert same_bits(forced, auto), (rows, group)


# ------------------------------------------------------------------------------------------------------------------- pool backward
def run_pool(x, g, storage="f32", plane_scale=1.0, add=None, res=None, c0=0, fill=SENTINEL):
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import PoolGrads
    B, C_, H, W = x.shape
    xb, xbind, xdec = store(x, storage, plane_scale, c0)
    gb, gv = wide(g, c0) if g is not None else (None, None)
    ab, av = wide(add, 0) if add is not None else (None, None)
    rgb, rgv = wide(res[0], 32) if res is not None else (None, None)
    ryb, rybind, rydec = store(res[1], storage, plane_scale, 32) if res is not None else (None, None, None)
    lay = PoolGrads("cuda", B, H, W, C_, xbind, gv, add=av, res=(rgv, rybind) if res is not None else None, fill=fill, guard=64)
    lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    assert lay.guards_intact(fill) and not bool((lay.da == fill).any())
    return lay.da.permute(0, 3, 1, 2).cpu(), xdec, rydec


POOL_CASES = {
    "2x2_random_c32": ("random", 1, 32, (2, 2), "f32", 1.0, False),
    "2x2_equal_c32_add": ("equal", 1, 32, (2, 2), "f32", 1.0, True),
    "2x2_two_max_c32": ("two_max", 1, 32, (2, 2), "f16x2", 16.0, False),
    "4x6_b2_two_max_c512_add": ("two_max", 2, 512, (4, 6), "bf16x3", 1.0, True),
    "4x6_b2_relu_c32_add_f16s1": ("relu", 2, 32, (4, 6), "f16x2", 1.0, True),
    "4x6_b2_equal_c512": ("equal", 2, 512, (4, 6), "f32", 1.0, False),
}


@pytest.mark.parametrize("name", list(POOL_CASES))
def test_pool_backward_is_bit_exact(hiplib, name):
    kind, B, C_, hw, storage, scale, with_add = POOL_CASES[name]
    gen = torch.Generator().manual_seed(91)
    x = BC.pool_input(kind, B, C_, hw, seed=90)
    g = torch.randn(B, C_, hw[0] // 2, hw[1] // 2, generator=gen)
    add = torch.randn(B, C_, hw[0], hw[1], generator=gen) if with_add else None
    got, xdec, _ = run_pool(x, g, storage, scale, add=add, c0=32 if storage != "f32" else 0)
    assert torch.equal(got, BO.pool_backward(xdec, g, torch.float32, add=add)), name
    if kind in ("equal", "two_max"):  # the first maximum in the order (0,0), (0,1), (1,0), (1,1) takes it all
        first = (0, 0) if kind == "equal" else (0, 1)
        base = add if add is not None else torch.zeros_like(got)
        for i in range(2):
            for j in range(2):
                want = base[:, :, i::2, j::2] + (g if (i, j) == first else 0.0)
                assert torch.equal(got[:, :, i::2, j::2], want), (name, i, j)
    again, _, _ = run_pool(x, g, storage, scale, add=add, c0=32 if storage != "f32" else 0, fill=7.5)
    assert torch.equal(again, got)


def test_pool_backward_with_a_masked_residual_part(hiplib):
    """A strided tree without a project: G_bottom = D_cat[bottom] + G_x1 * [x1 > 0], added before the selection."""
    gen = torch.Generator().manual_seed(92)
    x = BC.pool_input("relu", 2, 64, (4, 6), seed=93)
    g, rg, ry = (torch.randn(2, 64, 2, 3, generator=gen) for _ in range(3))
    add = torch.randn(2, 64, 4, 6, generator=gen)
    got, xdec, rydec = run_pool(x, g, "f16x2", 16.0, add=add, res=(rg, ry), c0=32)
    assert torch.equal(got, BO.pool_backward(xdec, g, torch.float32, add=add, res=(rg, rydec)))
    alone, xdec, rydec = run_pool(x, None, "f32", 1.0, res=(rg, ry))
    assert torch.equal(alone, BO.pool_backward(xdec, None, torch.float32, res=(rg, rydec)))


# ---------------------------------------------------------------------------------------------------------------------- mini DLA
def _mini_chain(dla, S, G, storage="f32", fill=SENTINEL):
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import dla_backward, dla_param_grads
    B = S["level1"].shape[0]
    keep, acts = [], {}
    for k, v in S.items():
        buf, bind, dec = store(v, storage)
        assert torch.equal(dec, v)  # (bf16x3 decodes exactly: the oracle's stored activations are the kernels')
        keep.append(buf)
        acts[k] = (bind, v.shape[2], v.shape[3], v.shape[1])
    Gd = {k: wide(v, 0, 0)[0] for k, v in G.items()}
    layers, g1 = dla_backward("cuda", B, dla, Gd, acts, lambda t: t.detach().float().contiguous().cuda(), fill=fill, guard=64)
    for lay in layers.values():
        lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    for lay in layers.values():
        assert lay.guards_intact(fill) and not bool((lay.da == fill).any())
    named = {id(p): f"backbone.bottom_up.{k}" for k, p in dla.named_parameters()}
    return {k: v.cpu() for k, v in dla_param_grads(named, layers).items()}, g1.permute(0, 3, 1, 2).cpu(), layers, keep


def check_named(params, g1, ref64, ref32, what):
    fams = {}
    for k in sorted(params):
        fams.setdefault(BO.family_of(k), []).append(k)
    rows = [(fam, [params[k] for k in ks], [ref64[0][k] for k in ks], [ref32[0][k] for k in ks]) for fam, ks in fams.items()]
    rows.append(("input", [g1], [ref64[1]], [ref32[1]]))
    for fam, c, a, b in rows:
        c, a, b = (torch.cat([v.reshape(-1).cpu() for v in vs]) for vs in (c, a, b))
        bar, d32, gmax = BO.bar(a.double(), b, torch.ones(a.shape[0], dtype=torch.bool))
        dev = float((c.double() - a.double()).abs().max())
        use = 8 * dev / bar if bar > 0 else 0.0
        WORST[fam] = max(WORST.get(fam, 0.0), use)
        print(f"[backbone_grads] {what} named {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8; "
              f"worst so far {WORST[fam]:.2f})")
        assert dev <= bar and gmax > 0.0, (what, fam, dev, bar)


@pytest.mark.parametrize("norm,storage", [("BN", "f32"), ("FrozenBN", "bf16x3"), ("", "f32")])
def test_mini_dla_chain(hiplib, norm, storage):
    """Channels 32/32/64/64/96/128 on a 32 x 64 level1 tensor, B = 2: a depth-1 tree with a project, a depth-2 level_root tree without
    one (the pooled tensor is the residual), one with, a depth-1 level_root tree -- the whole chain through engine.losses.dla_backward."""
    dla = BC.mini_dla(norm)
    level1, G = BC.mini_inputs(dla, 2, (32, 64))
    S = BO.stored_activations(dla, level1)
    params, g1, layers, _ = _mini_chain(dla, S, G, storage)
    named = dict(dla.named_parameters())
    assert sorted(params) == BO.param_names(dla) and all(params[k].shape == named[k[len("backbone.bottom_up."):]].shape for k in params)
    r64, r32 = BO.chain_grads(dla, S, G, torch.float64), BO.chain_grads(dla, S, G, torch.float32)
    check_named(params, g1, r64, r32, f"mini:{norm or 'none'}:{storage}")
    for key, lay in layers.items():  # the pools: a selection and float32 adds, bit for bit the float32 chain's
        if key.endswith(".pool"):
            g, add, res = lay.keep
            ref = BO.pool_backward(S[lay.src["x"][0]][:, lay.src["x"][1]:lay.src["x"][1] + lay.C], g.permute(0, 3, 1, 2).cpu() if g is not None else None,
                                   torch.float32, add=add.permute(0, 3, 1, 2).cpu(),
                                   res=(res[0].permute(0, 3, 1, 2).cpu(), S[lay.src["res_y"][0]][:, lay.src["res_y"][1]:lay.src["res_y"][1] + lay.C])
                                   if res is not None else None)
            assert torch.equal(lay.da.permute(0, 3, 1, 2).cpu(), ref), key
    again, g2, _, _ = _mini_chain(dla, S, G, storage, fill=7.5)
    assert all(torch.equal(again[k], params[k]) for k in params) and torch.equal(g2, g1)


def test_mini_dla_zero_upstream_gives_exact_zeros(hiplib):
    """An all-zero gradient at level3 .. level5 (no loss term reaches the backbone): every dw, dw_level, q, r, every handed-over gradient
    and the level1 gradient are exact zeros, whatever the scales, filters and stored activations hold."""
    dla = BC.mini_dla("BN")
    level1, G = BC.mini_inputs(dla, 2, (32, 64))
    S = BO.stored_activations(dla, level1)
    params, g1, layers, _ = _mini_chain(dla, S, {k: torch.zeros_like(v) for k, v in G.items()})
    assert float(g1.abs().max()) == 0.0 and sorted(params) == BO.param_names(dla)
    assert all(float(v.abs().max()) == 0.0 for v in params.values())
    for key, lay in layers.items():
        assert float(lay.da.abs().max()) == 0.0, key
        if not key.endswith(".pool"):
            assert all(float(t.abs().max()) == 0.0 for t in (lay.dw, lay.dw_level, lay.q, lay.r)), key


# -------------------------------------------------------------------------------------------------------------------- arguments
def test_bad_arguments_are_rejected(hiplib):
    from dd3d_amd import hip
    case = BC.ConvCase(hw=(6, 20), B=1, Cin=32, Cout=32, ksize=3, stride=1, seed=51, with_add=True, with_res=True)
    _, lay, _ = run_seam(case)
    lib, st = hip.lib(), hip.current_stream()
    a = lay.args
    both = (("dd3d_backbone_wgrad", lib.dd3d_backbone_wgrad), ("dd3d_backbone_dgrad", lib.dd3d_backbone_dgrad))
    for field, value, entries in (("Cin", 48, both), ("Cin", 1312, both), ("Cout", 16, both), ("Cout", 544, both), ("stride", 3, both), ("stride", 0, both),
                                  ("ksize", 2, both), ("ksize", 5, both), ("g_pitch", 34, both), ("g_pitch", 28, both), ("x_pitch", 34, both[:1]),
                                  ("x_pitch", 28, both[:1]), ("y_pitch", 28, both), ("x_mode", 7, both[:1]), ("y_mode", 7, both), ("res_y_mode", 7, both[1:]),
                                  ("res_y_pitch", 28, both[1:]), ("add_pitch", 28, both[1:]), ("res_pitch", 30, both[1:]), ("da_pitch", 28, both[1:]),
                                  ("n_slices", 0, both[:1]), ("dgrad_rows", 3, both), ("dgrad_group", 64, both), ("B", 0, both), ("H", 0, both)):
        old = getattr(a, field)
        setattr(a, field, value)
        for name, fn in entries:
            assert fn(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(name), (field, name)
        setattr(a, field, old)
    for field, entries in (("g", both), ("w", both), ("scale", both), ("x", both[:1]), ("da", both[1:]), ("res_y", both[1:]), ("part", both[:1]),
                           ("qpart", both[:1]), ("dw_level", both[:1]), ("dw", both[:1]), ("q", both[:1]), ("r", both[:1])):
        old = getattr(a, field)
        setattr(a, field, None)
        for name, fn in entries:
            assert fn(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(name), (field, name)
        setattr(a, field, old)
    assert lib.dd3d_backbone_grad_slices(None) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_backbone_grad_slices")
    assert lib.dd3d_backbone_wgrad(None, st) == -1 and lib.dd3d_backbone_dgrad(None, st) == -1
    assert lib.dd3d_backbone_wgrad(C.byref(a), st) == 0 and lib.dd3d_backbone_dgrad(C.byref(a), st) == 0  # the restored arguments still run
    torch.cuda.synchronize()
    frame_ok(lay)
    x = BC.pool_input("random", 1, 32, (4, 6))
    p = hip.PoolGradArgs()
    g = torch.zeros(1, 2, 3, 32, device="cuda")
    xb, da = wide(x)[0], torch.zeros(1, 4, 6, 32, device="cuda")
    p.x, p.g, p.da, p.B, p.H, p.W, p.C = xb.data_ptr(), g.data_ptr(), da.data_ptr(), 1, 4, 6, 32
    p.x_mode, p.x_pitch, p.g_pitch, p.da_pitch, p.x_plane_scale, p.res_y_plane_scale = hip.PG_ACT_F32, 36, 32, 32, 1.0, 1.0
    assert lib.dd3d_maxpool2x2_backward(C.byref(p), st) == 0
    for field, value in (("H", 5), ("W", 3), ("C", 48), ("C", 1312), ("x_mode", 9), ("x_pitch", 28), ("g_pitch", 30), ("da_pitch", 16), ("B", 0), ("x", None),
                         ("g", None), ("da", None)):
        old = getattr(p, field)
        setattr(p, field, value)
        assert lib.dd3d_maxpool2x2_backward(C.byref(p), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_maxpool2x2_backward"), field
        setattr(p, field, old)
    assert lib.dd3d_maxpool2x2_backward(None, st) == -1
    torch.cuda.synchronize()


def test_slice_count_is_a_pure_shape_query(hiplib):
    from dd3d_amd import hip
    bare = hip.BackboneGradArgs()  # the geometry, the channel counts and the convolution's form alone: no pointer is set
    for (B, h, w, ci, co, k, s) in ((1, 1, 1, 64, 64, 3, 1), (2, 12, 40, 64, 128, 3, 2), (1, 12, 40, 1280, 512, 1, 1), (1, 1, 257, 64, 64, 3, 1),
                                    (4, 24, 80, 512, 512, 3, 1), (6, 56, 100, 256, 256, 3, 1), (6, 224, 400, 64, 64, 3, 1)):
        bare.B, bare.H, bare.W, bare.Cin, bare.Cout, bare.ksize, bare.stride = B, h, w, ci, co, k, s
        n = hiplib.dd3d_backbone_grad_slices(C.byref(bare))
        assert n == hip.backbone_grad_slices(B, h, w, ci, co, k, s) and n * co * k * k * ci * 4 <= hip.TG_SLAB_BYTES, (B, h, w, ci, co, k, s)
    assert hip.backbone_grad_slices(1, 1, 1, 64, 64, 3, 1) == 1 and hip.backbone_grad_slices(2, 12, 40, 64, 128, 3, 2) == 3
    assert hip.backbone_grad_slices(4, 24, 80, 512, 512, 3, 1) == 16  # the slab's byte budget decides: at most 17 slices of 9.4 MB, 12 units each
    bare.ksize = 2
    assert hiplib.dd3d_backbone_grad_slices(C.byref(bare)) == -1 and hiplib.dd3d_last_error().decode().startswith("dd3d_backbone_grad_slices")


# ---------------------------------------------------------------------------------------------------------------------- end to end
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
    ref_losses, ref_grads, ref_params = model.compute_losses(inputs, fpn_grads=True)
    losses, grads, params = model.compute_losses(inputs, backbone_grads=True)
    # the loss dict and everything the FPN backward returns are those of fpn_grads=True, bit for bit
    assert list(losses) == list(ref_losses) and all(torch.equal(losses[k], ref_losses[k]) for k in losses)
    assert all(torch.equal(grads[k], ref_grads[k]) for k in ref_grads) and all(torch.equal(params[k], ref_params[k]) for k in ref_params)
    plan = model.get_loss_plan(*model.canvas_size(inputs), backbone_grads=True)
    dla = model.backbone.bottom_up
    cpu = GC.cpu_model(exp)
    cpu.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    cdla = cpu.backbone.bottom_up
    new_g, new_p = {k: v for k, v in grads.items() if k not in ref_grads}, {k: v.cpu() for k, v in params.items() if k not in ref_params}
    assert list(new_g) == ["backbone_level1"] and sorted(new_p) == BO.param_names(cdla)
    g1 = new_g["backbone_level1"]
    assert g1.shape == (B, dla.channels[1], plan.Hp // 2, plan.Wp // 2) and g1.dtype == torch.float32
    named = dict(cpu.named_parameters())
    assert all(v.shape == named[k].shape and v.dtype == torch.float32 for k, v in new_p.items())
    bufname = lambda key: f"level1.{len(dla.level1) - 1}" if key == "level1" else key
    T = lambda ref: decode(plan.bufs[bufname(ref[0])], ref[1], ref[2]) if ref is not None else None
    nchw = lambda t: t.permute(0, 3, 1, 2).cpu() if t is not None else None
    # every call: the raw outputs against the layer oracle fed the plan's own stored input and the gradient the call itself read
    S = {}
    for key, lay in plan.backbone_layers.items():
        assert lay.guards_intact(0.0)
        for ref in lay.src.values():
            if ref is not None and ref[0] not in S:
                S[ref[0]] = decode(plan.bufs[bufname(ref[0])])
        if key.endswith(".pool"):
            g, add, res = lay.keep
            assert res is None
            assert torch.equal(nchw(lay.da), BO.pool_backward(T(lay.src["x"]), nchw(g), torch.float32, add=nchw(add))), key
            continue
        g, w, scale, add, res, _ = lay.keep
        ref = {dt: BO.layer_grads(T(lay.src["x"]), T(lay.src["y"]), nchw(g), w.permute(0, 3, 1, 2).cpu(), scale.cpu(), lay.stride, dt, add=nchw(add),
                                  res=(nchw(res[0]), T(lay.src["res_y"])) if res is not None else None) for dt in (torch.float64, torch.float32)}
        check(collect(lay), ref[torch.float64], ref[torch.float32], f"e2e:{ds}:{key}")
    # the named parameters and the gradient at level1 against the chain oracle on the plan's stored activations
    G = {n: grads[f"backbone_{n}"].cpu() for n in model.backbone.in_features}
    r64, r32 = BO.chain_grads(cdla, S, G, torch.float64), BO.chain_grads(cdla, S, G, torch.float32)
    check_named(new_p, g1.cpu(), r64, r32, f"e2e:{ds}")
    # a second call is bit-equal; the captured graph equals launch-by-launch execution
    _, g2, p2 = model.compute_losses(inputs, backbone_grads=True)
    assert all(torch.equal(g2[k], grads[k]) for k in grads) and all(torch.equal(p2[k], params[k]) for k in params)
    names = [op.name for op in plan.ops]
    model.use_graph = False
    model.invalidate_plans()
    l3, g3, p3 = model.compute_losses(inputs, backbone_grads=True)
    assert all(torch.equal(l3[k], losses[k]) for k in losses)
    assert all(torch.equal(g3[k], grads[k]) for k in grads) and all(torch.equal(p3[k], params[k]) for k in params)
    return model, plan, names


def test_compute_losses_backbone_grads_kitti_dla34(hiplib):
    from dd3d_amd import hip
    model, plan, names = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti")
    first = names.index("backbone_grads.level5.root")
    assert names[first - 1] == "fpn_grads.lateral3" and all(n.startswith("backbone_grads.") for n in names[first:]) and names[-1] == "backbone_grads.level2.pool"
    a = plan.backbone_layers["level5.root"].args
    assert a.x_mode == hip.PG_ACT_F16X2 and a.x_plane_scale == 16.0 and a.Cin == 1280 and a.Cout == 512


def test_compute_losses_backbone_grads_bf16x3(hiplib):
    from dd3d_amd import hip
    _, plan, _ = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti", math="bf16x3")
    assert plan.backbone_layers["level2.tree1.conv1"].args.x_mode == hip.PG_ACT_BF16X3 and not plan.fused_stem


def test_compute_losses_backbone_grads_plane_scale_1(hiplib):
    _, plan, _ = _end_to_end("dd3d_kitti_dla34", "dla34_kitti", 2, 128, 384, "kitti", act_scale=1.0)
    assert plan.backbone_layers["level5.root"].args.x_plane_scale == 1.0


def test_compute_losses_backbone_grads_nusc_dla34(hiplib):
    _end_to_end("dd3d_nusc_dla34", "dla34_nusc", 6, 128, 224, "nusc")


def test_no_positives_gives_finite_results_and_exact_zeros(hiplib):
    from dd3d_amd.synthetic import make_gt_instances, make_inputs
    from tests.test_loss_grads_gpu import _model
    model = _model("dd3d_kitti_dla34", "dla34_kitti")
    inputs = make_inputs(2, 128, 384, dataset="kitti")
    for x, g in zip(inputs, make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, empty_images=(0, 1))):
        x["instances"] = g
    _, fg, fp = model.compute_losses(inputs, fpn_grads=True)
    _, grads, params = model.compute_losses(inputs, backbone_grads=True)
    assert all(bool(torch.isfinite(v).all()) for v in list(grads.values()) + list(params.values()))
    assert all(torch.equal(grads[k], fg[k]) for k in fg) and all(torch.equal(params[k], fp[k]) for k in fp)
    if all(float(fg[f"backbone_level{l}"].abs().max()) == 0.0 for l in (3, 4, 5)):  # (the classification loss has a gradient without positives too)
        assert float(grads["backbone_level1"].abs().max()) == 0.0
        assert all(float(v.abs().max()) == 0.0 for k, v in params.items() if k.startswith("backbone.bottom_up."))


def test_unsupported_models_name_themselves(hiplib):
    from tests.test_loss_grads_gpu import _model
    model = _model("dd3d_kitti_dla34", "dla34_kitti")
    model.math = "bf16x2"
    with pytest.raises(NotImplementedError, match="bf16x2"):
        model.get_loss_plan(1, 128, 128, backbone_grads=True)
    v99 = _model("dd3d_kitti_v99", "v99_kitti")
    with pytest.raises(NotImplementedError, match="V2-99"):
        v99.get_loss_plan(1, 128, 128, backbone_grads=True)
