"""Batch-statistics BN of the FPN on the MI355X at the C-ABI seam (csrc/fpn_bn.hip): dd3d_bn_apply_topdown_split,
dd3d_bn_backward_reduce_linear and dd3d_bn_backward_apply_linear called directly on synthetic c and G, at 32 and 256 channels.

Chains (finest segment first, every segment linked to the next): three stages (8,12) / (4,6) / (2,3) at B = 2; three stages (20,12) /
(10,6) / (5,3) at B = 1 -- N = 240 / 60 / 15: no multiple of the 64-pixel slice, one of them below it --; four stages (16,8) .. (2,1)
at B = 1; and one call of unlinked segments with differing N.

Bars: loss_grad_oracle.bar = 8 * max(d32, 2^-23 * max|ref64|), d32 the deviation of torch-CPU float32 (F.batch_norm, nearest
interpolation, autograd) from float64 on the same inputs.  The plane storages are compared bit for bit with the f32 output passed
through dd3d_split_planes(relu=False); the maskless backward bit for bit with the masked entry points fed a y of ones."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import tower_bn_oracle as BO
from tests.test_tower_bn_gpu import EPS, SENTINEL, SHAPES, Layer, framed, intact

pytestmark = pytest.mark.gpu

CHAINS = {
    "b2x3": [(2, 8, 12), (2, 4, 6), (2, 2, 3)],
    "odd3": [(1, 20, 12), (1, 10, 6), (1, 5, 3)],
    "deep4": [(1, 16, 8), (1, 8, 4), (1, 4, 2), (1, 2, 1)],
}
UNLINKED = [(2, 3, 5), (1, 8, 8), (1, 20, 12)]
WORST = {}


def linked(n):
    return list(range(1, n)) + [-1]


def within(got, ref64, ref32, what):
    bar, d32, gmax = BO.bar(ref64.reshape(-1), ref32.reshape(-1), torch.ones(ref64.numel(), dtype=torch.bool))
    dev = float((got.double() - ref64).abs().max())
    assert bool(torch.isfinite(got).all()), what
    use = 8 * dev / bar if bar > 0 else 0.0
    fam = what.split(":")[-1]
    WORST[fam] = max(WORST.get(fam, 0.0), use)
    print(f"[fpn_bn] {what}: max|ref64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
    assert dev <= bar, (what, dev, bar, d32, gmax)


def fpn_args(lay, up):
    """dd3d_fpn_bn_args around a copy of the layer's dd3d_tower_bn_args."""
    from dd3d_amd import hip
    f = hip.FpnBnArgs()
    C.memmove(C.addressof(f.bn), C.addressof(lay.args), C.sizeof(hip.TowerBnArgs))
    for s, (B, h, w) in enumerate(lay.shapes):
        f.up[s], f.B[s], f.H[s], f.W[s] = up[s], B, h, w
    return f


def apply(lay, up, f=None):
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    f = f or fpn_args(lay, up)
    hip.check(lib.dd3d_bn_batch_stats(C.byref(lay.args), st), "bn_batch_stats")
    hip.check(lib.dd3d_bn_apply_topdown_split(C.byref(f), st), "bn_apply_topdown_split")
    torch.cuda.synchronize()
    return f


def topdown_oracle(lay, up, dtype):
    """y of every segment: n_l = F.batch_norm(c_l, training=True), plus the nearest-x2 upsampled y of the coarser segment."""
    ys = [None] * lay.S
    for s in reversed(range(lay.S)):
        n = F.batch_norm(lay.c[s].to(dtype), None, None, lay.gamma[s].to(dtype), lay.beta[s].to(dtype), training=True, eps=EPS)
        ys[s] = n if up[s] < 0 else n + F.interpolate(ys[up[s]], scale_factor=2, mode="nearest")
    return ys


def cases():
    return [(k, v, linked(len(v))) for k, v in CHAINS.items()] + [("unlinked", UNLINKED, [-1] * len(UNLINKED))]


@pytest.mark.parametrize("Cn,col,pitch", [(32, 0, None), (256, 256, 512)])
@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_apply_against_the_oracle(hiplib, Cn, col, pitch, case):
    name, shapes, up = case
    lay = Layer(Cn, "f32", col=col, pitch=pitch, seed=Cn + len(shapes), shapes=shapes)
    apply(lay, up)
    y64, y32 = topdown_oracle(lay, up, torch.float64), topdown_oracle(lay, up, torch.float32)
    negative = False
    for s in range(lay.S):
        y = lay.y_decoded(s)
        within(y, y64[s], y32[s], f"{name}:C{Cn}:N{lay.N[s]}:y")
        # channel 5 is constant over the batch in every segment: beta, plus the coarser segments' betas, coarsest first -- exactly
        want, chain = None, [s]
        while up[chain[-1]] >= 0:
            chain.append(up[chain[-1]])
        for u in reversed(chain):
            want = lay.beta[u][5] if want is None else want + lay.beta[u][5]
        assert bool((y[:, 5] == want).all()), (name, s)
        negative |= bool((y < 0).any())
    assert negative  # no ReLU
    assert intact(lay.frames()) and int(lay.status) == 0
    first = [f[1].clone() for f in lay.y]
    for f in lay.y:
        f[1].fill_(SENTINEL)
    apply(lay, up)
    assert all(torch.equal(a, f[1]) for a, f in zip(first, lay.y))


@pytest.mark.parametrize("Cn", [32, 256])
@pytest.mark.parametrize("storage,scale", [("f16x2", 16.0), ("f16x2", 1.0), ("bf16x3", 1.0)])
def test_plane_storages_are_the_bits_of_split_planes(hiplib, Cn, storage, scale):
    """Every plane storage against the two-step statement: the f32 form of the same call, then dd3d_split_planes(relu=False) -- equal
    bits and the same status word; the optional f32 copy beside the planes is the f32 form's output.  At plane scale 16 a value past
    the half range (|y| > 4094) sets the overflow bit in both."""
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    for name, shapes, up in cases():
        for gain in ((1.0, 4000.0) if name == "b2x3" else (1.0, )):
            fused = Layer(Cn, storage, seed=3, gain=gain, plane_scale=scale, shapes=shapes)
            plain = Layer(Cn, "f32", seed=3, gain=gain, shapes=shapes)
            f = fpn_args(fused, up)
            copies = [framed(n * Cn) for n in fused.N]
            for s in range(fused.S):
                f.y32[s] = copies[s][1].data_ptr()
            f.y32_pitch = Cn
            apply(fused, up, f), apply(plain, up)
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            for s in range(plain.S):
                full, planes = framed(plain.N[s] * Cn * fused.np, torch.int16, fill=-12345)
                hip.check(lib.dd3d_split_planes(plain.y[s][1].data_ptr(), planes.data_ptr(), plain.N[s], Cn, Cn, fused.math, 0, scale, status.data_ptr(), st),
                          "split")
                torch.cuda.synchronize()
                assert torch.equal(planes, fused.y[s][1]), (name, storage, gain, s)
                assert torch.equal(copies[s][1], plain.y[s][1]), (name, storage, gain, s)
            big = max(float(y[1].abs().max()) for y in plain.y)
            expect = hip.STATUS_F16_OVERFLOW if storage == "f16x2" and big * scale > 65504.0 else 0
            assert gain == 1.0 or big > 4094.0
            assert (gain == 1.0 or scale != 16.0 or storage != "f16x2") or expect == hip.STATUS_F16_OVERFLOW
            assert int(status) == int(fused.status) == expect and int(plain.status) == 0
            assert all(bool((full[view.numel():] == -12345).all()) for full, view in fused.y) and intact(copies)


def test_apply_rejects_bad_links_and_null_pointers(hiplib):
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    name = "dd3d_bn_apply_topdown_split"
    shapes = CHAINS["b2x3"]
    lay = Layer(32, "f16x2", shapes=shapes)
    f = apply(lay, linked(3))
    before = [y[1].clone() for y in lay.y]

    def refused(what):
        assert lib.dd3d_bn_apply_topdown_split(C.byref(f), st) == -1 and lib.dd3d_last_error().decode().startswith(name), what

    for arr, idx, bad in ((f.H, 1, 5), (f.W, 2, 4), (f.B, 1, 1), (f.up, 0, 0), (f.up, 1, 0), (f.up, 2, 3), (f.up, 0, -2), (f.bn.N, 0, 100),
                          (f.bn.c, 1, None), (f.bn.stats, 2, None), (f.bn.y, 0, None), (f.bn.beta, 1, None)):
        old = arr[idx]
        arr[idx] = bad
        refused((idx, bad))
        arr[idx] = old
    for field, bad in (("C", 48), ("C", 288), ("c_pitch", 30), ("num_segs", 0), ("math_mode", 9), ("plane_scale", 0.0)):
        old = getattr(f.bn, field)
        setattr(f.bn, field, bad)
        refused(field)
        setattr(f.bn, field, old)
    assert lib.dd3d_bn_apply_topdown_split(None, st) == -1 and lib.dd3d_last_error().decode().startswith(name)
    # a skipped stage is a link too: (8,12) -> (2,3) is no exact halving
    f.up[0] = 2
    refused("skip")
    f.up[0] = 1
    apply(lay, None, f)  # the restored arguments still run, to the same bits
    assert all(torch.equal(a, y[1]) for a, y in zip(before, lay.y))


def backward(lay, linear):
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    hip.check(lib.dd3d_bn_batch_stats(C.byref(lay.args), st), "bn_batch_stats")
    if linear:
        hip.check(lib.dd3d_bn_backward_reduce_linear(C.byref(lay.args), st), "bn_backward_reduce_linear")
        hip.check(lib.dd3d_bn_backward_apply_linear(C.byref(lay.args), st), "bn_backward_apply_linear")
    else:
        for y in lay.y:
            y[1].fill_(1.0)
        hip.check(lib.dd3d_bn_backward_reduce(C.byref(lay.args), st), "bn_backward_reduce")
        hip.check(lib.dd3d_bn_backward_apply(C.byref(lay.args), st), "bn_backward_apply")
    torch.cuda.synchronize()


@pytest.mark.parametrize("Cn,col,pitch", [(32, 0, None), (256, 256, 512)])
@pytest.mark.parametrize("shapes", list(CHAINS.values()) + [SHAPES], ids=list(CHAINS) + ["multi"])
def test_maskless_backward(hiplib, Cn, col, pitch, shapes):
    """qp and G_c of the two linear entry points: the bits of the masked ones fed an f32 y of ones, within the bar of float64 autograd
    through F.batch_norm(training=True), no word beyond the outputs written, equal bits over two runs.  The linear layer's own y is
    left at its sentinel and its y pointers are cleared: nothing is read there."""
    masked = Layer(Cn, "f32", col=col, pitch=pitch, seed=7 + Cn, shapes=shapes)
    lin = Layer(Cn, "f32", col=col, pitch=pitch, seed=7 + Cn, shapes=shapes)
    for s in range(lin.S):
        lin.args.y[s] = None
    lin.args.y_mode, lin.args.y_pitch, lin.args.plane_scale = -1, 0, 0.0
    backward(masked, False), backward(lin, True)
    for s in range(lin.S):
        assert torch.equal(lin.qp[s][1], masked.qp[s][1]) and torch.equal(lin.gc[s][1], masked.gc[s][1]), s
        B, h, w = shapes[s]
        ones = torch.ones(B, Cn, h, w)
        q64, p64, gc64 = BO.backward_autograd(lin.c[s], ones, lin.G[s], lin.gamma[s], lin.beta[s], EPS, torch.float64)
        q32, p32, gc32 = BO.backward_autograd(lin.c[s], ones, lin.G[s], lin.gamma[s], lin.beta[s], EPS, torch.float32)
        qp = lin.qp[s][1].view(2, Cn).cpu()
        gc = lin.gc[s][1].view(B, h, w, Cn).permute(0, 3, 1, 2).cpu()
        tag = f"linear:C{Cn}:N{lin.N[s]}"
        within(qp[0], q64, q32, tag + ":q"), within(qp[1], p64, p32, tag + ":p"), within(gc, gc64, gc32, tag + ":G_c")
    assert intact(lin.frames()) and all(bool((y[1] == SENTINEL).all()) for y in lin.y)
    first = [f[1].clone() for f in lin.qp + lin.gc]
    for f in lin.qp + lin.gc:
        f[1].fill_(SENTINEL)
    backward(lin, True)
    assert all(torch.equal(a, f[1]) for a, f in zip(first, lin.qp + lin.gc))


def test_linear_backward_rejects_bad_arguments(hiplib):
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    lay = Layer(32, "f32", shapes=SHAPES[:2])
    a = lay.args
    entries = [("dd3d_bn_backward_reduce_linear", lib.dd3d_bn_backward_reduce_linear), ("dd3d_bn_backward_apply_linear", lib.dd3d_bn_backward_apply_linear)]

    def refused(which, what):
        for name, fn in entries:
            if name in which:
                assert fn(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(name), (what, name)

    both = [n for n, _ in entries]
    for field, bad, which in (("C", 48, both), ("c_pitch", 30, both), ("g_pitch", 34, both), ("num_segs", 25, both), ("n_slices", 1, both[:1])):
        old = getattr(a, field)
        setattr(a, field, bad)
        refused(which, field)
        setattr(a, field, old)
    for field, which in (("c", both), ("stats", both), ("g", both), ("qp", both), ("gc", both[1:])):
        arr = getattr(a, field)
        old = arr[1]
        arr[1] = None
        refused(which, field)
        arr[1] = old
    assert lib.dd3d_bn_backward_reduce_linear(None, st) == -1 and lib.dd3d_bn_backward_apply_linear(None, st) == -1
    backward(lay, True)
    assert intact(lay.frames())


def test_worst_use_of_the_bar_is_reported(hiplib):
    """(Runs last in this file.)  The largest share of the factor 8 any comparison above used, per family: what profiles/fpn_bn_errors.txt records."""
    for k, v in sorted(WORST.items()):
        print(f"[fpn_bn] worst use of the factor 8, {k}: {v:.2f}")
    assert all(v <= 8.0 for v in WORST.values())
