"""Batch-statistics BN of the DLA-34 bottom-up network on the MI355X at the C-ABI seam (csrc/backbone_bn.hip): dd3d_backbone_bn_batch_stats,
dd3d_backbone_bn_apply and the four backward entry points called directly on synthetic c, r and G at C = 16, 32, 128 and 512.

Segments (B, h, w): (2, 3, 5), N = 30, below a slice; (1, 8, 8), N = 64, exactly one slice; (1, 20, 12), N = 240, no multiple of the
slice; (1, 40, 52) at C = 16, N = 2080: many slices, few channels; (2, 4, 4) at C = 512, the level5 shape.  Every output is written both
as a whole buffer and as the channel slice at column C of a pitch-2C buffer, in f32 and in both plane storages; the residual is read in
each of its three storages; channel 5 is constant over the batch (v = 0), channel 7's ReLU clips every pixel (beta = -100).

Bars: mu, v, the running statistics, y, q, p and G_c each within loss_grad_oracle.bar = 8 * max(d32, 2^-23 * max|ref64|), d32 the deviation
of torch-CPU float32 from float64 on the same inputs.  Bit for bit: the plane stores against the f32 output passed through
dd3d_split_planes; the maskless backward against the masked one fed a y of ones; at C = 32 and 128 the statistics and the backward against
the towers' entry points on the same input (the order of every sum is kept); two runs; sentinel frames around every output."""
import ctypes as C

import pytest
import torch

from tests import backbone_bn_oracle as BN
from tests.test_tower_bn_gpu import EPS, POISON, SENTINEL, framed, intact

pytestmark = pytest.mark.gpu

WIDTHS = (16, 32, 128, 512)
COMMON = [(2, 3, 5), (1, 8, 8), (1, 20, 12)]
WORST = {}


def shapes_of(Cn):
    return COMMON + ([(1, 40, 52)] if Cn == 16 else []) + ([(2, 4, 4)] if Cn == 512 else [])


def within(got, ref64, ref32, what):
    bar, d32, gmax = BN.bar(ref64.reshape(-1), ref32.reshape(-1), torch.ones(ref64.numel(), dtype=torch.bool))
    dev = float((got.double().cpu() - ref64).abs().max())
    assert bool(torch.isfinite(got).all()), what
    use = 8 * dev / bar if bar > 0 else 0.0
    fam = what.split(":")[-1]
    WORST[fam] = max(WORST.get(fam, 0.0), use)
    print(f"[backbone_bn] {what}: max|ref64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
    assert dev <= bar, (what, dev, bar, d32, gmax)


NP = {"f32": 0, "f16x2": 2, "bf16x3": 3}


def math_of(storage):
    from dd3d_amd import hip
    return {"f32": hip.MATH_F32, "f16x2": hip.MATH_F16X2, "bf16x3": hip.MATH_BF16X3}[storage]


def act_mode_of(storage):
    from dd3d_amd import hip
    return {"f32": hip.PG_ACT_F32, "f16x2": hip.PG_ACT_F16X2, "bf16x3": hip.PG_ACT_BF16X3}[storage]


def decode_planes(t, Cn, N, storage, scale):
    """(N, C) float32 values of a split-plane tensor [C/32][N][NP][32] of int16."""
    t = t.view(Cn // 32, N, NP[storage], 32)
    t = t.view(torch.float16).float() / scale if storage == "f16x2" else (t.to(torch.int32) << 16).view(torch.float32)
    x = t[:, :, 0]
    for q in range(1, NP[storage]):
        x = x + t[:, :, q]
    return x.permute(1, 0, 2).reshape(N, Cn).cpu()


class Stored:
    """A tensor (N, C) on the device in one storage, either whole or as the channel slice at column C of a buffer of 2C channels, inside a
    sentinel frame.  `values`: what to store (planes: through dd3d_split_planes), or None for an output."""
    def __init__(self, N, Cn, storage, sliced, scale=16.0, values=None):
        from dd3d_amd import hip
        self.N, self.C, self.storage, self.sliced, self.scale = N, Cn, storage, sliced, scale
        self.other = SENTINEL if storage == "f32" else -12345  # what the other half of a wide buffer holds
        wide = 2 * Cn if sliced else Cn
        if storage == "f32":
            self.full, self.view = framed(N * wide)
            self.pitch, self.ptr = wide, self.view.data_ptr() + (4 * Cn if sliced else 0)
            if values is not None:  # (an input: the other half of a wide buffer holds a value no kernel may read)
                t = torch.full((N, wide), POISON)
                t[:, wide - Cn:] = values
                self.view.copy_(t.reshape(-1).cuda())
                self.other = POISON
        else:
            np_ = NP[storage]
            self.full, self.view = framed(N * wide * np_, torch.int16, fill=-12345)
            self.pitch, self.ptr = 0, self.view.data_ptr() + (2 * (Cn // 32) * N * np_ * 32 if sliced else 0)
            if values is not None:
                src = values.contiguous().cuda()
                hip.check(hip.lib().dd3d_split_planes(src.data_ptr(), self.ptr, N, Cn, Cn, math_of(storage), 0, scale, None, hip.current_stream()), "split")
                torch.cuda.synchronize()

    def own(self):
        """The slice's own words (a flat view)."""
        if self.storage == "f32":
            return self.view.view(self.N, self.pitch)[:, self.pitch - self.C:]
        half = self.view.numel() // 2
        return self.view[half:] if self.sliced else self.view

    def decoded(self):
        if self.storage == "f32":
            return self.own().cpu().contiguous()
        return decode_planes(self.own().contiguous(), self.C, self.N, self.storage, self.scale)

    def rest_intact(self):
        """The frame behind the buffer and, for a slice, the other half of the wide buffer are untouched."""
        fill = SENTINEL if self.storage == "f32" else -12345
        ok = bool((self.full[self.view.numel():] == fill).all())
        if self.sliced:
            other = self.view.view(self.N, self.pitch)[:, :self.C] if self.storage == "f32" else self.view[:self.view.numel() // 2]
            ok = ok and bool((other == self.other).all())
        return ok

    def binding(self):
        return act_mode_of(self.storage), self.ptr, self.pitch, self.scale


class Seg:
    """One seeded segment and every device buffer of the calls; `sliced_c`: c is the channel slice at column C of a pitch-2C buffer (the
    gradient G always is)."""
    def __init__(self, Cn, shape, seed=0, gain=1.0, sliced_c=False):
        from dd3d_amd import hip
        gen = torch.Generator().manual_seed(seed)
        B, h, w = shape
        self.C, self.N = Cn, B * h * w
        N = self.N
        self.c = torch.randn(N, Cn, generator=gen) * 1.5 + 0.3
        self.c[:, 5] = 0.5  # constant over the batch: v = 0
        self.r = torch.randn(N, Cn, generator=gen)
        self.G = torch.randn(N, Cn, generator=gen)
        self.gamma, self.beta = (0.5 + torch.rand(Cn, generator=gen)) * gain, torch.randn(Cn, generator=gen) * 0.3 * gain
        self.beta[7] = -100.0  # this channel's ReLU clips every pixel, with or without the residual
        self.rm, self.rv = torch.randn(Cn, generator=gen) * 0.2, 0.5 + torch.rand(Cn, generator=gen)
        self.raw = Stored(N, Cn, "f32", sliced_c, values=self.c)
        self.g = Stored(N, Cn, "f32", True, values=self.G)
        self.vecs = [v.contiguous().cuda() for v in (self.gamma, self.beta, self.rm, self.rv)]
        self.stats, self.qp, self.gc = framed(hip.BN_STAT_ROWS * Cn), framed(2 * Cn), framed(N * Cn)
        self.n_slices = hip.bn_slices([N])
        self.part = framed(self.n_slices * 2 * Cn)
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        f = hip.BackboneBnArgs()
        a = f.bn
        a.c[0], a.g[0], a.N[0] = self.raw.ptr, self.g.ptr, N
        a.gamma[0], a.beta[0], a.run_mean[0], a.run_var[0] = (v.data_ptr() for v in self.vecs)
        a.stats[0], a.qp[0], a.gc[0] = self.stats[1].data_ptr(), self.qp[1].data_ptr(), self.gc[1].data_ptr()
        a.part, a.n_slices, a.status = self.part[1].data_ptr(), self.n_slices, self.status.data_ptr()
        a.num_segs, a.C, a.c_pitch, a.g_pitch = 1, Cn, self.raw.pitch, self.g.pitch
        a.eps, a.momentum, a.plane_scale = EPS, hip.BN_MOMENTUM, 16.0
        f.res_plane_scale = 1.0
        self.f, self.args = f, a

    def frames(self):
        return [self.stats, self.qp, self.gc, self.part]

    def statistics(self, entry="dd3d_backbone_bn_batch_stats"):
        from dd3d_amd import hip
        hip.check(getattr(hip.lib(), entry)(C.byref(self.args), hip.current_stream()), entry)
        torch.cuda.synchronize()

    def row(self, r):
        return self.stats[1].view(-1, self.C)[r].cpu()

    def apply(self, act, out, res=None, y32=None):
        """One dd3d_backbone_bn_apply into the Stored `out` (and the f32 Stored `y32` beside planes)."""
        from dd3d_amd import hip
        f, a = self.f, self.args
        f.act = act
        a.math_mode, a.plane_scale = math_of(out.storage), out.scale
        a.y[0], a.y_pitch = out.ptr, out.pitch
        f.y32[0], f.y32_pitch = (y32.ptr, y32.pitch) if y32 is not None else (None, 0)
        if res is not None:
            f.res_mode, f.res[0], f.res_pitch, f.res_plane_scale = res.binding()
        else:
            f.res[0] = None
        hip.check(hip.lib().dd3d_backbone_bn_apply(C.byref(f), hip.current_stream()), "backbone_bn_apply")
        torch.cuda.synchronize()

    def backward(self, y=None, linear=False, tower=False):
        """The masked backward with the Stored `y` as the mask, or the maskless one; `tower`: through the towers' entry points."""
        from dd3d_amd import hip
        lib, st, a = hip.lib(), hip.current_stream(), self.args
        if y is not None:
            a.y_mode, a.y[0], a.y_pitch, a.plane_scale = y.binding()
        else:
            a.y[0], a.y_mode = None, -1
        stem = "dd3d_bn_backward" if tower else "dd3d_backbone_bn_backward"
        for name in (stem + "_reduce", stem + "_apply"):
            name += "_linear" if linear else ""
            hip.check(getattr(lib, name)(C.byref(a), st), name)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- statistics and apply
@pytest.mark.parametrize("Cn", WIDTHS)
def test_statistics_and_apply_against_the_oracle(hiplib, Cn):
    from dd3d_amd import hip
    F64, F32 = torch.float64, torch.float32
    for si, shape in enumerate(shapes_of(Cn)):
        seg = Seg(Cn, shape, seed=Cn + si, sliced_c=bool(si % 2))
        N = seg.N
        seg.statistics()
        first = seg.stats[1].clone()
        tag = f"C{Cn}:N{N}"
        _, mu64, v64 = BN.apply_closed(seg.c, seg.gamma, seg.beta, BN.LINEAR, dtype=F64)
        _, mu32, v32 = BN.apply_closed(seg.c, seg.gamma, seg.beta, BN.LINEAR, dtype=F32)
        within(seg.row(hip.BN_ROW_MU), mu64, mu32, tag + ":mu"), within(seg.row(hip.BN_ROW_VAR), v64, v32, tag + ":v")
        assert float(seg.row(hip.BN_ROW_VAR)[5]) == 0.0 and float(seg.row(hip.BN_ROW_MU)[5]) == 0.5
        run = lambda mu, v, d: ((1 - BN.MOMENTUM) * seg.rm.to(d) + BN.MOMENTUM * mu, (1 - BN.MOMENTUM) * seg.rv.to(d) + BN.MOMENTUM * v * (N / (N - 1)))
        (rm64, rv64), (rm32, rv32) = run(mu64, v64, F64), run(mu32, v32, F32)
        within(seg.row(hip.BN_ROW_RUN_MEAN), rm64, rm32, tag + ":running_mean"), within(seg.row(hip.BN_ROW_RUN_VAR), rv64, rv32, tag + ":running_var")
        res_storages = ("f32", "f16x2", "bf16x3") if Cn % 32 == 0 else ("f32", )
        for act, rs in [(hip.BBN_RELU, None), (hip.BBN_LINEAR, None)] + [(hip.BBN_RESIDUAL, s) for s in res_storages]:
            for sliced in (False, True):
                res = Stored(N, Cn, rs, sliced, values=seg.r) if rs else None
                r = res.decoded() if res is not None else None  # (what the storage holds: the f16x2 split of r is not r)
                out = Stored(N, Cn, "f32", sliced)
                seg.apply(act, out, res)
                y64, y32 = BN.apply_closed(seg.c, seg.gamma, seg.beta, act, r, dtype=F64)[0], BN.apply_closed(seg.c, seg.gamma, seg.beta, act, r, dtype=F32)[0]
                y = out.decoded()
                within(y, y64, y32, f"{tag}:{('relu', 'linear', 'residual')[act]}{'+' + rs if rs else ''}:y")
                if act == hip.BBN_LINEAR:  # the constant channel gives beta exactly; negative values are stored
                    assert bool((y[:, 5] == seg.beta[5]).all()) and bool((y < 0).any()) and bool((y[:, 7] < -90).all())
                else:
                    want5 = (seg.beta[5] + r[:, 5]).clamp(min=0) if act == hip.BBN_RESIDUAL else seg.beta[5].clamp(min=0).expand(N)
                    assert torch.equal(y[:, 5], want5) and bool((y[:, 7] == 0).all()) and bool((y >= 0).all())
                assert out.rest_intact() and (res is None or res.rest_intact()) and int(seg.status) == 0
                again = Stored(N, Cn, "f32", sliced)
                seg.apply(act, again, res)
                assert torch.equal(again.own(), out.own())
        seg.stats[1].fill_(SENTINEL)
        seg.statistics()
        assert torch.equal(seg.stats[1], first) and intact(seg.frames()) and seg.raw.rest_intact()


@pytest.mark.parametrize("Cn", [32, 128, 512])
@pytest.mark.parametrize("storage,scale", [("f16x2", 16.0), ("f16x2", 1.0), ("bf16x3", 1.0)])
def test_plane_stores_are_the_bits_of_split_planes(hiplib, Cn, storage, scale):
    """Every plane store, whole and as the slice at column C of a 2C-channel plane buffer, against the two-step statement: the f32 form of
    the same call, then dd3d_split_planes(relu=False) -- equal bits and the same status word; the optional f32 copy beside the planes is
    the f32 form's output.  At plane scale 16 a value past the half range (|y| > 4094) sets the overflow bit in both."""
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    for shape in shapes_of(Cn)[1:]:
        for act in (hip.BBN_RELU, hip.BBN_LINEAR, hip.BBN_RESIDUAL):
            for gain, sliced in ((1.0, False), (1.0, True), (4000.0, True)):
                seg = Seg(Cn, shape, seed=3, gain=gain)
                N = seg.N
                seg.statistics()
                res = Stored(N, Cn, storage, not sliced, scale=scale, values=seg.r) if act == hip.BBN_RESIDUAL else None
                plain, planes, copy = Stored(N, Cn, "f32", False), Stored(N, Cn, storage, sliced, scale=scale), Stored(N, Cn, "f32", sliced)
                seg.apply(act, plain, res)
                assert int(seg.status) == 0
                seg.apply(act, planes, res, y32=copy)
                status = torch.zeros(1, dtype=torch.int32, device="cuda")
                want = Stored(N, Cn, storage, sliced, scale=scale)
                hip.check(lib.dd3d_split_planes(plain.ptr, want.ptr, N, Cn, Cn, math_of(storage), 0, scale, status.data_ptr(), st), "split")
                torch.cuda.synchronize()
                assert torch.equal(planes.own(), want.own()) and torch.equal(copy.own(), plain.own()), (shape, act, gain, sliced)
                big = float(plain.own().abs().max())
                expect = hip.STATUS_F16_OVERFLOW if storage == "f16x2" and big * scale > 65504.0 else 0
                assert gain == 1.0 or big > 4094.0
                assert int(status) == int(seg.status) == expect
                assert planes.rest_intact() and copy.rest_intact() and plain.rest_intact()


# ------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("Cn", WIDTHS)
def test_backward_against_the_oracle(hiplib, Cn):
    """q, p and G_c of the masked entry points with the stored y in each storage, whole and sliced, against the closed form under the
    mask [decoded y > 0]; the maskless entry points bit for bit against the masked ones fed an f32 y of ones; two runs; frames."""
    from dd3d_amd import hip
    F64, F32 = torch.float64, torch.float32
    storages = ("f32", "f16x2", "bf16x3") if Cn % 32 == 0 else ("f32", )
    for si, shape in enumerate(shapes_of(Cn)):
        seg = Seg(Cn, shape, seed=40 + Cn + si, sliced_c=not si % 2)
        N = seg.N
        seg.statistics()
        tag = f"C{Cn}:N{N}"
        yv = BN.apply_closed(seg.c, seg.gamma, seg.beta, BN.RESIDUAL, seg.r, dtype=F32)[0]  # a stored output: relu(n + r)
        for k, storage in enumerate(storages):
            y = Stored(N, Cn, storage, bool((k + si) % 2), values=yv)
            mask = y.decoded() > 0
            assert not bool(mask[:, 7].any()) and bool(mask.any())
            seg.backward(y)
            (q64, p64, g64), (q32, p32, g32) = BN.backward_closed(seg.c, mask, seg.G, seg.gamma, dtype=F64), BN.backward_closed(seg.c, mask, seg.G, seg.gamma, dtype=F32)
            qp, gc = seg.qp[1].view(2, Cn).cpu(), seg.gc[1].view(N, Cn).cpu()
            within(qp[0], q64, q32, f"{tag}:{storage}:q"), within(qp[1], p64, p32, f"{tag}:{storage}:p"), within(gc, g64, g32, f"{tag}:{storage}:G_c")
            assert float(qp[0][7]) == 0.0 and float(qp[1][7]) == 0.0 and bool((gc[:, 7] == 0).all())  # the clipped channel passes nothing
            first = (seg.qp[1].clone(), seg.gc[1].clone())
            seg.qp[1].fill_(SENTINEL), seg.gc[1].fill_(SENTINEL)
            seg.backward(y)
            assert torch.equal(seg.qp[1], first[0]) and torch.equal(seg.gc[1], first[1]) and y.rest_intact() and intact(seg.frames())
        ones = Stored(N, Cn, "f32", False, values=torch.ones(N, Cn))
        seg.backward(ones)
        masked = (seg.qp[1].clone(), seg.gc[1].clone())
        seg.qp[1].fill_(SENTINEL), seg.gc[1].fill_(SENTINEL)
        seg.backward(None, linear=True)
        assert torch.equal(seg.qp[1], masked[0]) and torch.equal(seg.gc[1], masked[1])
        (q64, p64, g64), (q32, p32, g32) = BN.backward_closed(seg.c, None, seg.G, seg.gamma, dtype=F64), BN.backward_closed(seg.c, None, seg.G, seg.gamma, dtype=F32)
        qp, gc = seg.qp[1].view(2, Cn).cpu(), seg.gc[1].view(N, Cn).cpu()
        within(qp[0], q64, q32, f"{tag}:linear:q"), within(qp[1], p64, p32, f"{tag}:linear:p"), within(gc, g64, g32, f"{tag}:linear:G_c")
        assert intact(seg.frames()) and seg.g.rest_intact() and seg.raw.rest_intact()


@pytest.mark.parametrize("Cn", [32, 128])
def test_the_order_of_the_sums_is_the_towers(hiplib, Cn):
    """At the widths both families take, the new entry points return the bits of dd3d_bn_batch_stats / dd3d_bn_backward_reduce / _apply
    (and of the FPN's linear pair) on the same input: include/dd3d_hip.h states that the order of every sum is kept."""
    for si, shape in enumerate(COMMON + [(2, 24, 40)]):
        seg = Seg(Cn, shape, seed=70 + si, sliced_c=bool(si % 2))
        seg.statistics()
        mine = seg.stats[1].clone()
        seg.stats[1].fill_(SENTINEL)
        seg.statistics("dd3d_bn_batch_stats")
        assert torch.equal(seg.stats[1], mine), shape
        y = Stored(seg.N, Cn, "f16x2", True, values=BN.apply_closed(seg.c, seg.gamma, seg.beta, BN.RELU, dtype=torch.float32)[0])
        for linear in (False, True):
            seg.backward(None if linear else y, linear=linear)
            got = (seg.qp[1].clone(), seg.gc[1].clone())
            seg.qp[1].fill_(SENTINEL), seg.gc[1].fill_(SENTINEL)
            seg.backward(None if linear else y, linear=linear, tower=True)
            assert torch.equal(seg.qp[1], got[0]) and torch.equal(seg.gc[1], got[1]), (shape, linear)


def test_two_segments_in_one_call(hiplib):
    """DD3D_BN_MAX_SEGS allows grouping norms of equal width: a two-segment call returns what two one-segment calls return."""
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    a_, b_ = Seg(128, (1, 20, 12), seed=1), Seg(128, (2, 3, 5), seed=2)
    outs = []
    for s in (a_, b_):
        s.statistics()
        o = Stored(s.N, 128, "f16x2", False)
        s.apply(hip.BBN_RELU, o)
        outs.append(o)
    f = hip.BackboneBnArgs()
    C.memmove(C.addressof(f), C.addressof(a_.f), C.sizeof(f))
    a = f.bn
    stats, ys = [framed(hip.BN_STAT_ROWS * 128) for _ in range(2)], [Stored(a_.N, 128, "f16x2", False), Stored(b_.N, 128, "f16x2", False)]
    part = framed(hip.bn_slices([a_.N, b_.N]) * 2 * 128)
    a.num_segs, a.part, a.n_slices = 2, part[1].data_ptr(), hip.bn_slices([a_.N, b_.N])
    for i, s in enumerate((a_, b_)):
        a.c[i], a.N[i], a.stats[i], a.y[i] = s.raw.ptr, s.N, stats[i][1].data_ptr(), ys[i].ptr
        a.gamma[i], a.beta[i], a.run_mean[i], a.run_var[i] = (v.data_ptr() for v in s.vecs)
    assert a_.raw.pitch == b_.raw.pitch
    hip.check(lib.dd3d_backbone_bn_batch_stats(C.byref(a), st), "stats")
    hip.check(lib.dd3d_backbone_bn_apply(C.byref(f), st), "apply")
    torch.cuda.synchronize()
    for i, s in enumerate((a_, b_)):
        assert torch.equal(stats[i][1], s.stats[1]) and torch.equal(ys[i].own(), outs[i].own()) and ys[i].rest_intact()
    assert intact(stats + [part])


# ------------------------------------------------------------------------------------------------------------- rejections
def test_documented_rejections(hiplib):
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    seg = Seg(32, (1, 8, 8), seed=5)
    seg.statistics()
    out, res = Stored(seg.N, 32, "f16x2", False), Stored(seg.N, 32, "f32", False, values=seg.r)
    seg.apply(hip.BBN_RESIDUAL, out, res)
    before = out.own().clone()
    y = Stored(seg.N, 32, "f32", False, values=torch.ones(seg.N, 32))
    seg.backward(y)
    f, a = seg.f, seg.args
    tower = ["dd3d_backbone_bn_batch_stats", "dd3d_backbone_bn_backward_reduce", "dd3d_backbone_bn_backward_apply",
             "dd3d_backbone_bn_backward_reduce_linear", "dd3d_backbone_bn_backward_apply_linear"]
    every = tower + ["dd3d_backbone_bn_apply"]

    def refused(which, what):
        for name in which:
            arg = f if name == "dd3d_backbone_bn_apply" else a
            assert getattr(lib, name)(C.byref(arg), st) == -1 and lib.dd3d_last_error().decode().startswith(name + ":"), (what, name, lib.dd3d_last_error())

    for field, bad, which in (("C", 48, every), ("C", 8, every), ("C", 288, every), ("C", 1024, every), ("c_pitch", 30, every), ("num_segs", 0, every),
                              ("num_segs", 25, every), ("g_pitch", 34, tower[1:]), ("n_slices", 0, tower[:2] + tower[3:4]), ("eps", 0.0, tower[:1]),
                              ("momentum", 1.5, tower[:1]), ("y_mode", 9, tower[1:3]), ("math_mode", hip.MATH_BF16X2, every[-1:]),
                              ("plane_scale", 0.0, every[-1:])):
        old = getattr(a, field)
        setattr(a, field, bad)
        refused(which, (field, bad))
        setattr(a, field, old)
    for field, which in (("c", every), ("stats", every), ("g", tower[1:]), ("qp", tower[1:]), ("gc", [tower[2], tower[4]]), ("y", tower[1:3]),
                         ("gamma", tower[:1]), ("run_var", tower[:1]), ("beta", [tower[0], every[-1]])):
        arr = getattr(a, field)
        old = arr[0]
        arr[0] = None
        refused(which, field)
        arr[0] = old
    old = a.N[0]
    a.N[0] = 1
    refused(every, "N = 1")
    a.N[0] = old
    for field, bad in (("act", 5), ("res_mode", 4), ("res_pitch", 30), ("res_pitch", 34)):
        old = getattr(f, field)
        setattr(f, field, bad)
        refused(every[-1:], (field, bad))
        setattr(f, field, old)
    f.res[0] = None
    refused(every[-1:], "no residual")
    f.res[0] = res.ptr
    a.y[0] = None
    refused(every[-1:], "no output")
    a.y[0] = out.ptr
    for name in every:
        assert getattr(lib, name)(None, st) == -1 and lib.dd3d_last_error().decode().startswith(name + ":")
    # the towers' and the FPN's entry points keep their limits
    a16 = Seg(16, (1, 8, 8)).args
    for name in ("dd3d_bn_batch_stats", "dd3d_bn_backward_reduce_linear"):
        assert getattr(lib, name)(C.byref(a16), st) == -1 and lib.dd3d_last_error().decode().startswith(name)
    out.own().fill_(0)
    seg.apply(hip.BBN_RESIDUAL, out, res)  # the restored arguments still run, to the same bits
    assert torch.equal(out.own(), before)


def test_worst_use_of_the_bar_is_reported(hiplib):
    """(Runs last in this file.)  The largest share of the factor 8 any comparison above used, per quantity: what
    profiles/backbone_bn_errors.txt records."""
    for k, v in sorted(WORST.items()):
        print(f"[backbone_bn] worst use of the factor 8, {k}: {v:.2f}")
    assert all(v <= 8.0 for v in WORST.values())
