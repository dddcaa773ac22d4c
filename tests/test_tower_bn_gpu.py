"""Batch-statistics BN of the head towers on the MI355X at the C-ABI seam (csrc/tower_bn.hip): dd3d_bn_batch_stats,
dd3d_bn_apply_relu_split, dd3d_bn_backward_reduce and dd3d_bn_backward_apply called directly on synthetic c and G.  One call serves
five segments -- N = 2 (B = 2, 1 x 1), 30 (B = 2, 3 x 5: no multiple of any block), 64 (one slice of DD3D_BN_SLICE pixels), 256 (four
slices) and 1920 (B = 2, 24 x 40: thirty slices, several rounds of the second-level sum's eight lanes) -- at 32 and at 256 channels,
the latter as the slice at column 256 of a pitch-512 buffer; a channel constant over the batch (v = 0); a segment whose stored output
is all zero; f16x2, bf16x3 and f32 outputs; an activation past the half range.

Bars: mu, v, y, q, p, G_c each within loss_grad_oracle.bar = 8 * max(d32, 2^-23 * max|ref64|), d32 the deviation of torch-CPU float32
(F.batch_norm and its autograd) from float64 on the same inputs.  Equal bits over two runs; no word beyond the outputs is written.  The
calls expose no grid size, so there is no second geometry to compare."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from tests import tower_bn_oracle as BO

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
POISON = 3.0e30
GUARD = 64
SHAPES = [(2, 1, 1), (2, 3, 5), (1, 8, 8), (1, 16, 16), (2, 24, 40)]  # N = 2, 30, 64 (one slice), 256, 1920
EPS = 1e-5
WORST = {}


def framed(numel, dtype=torch.float32, fill=SENTINEL):
    t = torch.full((numel + GUARD, ), fill, dtype=dtype, device="cuda")
    return t, t[:numel]


def intact(frames, fill=SENTINEL):
    return all(bool((full[view.numel():] == fill).all()) for full, view in frames)


class Layer:
    """Seeded segments of one layer and every device buffer of the four calls."""
    def __init__(self, Cn, storage, col=0, pitch=None, plane_scale=16.0, seed=0, gain=1.0, masked=None, shapes=SHAPES):
        from dd3d_amd import hip
        gen = torch.Generator().manual_seed(seed)
        self.C, self.storage, self.shapes, self.S = Cn, storage, shapes, len(shapes)
        pitch = pitch or Cn
        self.c, self.G, self.gamma, self.beta, self.rm, self.rv = [], [], [], [], [], []
        for B, h, w in shapes:
            c = torch.randn(B, Cn, h, w, generator=gen) * 1.5 + 0.3
            c[:, 5] = 0.5  # constant over the batch: v = 0
            self.c.append(c)
            self.G.append(torch.randn(B, Cn, h, w, generator=gen))
            self.gamma.append((0.5 + torch.rand(Cn, generator=gen)) * gain), self.beta.append(torch.randn(Cn, generator=gen) * 0.3)
            self.rm.append(torch.randn(Cn, generator=gen) * 0.2), self.rv.append(0.5 + torch.rand(Cn, generator=gen))
        self.N = [B * h * w for B, h, w in shapes]
        self.raw = []
        for c in self.c:
            t = torch.full((c.shape[0], c.shape[2], c.shape[3], pitch), POISON)
            t[..., col:col + Cn] = c.permute(0, 2, 3, 1)
            self.raw.append(t.cuda())
        self.g = []
        for g in self.G:
            t = torch.full((g.shape[0], g.shape[2], g.shape[3], Cn + 4), POISON)
            t[..., :Cn] = g.permute(0, 2, 3, 1)
            self.g.append(t.cuda())
        dev = lambda xs: [x.contiguous().cuda() for x in xs]
        self.vecs = [dev(v) for v in (self.gamma, self.beta, self.rm, self.rv)]
        self.np = {"f32": 0, "f16x2": 2, "bf16x3": 3, "bf16x2": 2, "bf16": 1}[storage]
        self.math = {"f32": hip.MATH_F32, "f16x2": hip.MATH_F16X2, "bf16x3": hip.MATH_BF16X3, "bf16x2": hip.MATH_BF16X2, "bf16": hip.MATH_BF16}[storage]
        self.stats = [framed(hip.BN_STAT_ROWS * Cn) for _ in shapes]
        self.qp = [framed(2 * Cn) for _ in shapes]
        self.gc = [framed(n * Cn) for n in self.N]
        self.n_slices = hip.bn_slices(self.N)
        self.part = framed(self.n_slices * 2 * Cn)
        self.y = [framed(n * Cn, torch.float32) if storage == "f32" else framed(n * Cn * self.np, torch.int16, fill=-12345) for n in self.N]
        self.status = torch.zeros(1, dtype=torch.int32, device="cuda")
        a = hip.TowerBnArgs()
        for s in range(self.S):
            a.c[s], a.g[s], a.N[s] = self.raw[s].data_ptr() + 4 * col, self.g[s].data_ptr(), self.N[s]
            a.gamma[s], a.beta[s], a.run_mean[s], a.run_var[s] = (v[s].data_ptr() for v in self.vecs)
            a.stats[s], a.qp[s], a.gc[s], a.y[s] = self.stats[s][1].data_ptr(), self.qp[s][1].data_ptr(), self.gc[s][1].data_ptr(), self.y[s][1].data_ptr()
        a.part, a.n_slices, a.status = self.part[1].data_ptr(), self.n_slices, self.status.data_ptr()
        a.num_segs, a.C, a.c_pitch, a.g_pitch, a.math_mode, a.y_pitch = self.S, Cn, pitch, Cn + 4, self.math, Cn
        a.y_mode = {"f32": hip.PG_ACT_F32, "f16x2": hip.PG_ACT_F16X2, "bf16x3": hip.PG_ACT_BF16X3}.get(storage, -1)
        a.eps, a.momentum, a.plane_scale = EPS, hip.BN_MOMENTUM, plane_scale
        self.args, self.plane_scale, self.masked = a, plane_scale, masked

    def frames(self):
        return self.stats + self.qp + self.gc + [self.part] + [y for y in self.y if y[0].dtype == torch.float32]

    def forward(self):
        from dd3d_amd import hip
        lib, st = hip.lib(), hip.current_stream()
        hip.check(lib.dd3d_bn_batch_stats(C.byref(self.args), st), "bn_batch_stats")
        hip.check(lib.dd3d_bn_apply_relu_split(C.byref(self.args), st), "bn_apply_relu_split")
        torch.cuda.synchronize()

    def backward(self):
        from dd3d_amd import hip
        lib, st = hip.lib(), hip.current_stream()
        if self.masked is not None:
            self.y[self.masked][1].zero_()  # the stored output decides: an all-zero level masks every entry of G
        hip.check(lib.dd3d_bn_backward_reduce(C.byref(self.args), st), "bn_backward_reduce")
        hip.check(lib.dd3d_bn_backward_apply(C.byref(self.args), st), "bn_backward_apply")
        torch.cuda.synchronize()

    def y_decoded(self, s):
        """The float32 NCHW values segment s's stored output decodes to."""
        B, h, w = self.shapes[s]
        v = self.y[s][1]
        if self.storage == "f32":
            return v.view(B, h, w, self.C).permute(0, 3, 1, 2).cpu().contiguous()
        t = v.view(self.C // 32, self.N[s], self.np, 32)
        t = t.view(torch.float16).float() / self.plane_scale if self.storage == "f16x2" else (t.to(torch.int32) << 16).view(torch.float32)
        x = t[:, :, 0]
        for q in range(1, self.np):
            x = x + t[:, :, q]
        return x.permute(1, 0, 2).reshape(B, h, w, self.C).permute(0, 3, 1, 2).cpu().contiguous()

    def row(self, s, r):
        return self.stats[s][1].view(-1, self.C)[r].cpu()

    def outputs(self):
        return [f[1].clone() for f in self.stats + self.qp + self.gc + self.y]


def within(got, ref64, ref32, what):
    bar, d32, gmax = BO.bar(ref64.reshape(-1), ref32.reshape(-1), torch.ones(ref64.numel(), dtype=torch.bool))
    dev = float((got.double() - ref64).abs().max())
    assert bool(torch.isfinite(got).all()), what
    use = 8 * dev / bar if bar > 0 else 0.0
    WORST[what.split(":")[-1]] = max(WORST.get(what.split(":")[-1], 0.0), use)
    print(f"[tower_bn] {what}: max|ref64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
    assert dev <= bar, (what, dev, bar, d32, gmax)


def check_layer(lay, what):
    from dd3d_amd import hip
    lay.forward()
    first = lay.outputs()
    for s in range(lay.S):
        c, gamma, beta = lay.c[s], lay.gamma[s], lay.beta[s]
        mu64, v64, s64, t64, y64 = BO.forward_closed(c, gamma, beta, EPS, torch.float64)
        mu32, v32 = BO.stats(c, torch.float32)
        y32 = F.relu(F.batch_norm(c, None, None, gamma, beta, training=True, eps=EPS))
        tag = f"{what}:N{lay.N[s]}"
        within(lay.row(s, hip.BN_ROW_MU), mu64, mu32, tag + ":mu")
        within(lay.row(s, hip.BN_ROW_VAR), v64, v32, tag + ":v")
        y = lay.y_decoded(s)
        within(y, y64, y32, tag + ":y")
        # the constant channel: v = 0 exactly, nothing non-finite, y = relu(beta)
        assert float(lay.row(s, hip.BN_ROW_VAR)[5]) == 0.0 and float(lay.row(s, hip.BN_ROW_MU)[5]) == 0.5
        assert float((y[:, 5] - F.relu(beta[5])).abs().max()) <= 2.0**-21 * max(1.0, float(beta[5].abs()))
        n = lay.N[s]
        rm64, rv64 = BO.running_update(lay.rm[s].double(), lay.rv[s].double(), mu64, v64, n)
        rm32, rv32 = BO.running_update(lay.rm[s], lay.rv[s], mu32, v32, n)
        within(lay.row(s, hip.BN_ROW_RUN_MEAN), rm64, rm32, tag + ":running_mean")
        within(lay.row(s, hip.BN_ROW_RUN_VAR), rv64, rv32, tag + ":running_var")
    lay.backward()
    for s in range(lay.S):
        c, gamma, beta, G = lay.c[s], lay.gamma[s], lay.beta[s], lay.G[s]
        y = lay.y_decoded(s)
        q64, p64, gc64 = BO.backward_closed(c, y, G, gamma, EPS, torch.float64)
        q32, p32, gc32 = BO.backward_autograd(c, y, G, gamma, beta, EPS, torch.float32)
        tag = f"{what}:N{lay.N[s]}"
        B, h, w = lay.shapes[s]
        qp = lay.qp[s][1].view(2, lay.C).cpu()
        gc = lay.gc[s][1].view(B, h, w, lay.C).permute(0, 3, 1, 2).cpu()
        if s == lay.masked:
            assert not bool(qp.any()) and not bool(gc.any()) and not bool(y.any())  # exact zeros
            continue
        within(qp[0], q64, q32, tag + ":q"), within(qp[1], p64, p32, tag + ":p"), within(gc, gc64, gc32, tag + ":G_c")
    assert intact(lay.frames()) and all(bool((full[view.numel():] == -12345).all()) for full, view in lay.y if full.dtype == torch.int16)
    assert int(lay.status) == 0
    return first


@pytest.mark.parametrize("Cn,col,pitch", [(32, 0, None), (256, 256, 512)])
@pytest.mark.parametrize("storage", ["f16x2", "bf16x3", "f32"])
def test_four_calls_against_the_oracle(hiplib, Cn, col, pitch, storage):
    lay = Layer(Cn, storage, col=col, pitch=pitch, seed=Cn, masked=1 if storage == "f16x2" else None)
    check_layer(lay, f"{storage}:C{Cn}")
    final = lay.outputs()
    # a second run of all four calls: equal bits in every output (the masked level's y is zero from the first backward on)
    saved = [t.clone() for t in final]
    for f in lay.stats + lay.qp + lay.gc:
        f[1].fill_(SENTINEL)
    lay.forward(), lay.backward()
    assert all(torch.equal(a, b) for a, b in zip(saved, lay.outputs()))


@pytest.mark.parametrize("storage", ["f16x2", "bf16x3", "bf16x2", "bf16"])
def test_apply_writes_the_bits_of_split_planes_and_its_status(hiplib, storage):
    """The fused apply against its two-step statement: the f32 form of the same call, then dd3d_split_planes(relu) -- equal plane bits in
    every arithmetic mode, and the same status word: zero on ordinary activations, the overflow bit on an activation past the half range
    at plane scale 16 (|y| > 4094), where both set it."""
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    for gain, expect in ((1.0, 0), (4000.0, hip.STATUS_F16_OVERFLOW if storage == "f16x2" else 0)):
        fused, plain = Layer(64, storage, seed=9, gain=gain), Layer(64, "f32", seed=9, gain=gain)
        fused.forward(), plain.forward()
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        for s in range(plain.S):
            assert float(plain.y[s][1].max()) > (4094.0 if gain > 1 else 0.0)
            full, planes = framed(plain.N[s] * 64 * fused.np, torch.int16, fill=-12345)
            hip.check(lib.dd3d_split_planes(plain.y[s][1].data_ptr(), planes.data_ptr(), plain.N[s], 64, 64, fused.math, 1, 16.0, status.data_ptr(), st), "split")
            torch.cuda.synchronize()
            assert torch.equal(planes, fused.y[s][1]), (storage, gain, s)
            assert all(torch.equal(a[1], b[1]) for a, b in zip(fused.stats, plain.stats))
        assert int(status) == int(fused.status) == expect and int(plain.status) == 0
        assert all(bool((full[view.numel():] == -12345).all()) for full, view in fused.y)


def test_rejected_arguments(hiplib):
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    lay = Layer(32, "f16x2", shapes=SHAPES[:2])
    a = lay.args
    entries = [("dd3d_bn_batch_stats", lib.dd3d_bn_batch_stats), ("dd3d_bn_apply_relu_split", lib.dd3d_bn_apply_relu_split),
               ("dd3d_bn_backward_reduce", lib.dd3d_bn_backward_reduce), ("dd3d_bn_backward_apply", lib.dd3d_bn_backward_apply)]
    lay.forward(), lay.backward()
    before = lay.outputs()

    def refused(which, field):
        for name, fn in entries:
            if name in which:
                assert fn(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(name), (field, name)

    every = [n for n, _ in entries]
    for field, bad, which in (("C", 48, every), ("C", 288, every), ("c_pitch", 30, every), ("c_pitch", 28, every), ("num_segs", 0, every),
                              ("g_pitch", 34, every[2:]), ("g_pitch", 16, every[2:]), ("n_slices", 1, [every[0], every[2]]), ("y_mode", 7, every[2:]),
                              ("math_mode", 9, every[1:2]), ("plane_scale", 0.0, every[1:])):
        old = getattr(a, field)
        setattr(a, field, bad)
        refused(which, field)
        setattr(a, field, old)
    a.N[1] = 1
    refused(every, "N")
    a.N[1] = lay.N[1]
    for field, which in (("c", every), ("stats", every), ("gamma", every[:1]), ("run_var", every[:1]), ("y", every[1:]), ("g", every[2:]), ("qp", every[2:]),
                         ("gc", every[3:])):
        arr = getattr(a, field)
        old = arr[1]
        arr[1] = None
        refused(which, field)
        arr[1] = old
    old = a.part
    a.part = None
    refused([every[0], every[2]], "part")
    a.part = old
    assert lib.dd3d_bn_batch_stats(None, st) == -1
    lay.forward(), lay.backward()  # the restored arguments still run, to the same bits
    assert all(torch.equal(x, y) for x, y in zip(before, lay.outputs())) and intact(lay.frames())


def test_worst_use_of_the_bar_is_reported(hiplib):
    """(Runs last in this file.)  The largest share of the factor 8 any comparison above used, per quantity: what profiles/tower_bn_errors.txt records."""
    for k, v in sorted(WORST.items()):
        print(f"[tower_bn] worst use of the factor 8, {k}: {v:.2f}")
    assert all(v <= 8.0 for v in WORST.values())
