"""VoVNet-V2 stem_1 backward on the MI355X (csrc/stem_grads.hip, sg_wgrad_kernel<3, 2, 4, 64>): dd3d_vovnet_stem_wgrad at its C-ABI seam on
seeded 3 x 3, stride-2, 4 -> 64 convolutions (tests/vovnet_stem_grad_cases.py: backbone_grad_cases.ConvCase) against the float64 oracle
(backbone_grad_oracle.layer_grads) -- a single pixel, inputs smaller than a step, odd and even sizes, a partial last unit and MFMA step,
several units a wave, a partial last slice, more than one 64-slice sub-sum; the three storages of the stored output with poisoned
neighbours, operands as channel slices of wider buffers, a zero fourth input channel, an all-zero gradient, wgrad_blocks, every rejected
argument; sentinel-framed outputs, every case twice with equal bits.

The bar of a family (filter: dw and dw_level; q; r) in a case is the project's, 8 * max(d32, 2^-23 * max|g64|): d32 is the deviation of
the oracle's float32 run (torch's float32 convolution-backward, what float32 autograd runs) from its float64 run on the same case."""
import ctypes as C
import os

import pytest
import torch

from tests import backbone_grad_oracle as BO
from tests import vovnet_stem_grad_cases as VS
from tests.test_stem_grads_gpu import POISON, SENTINEL, collect, frame_ok, same_bits, store_y

pytestmark = pytest.mark.gpu

ERRORS = os.environ.get("DD3D_VOVNET_STEM_ERRORS_FILE")  # tests/gpu_vovnet_stem_grad_time.py sets it: the measured ratios go to profiles/


def wide(x, c0=0, tail=0, pad=POISON):
    """NCHW -> device [B, H, W, c0 + C + tail] with x in channels c0 .. c0 + C and `pad` elsewhere; returns (buffer, the slice view)."""
    B, C_, H, W = x.shape
    t = torch.full((B, H, W, c0 + C_ + tail), pad, dtype=torch.float32)
    t[..., c0:c0 + C_] = x.permute(0, 2, 3, 1)
    t = t.cuda()
    return t, t[..., c0:c0 + C_]


def run_seam(case, y_storage="f32", x_c0=0, g_c0=0, g_tail=0, y_c0=0, wgrad_blocks=0, fill=SENTINEL, g=None, x=None):
    """One call through VovnetStemGrads; returns (the outputs as NCHW CPU tensors, the call, the values the stored output decodes to)."""
    from dd3d_amd import hip
    from dd3d_amd.engine.losses import VovnetStemGrads
    xbuf, xv = wide(case.x if x is None else x, x_c0)
    ybuf, ybind, ydec = store_y(case.y, y_storage, c0=y_c0)
    gbuf, gv = wide(case.g if g is None else g, g_c0, g_tail)
    lay = VovnetStemGrads("cuda", case.B, case.hw[0], case.hw[1], xv, ybind, gv, case.w.permute(0, 2, 3, 1).contiguous().cuda(), case.scale.contiguous().cuda(),
                          fill=fill, guard=64, wgrad_blocks=wgrad_blocks)
    lay.da = None  # (tests.test_stem_grads_gpu.collect / frame_ok ask for it: the image has no gradient)
    lay.launch(hip.lib(), hip.current_stream())
    torch.cuda.synchronize()
    lay.keep_alive = (xbuf, ybuf, gbuf)
    return collect(lay), lay, ydec


def check(got, ref64, ref32, what):
    a, b, k = BO.family_vectors(ref64), BO.family_vectors(ref32), BO.family_vectors(got)
    lines = []
    for fam in ("filter", "bias", "norm_weight"):
        assert k[fam].numel() == a[fam].numel() > 0 and bool(torch.isfinite(k[fam]).all()), (what, fam)
        bar, d32, gmax = BO.bar(a[fam], b[fam], torch.ones(a[fam].shape[0], dtype=torch.bool))
        dev = float((k[fam].double() - a[fam]).abs().max())
        use = 8 * dev / bar if bar > 0 else 0.0
        lines.append(f"{what} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} kernel-dev {dev:.3e} bar {bar:.3e} (uses {use:.2f} of the factor 8)")
        print("[vovnet_stem_grads]", lines[-1])
        assert gmax > 0.0 and dev <= bar, (what, fam, dev, bar, d32, gmax)
    assert k["input"].numel() == 0
    if ERRORS:
        with open(ERRORS, "a") as f:
            f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("name", list(VS.SEAM_CASES))
def test_call_at_the_seam(hiplib, name):
    """Against the float64 oracle at the bar; framed outputs; two runs with equal bits; the slicing the case is there for."""
    case = VS.seam_case(name)
    got, lay, ydec = run_seam(case)
    frame_ok(lay)
    assert sorted(got) == ["dw", "dw_level", "q", "r"] and got["dw"].shape == (64, 4, 3, 3) and lay.n_slices == VS.SLICES[name]
    assert torch.equal(ydec, case.y)
    check(got, *VS.seam_refs(name), name)
    assert float(got["dw"][:, 3].abs().max()) > 0.0  # the fourth channel's column: computed and compared like the others
    again, lay2, _ = run_seam(case)
    frame_ok(lay2)
    assert same_bits(got, again)


@pytest.mark.parametrize("storage", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("name", ["c_5x9", "e_4x262", "f_18x331_b2"])
def test_stored_output_as_split_planes(hiplib, name, storage):
    """The mask from f16x2 and bf16x3 planes, two 32-channel chunks; the chunk behind them holds values that would unmask."""
    case = VS.seam_case(name)
    got, lay, ydec = run_seam(case, y_storage=storage)
    frame_ok(lay)
    r64, r32 = VS.seam_refs(name, storage)
    check(got, r64, r32, f"{name} {storage}")
    assert same_bits(got, run_seam(case, y_storage=storage)[0])
    if storage == "bf16x3":  # an exact split: the same masks as the f32 storage, so the same bits
        assert torch.equal(ydec, case.y) and same_bits(got, run_seam(case)[0])


@pytest.mark.parametrize("name", ["c_5x9", "f_18x331_b2"])
def test_operands_as_slices_of_wider_buffers(hiplib, name):
    """x at channels 4 .. 7 of a pitch-8 buffer, g at channels 16 .. 79 of a pitch-96 buffer, y (f32) at channels 8 .. 71 of a pitch-76
    buffer, all with poisoned neighbours: the bits of the plain call."""
    from dd3d_amd import hip
    case = VS.seam_case(name)
    plain, _, _ = run_seam(case)
    got, lay, _ = run_seam(case, x_c0=4, g_c0=16, g_tail=16, y_c0=8)
    assert (lay.args.x_pitch, lay.args.g_pitch, lay.args.y_pitch) == (8, 96, 76) and lay.args.y_mode == hip.PG_ACT_F32
    frame_ok(lay)
    assert same_bits(plain, got)


@pytest.mark.parametrize("name", ["d_6x8", "f_18x331_b2"])
def test_zero_fourth_channel_as_in_the_plan(hiplib, name):
    """The plan's image: the fourth channel holds zeros, so its dw column is exact zeros and the other three keep their bits."""
    case = VS.seam_case(name)
    plain, _, _ = run_seam(case)
    x = case.x.clone()
    x[:, 3] = 0.0
    got, lay, _ = run_seam(case, x=x)
    frame_ok(lay)
    for k in ("dw", "dw_level"):
        assert bool((got[k][:, 3] == 0).all()) and torch.equal(got[k][:, :3], plain[k][:, :3]), k
    assert torch.equal(got["q"], plain["q"])


@pytest.mark.parametrize("name", ["f_18x331_b2", "g_128x640_b2"])
def test_result_does_not_depend_on_wgrad_blocks(hiplib, name):
    """One block walking all slices, a few blocks walking several each, more blocks than slices: the bits of one block per slice."""
    case = VS.seam_case(name)
    auto, lay0, _ = run_seam(case)
    for blocks in (1, 3, lay0.n_slices - 1, 1000):
        forced, lay, _ = run_seam(case, wgrad_blocks=blocks, fill=7.5)
        frame_ok(lay, 7.5)
        assert same_bits(forced, auto), blocks


@pytest.mark.parametrize("name", ["a_1x1", "c_5x9", "f_18x331_b2"])
def test_zero_gradient_gives_exact_zeros(hiplib, name):
    case = VS.seam_case(name)
    got, lay, _ = run_seam(case, g=torch.zeros_like(case.g))
    frame_ok(lay)
    for k, v in got.items():
        assert bool((v == 0).all()), k


def test_fully_masked_layer_gives_exact_zeros(hiplib):
    case = VS.ConvCase((5, 7), 1, VS.CIN, VS.COUT, VS.KSIZE, VS.STRIDE, seed=48, negative_y=True)
    got, lay, _ = run_seam(case)
    frame_ok(lay)
    assert all(bool((v == 0).all()) for v in got.values())


def test_rejected_arguments(hiplib):
    from dd3d_amd import hip
    lib, st = hip.lib(), hip.current_stream()
    entry = "dd3d_vovnet_stem_wgrad"
    case = VS.seam_case("c_5x9")
    _, lay, _ = run_seam(case)
    bad = [("B", 0), ("H", 0), ("W", 0), ("Cin", 16), ("Cout", 32), ("ksize", 7), ("stride", 1), ("Cin", 8), ("Cout", 16), ("ksize", 5), ("stride", 3),
           ("g", None), ("w", None), ("scale", None), ("y", None), ("g_pitch", lay.args.g_pitch + 2), ("g_pitch", case.Cout - 4), ("y_mode", 3), ("y_pitch", 2),
           ("x", None), ("x_pitch", case.Cin + 1), ("x_pitch", case.Cin - 4), ("part", None), ("qpart", None), ("dw_level", None), ("dw", None), ("q", None),
           ("r", None), ("n_slices", 0), ("wgrad_blocks", -1), ("H", 1 << 14)]
    for field, value in bad:
        a = hip.StemGradArgs.from_buffer_copy(lay.args)
        if field == "H" and value == 1 << 14:
            a.W = 1 << 13  # 2^27 pixels
        setattr(a, field, value)
        assert getattr(lib, entry)(C.byref(a), st) == -1, (field, value)
        assert lib.dd3d_last_error().decode().startswith(entry), (field, lib.dd3d_last_error())
    for k, s, cin, cout in hip.STEM_GRAD_SHAPES:  # the DLA stem's shapes belong to dd3d_stem_wgrad
        a = hip.StemGradArgs.from_buffer_copy(lay.args)
        a.ksize, a.stride, a.Cin, a.Cout = k, s, cin, cout
        assert lib.dd3d_vovnet_stem_wgrad(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(entry + ": (ksize, stride, Cin, Cout)")
    a = hip.StemGradArgs.from_buffer_copy(lay.args)
    a.y_mode, a.y_plane_scale = hip.PG_ACT_F16X2, 0.0
    assert lib.dd3d_vovnet_stem_wgrad(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith(entry)
    assert lib.dd3d_vovnet_stem_wgrad(None, st) == -1 and lib.dd3d_last_error().decode().startswith(entry)
    # the DLA stem's entry points keep rejecting this shape
    a = hip.StemGradArgs.from_buffer_copy(lay.args)
    assert lib.dd3d_stem_wgrad(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_stem_wgrad: (ksize, stride, Cin, Cout)")
    a.da, a.da_pitch = lay.dw.data_ptr(), 4
    assert lib.dd3d_stem_dgrad(C.byref(a), st) == -1 and lib.dd3d_last_error().decode().startswith("dd3d_stem_dgrad")
    torch.cuda.synchronize()
    frame_ok(lay)  # no rejected call wrote anything
    again, _, _ = run_seam(case)
    assert same_bits(collect(lay), again)
