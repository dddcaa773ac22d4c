"""The memory-bound kernels that sit between the convolutions of every forward -- csrc/aux_kernels.hip and the pool / top-down / split
kernels of csrc/conv_planes.hip -- through the C ABI, against the plain references of tests/glue_cases.py.

Every launch writes into a buffer framed by PAD sentinel elements each side and, for NHWC and plane outputs, into a channel slice of
a wider buffer; after the launch the frame and the channels outside the slice must be untouched.  Bars are bit-exact (pooling,
top-down sum, preprocess, the range guard's words) or derived from the f32 arithmetic (aligned bilinear, intrinsics inverse); they are
stated in glue_cases.py next to the reference they belong to.

Sections: A pooling / top-down at edges, signs and special values; B the second, partial pass of every capped grid-stride loop;
C preprocess; D aligned bilinear + focal scaling; E intrinsics inverse; F fold_range_flags / pack_readback.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import glue_cases as G
from tests.glue_cases import PAD, POISON

pytestmark = pytest.mark.gpu

SENT = float(np.float32(G.SENT_F32))
ACT_SCALE = 16.0  # plane scale of the f16x2 mode in these tests (the engine's default)

# Block caps of the grid-stride launches, `grid = min(ceil(total / 256), cap)` in the entry point of each kernel:
#   8192   csrc/aux_kernels.hip: dd3d_preprocess_u8_nhwc4, dd3d_maxpool2x2_nhwc, dd3d_upsample2x_add_nhwc, dd3d_maxpool3x3s2_ceil_nhwc
#          (`const int grid = ... < 8192 ? ... : 8192`); csrc/conv_planes.hip: dd3d_split_planes, dd3d_maxpool2x2_planes,
#          dd3d_maxpool2x2_planes_in, dd3d_upsample2x_add_planes (`const int blocks = ... > 8192 ? 8192 : ...`)
#   16384  csrc/aux_kernels.hip: dd3d_aligned_bilinear_scale (`const int grid = ... < 16384 ? ... : 16384`)
CAP_BLOCKS, CAP_BLOCKS_BILINEAR, BLOCK = 8192, 16384, 256


def _modes():
    from dd3d_amd import hip
    return {"bf16x3": (hip.MATH_BF16X3, 3, False), "f16x2": (hip.MATH_F16X2, 2, True), "bf16x2": (hip.MATH_BF16X2, 2, False),
            "bf16": (hip.MATH_BF16, 1, False)}


MODE_NAMES = ["bf16x3", "f16x2", "bf16x2", "bf16"]
PLANE_STEP = {"bf16x3": 0.0, "f16x2": 2.0**-21, "bf16x2": 2.0**-15, "bf16": 2.0**-8}  # of max |ref| (tests/test_conv_planes_gpu.py)


# ------------------------------------------------------------------------------------------------------------ buffers
def framed(inner):
    """Host tensor -> (device buffer with PAD sentinels each side, view of the inner part with the tensor's shape)."""
    fill = {torch.float32: SENT, torch.int32: G.SENT_I32, torch.int16: G.SENT_I16, torch.uint8: 0x5A}[inner.dtype]
    n = inner.numel()
    flat = torch.full((n + 2 * PAD,), fill, dtype=inner.dtype)
    flat[PAD:PAD + n] = inner.reshape(-1)
    d = flat.cuda()
    return d, d[PAD:PAD + n].view(inner.shape), fill


def sentinel_out(shape, dtype=torch.float32):
    fill = {torch.float32: SENT, torch.int32: G.SENT_I32, torch.int16: G.SENT_I16}[dtype]
    return framed(torch.full(shape, fill, dtype=dtype))


def frame_intact(buf, n, fill):
    return bool((buf[:PAD] == fill).all()) and bool((buf[PAD + n:] == fill).all())


def all_sentinel(buf, fill):
    return bool((buf == fill).all())


def same_values(got, ref):
    """torch.equal over the whole tensors (value comparison: +0.0 == -0.0), on the device the result lives on."""
    return got.shape == ref.shape and torch.equal(got, ref.to(got.device))


def check_nhwc(buf, view, fill, c0, Cn, ref_nchw, what=""):
    """`view` [B, H, W, pitch]: channels c0 .. c0 + Cn equal the NCHW reference exactly, the others and the frame hold `fill`."""
    assert frame_intact(buf, view.numel(), fill), f"{what}: written outside the buffer"
    assert bool((view[..., :c0] == fill).all()) and bool((view[..., c0 + Cn:] == fill).all()), f"{what}: channels outside the slice written"
    got = view[..., c0:c0 + Cn].permute(0, 3, 1, 2)
    if not same_values(got, ref_nchw):
        bad = (got != ref_nchw.to(got.device)).nonzero()
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} differ, first at (b, c, y, x) {bad[:4].tolist()}")


def check_planes(buf, pview, k0, ref_rows, mode, what=""):
    """`pview` int16 [chunks][M][NP][32]: chunk images k0 .. k0 + C / 32 decode to `ref_rows` [M, C] within the mode's bar (exactly for
    the three-term split), the other chunk images and the frame keep the sentinel."""
    _, _, f16 = _modes()[mode]
    nch = ref_rows.shape[1] // 32
    assert frame_intact(buf, pview.numel(), G.SENT_I16), f"{what}: planes written outside the buffer"
    assert all_sentinel(pview[:k0], G.SENT_I16) and all_sentinel(pview[k0 + nch:], G.SENT_I16), f"{what}: neighbouring chunk images written"
    dec = G.decode_planes(pview[k0:k0 + nch], f16, ACT_SCALE)
    ref = ref_rows.to(dec.device)
    if mode == "bf16x3":
        assert torch.equal(dec, ref), f"{what}: three-term planes do not decode to the result"
    else:
        err, top = float((dec - ref).abs().max()), float(ref.abs().max())
        print(f"{what}/{mode}: planes max |err| {err:.3e}, bar {PLANE_STEP[mode] * top + 1e-8:.3e}")
        assert err <= PLANE_STEP[mode] * top + 1e-8, (what, mode, err, top)


def plane_ptr(pview, k0):
    return pview.data_ptr() + k0 * pview.shape[1] * pview.shape[2] * 64


def rows(x_nchw):
    return x_nchw.permute(0, 2, 3, 1).reshape(-1, x_nchw.shape[1])


def last_error(lib):
    return lib.dd3d_last_error().decode()


def status_word():
    return torch.zeros(1, dtype=torch.int32, device="cuda")


def stream():
    from dd3d_amd import hip
    return hip.current_stream()


# ------------------------------------------------------------------------------------------------------------ launchers
def run_pool_nhwc(lib, entry, x, ref, in_extra=8, in_c0=4, out_extra=8, out_c0=4, what=""):
    """dd3d_maxpool2x2_nhwc / dd3d_maxpool3x3s2_ceil_nhwc on an NCHW map held as a channel slice, into a channel slice."""
    B, Cn, H, W = x.shape
    in_pitch, out_pitch = Cn + in_extra, Cn + out_extra
    xin = G.nhwc_slice(x, in_pitch, in_c0, POISON).cuda()
    obuf, oview, fill = sentinel_out((B, ref.shape[2], ref.shape[3], out_pitch))
    rc = getattr(lib, entry)(xin.data_ptr() + 4 * in_c0, oview.data_ptr() + 4 * out_c0, B, H, W, Cn, in_pitch, out_pitch, stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    check_nhwc(obuf, oview, fill, out_c0, Cn, ref, what or entry)


def run_upsample_nhwc(lib, fine, coarse, fine_extra=8, fine_c0=4, coarse_extra=4, coarse_c0=4, what="upsample2x_add_nhwc"):
    B, Cn, H, W = fine.shape
    fp, cp = Cn + fine_extra, Cn + coarse_extra
    fbuf, fview, fill = framed(G.nhwc_slice(fine, fp, fine_c0, SENT))  # in place: the slice's neighbours are the sentinel
    cin = G.nhwc_slice(coarse, cp, coarse_c0, POISON).cuda()
    rc = lib.dd3d_upsample2x_add_nhwc(fview.data_ptr() + 4 * fine_c0, cin.data_ptr() + 4 * coarse_c0, B, H, W, Cn, fp, cp, stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    check_nhwc(fbuf, fview, fill, fine_c0, Cn, G.upsample2x_add(fine, coarse), what)


def run_pool_planes(lib, x, mode, with_f32, status=None, in_extra=8, in_c0=4, what="maxpool2x2_planes", check=True):
    """dd3d_maxpool2x2_planes: f32 slice in; f32 slice (optional) and a run of chunk images of a wider plane buffer out."""
    math, NP, f16 = _modes()[mode]
    B, Cn, H, W = x.shape
    ref = G.maxpool2x2(x)
    Mo = B * (H // 2) * (W // 2)
    in_pitch, out_pitch, out_c0 = Cn + in_extra, Cn + 8, 4
    xin = G.nhwc_slice(x, in_pitch, in_c0, POISON).cuda()
    obuf, oview, fill = sentinel_out((B, H // 2, W // 2, out_pitch))
    pbuf, pview, _ = sentinel_out((Cn // 32 + 2, Mo, NP, 32), torch.int16)
    st = status_word() if status is None else status
    rc = lib.dd3d_maxpool2x2_planes(xin.data_ptr() + 4 * in_c0, oview.data_ptr() + 4 * out_c0 if with_f32 else None, plane_ptr(pview, 1), B, H, W, Cn,
                                    in_pitch, out_pitch, math, ACT_SCALE if f16 else 1.0, st.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    assert frame_intact(obuf, oview.numel(), fill) and frame_intact(pbuf, pview.numel(), G.SENT_I16)
    if not with_f32:
        assert all_sentinel(obuf, fill), f"{what}: the f32 output was written although no pointer was passed"
    if check:  # (check=False: the caller compares the returned views itself)
        if with_f32:
            check_nhwc(obuf, oview, fill, out_c0, Cn, ref, what)
        check_planes(pbuf, pview, 1, rows(ref), mode, what)
        assert int(st.cpu()) == 0
    return oview, pview


def split_to_planes(lib, x_rows, mode, status=None):
    """f32 rows [M, C] -> device int16 [C / 32][M][NP][32] through dd3d_split_planes (framed; returns buffer and view)."""
    math, NP, f16 = _modes()[mode]
    M, Cn = x_rows.shape
    xin = x_rows.contiguous().cuda()
    pbuf, pview, _ = sentinel_out((Cn // 32, M, NP, 32), torch.int16)
    st = status_word() if status is None else status
    rc = lib.dd3d_split_planes(xin.data_ptr(), pview.data_ptr(), M, Cn, Cn, math, 0, ACT_SCALE if f16 else 1.0, st.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    assert frame_intact(pbuf, pview.numel(), G.SENT_I16)
    return pbuf, pview


def run_pool_planes_in(lib, x, mode, what="maxpool2x2_planes_in"):
    """dd3d_maxpool2x2_planes_in: the pooled planes decode, bit for bit in every mode, to max_pool2d of the decoded input planes."""
    math, NP, f16 = _modes()[mode]
    B, Cn, H, W = x.shape
    _, pin = split_to_planes(lib, rows(x), mode)
    held = G.rows_to_nchw(G.decode_planes(pin, f16, ACT_SCALE), B, H, W)  # what the input planes hold (lossy in the reduced modes)
    want = G.maxpool2x2(held.cpu())
    Mo = B * (H // 2) * (W // 2)
    pbuf, pview, _ = sentinel_out((Cn // 32 + 2, Mo, NP, 32), torch.int16)
    rc = lib.dd3d_maxpool2x2_planes_in(pin.data_ptr(), plane_ptr(pview, 1), B, H, W, Cn, math, stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    nch = Cn // 32
    assert frame_intact(pbuf, pview.numel(), G.SENT_I16), f"{what}: planes written outside the buffer"
    assert all_sentinel(pview[:1], G.SENT_I16) and all_sentinel(pview[1 + nch:], G.SENT_I16), f"{what}: neighbouring chunk images written"
    got = G.rows_to_nchw(G.decode_planes(pview[1:1 + nch], f16, ACT_SCALE), B, H // 2, W // 2)
    assert same_values(got, want), f"{what}/{mode}: pooled planes are not the winners' terms"
    return held, want


def run_upsample_planes(lib, fine, coarse, mode, status=None, what="upsample2x_add_planes", check=True):
    math, NP, f16 = _modes()[mode]
    B, Cn, H, W = fine.shape
    fp, fc0, cp, cc0 = Cn + 8, 4, Cn + 4, 4
    fbuf, fview, fill = framed(G.nhwc_slice(fine, fp, fc0, SENT))
    cin = G.nhwc_slice(coarse, cp, cc0, POISON).cuda()
    pbuf, pview, _ = sentinel_out((Cn // 32 + 2, B * H * W, NP, 32), torch.int16)
    st = status_word() if status is None else status
    rc = lib.dd3d_upsample2x_add_planes(fview.data_ptr() + 4 * fc0, cin.data_ptr() + 4 * cc0, plane_ptr(pview, 1), B, H, W, Cn, fp, cp, math,
                                        ACT_SCALE if f16 else 1.0, st.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    if check:
        ref = G.upsample2x_add(fine, coarse)
        check_nhwc(fbuf, fview, fill, fc0, Cn, ref, what)
        check_planes(pbuf, pview, 1, rows(ref), mode, what)
        assert int(st.cpu()) == 0
    return fview, pview


# ============================================================================================================ A. pooling / top-down
POOL2_NHWC_CASES = [(B, Cn, H, W) for (B, H, W), Cn in zip(G.POOL2_SHAPES, (4, 36, 36, 4))] + [(3, 36, 2, 2), (1, 4, 6, 10)]
POOL2_PLANES_CASES = [(B, Cn, H, W) for (B, H, W), Cn in zip(G.POOL2_SHAPES, (32, 96, 96, 32))] + [(3, 96, 2, 2), (1, 32, 6, 10)]
ids4 = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.mark.parametrize("kind", ["neg", "mixed"])
@pytest.mark.parametrize("shape", POOL2_NHWC_CASES, ids=ids4)
def test_maxpool2x2_nhwc(hiplib, shape, kind):
    x = G.signed_map(kind, *shape, seed=11)
    ref = G.maxpool2x2(x)
    assert kind != "neg" or bool((ref < 0).all())
    run_pool_nhwc(hiplib, "dd3d_maxpool2x2_nhwc", x, ref)


@pytest.mark.parametrize("kind", ["neg", "mixed"])
@pytest.mark.parametrize("shape", POOL2_NHWC_CASES, ids=ids4)
def test_upsample2x_add_nhwc(hiplib, shape, kind):
    B, Cn, H, W = shape
    fine = G.signed_map(kind, B, Cn, H, W, seed=12)
    coarse = G.signed_map(kind, B, Cn, H // 2, W // 2, seed=13)
    run_upsample_nhwc(hiplib, fine, coarse)


# 3x3 / stride 2 / ceil: (H, W, some window overhangs the bottom or right edge)
POOL3_CASES = [(H, W, H % 2 == 0 or W % 2 == 0) for H, W in G.POOL3_SIZES]


@pytest.mark.parametrize("kind", ["neg", "mixed"])
@pytest.mark.parametrize("B,Cn", [(1, 4), (3, 36)])
@pytest.mark.parametrize("H,W,overhangs", POOL3_CASES, ids=[f"{h}x{w}" for h, w, _ in POOL3_CASES])
def test_maxpool3x3s2_ceil_nhwc(hiplib, H, W, overhangs, B, Cn, kind):
    """A window that overhangs the edge takes the max over its present elements only: with an all-negative map, a kernel that read
    the overhang as 0 would return 0 there."""
    x = G.signed_map(kind, B, Cn, H, W, seed=14)
    ref = G.maxpool3x3s2_ceil(x)
    over = G.pool3_overhang(H, W)
    assert bool(over.any()) == overhangs
    if overhangs and kind == "neg":
        assert bool((ref[:, :, over] < 0).all())
    run_pool_nhwc(hiplib, "dd3d_maxpool3x3s2_ceil_nhwc", x, ref)


@pytest.mark.parametrize("kind", ["neg", "mixed"])
def test_maxpool3x3s2_ceil_at_the_v99_kitti_shapes(hiplib, kind):
    """Every 3x3 pool of the V2-99 / KITTI plan: the size engine/backbones.py allocates, the size the entry point writes (the whole
    allocated slice is compared, the frame must survive) and torch's ceil_mode size are the same."""
    assert G.V99_KITTI_POOLS[0][:2] == (96, 320)  # the stem's output at 384 x 1280
    for H, W, Cn, Ho, Wo in G.V99_KITTI_POOLS:  # (tests/test_glue_cases.py holds this list against the plan's allocations)
        x = G.signed_map(kind, 1, Cn, H, W, seed=15)
        ref = G.maxpool3x3s2_ceil(x)
        assert tuple(ref.shape[2:]) == (Ho, Wo), (H, W, ref.shape, Ho, Wo)
        over = G.pool3_overhang(H, W)
        assert bool(over.any()) and (kind != "neg" or bool((ref[:, :, over] < 0).all()))
        run_pool_nhwc(hiplib, "dd3d_maxpool3x3s2_ceil_nhwc", x, ref, what=f"pool3 {H}x{W}x{Cn}")


@pytest.mark.parametrize("with_f32", [True, False], ids=["f32+planes", "planes"])
@pytest.mark.parametrize("kind", ["neg", "mixed"])
@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("shape", POOL2_PLANES_CASES, ids=ids4)
def test_maxpool2x2_planes(hiplib, shape, mode, kind, with_f32):
    run_pool_planes(hiplib, G.signed_map(kind, *shape, seed=16), mode, with_f32)


@pytest.mark.parametrize("kind", ["neg", "mixed"])
@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("shape", POOL2_PLANES_CASES, ids=ids4)
def test_maxpool2x2_planes_in(hiplib, shape, mode, kind):
    held, want = run_pool_planes_in(hiplib, G.signed_map(kind, *shape, seed=17), mode)
    assert kind != "neg" or bool((want < 0).all())


@pytest.mark.parametrize("kind", ["neg", "mixed"])
@pytest.mark.parametrize("mode", MODE_NAMES)
@pytest.mark.parametrize("shape", POOL2_PLANES_CASES, ids=ids4)
def test_upsample2x_add_planes(hiplib, shape, mode, kind):
    B, Cn, H, W = shape
    run_upsample_planes(hiplib, G.signed_map(kind, B, Cn, H, W, seed=18), G.signed_map(kind, B, Cn, H // 2, W // 2, seed=19), mode)


def _special_survivors(ref, names):
    have = {"+inf": bool((ref == float("inf")).any()), "-inf": bool((ref == float("-inf")).any()), "fltmax": bool((ref == G.FLT_MAX).any()),
            "-fltmax": bool((ref == -G.FLT_MAX).any()), "zeros": bool((ref == 0).any()),
            "denormal": bool(((ref != 0) & (ref.abs() < 1e-38)).any())}
    return [n for n in names if not have[n]]


@pytest.mark.parametrize("kernel", ["maxpool2x2_nhwc", "maxpool3x3s2_ceil_nhwc", "upsample2x_add_nhwc", "maxpool2x2_planes_f32"])
def test_special_values(hiplib, kernel):
    """+-inf, +-FLT_MAX, subnormals (plain f32 kernels) and a window holding +0.0 and -0.0, compared by value."""
    Cn = 32 if kernel == "maxpool2x2_planes_f32" else 4
    if kernel == "maxpool3x3s2_ceil_nhwc":  # the special values sit in 3x3 blocks that are windows of this pool
        x, where = G.special_map(2, Cn, 9, 13, seed=20, k=3)
        ref = G.maxpool3x3s2_ceil(x)
        assert len(where) == 6 and not _special_survivors(ref, list(where))
        run_pool_nhwc(hiplib, "dd3d_maxpool3x3s2_ceil_nhwc", x, ref)
        return
    x, where = G.special_map(2, Cn, 8, 12, seed=20, denormals=kernel != "maxpool2x2_planes_f32")
    if kernel == "upsample2x_add_nhwc":
        coarse = torch.zeros(2, Cn, 4, 6)  # adding zero keeps every special value, and the subnormals exactly
        coarse[1] = G.signed_map("mixed", 1, Cn, 4, 6, seed=21)[0]
        assert not _special_survivors(G.upsample2x_add(x, coarse), list(where))
        run_upsample_nhwc(hiplib, x, coarse)
    else:
        ref = G.maxpool2x2(x)
        assert not _special_survivors(ref, list(where))
        if kernel == "maxpool2x2_nhwc":
            run_pool_nhwc(hiplib, "dd3d_maxpool2x2_nhwc", x, ref)
        else:  # the f32 output of the plane-writing kernel (three-term mode: no range status)
            oview, _ = run_pool_planes(hiplib, x, "bf16x3", True, check=False)
            assert same_values(oview[..., 4:4 + Cn].permute(0, 3, 1, 2), ref)
            assert bool((oview[..., :4] == SENT).all()) and bool((oview[..., 4 + Cn:] == SENT).all())


def test_nan_behaviour_is_pinned(hiplib):
    """NaN is OUTSIDE the contract of these kernels: fmaxf drops a NaN operand where torch's max_pool2d propagates it.  This test pins
    what the kernels do today, so that a change is a decision and not an accident; it does not say the behaviour is right.
      * a pooling window with one NaN yields the max of the other entries (2x2, 3x3 and the plane-writing 2x2);
      * under f16x2, a NaN that does reach the planes -- a window of NaN only, or NaN + x in the top-down sum -- sets
        DD3D_STATUS_F16_OVERFLOW; one that is dropped on the way does not."""
    from dd3d_amd import hip
    nan = float("nan")
    x = G.signed_map("mixed", 1, 32, 6, 8, seed=22)
    x[0, 0, 2, 3] = nan                      # one NaN in the 2x2 window (1, 1) and in the 3x3 windows (0..1, 1)
    others = x.clone()
    others[0, 0, 2, 3] = float("-inf")       # the max of the other entries
    run_pool_nhwc(hiplib, "dd3d_maxpool2x2_nhwc", x, G.maxpool2x2(others))
    run_pool_nhwc(hiplib, "dd3d_maxpool3x3s2_ceil_nhwc", x, G.maxpool3x3s2_ceil(others))
    st = status_word()
    oview, pview = run_pool_planes(hiplib, x, "f16x2", True, status=st, check=False)
    assert same_values(oview[..., 4:36].permute(0, 3, 1, 2), G.maxpool2x2(others)) and int(st.cpu()) == 0
    x[0, 0, 2:4, 2:4] = nan                  # a window of NaN only: the NaN reaches the output and the planes
    oview, _ = run_pool_planes(hiplib, x, "f16x2", True, status=st, check=False)
    got = oview[..., 4:36].permute(0, 3, 1, 2).cpu()
    assert bool(torch.isnan(got[0, 0, 1, 1])) and int(torch.isnan(got).sum()) == 1
    assert int(st.cpu()) == hip.STATUS_F16_OVERFLOW
    st.zero_()
    fine = G.signed_map("mixed", 1, 32, 4, 4, seed=23)
    fine[0, 5, 1, 2] = nan
    fview, _ = run_upsample_planes(hiplib, fine, G.signed_map("mixed", 1, 32, 2, 2, seed=24), "f16x2", status=st, check=False)
    got = fview[..., 4:36].permute(0, 3, 1, 2).cpu()
    assert bool(torch.isnan(got[0, 5, 1, 2])) and int(torch.isnan(got).sum()) == 1
    assert int(st.cpu()) == hip.STATUS_F16_OVERFLOW


def _reject_cases():
    """name -> (entry point, callable(lib, out_ptr, planes_ptr) -> rc) with arguments the entry point's own checks refuse before
    launching anything; the device buffers behind the pointers are large enough for the nearest valid shape."""
    from dd3d_amd import hip
    m = hip.MATH_BF16X3
    cases = {}
    for tag, (H, W, Cn) in {"odd_H": (5, 8, 32), "odd_W": (6, 7, 32)}.items():
        cases[f"maxpool2x2_nhwc/{tag}"] = ("dd3d_maxpool2x2_nhwc", lambda L, i, o, p, s, H=H, W=W, Cn=Cn: L.dd3d_maxpool2x2_nhwc(i, o, 1, H, W, Cn, Cn, Cn, s))
        cases[f"upsample2x_add_nhwc/{tag}"] = ("dd3d_upsample2x_add_nhwc", lambda L, i, o, p, s, H=H, W=W, Cn=Cn: L.dd3d_upsample2x_add_nhwc(o, i, 1, H, W, Cn, Cn, Cn, s))
        cases[f"maxpool2x2_planes/{tag}"] = ("dd3d_maxpool2x2_planes",
                                             lambda L, i, o, p, s, H=H, W=W, Cn=Cn: L.dd3d_maxpool2x2_planes(i, o, p, 1, H, W, Cn, Cn, Cn, m, 1.0, None, s))
        cases[f"maxpool2x2_planes_in/{tag}"] = ("dd3d_maxpool2x2_planes_in",
                                                lambda L, i, o, p, s, H=H, W=W, Cn=Cn: L.dd3d_maxpool2x2_planes_in(i, p, 1, H, W, Cn, m, s))
        cases[f"upsample2x_add_planes/{tag}"] = ("dd3d_upsample2x_add_planes",
                                                 lambda L, i, o, p, s, H=H, W=W, Cn=Cn: L.dd3d_upsample2x_add_planes(o, i, p, 1, H, W, Cn, Cn, Cn, m, 1.0, None, s))
    cases["maxpool2x2_nhwc/C6"] = ("dd3d_maxpool2x2_nhwc", lambda L, i, o, p, s: L.dd3d_maxpool2x2_nhwc(i, o, 1, 6, 8, 6, 8, 8, s))
    cases["upsample2x_add_nhwc/C6"] = ("dd3d_upsample2x_add_nhwc", lambda L, i, o, p, s: L.dd3d_upsample2x_add_nhwc(o, i, 1, 6, 8, 6, 8, 8, s))
    cases["maxpool3x3s2_ceil_nhwc/C6"] = ("dd3d_maxpool3x3s2_ceil_nhwc", lambda L, i, o, p, s: L.dd3d_maxpool3x3s2_ceil_nhwc(i, o, 1, 6, 8, 6, 8, 8, s))
    cases["maxpool2x2_planes/C16"] = ("dd3d_maxpool2x2_planes", lambda L, i, o, p, s: L.dd3d_maxpool2x2_planes(i, o, p, 1, 6, 8, 16, 16, 16, m, 1.0, None, s))
    cases["maxpool2x2_planes_in/C16"] = ("dd3d_maxpool2x2_planes_in", lambda L, i, o, p, s: L.dd3d_maxpool2x2_planes_in(i, p, 1, 6, 8, 16, m, s))
    cases["upsample2x_add_planes/C16"] = ("dd3d_upsample2x_add_planes",
                                          lambda L, i, o, p, s: L.dd3d_upsample2x_add_planes(o, i, p, 1, 6, 8, 16, 16, 16, m, 1.0, None, s))
    cases["split_planes/C16"] = ("dd3d_split_planes", lambda L, i, o, p, s: L.dd3d_split_planes(i, p, 48, 16, 16, m, 0, 1.0, None, s))
    return cases


REJECT_NAMES = [f"{k}/{t}" for t in ("odd_H", "odd_W") for k in ("maxpool2x2_nhwc", "upsample2x_add_nhwc", "maxpool2x2_planes", "maxpool2x2_planes_in",
                                                                "upsample2x_add_planes")] + \
    ["maxpool2x2_nhwc/C6", "upsample2x_add_nhwc/C6", "maxpool3x3s2_ceil_nhwc/C6", "maxpool2x2_planes/C16", "maxpool2x2_planes_in/C16",
     "upsample2x_add_planes/C16", "split_planes/C16"]


@pytest.mark.parametrize("name", REJECT_NAMES)
def test_bad_shapes_are_rejected_before_any_launch(hiplib, name):
    cases = _reject_cases()
    assert sorted(cases) == sorted(REJECT_NAMES)
    entry, call = cases[name]
    src = torch.randn(8 * 8 * 32).cuda()
    obuf, oview, fill = sentinel_out((8 * 8 * 32,))
    pbuf, pview, _ = sentinel_out((8 * 8 * 3 * 32,), torch.int16)
    rc = call(hiplib, src.data_ptr(), oview.data_ptr(), pview.data_ptr(), stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert entry in last_error(hiplib), last_error(hiplib)
    assert all_sentinel(obuf, fill) and all_sentinel(pbuf, G.SENT_I16)


# ============================================================================================================ B. the looping regime
def looping_total(total, cap=CAP_BLOCKS):
    """The case's work items cross the block cap by a quarter to a half, and the second pass ends mid-block."""
    assert total > cap * BLOCK
    assert 1.25 * cap * BLOCK <= total <= 1.5 * cap * BLOCK and total % BLOCK != 0, (total, cap * BLOCK)
    return total


LOOP_HW = (1283, 2045)     # 2,623,735 = 1.251 x 8192 x 256 pixels, 247 past a block
LOOP_PLANES_HW = (810, 810)  # 656,100 pixels x 4 channel groups of 8 = 2,624,400 = 1.251 x 8192 x 256, 144 past a block


def test_looping_preprocess(hiplib):
    Hp, Wp = LOOP_HW
    looping_total(Hp * Wp)
    img = torch.randint(0, 256, (1, 3, Hp, Wp), dtype=torch.uint8, generator=torch.Generator().manual_seed(30))
    from dd3d_amd import get_cfg
    cfg = get_cfg("dd3d_kitti_dla34")
    _check_preprocess(hiplib, img, [(Hp - 3, Wp - 5)], list(cfg.MODEL.PIXEL_MEAN), list(cfg.MODEL.PIXEL_STD))


@pytest.mark.parametrize("entry", ["dd3d_maxpool2x2_nhwc", "dd3d_maxpool3x3s2_ceil_nhwc"])
def test_looping_pools_nhwc(hiplib, entry):
    Ho, Wo = LOOP_HW
    x = G.big_map(1, 4, 2 * Ho, 2 * Wo, 31)
    ref = G.maxpool2x2(x) if entry == "dd3d_maxpool2x2_nhwc" else G.maxpool3x3s2_ceil(x)
    looping_total(ref.shape[2] * ref.shape[3] * (4 // 4))
    assert tuple(ref.shape[2:]) == (Ho, Wo)
    run_pool_nhwc(hiplib, entry, x, ref, in_extra=0, in_c0=0)


def test_looping_upsample2x_add_nhwc(hiplib):
    H, W = 1282, 2046
    looping_total(H * W * (4 // 4))
    run_upsample_nhwc(hiplib, G.big_map(1, 4, H, W, 32), G.big_map(1, 4, H // 2, W // 2, 132), coarse_extra=0, coarse_c0=0)


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3"])
def test_looping_split_planes(hiplib, mode):
    H, W = LOOP_PLANES_HW
    M = H * W
    looping_total(M * (32 // 8))
    x = torch.randn(M, 32, generator=torch.Generator().manual_seed(33))
    st = status_word()
    pbuf, pview = split_to_planes(hiplib, x, mode, status=st)
    check_planes(pbuf, pview, 0, x, mode, "split_planes")
    assert int(st.cpu()) == 0


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3"])
def test_looping_maxpool2x2_planes(hiplib, mode):
    Ho, Wo = LOOP_PLANES_HW
    looping_total(Ho * Wo * (32 // 8))
    x = G.big_map(1, 32, 2 * Ho, 2 * Wo, 34)
    run_pool_planes(hiplib, x, mode, True, in_extra=0, in_c0=0)


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3"])
def test_looping_maxpool2x2_planes_in(hiplib, mode):
    Ho, Wo = LOOP_PLANES_HW
    looping_total(Ho * Wo * (32 // 8))
    x = G.big_map(1, 32, 2 * Ho, 2 * Wo, 35)
    run_pool_planes_in(hiplib, x, mode)


@pytest.mark.parametrize("mode", ["f16x2", "bf16x3"])
def test_looping_upsample2x_add_planes(hiplib, mode):
    H, W = LOOP_PLANES_HW
    looping_total(H * W * (32 // 8))
    run_upsample_planes(hiplib, G.big_map(1, 32, H, W, 36), G.big_map(1, 32, H // 2, W // 2, 136), mode)


def test_looping_aligned_bilinear(hiplib):
    h, w, f = 701, 833, 3
    looping_total(h * f * w * f, CAP_BLOCKS_BILINEAR)
    rng = np.random.default_rng(37)
    src = (rng.standard_normal((1, h, w)) * 10).astype(np.float32)
    inv_K = np.zeros((1, 9), np.float32)
    inv_K[0, 0], inv_K[0, 4] = 1 / 721.5, 1 / 735.0
    _check_bilinear(hiplib, src, f, 1, 1, inv_K, 1.0 / 500.0, torch.from_numpy(G.aligned_bilinear64(src, f, 1)).cuda())


# ============================================================================================================ C. preprocess
def _check_preprocess(lib, img, sizes, mean, std):
    B, _, Hp, Wp = img.shape
    img_d = img.cuda()
    sizes_d = torch.tensor(sizes, dtype=torch.int32).cuda()
    obuf, oview, fill = sentinel_out((B, Hp, Wp, 4))
    rc = lib.dd3d_preprocess_u8_nhwc4(img_d.data_ptr(), sizes_d.data_ptr(), oview.data_ptr(), B, Hp, Wp, (C.c_float * 3)(*mean), (C.c_float * 3)(*std),
                                      stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    assert frame_intact(obuf, oview.numel(), fill)
    ref = G.preprocess_ref(img, sizes, mean, std)
    if not same_values(oview, ref):
        bad = (oview != ref.cuda()).nonzero()
        raise AssertionError(f"preprocess: {len(bad)} of {ref.numel()} differ, first at (b, y, x, c) {bad[:4].tolist()}")


@pytest.mark.parametrize("norm", ["shipped", "made_up"])
def test_preprocess_every_byte_value_and_every_size_class(hiplib, norm):
    """All 256 byte values in each channel; images that fill the canvas, are a single pixel, are empty, one column, one row."""
    from dd3d_amd import get_cfg
    cfg = get_cfg("dd3d_kitti_dla34")
    mean, std = (list(cfg.MODEL.PIXEL_MEAN), list(cfg.MODEL.PIXEL_STD)) if norm == "shipped" else ([0.0, 127.5, 255.0], [1.0, 0.5, 255.0])
    Hp, Wp = 16, 17
    assert (Hp * Wp) % 256 != 0
    sizes = [(Hp, Wp), (1, 1), (0, 0), (Hp, 1), (1, Wp)]
    img = G.byte_image(len(sizes), Hp, Wp)
    for c in range(3):
        assert len(torch.unique(img[0, c])) == 256
    _check_preprocess(hiplib, img, sizes, mean, std)


# ============================================================================================================ D. aligned bilinear
def _launch_bilinear(lib, src, f, half, pitch, inv_K, focal_factor):
    """-> (rc, output [B, f h, f w] on the device, its framed buffer, the fill); channel 0 of an NHWC-`pitch` map, the other channels
    poisoned."""
    B, h, w = src.shape
    s = torch.full((B, h, w, pitch), POISON)
    s[..., 0] = torch.from_numpy(src)
    s_d = s.cuda()
    k_d = torch.from_numpy(np.ascontiguousarray(inv_K, dtype=np.float32)).cuda() if inv_K is not None else None
    obuf, oview, fill = sentinel_out((B, h * f, w * f))
    rc = lib.dd3d_aligned_bilinear_scale(s_d.data_ptr(), oview.data_ptr(), k_d.data_ptr() if k_d is not None else None, B, h, w, pitch, f, half,
                                         float(focal_factor), stream())
    torch.cuda.synchronize()
    assert frame_intact(obuf, oview.numel(), fill)
    return rc, oview, obuf, fill


def _check_bilinear(lib, src, f, half, pitch, inv_K, focal_factor, ref0):
    """`ref0`: G.aligned_bilinear64(src, f, half) as a float64 tensor on the device (large maps are compared there, over every element)."""
    rc, got, _, _ = _launch_bilinear(lib, src, f, half, pitch, inv_K, focal_factor)
    assert rc == 0, last_error(lib)
    ref = ref0
    if focal_factor > 0:
        ref = ref0 / torch.from_numpy(G.focal_divisor(inv_K, focal_factor)).cuda().view(-1, 1, 1)
    lead, rel = G.bilinear_bar_terms(src, inv_K, focal_factor)
    bar = torch.from_numpy(lead).cuda().view(-1, 1, 1) + rel * ref.abs()
    err = (got.double() - ref).abs()
    worst = float((err / bar).max())
    print(f"aligned_bilinear f={f} half={half} map={src.shape[1:]} pitch={pitch} focal={focal_factor:g}: max err / bar = {worst:.3f}")
    assert bool(torch.isfinite(got).all()) and worst <= 1.0, (f, half, pitch, focal_factor, worst, (err > bar).nonzero()[:4].tolist())
    return got


BILINEAR_INV_K = np.zeros((3, 9), np.float32)
BILINEAR_INV_K[:, 0] = [1 / 721.5377, 1 / 1266.4, 1 / 350.0]
BILINEAR_INV_K[:, 4] = [1 / 721.5377, 1 / 1266.4, 1 / 410.0]   # the third image: invK00 != invK11
BILINEAR_INV_K[:, [1, 2, 3, 5, 6, 7, 8]] = POISON               # entries the scaling must not read


@pytest.mark.parametrize("hw", G.BILINEAR_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("f", G.BILINEAR_FACTORS)
def test_aligned_bilinear_scale(hiplib, f, half, hw):
    h, w = hw
    rng = np.random.default_rng(1000 * f + 10 * h + w + half)
    src = (rng.standard_normal((3, h, w)) * 10).astype(np.float32)  # rough data: a wrong neighbour or weight is an error of order |src|
    ref0 = torch.from_numpy(G.aligned_bilinear64(src, f, half)).cuda()
    plain = None
    for pitch in (1, 4):
        got = _check_bilinear(hiplib, src, f, half, pitch, None, 0.0, ref0)
        assert plain is None or torch.equal(plain, got)  # the pitch changes addresses only
        plain = got
        _check_bilinear(hiplib, src, f, half, pitch, BILINEAR_INV_K, 1.0 / 500.0, ref0)
    src_d = torch.from_numpy(src).cuda()
    if f == 1:
        assert torch.equal(plain, src_d)  # the identity, bit for bit
    elif half == 0 and f & (f - 1) == 0:
        assert torch.equal(plain[:, ::f, ::f], src_d)  # power-of-two factor: samples on the coarse grid are the source, bit for bit


def test_aligned_bilinear_focal_scaling_needs_inv_K(hiplib):
    src = np.ones((1, 3, 4), np.float32)
    rc, _, obuf, fill = _launch_bilinear(hiplib, src, 2, 0, 1, None, 0.5)
    assert rc != 0 and "dd3d_aligned_bilinear_scale" in last_error(hiplib) and all_sentinel(obuf, fill)
    rc, _, _, _ = _launch_bilinear(hiplib, src, 2, 0, 1, None, 0.0)
    assert rc == 0


# ============================================================================================================ E. intrinsics inverse
def _invert(lib, K):
    K = np.ascontiguousarray(K, dtype=np.float32).reshape(-1, 3, 3)
    k_d = torch.from_numpy(K).cuda()
    obuf, oview, fill = sentinel_out((len(K), 3, 3))
    rc = lib.dd3d_invert_intrinsics(k_d.data_ptr(), oview.data_ptr(), len(K), stream())
    torch.cuda.synchronize()
    assert rc == 0, last_error(lib)
    assert frame_intact(obuf, oview.numel(), fill)
    return oview.cpu().numpy()


def _check_pinhole_inverse(lib, K):
    got = _invert(lib, K).astype(np.float64)
    ref = G.invert64(K)
    nz = ref != 0
    assert nz.reshape(len(ref), 9).sum(1).tolist() == [5] * len(ref)  # 1/fx, 1/fy, -cx/fx, -cy/fy, 1
    rel = np.abs(got[nz] - ref[nz]) / np.abs(ref[nz])
    print(f"invert_intrinsics, {len(ref)} pinhole matrices: max relative error {rel.max() / G.EPS:.2f} x 2^-24")
    assert rel.max() <= G.INV_REL, (rel.max(), np.argwhere(np.abs(got - ref) > G.INV_REL * np.abs(ref))[:4].tolist())
    assert (got[~nz] == 0).all()


def shipped_intrinsics():
    from dd3d_amd import get_cfg
    from dd3d_amd.synthetic import KITTI_K, NUSC_K, make_inputs
    base = [np.asarray(KITTI_K, np.float32), np.asarray(NUSC_K, np.float32), make_inputs(1, 384, 1280)[0]["intrinsics"].numpy(),
            make_inputs(1, 896, 1600, dataset="nusc")[0]["intrinsics"].numpy()]
    cfg = get_cfg("dd3d_kitti_dla34")
    factors = [float(s) / float(cfg.INPUT.RESIZE.MIN_SIZE_TEST) for s in cfg.TEST.AUG.MIN_SIZES]
    assert len(factors) > 1
    scaled = [(k.astype(np.float64) * np.array([[s], [s], [1.0]])).astype(np.float32) for k in base for s in factors]
    return np.stack(base + scaled)


def test_invert_intrinsics_shipped_cameras(hiplib):
    _check_pinhole_inverse(hiplib, shipped_intrinsics())


@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_invert_intrinsics_batches_around_the_block_size(hiplib, B):
    """64-thread blocks: one block exactly, one thread into the second, two and a bit; every image a different matrix."""
    K = G.pinhole_matrices(B, seed=B)
    assert len(np.unique(K.reshape(B, 9), axis=0)) == B
    _check_pinhole_inverse(hiplib, K)


def test_invert_intrinsics_general_matrices(hiplib):
    got = _invert(hiplib, G.GENERAL_MATRICES)
    res, size = G.inverse_residual(G.GENERAL_MATRICES, got)
    print("invert_intrinsics, general matrices: residual / (2^-24 max(|K| |inv|)) =", (res / (G.EPS * size)).round(2).tolist())
    assert (res <= G.INV_RESIDUAL * size).all(), (res, size)
    ref = G.invert64(G.GENERAL_MATRICES)
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max()  # (and it is the inverse, not merely a small residual by accident)


# ============================================================================================================ F. range guard words
def _floor():
    from dd3d_amd.engine import PlanBase
    return float(PlanBase.AMAX_FLOOR)


def _fold(lib, status, amax_flat, n, floor, null_amax=False):
    st_d = torch.tensor([status], dtype=torch.int32).cuda() if status is not None else None
    a_d = torch.from_numpy(amax_flat).cuda()
    obuf, oview, fill = sentinel_out((2,), torch.int32)
    rc = lib.dd3d_fold_range_flags(st_d.data_ptr() if st_d is not None else None, None if null_amax else a_d.data_ptr(), n, floor, oview.data_ptr(),
                                   stream())
    torch.cuda.synchronize()
    assert frame_intact(obuf, 2, fill)
    return rc, oview.cpu().numpy()


FOLD_CASES = G.fold_cases(1.0)  # (only the names are used here: the test builds the sub-maxima around the floor it reads from PlanBase)


@pytest.mark.parametrize("poison", [1e30, float("nan")], ids=["1e30", "nan"])
@pytest.mark.parametrize("name", [c[0] for c in FOLD_CASES])
def test_fold_range_flags(hiplib, name, poison):
    floor = _floor()
    maxima = dict(G.fold_cases(floor))[name]
    n = len(maxima)
    flat = G.build_amax(maxima, poison)
    for status in (None, 0, 1, 0x7F00FF01):
        rc, got = _fold(hiplib, status, flat, n, floor)
        assert rc == 0, last_error(hiplib)
        want = G.fold_ref(status, flat, n, floor)
        assert got.tolist() == want.tolist(), (name, status, got, want)
    expect_low = ("low" in name or "just_below" in name)
    assert bool(want[1]) == expect_low, (name, want)


def test_fold_range_flags_cases_reach_both_verdicts_and_null_pointers(hiplib):
    floor = _floor()
    verdicts = {int(G.fold_ref(0, G.build_amax(m, 1e30), len(m), floor)[1]) for _, m in G.fold_cases(floor)}
    assert verdicts == {0, 1}
    rc, got = _fold(hiplib, 5, G.build_amax(np.zeros((0, 16)), 1e30), 0, floor, null_amax=True)  # no launches: no array needed
    assert rc == 0 and got.tolist() == [5, 0]
    rc, got = _fold(hiplib, 5, G.build_amax(np.ones((3, 16)), 1e30), 3, floor, null_amax=True)
    assert rc != 0 and "dd3d_fold_range_flags" in last_error(hiplib) and got.tolist() == [G.SENT_I32] * 2


def _pack(lib, det_count, status, amax_flat, n, flags, nrec, stride, null=()):
    Gn = 0 if det_count is None else len(det_count)
    words = 4 + Gn + n + 2 * nrec
    dc_d = torch.from_numpy(np.asarray(det_count, np.int32)).cuda() if Gn else torch.zeros(1, dtype=torch.int32).cuda()
    st_d = torch.tensor([status], dtype=torch.int32).cuda() if status is not None else None
    a_d = torch.from_numpy(amax_flat).cuda()
    f_d = torch.from_numpy(np.asarray(flags, np.int32)).cuda() if nrec else torch.zeros(2, dtype=torch.int32).cuda()
    obuf, oview, fill = sentinel_out((words + 32,), torch.int32)  # 32 more words after the record: they keep the sentinel too
    ptr = lambda t, key, count: None if (key in null or count == 0) else t.data_ptr()  # noqa: E731
    rc = lib.dd3d_pack_readback(ptr(dc_d, "det_count", Gn), Gn, st_d.data_ptr() if st_d is not None else None, ptr(a_d, "amax", n), n,
                                ptr(f_d, "flags", nrec), nrec, stride, oview.data_ptr(), stream())
    torch.cuda.synchronize()
    assert frame_intact(obuf, words + 32, fill)
    host = oview.cpu().numpy()
    return rc, host[:words], host[words:]


@pytest.mark.parametrize("stride", [2, 8])
@pytest.mark.parametrize("nrec", [0, 1, 9])
@pytest.mark.parametrize("n", [0, 257])
@pytest.mark.parametrize("Gn", [0, 1, 300])
def test_pack_readback(hiplib, Gn, n, nrec, stride):
    """The whole record word for word; null det_count / amax / flags are passed exactly when their count is zero."""
    rng = np.random.default_rng(Gn + 7 * n + 3 * nrec + stride)
    det_count = rng.integers(0, 100000, Gn).astype(np.int32) if Gn else None
    maxima = rng.uniform(0.0, 50.0, (n, 16)).astype(np.float32)
    maxima[rng.random((n, 16)) < 0.2] = 0.0
    if n:
        maxima[5] = 0.0                 # a launch that stored nothing
        maxima[6, 1:] = 0.0             # its maximum in sub-slot 0 ...
        maxima[7, :15] = 0.0            # ... and in sub-slot 15
        maxima[7, 15] = 3.25
    flags = rng.integers(-2**31, 2**31 - 1, max(1, nrec) * stride).astype(np.int32)
    for poison in (1e30, float("nan")):
        flat = G.build_amax(maxima, poison)
        for status in (None, 0x01020304):
            rc, rec, after = _pack(hiplib, det_count, status, flat, n, flags, nrec, stride)
            assert rc == 0, last_error(hiplib)
            want = G.pack_ref(det_count, status, flat, n, flags, nrec, stride)
            assert rec.tolist() == want.tolist(), (np.argwhere(rec != want)[:4].tolist(), rec[:8], want[:8])
            assert (after == G.SENT_I32).all()
    if n:
        m = rec[4 + Gn:4 + Gn + n].view(np.float32)
        assert m[5] == 0.0 and m[6] == maxima[6, 0] and m[7] == np.float32(3.25)


@pytest.mark.parametrize("missing", ["det_count", "amax", "flags"])
def test_pack_readback_rejects_a_null_array_with_a_non_zero_count(hiplib, missing):
    maxima = np.ones((3, 16), np.float32)
    rc, rec, after = _pack(hiplib, np.arange(4, dtype=np.int32), 0, G.build_amax(maxima, 1e30), 3, np.arange(16, dtype=np.int32), 2, 8, null=(missing,))
    assert rc != 0 and "dd3d_pack_readback" in last_error(hiplib)
    assert (rec == G.SENT_I32).all() and (after == G.SENT_I32).all()
