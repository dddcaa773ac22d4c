"""The references of tests/glue_cases.py, checked without a GPU: each one against an independent implementation or against words typed
out by hand, so that tests/test_glue_kernels_gpu.py compares the kernels with something that is itself pinned."""
import numpy as np
import pytest
import torch

from tests import glue_cases as G


@pytest.mark.parametrize("hw", G.BILINEAR_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("f", G.BILINEAR_FACTORS + [4, 5, 6, 7, 12, 32, 64])
def test_aligned_bilinear64_against_the_oracle(f, half, hw):
    """The float64 blend with torch's float32 coordinate vs the oracle's F.pad + F.interpolate(align_corners=True) in f32, within the
    bar the kernel is held to (the oracle itself measures at most 2.5 * 2^-24 of max |src|)."""
    from oracle.dense_depth_oracle import aligned_bilinear
    h, w = hw
    rng = np.random.default_rng(1000 * f + 10 * h + w + half)
    src = (rng.standard_normal((3, h, w)) * 10).astype(np.float32)
    ref = G.aligned_bilinear64(src, f, half)
    got = aligned_bilinear(torch.from_numpy(src)[:, None], f, "half" if half else "none")[:, 0].numpy().astype(np.float64)
    assert got.shape == ref.shape == (3, h * f, w * f)
    assert (np.abs(got - ref) <= G.bilinear_bar(src, ref)).all(), float((np.abs(got - ref) / G.bilinear_bar(src, ref)).max())


def test_aligned_bilinear64_focal_scaling():
    src = np.arange(24, dtype=np.float32).reshape(2, 3, 4)
    inv_K = np.zeros((2, 9), np.float32)
    inv_K[:, 0], inv_K[:, 4] = [0.003, 0.004], [0.004, 0.003]
    ref = G.aligned_bilinear64(src, 2, 0, inv_K, 0.5)
    assert np.allclose(ref, G.aligned_bilinear64(src, 2, 0) / 0.0025, rtol=1e-6)  # |(3, 4)| = 5, times the factor 0.5, times 1e-3
    assert np.array_equal(G.aligned_bilinear64(src, 1, 1), src.astype(np.float64))


def test_invert64_against_linalg():
    K = np.concatenate([G.pinhole_matrices(40, seed=3), G.GENERAL_MATRICES])
    ref = torch.linalg.inv(torch.from_numpy(K).double()).numpy()
    got = G.invert64(K)
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
    res, size = G.inverse_residual(K, got)
    assert (res <= 1e-13 * size).all()
    zero_skew = G.invert64(G.pinhole_matrices(7))
    assert (np.count_nonzero(zero_skew.reshape(7, 9), axis=1) == 5).all()


def test_fold_and_pack_references_on_hand_written_records():
    floor = 0.03125
    maxima = np.zeros((3, 16), np.float32)
    maxima[0, 3], maxima[1, 15], maxima[2, 0] = 2.0, 0.03125, 7.5  # launch 1 sits exactly on the floor: not low
    flat = G.build_amax(maxima, 1e30)
    assert flat.shape == (3 * 16 * 32,) and flat[3 * 32] == 2.0 and flat[(16 + 15) * 32] == 0.03125 and flat[1] == np.float32(1e30)
    assert G.fold_ref(None, flat, 3, floor).tolist() == [0, 0]
    assert G.fold_ref(9, flat, 3, floor).tolist() == [9, 0]
    flat[(16 + 15) * 32] = 0.03124
    assert G.fold_ref(1, flat, 3, floor).tolist() == [1, 1]
    flat[(16 + 15) * 32] = 0.0  # nothing stored: not low
    assert G.fold_ref(1, flat, 3, floor).tolist() == [1, 0]
    # the record: header (status, G, n, nrec), two counts, three maxima as bit patterns, two records' first two words at stride 4
    flags = np.array([10, 11, 12, 13, 20, 21, 22, 23], np.int32)
    rec = G.pack_ref([5, 6], 3, flat, 3, flags, 2, 4)
    assert rec.tolist() == [3, 2, 3, 2, 5, 6, 0x40000000, 0, 0x40F00000, 10, 11, 20, 21]
    rec = G.pack_ref(None, None, G.build_amax(np.zeros((0, 16)), float("nan")), 0, None, 0, 2)
    assert rec.tolist() == [0, 0, 0, 0]
    nan_flat = G.build_amax(maxima, float("nan"))  # NaN between the sub-maxima is never looked at
    assert G.pack_ref([1], 0, nan_flat, 3, flags, 1, 2).tolist() == [0, 1, 3, 1, 1, 0x40000000, 0x3D000000, 0x40F00000, 10, 11]


def test_fold_cases_reach_both_verdicts():
    floor = 2.0**-5
    verdict = {name: int(G.fold_ref(0, G.build_amax(m, 1e30), len(m), floor)[1]) for name, m in G.fold_cases(floor)}
    assert set(verdict.values()) == {0, 1}
    for name, v in verdict.items():
        assert v == int("low" in name or "just_below" in name), name
    assert {len(m) for _, m in G.fold_cases(floor)} >= {0, 1, 255, 256, 257, 700}


def test_ceil_mode_output_sizes():
    """torch's rule for 3x3 / stride 2 / ceil_mode: the last window must start inside the input."""
    sizes = [G.maxpool3x3s2_ceil(torch.zeros(1, 1, H, 3)).shape[2] for H in range(3, 12)]
    assert sizes == [1, 2, 2, 3, 3, 4, 4, 5, 5]
    assert [bool(G.pool3_overhang(H, H).any()) for H in (3, 4, 5, 6)] == [False, True, False, True]
    x = -torch.ones(1, 1, 4, 4)
    assert bool((G.maxpool3x3s2_ceil(x) == -1).all())  # the overhang is absent, not zero


def test_plan_allocates_torchs_ceil_mode_size_for_the_v99_pools(hiplib):
    """engine/backbones.py computes the pooled size itself; pin it to torch's at the KITTI geometry (the entry point's copy of the rule
    is pinned on the device: tests/test_glue_kernels_gpu.py writes exactly this allocation).  A dry-run plan needs no device, but the
    engine loads the built library, hence the fixture."""
    shapes = G.v99_kitti_pool_shapes()
    assert shapes == G.V99_KITTI_POOLS  # (the list the GPU module pools, so that it need not build a plan)
    assert shapes[0][:2] == (96, 320)  # the stem's output at 384 x 1280
    for H, W, _, Ho, Wo in shapes:
        assert tuple(G.maxpool3x3s2_ceil(torch.zeros(1, 1, H, W)).shape[2:]) == (Ho, Wo)


def test_special_map_and_byte_image():
    for k, (H, W), pool in ((2, (8, 12), G.maxpool2x2), (3, (9, 13), G.maxpool3x3s2_ceil)):
        x, where = G.special_map(2, 4, H, W, seed=1, k=k)
        ref = pool(x)
        assert len(where) == 6
        for name, (y, xx) in where.items():  # the block at (y, x) is the window (y / 2, x / 2) of the stride-2 pool
            v = float(ref[0, 0, y // 2, xx // 2])
            assert {"+inf": v == float("inf"), "-inf": v == float("-inf"), "fltmax": v == G.FLT_MAX, "-fltmax": v == -G.FLT_MAX, "zeros": v == 0.0,
                    "denormal": 0 < v < 1e-38}[name], (k, name, v)
    img = G.byte_image(2, 16, 17)
    assert all(len(torch.unique(img[b, c])) == 256 for b in range(2) for c in range(3))
    ref = G.preprocess_ref(img, [(16, 17), (1, 1)], [0.0, 127.5, 255.0], [1.0, 0.5, 255.0])
    assert ref.shape == (2, 16, 17, 4) and float(ref[0, 3, 4, 0]) == float(img[0, 0, 3, 4]) and float(ref[0, 0, 0, 2]) == float(np.float32(170 - 255.0) / np.float32(255.0))
    assert float(ref[1].abs().sum()) == float(ref[1, 0, 0].abs().sum()) and bool((ref[..., 3] == 0).all())
