"""HIP evaluator-side overlap kernels (through the C ABI) vs the golden vectors of the reference's own functions, vs the oracle on
a larger random problem, and -- on the box-pair families of tests/eval_overlap_cases.py (identical, nested, touching, axis-aligned,
eight crossings, far range, ...) -- vs the oracle and a float64 clipping of the same boxes, at shapes around the 64 x 4 tile.
Whole file on the MI355X host: 5 s."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(os.path.dirname(__file__), "golden", "rotate_iou.npz"))


@pytest.mark.parametrize("crit", [-1, 0, 1, 2])
def test_rotate_iou_matches_reference_golden(hiplib, crit):
    from dd3d_amd.evaluators import rotate_iou_gpu_eval
    got = rotate_iou_gpu_eval(G["boxes"], G["qboxes"], crit)
    ref = G[f"riou_{crit}"]
    assert got.shape == ref.shape and (got > 0).sum() == (ref > 0).sum()
    assert np.allclose(got, ref, rtol=1e-4, atol=1e-5)


def test_d3_and_image_overlap_match_reference_golden(hiplib):
    from dd3d_amd.evaluators import d3_box_overlap, d3_box_overlap_kernel, image_box_overlap
    for crit in (-1, 0, 1):
        for cam in (True, False):
            rinc = G["riou_2"].copy()
            d3_box_overlap_kernel(G["boxes3d"], G["qboxes3d"], rinc, crit, cam)
            assert np.allclose(rinc, G[f"d3_{crit}_{int(cam)}"], rtol=1e-4, atol=1e-5)
        assert np.allclose(image_box_overlap(G["iboxes"], G["iqboxes"], crit), G[f"image_{crit}"], rtol=1e-5, atol=1e-6)
    assert np.allclose(d3_box_overlap(G["boxes3d"], G["qboxes3d"], -1, True), G["d3_-1_1"], rtol=1e-4, atol=1e-5)


def test_rotate_iou_large_random_vs_oracle_and_properties(hiplib):
    from dd3d_amd.evaluators import rotate_iou_gpu_eval
    from oracle import rotate_iou_oracle as R
    from tests.golden.make_rotate_iou_golden import make_boxes
    rng = np.random.default_rng(11)
    boxes, q = make_boxes(rng, 300, spread=10.0), make_boxes(rng, 257, spread=10.0)
    got = rotate_iou_gpu_eval(boxes, q, -1)
    assert got.shape == (300, 257) and float(got.min()) >= 0.0 and float(got.max()) <= 1.0 + 1e-5
    sub = R.rotate_iou_eval(boxes[:40], q[:50], -1)
    assert np.allclose(got[:40, :50], sub, rtol=1e-4, atol=1e-5)
    # symmetry of the IoU, and IoU(b, b) == 1
    assert np.allclose(rotate_iou_gpu_eval(q, boxes, -1), got.T, rtol=1e-4, atol=1e-5)
    assert np.allclose(np.diag(rotate_iou_gpu_eval(boxes, boxes, -1)), 1.0, atol=1e-4)
    assert rotate_iou_gpu_eval(boxes[:0], q, -1).shape == (0, 257)


# ---- the kernels against the oracle and a float64 truth on the families of tests/eval_overlap_cases.py -----------------------------
import torch  # noqa: E402

from oracle import rotate_iou_oracle as R  # noqa: E402
from tests import eval_overlap_cases as C  # noqa: E402

FILL = -7.5  # no overlap is negative: an element that still holds it was not written


def _raw(entry, boxes, qboxes, tail_args, out=None, pad=0):
    """One of the three entry points through the C ABI on an output the test owns: `pad` extra elements after the [N][K] matrix,
    everything pre-filled with FILL (or with `out`).  -> the whole buffer, on the host."""
    from dd3d_amd import hip
    N, K = len(boxes), len(qboxes)
    b = torch.as_tensor(np.ascontiguousarray(boxes, dtype=np.float32)).cuda()
    q = torch.as_tensor(np.ascontiguousarray(qboxes, dtype=np.float32)).cuda()
    buf = torch.full((N * K + pad,), FILL, dtype=torch.float32, device="cuda")
    if out is not None:
        buf[:N * K] = torch.as_tensor(np.ascontiguousarray(out, dtype=np.float32).reshape(-1)).cuda()
    hip.check(getattr(hip.lib(), entry)(b.data_ptr(), q.data_ptr(), buf.data_ptr(), N, K, *tail_args, hip.current_stream()), entry)
    torch.cuda.synchronize()
    return buf.cpu().numpy()


def _oracle_diag(b, q, crit):
    with np.errstate(all="ignore"):
        return np.array([R.rotate_iou_eval(b[i:i + 1], q[i:i + 1], crit)[0, 0] for i in range(len(b))], dtype=np.float32)


def _same_as_oracle(got, ref, what):
    """The bar this file uses against the reference's arithmetic, and the same pairs overlapping on both sides."""
    err = np.abs(got - ref) - 1e-4 * np.abs(ref)
    print(f"{what}: worst |got - ref| - 1e-4 |ref| = {err.max() if err.size else 0.0:.3e} (bar 1e-5), {int((ref > 0).sum())} / {ref.size} overlap")
    assert np.allclose(got, ref, rtol=1e-4, atol=1e-5), what
    assert np.array_equal(got > 0, ref > 0), what


@pytest.mark.parametrize("family", C.STABLE_FAMILIES)
def test_family_against_oracle_and_float64_truth(hiplib, family):
    """Pair i is element [i, i] of one n x n call per criterion.  On the pairs that pass `stable()`: the kernel equals the oracle to
    the file's bar, and is within E_FAMILY + STABLE_SPREAD of the float64 truth -- E_FAMILY is the oracle's own measured error and
    STABLE_SPREAD what a last-bit difference of cosf / sinf may add, the only way the device arithmetic may differ.  The leading
    8 x 8 block is compared as a matrix as well (off-diagonal pairs, each checked for stability first).
    Found with this test: with the device's cosf / sinf in `rbox_corners`, pair 136 of far_octagon (stable, spread 8.5e-5) gave an IoU
    1.25e-4 from the oracle's, beyond rtol 1e-4 + atol 1e-5 -- the kernel's value was, bit for bit, the oracle's with sin moved one
    float32 step.  The kernel now rounds float64 cos / sin once, as the oracle does."""
    from dd3d_amd.evaluators import rotate_iou_gpu_eval
    b, q = C.pairs(family)
    m = C.measured(family)
    s = m["stable"]
    assert (~s).sum() <= C.MAX_UNSTABLE_SHARE * len(s)
    bar = C.E_FAMILY[family] + C.STABLE_SPREAD
    full = {crit: rotate_iou_gpu_eval(b, q, crit) for crit in (-1, 0, 1, 2)}
    for crit in (-1, 0, 1, 2):
        assert full[crit].shape == (len(b), len(q)) and full[crit].dtype == np.float32
        _same_as_oracle(np.diag(full[crit])[s], _oracle_diag(b, q, crit)[s], f"{family} diagonal criterion {crit}")
    area_b, area_q = b[:, 2].astype(np.float64) * b[:, 3], q[:, 2].astype(np.float64) * q[:, 3]
    e_int = np.abs(np.diag(full[2]) - m["truth"]) / m["small"]
    e_iou = np.abs(np.diag(full[-1]) - m["truth"] / (area_b + area_q - m["truth"]))
    print(f"{family}: kernel vs truth e_int {e_int[s].max():.3e}, e_iou {e_iou[s].max():.3e}, bar {bar:.3e} (E_FAMILY {C.E_FAMILY[family]:.3e})")
    assert e_int[s].max() <= bar and e_iou[s].max() <= bar
    # the leading block as a matrix
    n = 8
    with np.errstate(all="ignore"):
        spread = np.array([[C.oracle_spread(b[i], q[j])[1] for j in range(n)] for i in range(n)])
        ok = spread <= C.STABLE_SPREAD
        for crit in (-1, 0, 1, 2):
            _same_as_oracle(full[crit][:n, :n][ok], R.rotate_iou_eval(b[:n], q[:n], crit)[ok], f"{family} block criterion {crit}")
    truth = np.array([[C.truth_intersection(b[i], q[j]) for j in range(n)] for i in range(n)])
    small = np.array([[C.smaller_area(b[i], q[j]) for j in range(n)] for i in range(n)])
    assert ok.mean() > 0.9 and (np.abs(full[2][:n, :n] - truth) / small)[ok].max() <= bar


def test_exact_results(hiplib):
    """Disjoint pairs and KITTI DontCare rows give exactly 0 under every criterion (and no NaN); identical axis-aligned boxes with
    small integer sides give their area exactly."""
    from dd3d_amd.evaluators import rotate_iou_gpu_eval
    for crit in (-1, 0, 1, 2):
        b, q = C.pairs("disjoint")
        assert not np.diag(rotate_iou_gpu_eval(b, q, crit)).any()
        b, q = C.pairs("dontcare")
        out = rotate_iou_gpu_eval(b, q, crit)
        assert np.isfinite(out).all() and not out.any()
        assert not rotate_iou_gpu_eval(q[:3], b, crit).any()  # DontCare on the detection side
    rng = np.random.default_rng(5)
    n = 64
    b = np.stack([rng.integers(-10, 11, n), rng.integers(5, 60, n), rng.integers(1, 7, n), rng.integers(1, 7, n), np.zeros(n)], 1).astype(np.float32)
    area = (b[:, 2] * b[:, 3]).astype(np.float32)
    assert np.array_equal(_oracle_diag(b, b, 2), area)  # the reference's arithmetic is exact here ...
    assert np.array_equal(np.diag(rotate_iou_gpu_eval(b, b, 2)), area)  # ... and so is the kernel's
    assert np.array_equal(np.diag(rotate_iou_gpu_eval(b, b, -1)), np.ones(n, dtype=np.float32))


@pytest.mark.parametrize("family", C.UNSTABLE_FAMILIES)
def test_ill_conditioned_pairs_run_and_write_every_element(hiplib, family):
    """Nearly parallel, nearly coincident edges: the reference's algorithm is ill-conditioned there and no value is
    asserted; the call succeeds and overwrites every element."""
    b, q = C.pairs(family)
    for crit in (-1, 2):
        buf = _raw("dd3d_rotate_iou_eval", b, q, (crit,), pad=5)
        assert not (buf[:len(b) * len(q)] == FILL).any() and (buf[len(b) * len(q):] == FILL).all()


def _cluster(rng, n):
    """Boxes within a few metres of one another: most pairs overlap."""
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(20, 24, n), rng.uniform(1, 5, n), rng.uniform(1, 5, n), rng.uniform(-3.14, 3.14, n)], 1).astype(np.float32)


@pytest.mark.parametrize("N", [1, 3, 4, 5, 9])
def test_shapes_around_the_tile(hiplib, N):
    """TILE_Q = 64 query columns in LDS, TILE_B = 4 rows: every element of the matrix is written, nothing after it, and a pair's
    value does not depend on its place in a tile -- it equals the 1 x 1 call on that pair bit for bit."""
    from dd3d_amd import hip
    rng = np.random.default_rng(N)
    L = hip.lib()
    for K in (1, 63, 64, 65, 129):
        b, q = _cluster(rng, N), _cluster(rng, K)
        for crit in (-1, 2):
            buf = _raw("dd3d_rotate_iou_eval", b, q, (crit,), pad=70)
            out = buf[:N * K].reshape(N, K)
            assert not (out == FILL).any() and (buf[N * K:] == FILL).all() and (out > 0).mean() > 0.3
        bd, qd = torch.as_tensor(b).cuda(), torch.as_tensor(q).cuda()
        single = torch.full((N, K), FILL, dtype=torch.float32, device="cuda")
        for i in range(N):
            for j in range(K):
                hip.check(L.dd3d_rotate_iou_eval(bd[i].data_ptr(), qd[j].data_ptr(), single[i, j].data_ptr(), 1, 1, 2, hip.current_stream()), "1 x 1")
        torch.cuda.synchronize()
        assert single.cpu().numpy().tobytes() == out.tobytes(), (N, K)


@pytest.mark.parametrize("camera", [True, False])
@pytest.mark.parametrize("family", C.D3_FAMILIES)
def test_d3_overlap_against_oracle_and_float64_truth(hiplib, family, camera):
    """d3_box_overlap_kernel multiplies a BEV intersection by the vertical overlap.  Against the oracle fed the same `rinc` the only
    difference left is float32 rounding of the same operations (no trigonometry): 8 roundings, rtol 2^-21.  Against the truth
    (float64 BEV truth x float64 vertical overlap) on the stable pairs the bar is E_3D + STABLE_SPREAD for criteria 0 / 1: a BEV
    difference of STABLE_SPREAD x the smaller area times an overlap height of at most the smaller height is at most STABLE_SPREAD
    x either volume.  For the IoU x / (v1 + v2 - x), x <= (v1 + v2) / 2, the slope is at most 2 / smaller volume: 2 x STABLE_SPREAD."""
    from dd3d_amd.evaluators import d3_box_overlap_kernel, rotate_iou_gpu_eval
    b3, q3 = C.boxes3d(family, camera)
    cols = C.BEV_COLS[camera]
    m = C.measured(family)
    s = m["stable"]
    bev = rotate_iou_gpu_eval(b3[:, cols], q3[:, cols], 2)
    assert np.array_equal(bev, rotate_iou_gpu_eval(*C.pairs(family), 2))  # the same pairs
    for crit in (-1, 0, 1, 2):
        got = bev.copy()
        d3_box_overlap_kernel(b3, q3, got, crit, camera)
        with np.errstate(all="ignore"):
            ref = R.d3_box_overlap(b3, q3, bev, crit, camera)
        assert np.allclose(got, ref, rtol=2.0 ** -21, atol=0, equal_nan=True) and np.array_equal(got > 0, ref > 0), (family, crit)
        if crit == 2:
            continue  # inc / inc: 1 wherever the boxes meet
        truth = np.array([C.d3_from_bev(m["truth"][i], b3[i], q3[i], crit, camera) for i in range(len(b3))])
        err = np.abs(np.diag(got) - truth)[s].max()
        bar = C.E_3D[family] + (2 if crit == -1 else 1) * C.STABLE_SPREAD
        print(f"{family} camera={camera} criterion {crit}: kernel vs truth {err:.3e}, bar {bar:.3e}")
        assert err <= bar
    touching = np.diag(got)[0::4]
    assert not touching.any() and not np.diag(got)[1::4].any() and np.diag(got)[2::4].any()  # overlap height 0 (touching) and below 0 give 0


def test_d3_overlap_leaves_nonpositive_and_nan_entries_alone(hiplib):
    """The reference's kernel enters only `if rinc[i, j] > 0` (rotate_iou.py:337) and writes nothing otherwise, so an entry that is
    0, -0, negative, -inf or NaN on entry keeps its bits; the oracle does the same, and the kernel is held to it."""
    from dd3d_amd.evaluators import d3_box_overlap_kernel
    b3, q3 = C.boxes3d("identical", True)
    b3, q3 = b3[:9], q3[:70]
    rng = np.random.default_rng(9)
    rinc = rng.uniform(0.5, 3.0, (9, 70)).astype(np.float32)
    special = np.array([0.0, -0.0, -2.5, -np.inf, np.nan, -1e-30], dtype=np.float32)
    at = rng.random(rinc.shape) < 0.4
    rinc[at] = rng.choice(special, size=int(at.sum()))
    for crit in (-1, 0, 1, 2):
        for camera in (True, False):
            got = rinc.copy()
            d3_box_overlap_kernel(b3, q3, got, crit, camera)
            with np.errstate(all="ignore"):
                ref = R.d3_box_overlap(b3, q3, rinc, crit, camera)
            assert got[at].tobytes() == rinc[at].tobytes() == ref[at].tobytes()
            assert np.allclose(got[~at], ref[~at], rtol=2.0 ** -21, atol=0) and (got[~at] != rinc[~at]).any()


@pytest.mark.parametrize("N,K", [(1, 255), (1, 257), (3, 171), (2, 256), (257, 1), (5, 103)])
def test_image_box_overlap_against_float64(hiplib, N, K):
    """2D boxes (x1, y1, x2, y2) around the kernel's block of 256 pairs: touching boxes and zero-area boxes give exactly 0, every
    element is written and nothing after it, and the values equal float64 numpy on the same float32 inputs to float32 rounding
    of the dozen operations involved (rtol 32 x 2^-24)."""
    rng = np.random.default_rng(N * 1000 + K)

    def boxes(n):
        x1, y1 = rng.integers(0, 1100, n) / 4.0, rng.integers(0, 300, n) / 4.0
        return np.stack([x1, y1, x1 + rng.uniform(5, 900, n), y1 + rng.uniform(5, 250, n)], 1).astype(np.float32)
    b, q = boxes(N), boxes(K)
    q[0::5, 0] = b[0, 2]  # touches the first box: left edge on its right edge
    q[0::5, 2] = q[0::5, 0] + 10
    q[1::7, 2] = q[1::7, 0]  # zero width
    b[N // 2, 3] = b[N // 2, 1] if N > 2 else b[N // 2, 3]  # zero height
    b64, q64 = b.astype(np.float64)[:, None, :], q.astype(np.float64)[None, :, :]
    iw = np.minimum(b64[..., 2], q64[..., 2]) - np.maximum(b64[..., 0], q64[..., 0])
    ih = np.minimum(b64[..., 3], q64[..., 3]) - np.maximum(b64[..., 1], q64[..., 1])
    ba, qa = (b64[..., 2] - b64[..., 0]) * (b64[..., 3] - b64[..., 1]), (q64[..., 2] - q64[..., 0]) * (q64[..., 3] - q64[..., 1])
    hit = (iw > 0) & (ih > 0)
    for crit in (-1, 0, 1, 2):
        ua = (ba + qa - iw * ih) if crit == -1 else ba + 0 * qa if crit == 0 else qa + 0 * ba if crit == 1 else np.ones_like(iw)
        with np.errstate(all="ignore"):
            want = np.where(hit, iw * ih / ua, 0.0)
        buf = _raw("dd3d_image_box_overlap", b, q, (crit,), pad=300)
        got = buf[:N * K].reshape(N, K)
        assert (buf[N * K:] == FILL).all() and not (got == FILL).any()
        assert np.array_equal(got == 0, ~hit) and not got[0, 0::5].any() and not got[:, 1::7].any()
        assert np.allclose(got, want, rtol=32 * 2.0 ** -24, atol=0), (crit, np.abs(got - want).max())
        with np.errstate(all="ignore"):
            assert np.allclose(got, R.image_box_overlap(b, q, crit), rtol=32 * 2.0 ** -24, atol=0)
    assert hit.any()
