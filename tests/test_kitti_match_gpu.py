"""`dd3d_kitti_tp_scores` / `dd3d_kitti_pr_counts` through the C ABI on hand-built overlap blocks, scores and ignore codes
(tests/kitti_match_cases.py), against the sequential state machines of tests/kitti_ap_oracle.py.  Every comparison is exact and
covers every (class x difficulty, overlap) slot and every threshold row: the outputs are integers and verbatim copies of input
scores.  The cases reach what a KITTI-sized golden never does: more than 64 detections per image (the chunk loop), the second
flag word (detections 4096..8191), ties the butterfly must break by index, blocks whose last image or task is missing.

Wall time of this file, measured: about 6 s of oracle work on the CPU (the hand-placed ties with 4097 .. 8192 detections are
most of it) and 3.7 s in all on the MI355X host, launches included; the kernels themselves take milliseconds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import kitti_match_cases as K
from tests.kitti_match_cases import F32, FILL, MIN_OVERLAP

pytestmark = pytest.mark.gpu

MAX_DT, MAX_GT, MAX_OVERLAPS, MAX_THRESHOLDS = 8192, 1024, 8, 256  # include/dd3d_hip.h DD3D_KITTI_MAX_*
COUNT_FILL = 0x5a5a5a5a5a5a  # tp_fp_fn before the call: the entry point clears it


def launch(images, min_overlap, thresh, n_thresh, override=None, pad=None):
    """Both entry points on `images`.  `override` replaces fields of the packed arguments (the bounds-guard cases declare less than
    is allocated); `pad` appends unused elements to device arrays.  -> (tp_score, tp_fp_fn) on the host, twice-run checked."""
    from dd3d_amd import hip
    p = K.pack(images)
    for name, extra in (pad or {}).items():
        p[name] = np.concatenate([p[name], extra])
    p.update(override or {})
    dev = {k: torch.as_tensor(np.ascontiguousarray(v)).cuda() for k, v in p.items() if isinstance(v, np.ndarray)}
    mo = np.ascontiguousarray(min_overlap, dtype=np.float64)
    n_cd, n_o = p["n_cd"], len(mo)
    thresh = np.ascontiguousarray(thresh, dtype=np.float64).reshape(n_cd * n_o, -1)
    t_max = thresh.shape[1]
    args = hip.KittiMatchArgs(
        ov=dev["ov"].data_ptr(), ov_off=dev["ov_off"].data_ptr(), dt_begin=dev["dt_begin"].data_ptr(), gt_begin=dev["gt_begin"].data_ptr(),
        dt_score=dev["dt_score"].data_ptr(), ign_dt=dev["ign_dt"].data_ptr(), ign_gt=dev["ign_gt"].data_ptr(),
        min_overlap=mo.ctypes.data_as(C.c_void_p), n_ov=p["n_ov"], n_img=p["n_img"], n_dt=p["n_dt"], n_gt=p["n_gt"], n_cd=n_cd, n_o=n_o,
        max_dt=p["max_dt"], max_gt=p["max_gt"])
    th_d = torch.as_tensor(thresh).cuda()
    nt_d = torch.as_tensor(np.ascontiguousarray(n_thresh, dtype=np.int32)).cuda()
    L = hip.lib()
    runs = []
    for _ in range(2):
        tp = torch.full((n_cd, n_o, p["n_gt"]), FILL, dtype=torch.float64, device="cuda")
        counts = torch.full((n_cd, n_o, t_max, 3), COUNT_FILL, dtype=torch.int64, device="cuda")
        hip.check(L.dd3d_kitti_tp_scores(C.byref(args), tp.data_ptr(), hip.current_stream()), "kitti_tp_scores")
        hip.check(L.dd3d_kitti_pr_counts(C.byref(args), th_d.data_ptr(), nt_d.data_ptr(), t_max, counts.data_ptr(), hip.current_stream()),
                  "kitti_pr_counts")
        torch.cuda.synchronize()
        runs.append((tp.cpu().numpy(), counts.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()  # two calls, identical bytes
    return runs[0]


def check(images, min_overlap, thresh, n_thresh, skip=(), **kw):
    """Launch and compare every slot and every threshold row with the oracle, exactly.  -> (tp_score, tp_fp_fn) for further asserts."""
    n_thresh = np.asarray(n_thresh, dtype=np.int32)
    tp, counts = launch(images, min_overlap, thresh, n_thresh, **kw)
    want_tp, want_counts = K.expected(images, min_overlap, thresh, n_thresh, skip)
    assert tp.shape == want_tp.shape and counts.shape == want_counts.shape
    for s in range(want_counts.shape[0] * want_counts.shape[1]):  # rows t >= n_thresh[slot] are zero (the oracle never adds to them)
        assert not want_counts.reshape(-1, *want_counts.shape[2:])[s, n_thresh[s]:].any()
    bad = np.argwhere(tp != want_tp)  # (no NaN on either side: a NaN score is never recorded)
    assert np.array_equal(tp, want_tp), f"tp_score differs at (cd, o, gt) {bad[:5].tolist()} of {len(bad)}"
    bad = np.argwhere(counts != want_counts)
    assert np.array_equal(counts, want_counts), f"tp_fp_fn differs at (cd, o, t, field) {bad[:5].tolist()} of {len(bad)}"
    return tp, counts


def few_thresholds(rng, n_cd, n_o, t_max=4):
    n_thresh = rng.integers(1, t_max + 1, size=n_cd * n_o)
    n_thresh[0] = t_max
    return K.thresholds_from_scores(rng, n_cd * n_o, t_max, n_thresh), n_thresh


def test_giant_images_next_to_empty_ones(hiplib):
    """nd at and around every chunk and flag-word edge up to DD3D_KITTI_MAX_DT_PER_IMAGE, in one launch.  The first pass-1 block
    (4 images) and the first pass-2 block (8 images) each hold a giant next to an empty image; 13 images leave both kernels'
    last block partial."""
    rng = np.random.default_rng(8192)
    n_cd = 3
    sizes = [(MAX_DT, 3), (0, 2), (4097, 2), (1, 1), (4096, 7), (63, 0), (4095, 2), (64, 1), (8191, 1), (65, 2), (129, 7), (127, 2), (128, 1)]
    images = [K.sparse_image(rng, nd, ng, n_cd, n_cand=40) if nd > 300 else K.dense_image(rng, nd, ng, n_cd) for nd, ng in sizes]
    th, nt = few_thresholds(rng, n_cd, 2)
    tp, counts = check(images, MIN_OVERLAP, th, nt)
    assert np.isfinite(tp).sum() >= 10 and counts[..., 0].max() >= 5  # the giants do match
    # the same edges with every detection a candidate of every GT and distinct scores: the recorded score names the pick
    dense = [K.dense_image(rng, nd, ng, n_cd, scores=None) for nd, ng in [(MAX_DT, 2), (0, 0), (4097, 3), (8191, 1)]]
    check(dense, MIN_OVERLAP, th, nt)


@pytest.mark.parametrize("n_img", [1, 3, 4, 5, 7, 8, 9, 13, 33])
def test_image_counts_around_the_block_sizes(hiplib, n_img):
    """Images of every small size class interleaved, so that the last pass-1 block (4 images) and pass-2 block (8) is partial."""
    rng = np.random.default_rng(100 + n_img)
    nds, ngs = [0, 1, 63, 64, 65, 127, 128, 129, 300], [0, 1, 2, 7, 64]
    n_cd = 2
    images = []
    for i in range(n_img):
        nd, ng = nds[(i * 5 + n_img) % len(nds)], ngs[(i * 3 + n_img) % len(ngs)]
        images.append(K.dense_image(rng, nd, ng, n_cd, scores=None if i % 4 == 1 else K.SCORES, zeros=10 * (i % 3)) if i % 2 else K.sparse_image(rng, nd, ng, n_cd))
    th, nt = few_thresholds(rng, n_cd, 2, t_max=3)
    check(images, MIN_OVERLAP, th, nt)


def test_most_ground_truth_one_image_takes(hiplib):
    rng = np.random.default_rng(1024)
    images = [K.dense_image(rng, 5, MAX_GT, 2), K.dense_image(rng, 0, 0, 2), K.dense_image(rng, 70, MAX_GT, 2)]
    th, nt = few_thresholds(rng, 2, 2)
    tp, _ = check(images, MIN_OVERLAP, th, nt)
    assert np.isfinite(tp[:, :, MAX_GT:]).sum() > 20


@pytest.mark.parametrize("a,b", K.TIE_PAIRS)
def test_hand_placed_ties_are_broken_by_index(hiplib, a, b):
    """Two detections that are the only candidates of GT 0 and tie exactly (see kitti_match_cases.tie_images), one launch per
    image so that counts can be read per image.  The oracle decides every slot of every image; the rows spelt out below show
    that the two possible outcomes of the tie differ, in pass 1 and in pass 2."""
    images = K.tie_images(a, b)
    n_slots = K.TIE_N_CD * 2
    th = np.tile(np.array(K.TIE_THRESH), (n_slots, 1))
    got = [check([im], MIN_OVERLAP, th, [len(K.TIE_THRESH)] * n_slots) for im in images]
    tp = lambda im, row: got[im][0][row, 0].tolist()  # noqa: E731
    cnt = lambda im, row, t: got[im][1][row, 0, t].tolist()  # noqa: E731
    ninf = -np.inf
    n_by = sum(1 for j in range(0, b + 1, 7) if j not in (a, b))  # valid bystanders, score 0.95, no overlap: always false positives
    # images: 0-2 GT 1 overlaps both, 3-5 only a, 6-8 only b; scores (a, b) = (0.5, 0.5), (0.4, 0.6), (0.6, 0.4).
    # rows: 0 every code 0; 3 ign_dt (a, b) = (0, 1); 6 ign_dt = (1, 0).
    # pass 1, tied scores: GT 0 takes a, the lower index
    assert tp(3, 0) == [0.5, ninf]  # GT 1 overlaps only a and finds it taken (b taken instead would give [0.5, 0.5])
    assert tp(6, 0) == [0.5, 0.5]   # GT 1 overlaps only b and takes it (b taken by GT 0 would give [0.5, -inf])
    assert tp(0, 3) == [0.5, ninf]  # a valid, b ignored: GT 0 records a, GT 1 takes the ignored b
    assert tp(0, 6) == [ninf, 0.5]  # a ignored, b valid: the other way round
    assert tp(1, 0) == [0.6, 0.4] and tp(2, 0) == [0.6, 0.4]  # untied scores: the larger first, wherever it sits
    # pass 2 at threshold 0.3 (both kept, tied on the overlap): GT 0 takes a although b has the larger score
    assert cnt(4, 0, 0) == [1, n_by + 1, 1]  # GT 1 overlaps only a: a miss, b left over (b taken instead: [2, n_by, 0])
    assert cnt(7, 0, 0) == [2, n_by, 0]      # GT 1 overlaps only b
    assert cnt(4, 0, 2) == [1, n_by, 1]      # threshold 0.5 drops a (0.4): GT 0 takes b
    # rank before index: a valid detection beats an ignored one at a lower index, and an ignored one is taken when it is all there is
    assert cnt(1, 6, 0) == [1, n_by, 0]      # a ignored, b valid: GT 0 takes b (tp), GT 1 the ignored a (neither tp nor fn)
    assert cnt(7, 3, 0) == [1, n_by, 0]      # a valid, b ignored, GT 1 overlaps only b: GT 0 takes a, GT 1 the ignored b
    assert cnt(7, 3, 2) == [0, n_by, 1]      # ... threshold 0.5 drops a: GT 0 takes the ignored b, GT 1 misses


def test_assignment_carries_over_64_ground_truth(hiplib):
    """64 GT compete for the same 130 / 200 detections: flags set by one GT in chunks 1 and 2 decide the later ones."""
    rng = np.random.default_rng(64)
    images = [K.dense_image(rng, 130, 64, 3), K.dense_image(rng, 200, 64, 3, levels=np.array([0.0, 0.6, 0.75, 0.9], dtype=F32)),
              K.dense_image(rng, 130, 64, 3, scores=np.array([0.5])), K.dense_image(rng, 130, 64, 3, scores=None, zeros=20)]
    for im in images:
        im[2][0], im[3][0] = 0, 0  # one row with every code valid: every GT finds a detection until they run out
    th, nt = few_thresholds(rng, 3, 2)
    tp, counts = check(images, MIN_OVERLAP, th, nt)
    assert np.isfinite(tp[0, 0]).sum() > 150


def test_ignore_codes_per_row_and_thresholds_per_slot(hiplib):
    """The shipped shape (n_cd = 15, n_o = 2, t_max = 41) with codes that differ between the class x difficulty rows, images whose
    detections / GT are all ignored or all of another class, and a different n_thresh in every slot (0, 1 and 41 included)."""
    rng = np.random.default_rng(15)
    n_cd, n_o, t_max = 15, 2, 41
    images = [K.dense_image(rng, nd, ng, n_cd) for nd, ng in [(130, 7), (300, 2), (65, 7), (200, 8), (100, 8), (64, 1), (129, 2), (40, 7)]]
    images[2][2][:] = 1   # every detection ignored (too small)
    images[3][2][:] = -1  # every detection of another class
    images[4][3][:] = -1  # every GT of another class
    images[5][3][:] = 1   # every GT ignored
    images[6][2][::2], images[6][3][1::2] = 1, 1  # ... in every other row only
    images[7][2][:5], images[7][3][5:10] = -1, -1
    images.insert(3, K.dense_image(rng, 0, 0, n_cd))
    n_thresh = rng.integers(2, t_max, size=n_cd * n_o)
    n_thresh[[0, 7, 29]], n_thresh[[3, 11]], n_thresh[[5, 28]] = 0, 1, t_max
    th = K.thresholds_from_scores(rng, n_cd * n_o, t_max, n_thresh)
    tp, counts = check(images, MIN_OVERLAP, th, n_thresh)
    assert len({counts[cd].tobytes() for cd in range(n_cd)}) == n_cd  # the rows do differ


def test_most_overlap_cuts_and_most_thresholds(hiplib):
    rng = np.random.default_rng(256)
    images = [K.dense_image(rng, nd, ng, 2, scores=None, zeros=40) for nd, ng in [(130, 7), (70, 8), (0, 3), (64, 2), (200, 5)]]
    mo = [0.1, 0.4, 0.5, 0.55, 0.65, 0.7, 0.8, 0.95]  # DD3D_KITTI_MAX_OVERLAPS cuts: a different set of the levels passes each (none the last)
    assert len(mo) == MAX_OVERLAPS
    th, nt = few_thresholds(rng, 2, MAX_OVERLAPS)
    tp, counts = check(images, mo, th, nt)
    assert len({tp[0, o].tobytes() for o in range(MAX_OVERLAPS)}) == MAX_OVERLAPS and not np.isfinite(tp[:, 7]).any()
    n_thresh = np.array([MAX_THRESHOLDS, 17], dtype=np.int32)
    th = K.thresholds_from_scores(rng, 2, MAX_THRESHOLDS, n_thresh)
    check([im[:2] + (im[2][:1], im[3][:1]) for im in images], MIN_OVERLAP, th, n_thresh)


def test_comparisons_at_the_cuts(hiplib):
    """float32(0.7) < 0.7 and float32(0.5) == 0.5 once widened: neither passes `> min_overlap`; the next float32 above does.  NaN
    overlaps never match, NaN scores are never matched or counted, a score equal to the threshold is kept, one step below is not."""
    z = lambda *s: np.zeros(s, dtype=np.int8)  # noqa: E731
    one = lambda v, s: (np.array([[v]], dtype=F32), np.array([s], dtype=np.float64), z(1, 1), z(1, 1))  # noqa: E731
    up = lambda v: np.nextafter(F32(v), F32(1))  # noqa: E731
    t = 0.6
    images = [one(0.5, 0.9), one(up(0.5), 0.9), one(0.7, 0.9), one(up(0.7), 0.9), one(np.nan, 0.9), one(0.9, np.nan), one(0.9, t),
              one(0.9, np.nextafter(t, 0.0)), one(0.9, np.nextafter(t, 1.0))]
    th = np.array([[t], [t]])
    tp, counts = check(images, MIN_OVERLAP, th, [1, 1])
    ninf = -np.inf
    assert tp[0, 0].tolist() == [ninf, 0.9, 0.9, 0.9, ninf, ninf, t, np.nextafter(t, 0.0), np.nextafter(t, 1.0)]  # cut 0.5
    assert tp[0, 1].tolist() == [ninf, ninf, ninf, 0.9, ninf, ninf, t, np.nextafter(t, 0.0), np.nextafter(t, 1.0)]  # cut 0.7
    # threshold 0.6: images 0..4 keep their detection (matched or a false positive), 5 (NaN score) and 7 (one step below) drop it
    assert counts[0, 0, 0].tolist() == [5, 2, 4] and counts[0, 1, 0].tolist() == [3, 4, 6]
    # the same values inside larger images: NaN and cut levels mixed into the random draw, NaN among the scores
    rng = np.random.default_rng(7)
    levels = np.concatenate([K.LEVELS, np.array([np.nan, np.nan], dtype=F32)])
    scores = np.concatenate([K.SCORES, [np.nan]])
    big = [K.dense_image(rng, nd, ng, 3, levels=levels, scores=scores) for nd, ng in [(130, 7), (300, 8), (64, 64)]]
    th, nt = few_thresholds(rng, 3, 2)
    check(big, MIN_OVERLAP, th, nt)


def test_images_that_break_the_declared_bounds_are_skipped(hiplib):
    """An image whose offsets break the bounds the caller declared contributes nothing: its tp_score entries keep the caller's
    fill, it adds no count, and every other image is exact.  Both cases stay inside the allocations even for a kernel that had
    no guard: the declared bound is smaller than what is allocated, never the other way round."""
    rng = np.random.default_rng(3)
    n_cd = 3
    images = [K.dense_image(rng, nd, ng, n_cd) for nd, ng in [(130, 7), (200, 2), (300, 5), (64, 8), (0, 1), (199, 7), (10, 2), (70, 3), (5, 5)]]
    th, nt = few_thresholds(rng, n_cd, 2)
    # image 2 has 300 detections (allocated, in range of every array) while the launch declares max_dt = 200
    tp, counts = check(images, MIN_OVERLAP, th, nt, skip=(2,), override=dict(max_dt=200))
    g0 = 7 + 2
    assert (tp[:, :, g0:g0 + 5] == FILL).all() and not (tp[:, :, :g0] == FILL).any() and not (tp[:, :, g0 + 5:] == FILL).any()
    # ... and 8 GT in image 3 while max_gt = 7 is declared
    check(images, MIN_OVERLAP, th, nt, skip=(3,), override=dict(max_gt=7))
    # image 5's block lies past the declared n_ov: the buffer is allocated longer than declared and the block sits in its tail
    p = K.pack(images)
    n_ov = p["n_ov"]
    tail = images[5][0].reshape(-1)
    ov_off = p["ov_off"].copy()
    ov_off[5] = n_ov  # == n_ov - nd * ng + nd * ng: past the last start the declared size allows, inside the padded allocation
    tp, counts = check(images, MIN_OVERLAP, th, nt, skip=(5,), override=dict(ov_off=ov_off), pad=dict(ov=tail))
    g0 = 7 + 2 + 5 + 8 + 1
    assert (tp[:, :, g0:g0 + 7] == FILL).all() and (tp == FILL).sum() == 7 * n_cd * 2
    # ... and the same block declared in range is used (the guard does not reject what is allowed): n_ov grown to cover the tail
    check(images, MIN_OVERLAP, th, nt, override=dict(ov_off=ov_off, n_ov=n_ov + len(tail)), pad=dict(ov=tail))
