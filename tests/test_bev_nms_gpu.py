"""dd3d_bev_nms_aggregate called directly (C ABI): global transform, rotated-IoU BEV NMS, cap and write-out.

Detection rows (the DD3D_DET_FIELDS layout of include/dd3d_hip.h) are built directly.  With inv_K = I and an object rotation that is
a yaw about the world's vertical, every BEV footprint is chosen: the row's proj_ctr / depth / quaternion are the camera-frame image
of a world box under a nuScenes-scale pose (hundreds of metres of translation).  Pairs of boxes share a category (class + sample *
num_classes), so one launch decides thousands of IoU-versus-threshold questions while the reference evaluates only pairs inside a
category, as the kernel does.

References.  The IoU of every evaluated pair is recomputed in float64 (tests/bev_iou64.py, convex clipping) from the same float32
offset boxes the kernel sees (its sorted work array `sbox`), so only the hull arithmetic differs.  Each mask bit must equal
IoU64 > thr unless |IoU64 - thr| <= iou_margin (reported).  The margin is not only rounding: detectron2's box_iou_rotated (which
the kernel restates) accepts a vertex as inside when its edge dot products are within EPS = 1e-5 of the bounds, in squared-length
units, so the intersection area it measures is off by up to ~EPS / (shortest side)^2 relative (3e-5 measured on identical
2 m boxes, 2.5e-2 on 1 cm slivers); hence iou_margin = 1e-4 + 1e-5 / (shortest side)^2.  The kept set the kept set must be the greedy result over those decisions.  The
sort must be the stable descending score_3d order, the cap the first max_dets of the batch-global keep list, and the output each
image's survivors in their original order.  Random cases are also compared exactly with the float32 oracle
(oracle.nuscenes_oracle.nuscenes_sample_aggregate).  Fields 22-28 (write_global) are compared with float64 boxes_to_global: the
quaternion sign-free (absolute, TOL_GQUAT: quat_to_mat, a 3x3 product and matrix_to_quaternion, ~8 u; measured 1.6e-7), the
translation relative to max(1, |t_cam|, |t|) (TOL_GT): each component is a 3-term dot product of magnitude |t_cam| plus the
pose translation, so its error is a few ulp of the larger of the two, ~ 2-3 u ~ 1.5e-7 (measured 1.2e-7; a component that
cancels to ~0, like the height, cannot be held relative to itself).
"""
import ctypes as C
import math
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import bev_iou64

pytestmark = pytest.mark.gpu

F32 = np.float32
NC = 10  # num_classes
IOU_MARGIN = 1e-4  # + IOU_EPS_AREA / (shortest side)^2, see iou_margin
IOU_EPS_AREA = 1e-5
TOL_GQUAT, TOL_GT = 2.5e-7, 1.5e-7
SENT = np.int32(0x7FBADBAD)
ID_FIELD = 8  # copied verbatim into the output row: carries the row's global input index

_REPORTED = []


def _quat_of(R):
    """float64 unit quaternion (w, x, y, z) of a rotation matrix."""
    from oracle import dd3d_oracle as O
    q = O.matrix_to_quaternion(torch.from_numpy(np.asarray(R, dtype=np.float64))[None])[0].numpy()
    return q / np.linalg.norm(q)


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# camera axes in the world: x -> -y_w, y -> -z_w, z -> +x_w (looking along +x_w), then a heading about the vertical
_CAM = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])


def make_pose(heading_deg, t):
    h = math.radians(heading_deg)
    Rz = np.array([[math.cos(h), -math.sin(h), 0.0], [math.sin(h), math.cos(h), 0.0], [0.0, 0.0, 1.0]])
    q = _quat_of(Rz @ _CAM)
    return np.concatenate([q, np.asarray(t, dtype=np.float64)]).astype(F32)


def rows_for(boxes, pose, scores, classes, rng=None):
    """Detection rows [n, 32] for world boxes (x, y, z, W, L, H, yaw_deg) seen by a camera at `pose` (inv_K = I)."""
    n = len(boxes)
    d = np.zeros((n, 32), dtype=F32)
    R_WS, t_WS = _rot(pose[:4].astype(np.float64)), pose[4:].astype(np.float64)
    for i, (x, y, z, W, L, H, yaw) in enumerate(boxes):
        a = math.radians(yaw)
        R_WO = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
        tS = R_WS.T @ (np.array([x, y, z]) - t_WS)
        assert tS[2] > 0.5
        d[i, 10:14] = _quat_of(R_WS.T @ R_WO)
        d[i, 14:16] = tS[:2] / tS[2]
        d[i, 16] = tS[2]
        d[i, 17:20] = (W, L, H)
    rng = np.random.default_rng(n) if rng is None else rng
    x1, y1 = rng.uniform(0, 1100, n), rng.uniform(0, 300, n)
    d[:, 0:4] = np.stack([x1, y1, x1 + rng.uniform(5, 200, n), y1 + rng.uniform(5, 100, n)], 1)
    d[:, 4] = scores
    d[:, 5] = scores
    d[:, 6] = classes
    d[:, 7] = 1.0
    d[:, 20:22] = (2.0, 0.5)
    return d


def run_bev(imgs, *, det_cap, poses, group=None, thr=0.3, max_dets=0, write_global=1, do_post=0, out_size=None, count_in=None, record=None):
    """imgs: per image a [m, 32] row array (m <= det_cap, or more rows to test the count_in clamp).  Returns a dict of host arrays.
    record = (img_first, img_per_rec, pad_words): read inv_K / pose / out_size from padded records instead of dense arrays."""
    from dd3d_amd import hip
    lib = hip.lib()
    dev = torch.device("cuda")
    G = len(imgs)
    det_in = np.zeros((G, det_cap, 32), dtype=F32)
    cin = np.zeros(G, dtype=np.int32)
    gid = 0
    for g, r in enumerate(imgs):
        m = min(len(r), det_cap)
        det_in[g, :m] = r[:m]
        det_in[g, :m, ID_FIELD] = np.arange(gid, gid + m)
        gid += m
        cin[g] = len(r)
    if count_in is not None:
        cin[:] = count_in
    group = np.arange(G, dtype=np.int32) if group is None else np.asarray(group, dtype=np.int32)
    inv_k = np.tile(np.eye(3, dtype=F32).reshape(1, 9), (G, 1))
    poses = np.asarray(poses, dtype=F32).reshape(G, 7)
    osz = np.tile(np.array([400.0, 1000.0, 800.0, 1600.0], F32), (G, 1)) if out_size is None else np.asarray(out_size, F32).reshape(G, 4)
    ntot = G * det_cap
    mcap = min((ntot + 63) // 64 * 64, 8192)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    keep = []
    t_det, t_cin, t_grp = T(det_in), T(cin), T(group)
    a = hip.BevArgs()
    if record is None:
        t_k, t_p, t_o = T(inv_k), T(poses), T(osz)
        a.inv_K, a.pose, a.out_size = t_k.data_ptr(), t_p.data_ptr(), t_o.data_ptr()
        a.img_first, a.img_per_rec, a.rec_stride = 0, 0, 0
    else:
        first, P, pad = record
        stride = P * 20 + pad
        nrec = (first + G + P - 1) // P
        buf = np.full((nrec, stride), np.nan, dtype=F32)
        for g in range(G):
            r, j = divmod(first + g, P)
            buf[r, j * 9:j * 9 + 9] = inv_k[g]
            buf[r, P * 9 + j * 7:P * 9 + j * 7 + 7] = poses[g]
            buf[r, P * 16 + j * 4:P * 16 + j * 4 + 4] = osz[g]
        t_b = T(buf)
        keep.append(t_b)
        base = t_b.data_ptr()
        a.inv_K, a.pose, a.out_size = base, base + 4 * P * 9, base + 4 * P * 16
        a.img_first, a.img_per_rec, a.rec_stride = first, P, stride
    work = torch.zeros((ntot, 16), dtype=torch.float32, device=dev)
    sbox = torch.zeros((ntot, 8), dtype=torch.float32, device=dev)
    mask = torch.zeros((mcap, mcap // 64), dtype=torch.int64, device=dev)
    meta = torch.zeros(4, dtype=torch.int32, device=dev)
    det_out = torch.full((G * det_cap * 32 + 64, ), int(SENT), dtype=torch.int32, device=dev)
    cnt = torch.full((G + 16, ), -77, dtype=torch.int32, device=dev)
    a.det_in, a.count_in, a.group = t_det.data_ptr(), t_cin.data_ptr(), t_grp.data_ptr()
    a.G, a.det_cap, a.num_classes, a.iou_thresh, a.max_dets = G, det_cap, NC, thr, max_dets
    a.write_global, a.do_postprocess = write_global, do_post
    a.work, a.sbox, a.mask, a.meta, a.det_out, a.count_out = work.data_ptr(), sbox.data_ptr(), mask.data_ptr(), meta.data_ptr(), det_out.data_ptr(), cnt.data_ptr()
    hip.check(lib.dd3d_bev_nms_aggregate(C.byref(a), hip.current_stream()), "bev")
    torch.cuda.synchronize()
    det_out, cnt = det_out.cpu().numpy(), cnt.cpu().numpy()
    assert (det_out[G * det_cap * 32:] == SENT).all() and (cnt[G:] == -77).all()
    out = dict(det_in=det_in, cin=np.minimum(cin, det_cap), count=cnt[:G], det_out=det_out[:G * det_cap * 32].view(F32).reshape(G, det_cap, 32),
               work=work.cpu().numpy(), sbox=sbox.cpu().numpy(), mask=mask.cpu().numpy().view(np.uint64), meta=meta.cpu().numpy(),
               poses=poses, osz=osz, group=group, thr=thr, max_dets=max_dets, mw=mcap // 64)
    return out


def iou_margin(b1, b2):
    return IOU_MARGIN + IOU_EPS_AREA / max(min(float(b1[2]), float(b1[3]), float(b2[2]), float(b2[3])), 1e-3)**2


def _bit(mask, mw, i, j):
    """Mask decision of sorted positions i < j (row form above the diagonal block, column form on it)."""
    if i // 64 == j // 64:
        return bool((int(mask[j * mw + j // 64]) >> (i % 64)) & 1)
    return bool((int(mask[i * mw + j // 64]) >> (j % 64)) & 1)


def check_bev(out, case, iou_pairs=None):
    """Sort order, every same-category mask bit against IoU64, greedy keep, cap, per-image ordered write-out, unwritten rows."""
    n = int(out["cin"].sum())
    G, det_cap = out["det_out"].shape[:2]
    assert out["meta"][0] == n and out["meta"][1] == 0
    # stable descending score_3d order, ties by the concatenated index
    rows = np.concatenate([out["det_in"][g, :out["cin"][g]] for g in range(G)]) if n else np.zeros((0, 32), F32)
    order = np.lexsort((np.arange(n), -rows[:, 5].astype(np.float64))) if n else np.zeros(0, np.int64)
    sb = out["sbox"][:n]
    assert np.array_equal(sb[:, 6].view(np.int32), order), (case, "sort order")
    cat = sb[:, 5].view(np.int32)
    img_of = np.repeat(np.arange(G), out["cin"])
    assert np.array_equal(cat, (rows[order, 6].astype(np.int32) + out["group"][img_of[order]] * NC))
    mask = out["mask"].reshape(-1)
    # greedy over the sorted list with float64 IoU decisions, the kernel's bit where the IoU is within the margin
    removed = np.zeros(n, dtype=bool)
    keep = []
    by_cat = {}
    for p in range(n):
        by_cat.setdefault(int(cat[p]), []).append(p)
    n_pairs, marg = 0, 0
    for p in range(n):
        if removed[p]:
            continue
        keep.append(p)
        for q in by_cat[int(cat[p])]:
            if q <= p:
                continue
            i64 = bev_iou64.iou(sb[p, :5].astype(np.float64), sb[q, :5].astype(np.float64))
            if iou_pairs is not None:
                iou_pairs.append(abs(i64 - out["thr"]) - iou_margin(sb[p], sb[q]))
            bit = _bit(mask, out["mw"], p, q)
            n_pairs += 1
            if abs(i64 - out["thr"]) <= iou_margin(sb[p], sb[q]):
                if bit != (i64 > out["thr"]):
                    marg += 1
                    _REPORTED.append((case, p, q, i64))
                dec = bit
            else:
                assert bit == (i64 > out["thr"]), (case, "IoU decision", p, q, i64, sb[p, :5], sb[q, :5])
                dec = bit
            if dec:
                removed[q] = True
    assert marg <= max(2, n_pairs // 200), (case, "too many within-margin IoU disagreements", marg)
    if marg:
        print(f"[bev] {case}: {marg} IoU decisions within the margin of the threshold differ from float64: {_REPORTED[-marg:][:6]}")
    cap = out["max_dets"] if out["max_dets"] > 0 else n
    kept_idx = set(order[np.array(keep[:cap], dtype=np.int64)].tolist())
    # write-out: each image's survivors in their original order
    gid = 0
    for g in range(G):
        m = int(out["cin"][g])
        want = [i for i in range(gid, gid + m) if i in kept_idx]
        gid += m
        k = int(out["count"][g])
        assert k == len(want), (case, g, k, len(want))
        got = out["det_out"][g, :k]
        assert np.array_equal(got[:, ID_FIELD].astype(np.int64), np.array(want, dtype=np.int64)), (case, "output order", g)
        assert (out["det_out"][g, k:].view(np.int32) == SENT).all(), (case, "row beyond count_out written", g)
        src = rows[np.array(want, dtype=np.int64)] if want else np.zeros((0, 32), F32)
        assert np.array_equal(got[:, 4:22].view(np.int32), src[:, 4:22].view(np.int32))
        assert (got[:, 29:32] == 0).all()
    return kept_idx


def check_global(out, case):
    """Fields 22-28 against float64 boxes_to_global (write_global) or zeros."""
    from oracle import nuscenes_oracle as N
    G = out["det_out"].shape[0]
    err_q = err_t = 0.0
    for g in range(G):
        k = int(out["count"][g])
        if k == 0:
            continue
        got = out["det_out"][g, :k]
        src = out["det_in"][g][got[:, ID_FIELD].astype(np.int64) - int(out["cin"][:g].sum())].astype(np.float64)
        tvec = np.stack([src[:, 14] * src[:, 16], src[:, 15] * src[:, 16], src[:, 16]], 1)  # K^-1 [u, v, 1] * depth, inv_K = I
        vec = torch.from_numpy(np.concatenate([src[:, 10:14], tvec, src[:, 17:20]], 1))
        p = out["poses"][g].astype(np.float64)
        ref = N.boxes_to_global(vec, p[:4].tolist(), p[4:].tolist()).numpy()
        assert ref.dtype == np.float64
        q, t = got[:, 22:26].astype(np.float64), got[:, 26:29].astype(np.float64)
        err_q = max(err_q, float(np.minimum(np.abs(q - ref[:, :4]).max(1), np.abs(q + ref[:, :4]).max(1)).max()))
        scale = np.maximum(np.maximum(1.0, np.linalg.norm(tvec, axis=1))[:, None], np.abs(ref[:, 4:7]))
        err_t = max(err_t, float((np.abs(t - ref[:, 4:7]) / scale).max()))
    print(f"[bev] {case}: global quat err {err_q:.3g}, tvec err {err_t:.3g}")
    assert err_q <= TOL_GQUAT and err_t <= TOL_GT, (case, err_q, err_t)


# ------------------------------------------------------------------------------------------------------------------------ scenes
POSE0 = (35.0, (412.5, 1103.25, 1.5))


def pair_scene(rng, kinds, npairs):
    """`npairs` pairs of world boxes, each pair one kind: returns boxes [2*npairs, 7] in front of POSE0's camera."""
    boxes = []
    h = math.radians(POSE0[0])
    fwd, left = np.array([math.cos(h), math.sin(h)]), np.array([-math.sin(h), math.cos(h)])
    for i in range(npairs):
        kind = kinds[i % len(kinds)]
        c = np.array(POSE0[1][:2]) + fwd * rng.uniform(8, 70) + left * rng.uniform(-30, 30)
        yaw = rng.uniform(-180, 180)
        W, L = rng.uniform(1.5, 3.0), rng.uniform(3.5, 6.0)
        a, b = (c[0], c[1], 0.8, W, L, 1.6, yaw), None
        ax = np.array([math.cos(math.radians(yaw)), math.sin(math.radians(yaw))])
        pe = np.array([-ax[1], ax[0]])
        if kind == "identical":
            b = a
        elif kind == "shared_edge":
            cc = c + pe * W
            b = (cc[0], cc[1], 0.8, W, L, 1.6, yaw)
        elif kind == "inside":
            b = (c[0] + 0.1, c[1] - 0.1, 0.8, W * 0.5, L * 0.5, 1.6, yaw)
        elif kind == "square90":
            a = (c[0], c[1], 0.8, W, W, 1.6, yaw)
            b = (c[0], c[1], 0.8, W, W, 1.6, yaw + 90.0)
        elif kind == "cross45":
            b = (c[0], c[1], 0.8, W, L, 1.6, yaw + 45.0)
        elif kind == "near_parallel":
            cc = c + pe * W * 0.3
            b = (cc[0], cc[1], 0.8, W, L, 1.6, yaw + rng.uniform(-0.01, 0.01))
        elif kind == "sliver":
            a = (c[0], c[1], 0.8, 0.01, L, 1.6, yaw)
            b = (c[0] + 0.001, c[1], 0.8, 0.01, L, 1.6, yaw + 0.5)
        elif kind == "zero_area":
            a = (c[0], c[1], 0.8, 0.0, L, 1.6, yaw)
            b = (c[0], c[1], 0.8, W, L, 1.6, yaw)
        elif kind == "disjoint":
            cc = c + ax * (L + 1.0)
            b = (cc[0], cc[1], 0.8, W, L, 1.6, yaw)
        else:  # "near_thr": shifted along the axis (and by W/4 sideways, so no edges are collinear) to an IoU around 0.3
            s = L * (1.0 - 0.6 / (1.3 * 0.75)) * rng.uniform(0.97, 1.03)
            cc = c + ax * s + pe * 0.25 * W
            b = (cc[0], cc[1], 0.8, W, L, 1.6, yaw)
        boxes += [a, b]
    return np.array(boxes, dtype=np.float64)


KINDS = ["identical", "shared_edge", "inside", "square90", "cross45", "near_parallel", "sliver", "zero_area", "disjoint", "near_thr"]


def _images_of_pairs(rng, n, per_img, kinds=KINDS, tie=False):
    """n boxes in pairs, per_img boxes (an even number) per image, one category per pair (class = pair index inside the image)."""
    pose = make_pose(*POSE0)
    boxes = pair_scene(rng, kinds, (n + 1) // 2)[:n]
    imgs = []
    for s in range(0, n, per_img):
        m = min(per_img, n - s)
        sc = rng.uniform(0.05, 0.95, m).astype(F32)
        if tie:
            sc = np.round(sc * 4) / 4 + F32(0.01)
        cls = (np.arange(m) // 2).astype(F32)
        imgs.append(rows_for(boxes[s:s + m], pose, sc, cls, rng))
    return imgs, [pose] * len(imgs)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1023, 1024, 1025, 4096, 8192])
def test_sizes_and_geometry(hiplib, n):
    rng = np.random.default_rng(n)
    per_img = 16 if n <= 1025 else 8  # one category (class = pair index < NC) per pair; 8192 boxes -> 1024 images
    imgs, poses = _images_of_pairs(rng, n, per_img)
    if not imgs:
        imgs, poses = [np.zeros((0, 32), F32)], [make_pose(*POSE0)]
    out = run_bev(imgs, det_cap=max(per_img, 1), poses=poses, thr=0.3)
    check_bev(out, f"n={n}")
    check_global(out, f"n={n}")


def test_overflow_8193_reports_minus_one_everywhere(hiplib):
    rng = np.random.default_rng(8193)
    imgs, poses = _images_of_pairs(rng, 8193, 20)
    assert len(imgs) == 410
    out = run_bev(imgs, det_cap=21, poses=poses)
    assert out["meta"][1] == 1
    assert (out["count"] == -1).all()
    assert (out["det_out"].view(np.int32) == SENT).all()  # no other output


def test_many_slots_few_boxes(hiplib):
    """G * det_cap > 8192 with few boxes: the mask rows stride min(ncap, 8192) / 64 words."""
    rng = np.random.default_rng(5)
    imgs, poses = _images_of_pairs(rng, 600, 2)
    imgs = imgs + [np.zeros((0, 32), F32)] * 100
    poses = poses + [make_pose(*POSE0)] * 100
    out = run_bev(imgs, det_cap=40, poses=poses)
    check_bev(out, "G*det_cap > 8192")


def test_iou_threshold_zero_disjoint_and_touching_survive(hiplib):
    """Axis-aligned boxes under an exact pose (0/+-1 rotation, depths that are powers of two, half-integer coordinates): every
    float32 step of the transform and of the category offsets is exact, so edge-touching boxes have IoU exactly 0."""
    pose = np.array([0.5, -0.5, 0.5, -0.5, 512.0, 1024.0, 2.0], dtype=F32)  # camera z -> world x, x -> -y, y -> -z
    assert np.allclose(_rot(pose[:4].astype(np.float64)), _CAM)
    boxes = []
    for i in range(400):
        x, y, yaw = 512.0 + 2.0**(3 + i % 4), 1000.0 + 5.0 * (i // 4), 180.0 * (i % 3 == 0)
        gap = 0.0 if i % 2 == 0 else 0.5  # touching along the 1 m side, or disjoint
        boxes += [(x, y, 1.0, 1.0, 2.0, 1.0, yaw), (x, y + 1.0 + gap, 1.0, 1.0, 2.0, 1.0, yaw)]
    boxes = np.array(boxes)
    rng = np.random.default_rng(1)
    imgs = []
    for s in range(0, len(boxes), 20):
        imgs.append(rows_for(boxes[s:s + 20], pose, rng.uniform(0.1, 0.9, 20).astype(F32), (np.arange(20) // 2).astype(F32)))
    out = run_bev(imgs, det_cap=20, poses=[pose] * len(imgs), thr=0.0)
    kept = check_bev(out, "iou_thresh=0")
    assert len(kept) == len(boxes), "a pair with IoU exactly 0 was suppressed at iou_thresh = 0"


def test_cap_inside_a_block_with_ties_and_across_images(hiplib):
    rng = np.random.default_rng(77)
    imgs, poses = _images_of_pairs(rng, 600, 20, kinds=["disjoint", "identical", "near_thr"], tie=True)
    full = check_bev(run_bev(imgs, det_cap=20, poses=poses), "no cap")
    for max_dets in (1, 100, 129, 190, 5000):  # 100 and 190: inside a 64-row block of the sorted list
        out = run_bev(imgs, det_cap=20, poses=poses, max_dets=max_dets)
        kept = check_bev(out, f"max_dets={max_dets}")
        assert len(kept) == min(max_dets, len(full)) and kept <= full


def test_count_in_clamp_empty_images_and_categories(hiplib):
    rng = np.random.default_rng(300)
    pose = make_pose(*POSE0)
    imgs, groups = [], []
    base = pair_scene(rng, ["identical"], 150)  # 150 identical pairs
    for g in range(300):
        if g % 3:  # two of three images empty, in the middle of the walk
            imgs.append(np.zeros((0, 32), F32))
        else:
            j = g // 6  # images g and g + 3 (different samples) see the same boxes
            two = base[2 * (j % 150):2 * (j % 150) + 2]
            # the same class in two samples (different groups) and two classes in one sample: none suppresses another
            r = rows_for(np.concatenate([two, two]), pose, np.array([0.9, 0.8, 0.7, 0.6], F32), np.array([1, 1, 2, 2], F32), rng)
            imgs.append(r)
        groups.append(g // 2)
    out = run_bev(imgs, det_cap=4, poses=[pose] * 300, group=groups)
    kept = check_bev(out, "300 images")
    assert len(kept) == 2 * 100  # one survivor per identical pair, i.e. per (class, image): nothing across classes or samples
    # count_in above det_cap is clamped to det_cap
    out = run_bev(imgs[:6], det_cap=3, poses=[pose] * 6, count_in=[4, 0, 0, 4, 0, 0])
    assert (out["cin"] == [3, 0, 0, 3, 0, 0]).all()
    check_bev(out, "count_in > det_cap")


def test_write_global_and_postprocess(hiplib):
    rng = np.random.default_rng(8)
    imgs, _ = _images_of_pairs(rng, 200, 20, kinds=["disjoint"])
    # camera-frame rows are valid under any pose: random headings and translations of hundreds of metres
    poses = [make_pose(rng.uniform(-180, 180), (rng.uniform(-900, 900), rng.uniform(-900, 900), 1.2)) for _ in imgs]
    out = run_bev(imgs, det_cap=20, poses=poses, write_global=1)
    check_bev(out, "write_global")
    check_global(out, "write_global")
    out0 = run_bev(imgs, det_cap=20, poses=poses, write_global=0)
    check_bev(out0, "no write_global")
    for g in range(len(imgs)):
        assert (out0["det_out"][g, :out0["count"][g], 22:29] == 0).all()
    # do_postprocess: scale by (out_w / in_w, out_h / in_h), clip to the output, drop boxes that end up empty
    for r in imgs:
        r[0, 0:4] = (5000.0, 10.0, 6000.0, 40.0)  # right of the image: clipped to zero width
        r[2, 0:4] = (-50.0, -20.0, -10.0, 30.0)  # left of it
        r[4, 0:4] = (30.0, 30.0, 30.0, 90.0)  # zero width in the input
    osz = np.tile(np.array([375.0, 1242.0, 900.0, 1600.0], F32), (len(imgs), 1))
    ref = run_bev(imgs, det_cap=20, poses=poses, write_global=0)
    out = run_bev(imgs, det_cap=20, poses=poses, write_global=0, do_post=1, out_size=osz)
    sx, sy = F32(1600.0) / F32(1242.0), F32(900.0) / F32(375.0)
    for g in range(len(imgs)):
        r = ref["det_out"][g, :ref["count"][g]]
        x1, x2 = np.minimum(np.maximum(r[:, 0] * sx, F32(0)), F32(1600)), np.minimum(np.maximum(r[:, 2] * sx, F32(0)), F32(1600))
        y1, y2 = np.minimum(np.maximum(r[:, 1] * sy, F32(0)), F32(900)), np.minimum(np.maximum(r[:, 3] * sy, F32(0)), F32(900))
        ok = ((x2 - x1) > 0) & ((y2 - y1) > 0)
        assert ok.sum() < len(r)
        got = out["det_out"][g, :out["count"][g]]
        assert np.array_equal(got[:, ID_FIELD], r[ok, ID_FIELD])
        assert np.array_equal(got[:, 0:4], np.stack([x1, y1, x2, y2], 1)[ok])


def test_random_scene_matches_the_oracle(hiplib):
    """Random pairs (several kinds) through oracle.nuscenes_sample_aggregate: the kept set must be identical."""
    from oracle import nuscenes_oracle as N
    rng = np.random.default_rng(123)
    imgs, poses = _images_of_pairs(rng, 240, 20, kinds=["disjoint", "cross45", "inside", "near_parallel", "identical"])
    groups = [g // 2 for g in range(len(imgs))]
    pairs = []  # float64 IoU of every evaluated pair
    out = run_bev(imgs, det_cap=20, poses=poses, group=groups, thr=0.3)
    kept = check_bev(out, "oracle scene", iou_pairs=pairs)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    inst = []
    for r in imgs:
        inst.append(dict(pred_classes=t(r[:, 6].astype(np.int64)), scores_3d=t(r[:, 5]),
                         pred_boxes3d=dict(quat=t(r[:, 10:14]), proj_ctr=t(r[:, 14:16]), depth=t(r[:, 16:17]), size=t(r[:, 17:20]),
                                           inv_intrinsics=t(np.tile(np.eye(3, dtype=F32), (len(r), 1, 1))))))
    grp = OrderedDict()
    for g, s in enumerate(groups):
        grp.setdefault(s, []).append(g)
    _, agg = N.nuscenes_sample_aggregate(inst, grp, NC, [(p[:4].tolist(), p[4:].tolist()) for p in poses], 0.3)
    ref = set(agg["keep"].tolist())
    if ref != kept:
        assert min(pairs, default=1.0) <= 0.0, ("kept set differs from the oracle's with no IoU near the threshold", sorted(ref ^ kept))
        print("[bev] oracle scene: kept sets differ, with an IoU within the margin of the threshold")


def test_record_addressing_is_bit_identical_to_dense(hiplib):
    rng = np.random.default_rng(17)
    imgs, _ = _images_of_pairs(rng, 120, 20, kinds=["disjoint", "cross45", "identical"])
    poses = [make_pose(POSE0[0] + 3.0 * g, (POSE0[1][0] + 0.25 * g, POSE0[1][1] - 0.5 * g, 1.5)) for g in range(len(imgs))]
    osz = np.array([[375.0 + g, 1242.0, 900.0, 1600.0 - g] for g in range(len(imgs))], F32)
    dense = run_bev(imgs, det_cap=20, poses=poses, do_post=1, out_size=osz)
    check_bev(dense, "dense records")
    rec = run_bev(imgs, det_cap=20, poses=poses, do_post=1, out_size=osz, record=(3, 4, 5))
    assert np.array_equal(dense["count"], rec["count"])
    assert np.array_equal(dense["det_out"].view(np.int32), rec["det_out"].view(np.int32))
