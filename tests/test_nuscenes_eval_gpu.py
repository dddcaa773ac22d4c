"""nuScenes detection metrics on the MI355X: the matching kernel (dd3d_nusc_center_match) at its seam against the devkit's sequential
loop, decision for decision; the engine against the plain-Python oracle (tests/nuscenes_eval_oracle.py); NuscenesDD3D -> process ->
evaluate end to end on the synthetic nuScenes golden inputs; and the distributed gather (gloo, two ranks on the one GPU)."""
import ctypes as C
import json
import math
import multiprocessing as mp
import os

import numpy as np
import pytest
import torch

from tests import nuscenes_eval_oracle as O
from tests.test_nuscenes_eval import check_ex1, check_ex2, check_ex3, ex1, ex2, ex3, random_set, same_metrics, sequential_match

pytestmark = pytest.mark.gpu

SENTINEL = -777
PAD = 64


def launch(segments, ths, n_pred_extra=0):
    """segments: [(pred_xy [n][2], gt_xy [m][2])].  Returns (rc, match [n_thr][n_pred]); the match buffer is framed by sentinels,
    which must survive."""
    pb = np.concatenate([[0], np.cumsum([len(p) for p, _ in segments])]).astype(np.int32)
    gb = np.concatenate([[0], np.cumsum([len(g) for _, g in segments])]).astype(np.int32)
    pred = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p, _ in segments]) if segments else np.zeros((0, 2))
    gt = np.concatenate([np.asarray(g, np.float64).reshape(-1, 2) for _, g in segments]) if segments else np.zeros((0, 2))
    return launch_raw(pred, gt, pb, gb, ths, n_pred=len(pred) + n_pred_extra)


def launch_raw(pred, gt, pb, gb, ths, n_pred=None, n_thr=None):
    from dd3d_amd import hip
    n_pred = len(pred) if n_pred is None else n_pred
    n_thr = len(ths) if n_thr is None else n_thr
    dev = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dt)  # noqa: E731
    pred_d = dev(np.concatenate([pred, np.zeros((max(0, n_pred - len(pred)), 2))]) if len(pred) or n_pred else np.zeros((1, 2)), torch.float64)
    gt_d = dev(gt if len(gt) else np.zeros((1, 2)), torch.float64)
    pb_d, gb_d = dev(pb, torch.int32), dev(gb, torch.int32)
    n_out = max(1, n_thr) * n_pred
    buf = torch.full((n_out + 2 * PAD,), SENTINEL, dtype=torch.int32, device="cuda")
    args = hip.NuscMatchArgs(pred_xy=pred_d.data_ptr(), gt_xy=gt_d.data_ptr(), pred_begin=pb_d.data_ptr(), gt_begin=gb_d.data_ptr(),
                             pred_begin_host=pb.ctypes.data_as(C.c_void_p), gt_begin_host=gb.ctypes.data_as(C.c_void_p), n_seg=len(pb) - 1,
                             n_pred=n_pred, n_gt=len(gt), n_thr=n_thr)
    for i, t in enumerate(ths[:8]):
        args.thr[i] = t
    rc = hip.lib().dd3d_nusc_center_match(C.byref(args), buf[PAD:].data_ptr(), hip.current_stream())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:PAD] == SENTINEL).all() and (host[PAD + n_out:] == SENTINEL).all(), "match written outside [n_thr][n_pred]"
    return rc, host[PAD:PAD + n_out].reshape(max(1, n_thr), n_pred)


def want_match(segments, ths):
    out = []
    g0 = 0
    for t in ths:
        row = []
        g0 = 0
        for p, g in segments:
            row += [g0 + m if m >= 0 else -1 for m in sequential_match(np.asarray(p).tolist(), np.asarray(g).tolist(), t)]
            g0 += len(g)
        out.append(row)
    return np.array(out, dtype=np.int64).reshape(len(ths), -1)


THS = [0.5, 1.0, 2.0, 4.0]


def near(rng, g, n, sigma):
    g = np.asarray(g).reshape(-1, 2)
    if len(g) == 0:
        return rng.uniform(-2000, 2000, (n, 2))
    return g[rng.integers(len(g), size=n)] + rng.normal(0, sigma, (n, 2))


def test_kernel_random_segments_at_map_scale(hiplib):
    rng = np.random.default_rng(1)
    segs = []
    for _ in range(300):
        ng = int(rng.choice([0, 1, 3, 10, 40]))
        c = rng.uniform(-2000, 2000, 2)
        g = c + rng.uniform(-30, 30, (ng, 2))
        segs.append((near(rng, g, int(rng.integers(0, 60)), rng.choice([0.3, 1.0, 3.0])), g))
    for ths in (THS, [0.25, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 8.0]):
        rc, got = launch(segs, ths)
        want = want_match(segs, ths)
        assert rc == 0 and np.array_equal(got, want)
        assert 0.1 < (want >= 0).mean() < 0.9


def test_kernel_edge_cases(hiplib):
    """Equidistant GT (within a lane's chunks and across lanes), distances exactly at a threshold and one float64 step either side,
    distances one bit apart, 63 / 64 / 65 / 4096 GT, 500 predictions, segments whose GT are all taken early, samples without GT."""
    rng = np.random.default_rng(2)
    segs = []
    o = np.array([1234.5, -987.25])
    segs.append(([o, o, o], [o + (1, 0), o - (1, 0), o + (0, 1)]))  # three GT at distance 1: taken in index order
    ring = np.zeros((70, 2)) + o + 50
    ring[[67, 3, 5, 66]] = o + [(0, 0.75), (0.75, 0), (-0.75, 0), (0, -0.75)]  # same lane (3, 67) and other lanes, all at 0.75
    segs.append(([o] * 5, ring))
    for th in THS:  # GT at the origin: the distance is exactly the x offset
        for x in (th, np.nextafter(th, 0.0), np.nextafter(th, np.inf)):
            assert math.sqrt(x * x) == x
            segs.append(([(x, 0.0)], [(0.0, 0.0)]))
    d = 1.5
    segs.append(([(0.0, 0.0)] * 3, [(np.nextafter(d, np.inf), 0.0), (d, 0.0), (0.0, np.nextafter(d, 0.0))]))  # last-bit differences
    for ng in (63, 64, 65, 4096):
        g = o + rng.uniform(-40, 40, (ng, 2))
        segs.append((near(rng, g, 120 if ng == 4096 else 90, 0.8), g))
    g = o + rng.uniform(-60, 60, (300, 2))
    segs.append((near(rng, g, 500, 1.0), g))  # 500 predictions
    segs.append((near(rng, [o], 50, 0.1), [o, o + (0.05, 0), o - (0.05, 0)]))  # all GT taken after three predictions
    segs.append((rng.uniform(-2000, 2000, (20, 2)), np.zeros((0, 2))))  # no GT
    segs.append((np.zeros((0, 2)), o + rng.uniform(-5, 5, (7, 2))))  # GT, no prediction
    rc, got = launch(segs, THS)
    want = want_match(segs, THS)
    assert rc == 0 and np.array_equal(got, want)
    assert got[:, :3].tolist() == [[-1, -1, -1], [-1, -1, -1], [0, 1, 2], [0, 1, 2]]  # distance 1 is not < 1.0
    assert got[1:, 3:8].tolist() == [[3 + 3, 3 + 5, 3 + 66, 3 + 67, -1]] * 3  # 0.75 ties: lowest index first
    for i, th in enumerate(THS):  # at the threshold no match, one step below a match, one step above none; every larger one matches
        t, r, g0 = THS.index(th), 8 + 3 * i, 73 + 3 * i
        assert got[t, r:r + 3].tolist() == [-1, g0 + 1, -1], (th, got[t, r:r + 3])
        assert all(got[u, r:r + 3].tolist() == [g0, g0 + 1, g0 + 2] for u in range(t + 1, 4))
    assert got[2:, 20:23].tolist() == [[87, 86, 85]] * 2  # distances one bit apart: the smaller first, whatever the index
    assert (got[:, -20:] == -1).all()


def test_kernel_is_deterministic_and_rejects_bad_arguments(hiplib):
    from dd3d_amd import hip
    rng = np.random.default_rng(3)
    g = rng.uniform(-100, 100, (50, 2))
    segs = [(near(rng, g, 100, 1.0), g)] * 3
    a, b = launch(segs, THS), launch(segs, THS)
    assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1])
    pred, gt = rng.uniform(0, 10, (600, 2)), rng.uniform(0, 10, (4200, 2))
    err = lambda: hip.lib().dd3d_last_error().decode()  # noqa: E731
    cases = [
        (dict(pb=np.array([0, 5], np.int32), gb=np.array([0, 5], np.int32), ths=THS, n_thr=0), "n_thr"),
        (dict(pb=np.array([0, 5], np.int32), gb=np.array([0, 5], np.int32), ths=THS * 3, n_thr=9), "n_thr"),
        (dict(pb=np.array([0, 501], np.int32), gb=np.array([0, 5], np.int32), ths=THS), "501 predictions"),
        (dict(pb=np.array([0, 5], np.int32), gb=np.array([0, 4097], np.int32), ths=THS), "4097 ground-truth"),
        (dict(pb=np.array([0, 5, 3, 8], np.int32), gb=np.array([0, 1, 2, 3], np.int32), ths=THS), "decrease"),
        (dict(pb=np.array([0, 5, 9], np.int32), gb=np.array([0, 1, 2], np.int32), ths=THS, n_pred=8), "past"),
        (dict(pb=np.array([-1, 5], np.int32), gb=np.array([0, 1], np.int32), ths=THS), "negative"),
    ]
    for kw, msg in cases:
        n_pred = kw.pop("n_pred", None)
        rc, out = launch_raw(pred[:n_pred or 600], gt, kw["pb"], kw["gb"], kw["ths"], n_pred=n_pred, n_thr=kw.get("n_thr"))
        assert rc < 0 and msg in err(), (msg, err())
        assert (out == SENTINEL).all()  # nothing enqueued
    assert launch([], THS)[0] == 0


# ---- the engine ----------------------------------------------------------------------------------------------------------------------
def gpu_engine(results, gt, ego, racks=None, timings=None):
    from dd3d_amd.evaluators import NuscenesDetectionEval, NuscenesGroundTruth
    return NuscenesDetectionEval(NuscenesGroundTruth(gt, ego, racks)).evaluate(results, timings=timings)


def test_engine_worked_examples(hiplib):
    check_ex1(gpu_engine(*ex1()))
    for a_first in (True, False):
        check_ex2(gpu_engine(*ex2(a_first)), a_first)
    check_ex3(gpu_engine(*ex3()))


def test_engine_matches_oracle(hiplib):
    res, gt, ego, racks = random_set(np.random.default_rng(21), 150)
    timings = {}
    got = gpu_engine(res, gt, ego, racks, timings=timings)
    want = O.evaluate(res, gt, ego, racks)
    same_metrics(got, want)
    assert sum(v > 0 for d in want["label_aps"].values() for v in d.values()) >= 36
    assert set(timings) >= {"prepare", "upload", "kernel", "kernel_events", "accumulate"}
    again = gpu_engine(res, gt, ego, racks)
    assert json.dumps(again, default=float) == json.dumps(got, default=float)


# ---- NuscenesDD3D -> process -> evaluate ----------------------------------------------------------------------------------------------
def _forward_and_process(ev, inputs):
    from tests.util import bundle, gpu_model
    cfg, sd = bundle("dd3d_nusc_dla34", "dla34_nusc")
    model = gpu_model(cfg, sd, use_graph=False)
    with torch.no_grad():
        out = model(inputs)
    ev.process(inputs, out)
    return ev


def _self_gt(results):
    """GT = the detections themselves (same translation, size, rotation, velocity, attribute).  The synthetic weights put the
    detections far beyond the class ranges from the inputs' ego poses, so each sample's ego translation is placed at its top-scoring
    detection: the range filter then keeps that one and whatever lies within range of it."""
    from dd3d_amd.evaluators import NuscenesGroundTruth
    gt = {t: [dict(b, detection_score=-1.0, num_pts=1) for b in boxes] for t, boxes in results.items()}
    ego = {t: (max(boxes, key=lambda b: b["detection_score"])["translation"] if boxes else [0.0, 0.0, 0.0]) for t, boxes in results.items()}
    return NuscenesGroundTruth(gt, ego)


def test_end_to_end_on_golden_inputs(hiplib, tmp_path):
    from dd3d_amd.evaluators import NuscenesEvaluator
    from tests.golden.make_golden import case_inputs
    inputs = case_inputs(6, 128, 224, False, "nusc")
    ev = _forward_and_process(NuscenesEvaluator(None, "nusc_val", None), inputs)
    results = dict(ev._nusc_sample_results)
    assert sum(len(v) for v in results.values()) > 10
    gt = _self_gt(results)
    gt.to_json(tmp_path / "gt.json")
    got = NuscenesEvaluator(None, "nusc_val", str(tmp_path / "out"), ground_truth=str(tmp_path / "gt.json"))
    got._predictions_as_json, got._nusc_sample_results = ev._predictions_as_json, ev._nusc_sample_results
    r = got.evaluate()
    assert (tmp_path / "out" / "nuscenes_submission.json").exists()
    kept = O.filter_boxes(results, gt.ego_translation, {})
    present = {b["detection_name"] for bs in kept.values() for b in bs}
    assert len(present) >= 1, {c: sum(b['detection_name'] == c for bs in results.values() for b in bs) for c in O.CLASS_NAMES}
    for c in O.CLASS_NAMES:
        for th in O.DIST_THS:
            assert abs(r["label_aps"][c][th] - (1.0 if c in present else 0.0)) < 1e-12, (c, th)
        for m in O.TP_METRICS:
            v = r["label_tp_errors"][c][m]
            if (c == "traffic_cone" and m in ("attr_err", "vel_err", "orient_err")) or (c == "barrier" and m in ("attr_err", "vel_err")):
                assert math.isnan(v), (c, m)
            else:
                assert abs(v - (0.0 if c in present else 1.0)) < 1e-12, (c, m, v)
    same_metrics(r, O.evaluate(results, gt.boxes, gt.ego_translation))


# ---- two ranks ----------------------------------------------------------------------------------------------------------------------
def _rank_main(rank, init_file, data_path, out_dir):
    import torch.distributed as dist
    from dd3d_amd.evaluators import NuscenesEvaluator
    dist.init_process_group("gloo", init_method="file://" + init_file, rank=rank, world_size=2)
    try:
        d = json.load(open(data_path))
        ev = NuscenesEvaluator(None, "nusc_val", out_dir, ground_truth=d["gt_path"], distributed=True)
        tokens = list(d["results"])
        half = tokens[:len(tokens) // 2] if rank == 0 else tokens[len(tokens) // 2:]
        for t in half:
            ev._nusc_sample_results[t] = d["results"][t]
            ev._predictions_as_json.append({"token": t, "rank": rank})
        res = ev.evaluate()
        with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
            json.dump(None if res is None else res, f, default=float)
    finally:
        dist.destroy_process_group()


def test_distributed_gather_two_ranks(hiplib, tmp_path):
    from dd3d_amd.evaluators import NuscenesGroundTruth
    res, gt, ego, racks = random_set(np.random.default_rng(31), 40)
    g = NuscenesGroundTruth(gt, ego, racks)
    g.to_json(tmp_path / "gt.json")
    json.dump({"results": res, "gt_path": str(tmp_path / "gt.json")}, open(tmp_path / "data.json", "w"))
    one = gpu_engine(res, gt, ego, racks)
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_main, args=(r, str(tmp_path / "rdv"), str(tmp_path / "data.json"), str(tmp_path))) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(timeout=600)
    alive = [pr for pr in procs if pr.is_alive()]
    for pr in alive:
        pr.kill()
    assert not alive and [pr.exitcode for pr in procs] == [0, 0]
    assert json.load(open(tmp_path / "rank1.json")) is None
    assert open(tmp_path / "rank0.json").read() == json.dumps(one, default=float)  # (a string compare: NaN errors included)
    assert [p["rank"] for p in json.load(open(tmp_path / "bbox3d_predictions.json"))] == [0] * 20 + [1] * 20
    assert list(json.load(open(tmp_path / "nuscenes_submission.json"))["results"]) == list(res)
