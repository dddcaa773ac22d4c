"""KITTI AP engine, host side and rules (no GPU): the plain-Python oracle (tests/kitti_ap_oracle.py) against the reference's own
results (tests/golden/kitti_ap.npz, tests/golden/make_kitti_ap_golden.py); the product's host pieces (ignore codes, thresholds,
formatting, shards, AP arithmetic) against the same golden; the wave-parallel selection rule of dd3d_amd/csrc/kitti_ap.hip against
the reference's sequential state machine; the C entry points' argument checks."""
import ctypes as C
import json
import os

import numpy as np
import pandas as pd
import pytest

from tests import kitti_ap_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "kitti_ap.npz")
CLASSES = ["Car", "Pedestrian", "Cyclist", "Van", "Truck"]
ID_TO_NAME = dict(enumerate(CLASSES))
THRESHOLDS = [0.5, 0.7]


def load_golden():
    return dict(np.load(GOLDEN, allow_pickle=False))


def golden_frames(g):
    """The engine set's per-image KITTI rows as DataFrames (ground truth 15 columns, predictions 16)."""
    out = []
    for prefix in ("gt", "dt"):
        names, vals, counts = g[prefix + "_names"], g[prefix + "_values"], g[prefix + "_counts"]
        frames, k = [], 0
        for n in counts:
            rows = [[str(names[k + i])] + vals[k + i].tolist() for i in range(n)]
            frames.append(pd.DataFrame(rows))
            k += n
        out.append(frames)
    return out


def golden_annos(g):
    from dd3d_amd.evaluators.kitti_ap import KITTIEvaluationEngine
    gt_frames, dt_frames = golden_frames(g)
    gt = [KITTIEvaluationEngine._format(i, f, False) for i, f in enumerate(gt_frames)]
    dt = [KITTIEvaluationEngine._format(i, f, True) for i, f in enumerate(dt_frames)]
    return gt, dt


def golden_blocks(g, metric, gt, dt):
    """Per-image [det][gt] float64 overlap blocks of the reference."""
    vals = g[f"{metric}_block_values"].astype(np.float64)
    out, k = [], 0
    for a, b in zip(gt, dt):
        n, m = len(b["name"]), len(a["name"])
        out.append(vals[k:k + n * m].reshape(n, m))
        k += n * m
    return out


def golden_dict(g, prefix=""):
    return list(g[prefix + "result_keys"]), g[prefix + "result_values"]


def same_dict(got, keys, values):
    assert list(got.keys()) == keys
    v = np.array([float(x) for x in got.values()])
    assert np.array_equal(v, values, equal_nan=True), np.nonzero(~((v == values) | (np.isnan(v) & np.isnan(values))))


@pytest.fixture(scope="module")
def golden():
    return load_golden()


# ---- the oracle reproduces the reference ------------------------------------------------------------------------------------------------
def test_oracle_reproduces_reference_golden(golden):
    gt, dt = golden_annos(golden)
    assert int(golden["n_shards"]) == 51 and len(gt) == 120
    aps = {}
    for metric in ("box3d", "bev"):
        r = O.eval_metric_counts(golden_blocks(golden, metric, gt, dt), gt, dt, ID_TO_NAME, THRESHOLDS)
        for c in range(5):
            for d in range(3):
                cd = c * 3 + d
                assert np.concatenate(r["ign_gt"][c, d]).tolist() == golden["ign_gt"][cd].tolist()
                assert np.concatenate(r["ign_dt"][c, d]).tolist() == golden["ign_dt"][cd].tolist()
                for o in range(2):
                    tps = golden[f"{metric}_tp_scores"][cd, o]
                    assert [s for p in r["tp_scores"][c, d, o] for s in p] == tps[tps != -np.inf].tolist()
                    n = int(golden[f"{metric}_n_thresholds"][cd, o])
                    assert r["thresholds"][c, d, o] == golden[f"{metric}_thresholds"][cd, o, :n].tolist()
                    assert np.array_equal(r["counts"][c, d, o], golden[f"{metric}_counts"][cd, o, :n])
        assert np.array_equal(r["recall"], golden[f"{metric}_recall"], equal_nan=True)
        assert np.array_equal(r["precision"], golden[f"{metric}_precision"], equal_nan=True)
        aps[metric] = O.mean_ap(r["precision"], r["recall"])
    same_dict(O.results(aps["box3d"], aps["bev"], ID_TO_NAME, THRESHOLDS), *golden_dict(golden))


# ---- the product's host pieces ----------------------------------------------------------------------------------------------------------
def test_product_codes_thresholds_and_ap_match_golden(golden):
    from dd3d_amd.evaluators import KITTIEvaluationEngine
    from dd3d_amd.evaluators.kitti_ap import clean_kitti_data, get_thresholds
    eng = KITTIEvaluationEngine(ID_TO_NAME)
    assert eng.get_shards(120, 50) == [2] * 50 + [20] and eng.get_shards(3769, 50) == [75] * 50 + [19]
    assert eng.get_shards(7, 50) == [7] and eng.get_shards(100, 50) == [2] * 50
    gt, dt = golden_annos(golden)
    assert gt[0]["dimensions"].shape[1] == 3 and np.array_equal(gt[0]["dimensions"][:, 0], golden["gt_values"][:len(gt[0]["name"]), 9])
    p = eng._prepare(gt, dt, THRESHOLDS)
    assert np.array_equal(p.ign_gt, golden["ign_gt"]) and np.array_equal(p.ign_dt, golden["ign_dt"])
    assert p.num_valid_gt.tolist() == golden["num_valid_gt"].tolist()
    # the per-image wrapper with the reference's signature and results
    for i in (0, 1, 3, 8, 40):
        for c in range(5):
            for d in range(3):
                got = clean_kitti_data(gt[i], dt[i], c, d, ID_TO_NAME, eng._DEFAULT_KITTI_LEVEL_TO_PARAMETER)
                want = O.clean_kitti_data(gt[i], dt[i], c, d, ID_TO_NAME)
                assert got[:3] == want[:3] and len(got[3]) == len(want[3])
    for metric in ("box3d", "bev"):
        tps = golden[f"{metric}_tp_scores"]
        ths = [get_thresholds(tps[cd, o][tps[cd, o] != -np.inf], int(golden["num_valid_gt"][cd])) for cd in range(15) for o in range(2)]
        for cd in range(15):
            for o in range(2):
                n = int(golden[f"{metric}_n_thresholds"][cd, o])
                assert ths[cd * 2 + o] == golden[f"{metric}_thresholds"][cd, o, :n].tolist()
                assert ths[cd * 2 + o] == O.get_thresholds(tps[cd, o][tps[cd, o] != -np.inf].tolist(), int(golden["num_valid_gt"][cd]))
        recall, precision = eng._curves(p, ths, golden[f"{metric}_counts"])
        assert np.array_equal(recall, golden[f"{metric}_recall"], equal_nan=True)
        assert np.array_equal(precision, golden[f"{metric}_precision"], equal_nan=True)
    # AP arithmetic from the golden curves, NaN positions included
    ap3 = eng.get_mAP(golden["box3d_precision"], golden["box3d_recall"])
    apb = eng.get_mAP(golden["bev_precision"], golden["bev_recall"])
    same_dict(O.results(ap3, apb, ID_TO_NAME, THRESHOLDS), *golden_dict(golden))
    nan_p = golden["box3d_precision"].copy()
    nan_p[0, 1, 0, 0] = np.nan
    assert np.isnan(eng.get_mAP(nan_p, golden["box3d_recall"])[0, 1, 0]) == np.isnan(O.mean_ap(nan_p, golden["box3d_recall"])[0, 1, 0])


def test_get_thresholds_edge_cases():
    from dd3d_amd.evaluators.kitti_ap import get_thresholds
    rng = np.random.default_rng(3)
    assert get_thresholds(np.array([]), 0) == []
    for n_gt in (1, 2, 7, 40, 41, 100, 997):
        for n in (1, 2, 5, n_gt // 2 + 1, n_gt):
            s = np.round(rng.uniform(0, 1, n), int(rng.integers(1, 4)))
            keep = s.copy()
            assert get_thresholds(s, n_gt) == O.get_thresholds(s.tolist(), n_gt)
            assert np.array_equal(s, keep)  # the caller's array is not sorted in place


def test_format_empty_and_validate():
    from dd3d_amd.evaluators import KITTIEvaluationEngine
    e = KITTIEvaluationEngine._format(4, pd.DataFrame(columns=list(range(16))), True)
    assert e["id"] == "000004" and e["bbox"].shape == (0, 4) and e["name"] == []
    row = ["Car", -1, -1, 0.5, 1.0, 2.0, 3.0, 4.0, 1.5, 1.6, 3.9, 1.0, 2.0, 30.0, 0.1, 0.9]
    f = KITTIEvaluationEngine._format(0, pd.DataFrame([row]), True)
    assert f["dimensions"].tolist() == [[3.9, 1.5, 1.6]] and f["score"].tolist() == [0.9] and f["occluded"].dtype == np.int64
    g = KITTIEvaluationEngine._format(0, pd.DataFrame([row[:15]]), False)
    assert g["score"].tolist() == [0.0]
    gg, dd = KITTIEvaluationEngine.validate_anno_format([dict(g, rotation_y=g["rotation_y"][None])], [f])
    assert gg[0]["rotation_y"].shape == (1,)


# ---- the wave-parallel rule of kitti_ap.hip == the reference's state machines --------------------------------------------------------
def _lanes(n):
    """Detection indices per lane, in the order a lane visits them (chunk k: detection 64k + lane)."""
    return [list(range(lane, n, 64)) for lane in range(64)]


def wave_pass1(ov, scores, ig, idt, mo):
    """kitti_tp_scores_kernel in Python: per-lane running best (score, lowest index), then the butterfly argmax."""
    n = len(scores)
    taken = [idt[d] == -1 for d in range(n)]
    out = []
    for g in range(len(ig)):
        if ig[g] == -1:
            continue
        lane_best = []
        for ds in _lanes(n):
            best, bj = O.NO_DETECTION, None
            for d in ds:
                if not taken[d] and ov[d][g] > mo and scores[d] > best:
                    best, bj = scores[d], d
            lane_best.append((best, bj))
        best, bj = lane_best[0]
        for s, j in lane_best[1:]:
            if s > best or (s == best and j is not None and (bj is None or j < bj)):
                best, bj = s, j
        if bj is None:
            continue
        taken[bj] = True
        if not (ig[g] == 1 or idt[bj] == 1):
            out.append(scores[bj])
    return out


def wave_pass2(ov, scores, ig, idt, mo, thresh):
    """kitti_pr_counts_kernel in Python: key (rank, overlap, -index), rank 2 for ign_dt 0, 1 for ign_dt 1."""
    n = len(scores)
    taken = [idt[d] == -1 or not (scores[d] >= thresh) for d in range(n)]
    tp = fn = 0
    for g in range(len(ig)):
        if ig[g] == -1:
            continue
        keys = []
        for ds in _lanes(n):
            r, v, bj = 0, 0.0, None
            for d in ds:
                if taken[d] or not (ov[d][g] > mo):
                    continue
                if idt[d] == 0 and (r < 2 or ov[d][g] > v):
                    r, v, bj = 2, ov[d][g], d
                elif idt[d] == 1 and r == 0:
                    r, bj = 1, d
            keys.append((r, v, bj))
        r, v, bj = keys[0]
        for r2, v2, j2 in keys[1:]:
            if r2 > r or (r2 == r and (v2 > v or (v2 == v and j2 is not None and (bj is None or j2 < bj)))):
                r, v, bj = r2, v2, j2
        if r == 0:
            fn += ig[g] == 0
        else:
            taken[bj] = True
            tp += not (ig[g] == 1 or idt[bj] == 1)
    fp = sum(1 for d in range(n) if not taken[d] and idt[d] != 1)
    return tp, fp, fn


def test_parallel_rule_equals_sequential_state_machine():
    rng = np.random.default_rng(12345)
    for case in range(400):
        n_dt = int(rng.choice([0, 1, 3, 10, 63, 64, 65, 130]))
        n_gt = int(rng.integers(0, 7))
        levels = np.float32([0.0, 0.3, 0.5, 0.55, 0.7, 0.9, 1.0])
        ov = rng.choice(levels, (n_dt, n_gt)) if case % 2 else rng.uniform(0, 1, (n_dt, n_gt)).astype(np.float32)
        if case % 5 == 0 and ov.size:
            ov.flat[rng.integers(0, ov.size, 3)] = np.nan  # NaN overlaps are never candidates
        ov = ov.astype(np.float64)  # the reference compares the float32 values in float64
        scores = rng.choice([0.1, 0.2, 0.5, 0.9], n_dt) if case % 3 == 0 else rng.uniform(0, 1, n_dt)  # ties
        if case % 7 == 0 and n_dt:
            scores[rng.integers(0, n_dt)] = np.nan
        mode = case % 4  # all ignored / ign 1 before and after ign 0 / mixed
        idt = (np.full(n_dt, 1) if mode == 0 else rng.choice([-1, 0, 1], n_dt, p=[0.2, 0.4, 0.4])).tolist()
        ig = rng.choice([-1, 0, 1], n_gt).tolist()
        for mo in (0.5, 0.7):
            assert wave_pass1(ov, scores, ig, idt, mo) == O.tp_scores(ov, scores, ig, idt, mo), case
            for thresh in (0.0, 0.2, 0.5, float(np.nanmax(scores)) if n_dt and not np.isnan(scores).all() else 1.0):
                assert wave_pass2(ov, scores, ig, idt, mo, thresh) == O.pr_counts(ov, scores, ig, idt, mo, thresh), case


# ---- C entry points: argument checks, no GPU needed --------------------------------------------------------------------------------------
def test_entry_points_reject_bad_arguments(hiplib):
    from dd3d_amd import hip
    mo = np.array([0.5, 0.7])
    dummy = C.c_void_p(16)  # never dereferenced: every call below returns before a launch

    def args(**kw):
        a = dict(ov=dummy, ov_off=dummy, dt_begin=dummy, gt_begin=dummy, dt_score=dummy, ign_dt=dummy, ign_gt=dummy,
                 min_overlap=mo.ctypes.data_as(C.c_void_p), n_ov=10, n_img=2, n_dt=5, n_gt=3, n_cd=15, n_o=2, max_dt=4, max_gt=2)
        a.update(kw)
        return hip.KittiMatchArgs(**a)

    def err(rc):
        assert rc < 0
        return hiplib.dd3d_last_error().decode()

    assert "null" in err(hiplib.dd3d_kitti_tp_scores(None, dummy, None))
    assert "null" in err(hiplib.dd3d_kitti_pr_counts(None, dummy, dummy, 41, dummy, None))
    hdr = open(os.path.join(ROOT, "include", "dd3d_hip.h")).read()
    for name in ("KITTI_MAX_DT_PER_IMAGE", "KITTI_MAX_GT_PER_IMAGE", "KITTI_MAX_OVERLAPS", "KITTI_MAX_THRESHOLDS"):
        assert f"#define DD3D_{name} {getattr(hip, name)}\n" in hdr, name
    cap_dt, cap_gt = hip.KITTI_MAX_DT_PER_IMAGE, hip.KITTI_MAX_GT_PER_IMAGE
    assert str(cap_dt) in err(hiplib.dd3d_kitti_tp_scores(C.byref(args(max_dt=cap_dt + 1)), dummy, None))
    assert str(cap_gt) in err(hiplib.dd3d_kitti_pr_counts(C.byref(args(max_gt=cap_gt + 1)), dummy, dummy, 41, dummy, None))
    assert hiplib.dd3d_kitti_tp_scores(C.byref(args(max_dt=cap_dt, n_img=0)), None, None) == 0
    assert "negative" in err(hiplib.dd3d_kitti_tp_scores(C.byref(args(n_img=-1)), dummy, None))
    assert "overlap thresholds" in err(hiplib.dd3d_kitti_tp_scores(C.byref(args(n_o=hip.KITTI_MAX_OVERLAPS + 1)), dummy, None))
    assert "t_max" in err(hiplib.dd3d_kitti_pr_counts(C.byref(args()), dummy, dummy, hip.KITTI_MAX_THRESHOLDS + 1, dummy, None))
    assert "null" in err(hiplib.dd3d_kitti_tp_scores(C.byref(args(dt_begin=None)), dummy, None))
    assert "null" in err(hiplib.dd3d_kitti_tp_scores(C.byref(args()), None, None))
    assert "null" in err(hiplib.dd3d_kitti_pr_counts(C.byref(args()), dummy, None, 41, dummy, None))
    low = np.array([0.5, -np.inf])
    assert "FLT_MAX" in err(hiplib.dd3d_kitti_tp_scores(C.byref(args(min_overlap=low.ctypes.data_as(C.c_void_p))), dummy, None))
    # empty work: 0, nothing enqueued (null data pointers are fine then)
    for kw in (dict(n_img=0), dict(n_cd=0), dict(n_o=0)):
        empty = args(ov=None, ov_off=None, dt_begin=None, gt_begin=None, dt_score=None, ign_dt=None, ign_gt=None, **kw)
        assert hiplib.dd3d_kitti_tp_scores(C.byref(empty), None, None) == 0
        assert hiplib.dd3d_kitti_pr_counts(C.byref(empty), None, None, 41, None, None) == 0
    assert hiplib.dd3d_kitti_tp_scores(C.byref(args(n_gt=0, ign_gt=None)), None, None) == 0  # no GT: nothing to write
    assert hiplib.dd3d_kitti_pr_counts(C.byref(args()), None, None, 0, None, None) == 0
    assert C.sizeof(hip.KittiMatchArgs) == 104


# ---- public surface without a GPU ------------------------------------------------------------------------------------------------------
def test_engine_refuses_to_run_without_gpu(golden, monkeypatch):
    import torch
    from dd3d_amd.evaluators import KITTIEvaluationEngine
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    gt, dt = golden_annos(golden)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        KITTIEvaluationEngine(ID_TO_NAME).evaluate(gt[:3], dt[:3], THRESHOLDS)


def test_evaluator_arguments_and_submission(tmp_path):
    from dd3d_amd.evaluators import KITTI3DEvaluator
    ev = KITTI3DEvaluator("kitti_3d_val", dataset_dicts=[], class_names=CLASSES)
    assert ev._id_to_name == ID_TO_NAME
    with pytest.raises(ValueError, match=r"EVALUATORS\.KITTI3D\.IOU_THRESHOLDS"):
        ev.evaluate()
    ev = KITTI3DEvaluator("kitti_3d_val", iou_thresholds=THRESHOLDS, dataset_dicts=[], class_names=CLASSES, id_to_name={0: "Car"})
    assert ev._id_to_name == {0: "Car"}
    out = str(tmp_path / "out")
    ev = KITTI3DEvaluator("kitti_3d_val", only_prepare_submission=True, output_dir=out, dataset_dicts=[], class_names=CLASSES)
    ev._predictions_kitti_format = [pd.DataFrame([["Car", -1, -1, 0.1, 1, 2, 3, 4, 1.5, 1.6, 3.9, 1, 2, 30, 0.1, 0.9]]), pd.DataFrame([])]
    ev._predictions_as_json = [{"category": "Car", "score": 0.9}]
    assert ev.evaluate() == {}
    assert json.load(open(os.path.join(out, "bbox3d_predictions.json"))) == [{"category": "Car", "score": 0.9}]
    assert sorted(os.listdir(os.path.join(out, "kitti_3d_submission"))) == ["000000.txt", "000001.txt"]
