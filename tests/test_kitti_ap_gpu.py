"""KITTI AP engine on the MI355X against the reference's own results (tests/golden/kitti_ap.npz): the two HIP passes fed the
reference's overlaps, the engine end to end on HIP overlaps, KITTI3DEvaluator.process + evaluate, a 500-image KITTI-shaped set
against the plain-Python oracle (one slot), a 320-image set with up to 100 and three times 390 detections per image against the
oracle in every slot of both metrics, and the distributed gather (gloo, two ranks on the one GPU)."""
import json
import multiprocessing as mp
import os

import numpy as np
import pandas as pd
import pytest
import torch

from tests import kitti_ap_oracle as O
from tests.test_kitti_ap import CLASSES, ID_TO_NAME, THRESHOLDS, golden_annos, golden_dict, load_golden, same_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_golden()


def _instances(rec, device):
    from dd3d_amd.structures import Boxes, GenericBoxes3D, Instances
    n = len(rec["scores"])
    inst = Instances((375, 1242))
    inst.pred_boxes = Boxes(torch.tensor(rec["pred_boxes"], dtype=torch.float32, device=device).reshape(n, 4))
    inst.pred_classes = torch.tensor(rec["pred_classes"], dtype=torch.int64, device=device)
    inst.scores = torch.tensor(rec["scores"], dtype=torch.float32, device=device)
    inst.scores_3d = torch.tensor(rec["scores_3d"], dtype=torch.float32, device=device)
    v = torch.tensor(rec["box3d_vec"], dtype=torch.float32, device=device).reshape(n, 10)
    inst.pred_boxes3d = GenericBoxes3D(v[:, :4], v[:, 4:7], v[:, 7:])
    return {"instances": inst}


def _evaluator_inputs(golden):
    e = json.loads(str(golden["ev_json"]))
    dds = []
    for d, raw in zip(e["dataset_dicts"], e["raw"]):
        d = dict(d)
        if raw is not None:
            d["raw_kitti_annotations"] = pd.DataFrame(raw) if raw else pd.DataFrame(columns=list(range(16)))
        dds.append(d)
    return e, dds


def test_kernels_on_reference_overlaps(golden, hiplib):
    from dd3d_amd.evaluators import KITTIEvaluationEngine
    eng = KITTIEvaluationEngine(ID_TO_NAME)
    gt, dt = golden_annos(golden)
    p = eng._prepare(gt, dt, THRESHOLDS)
    eng._upload(p, torch.device("cuda"))
    for metric in ("box3d", "bev"):
        ov = torch.tensor(golden[f"{metric}_block_values"], device="cuda")
        runs = []
        for _ in range(2):
            tps = eng._tp_scores(p, ov)
            ths = eng._thresholds(p, tps)
            runs.append((tps, ths, eng._pr_counts(p, ov, ths)))
        tps, ths, counts = runs[0]
        assert np.array_equal(tps, golden[f"{metric}_tp_scores"])
        n_th = golden[f"{metric}_n_thresholds"].reshape(-1)
        assert [len(t) for t in ths] == n_th.tolist()
        t_max = counts.shape[2]
        assert t_max == n_th.max() and np.array_equal(counts, golden[f"{metric}_counts"][:, :, :t_max])
        assert np.array_equal(runs[1][0], tps) and runs[1][1] == ths and np.array_equal(runs[1][2], counts)


def test_engine_end_to_end_matches_reference(golden, hiplib):
    from dd3d_amd.evaluators import KITTIEvaluationEngine
    gt, dt = golden_annos(golden)
    res = KITTIEvaluationEngine(ID_TO_NAME).evaluate(gt, dt, THRESHOLDS)
    same_dict(res, *golden_dict(golden))
    assert len(res) == 2 * len(CLASSES) * 3 * len(THRESHOLDS)
    # the HIP overlap blocks agree with the reference's to float32 rounding
    eng = KITTIEvaluationEngine(ID_TO_NAME)
    p = eng._prepare(gt, dt, THRESHOLDS)
    for metric, name in (("BOX3D_AP", "box3d"), ("BEV_AP", "bev")):
        got = eng._overlap_blocks(p, metric, torch.device("cuda")).cpu().numpy()
        np.testing.assert_allclose(got, golden[f"{name}_block_values"], rtol=0, atol=1e-4)


def test_evaluator_process_evaluate_matches_reference(golden, tmp_path, hiplib):
    from dd3d_amd.evaluators import KITTI3DEvaluator
    e, dds = _evaluator_inputs(golden)
    outputs = [_instances(r, "cuda") for r in e["outputs"]]
    out = str(tmp_path / "eval")
    ev = KITTI3DEvaluator("kitti_3d_val", iou_thresholds=e["thresholds"], output_dir=out, dataset_dicts=dds, class_names=e["class_names"])
    ev.reset()
    ev.process(e["inputs"], outputs)
    res = ev.evaluate()
    same_dict(res, *golden_dict(golden, "ev_"))
    assert len(json.load(open(os.path.join(out, "bbox3d_predictions.json")))) == sum(len(r["scores"]) for r in e["outputs"])
    sub_out = str(tmp_path / "sub")
    ev = KITTI3DEvaluator("kitti_3d_val", only_prepare_submission=True, output_dir=sub_out, dataset_dicts=dds, class_names=e["class_names"])
    ev.process(e["inputs"], outputs)
    assert ev.evaluate() == {}
    sub = os.path.join(sub_out, "kitti_3d_submission")
    assert sorted(os.listdir(sub)) == golden["ev_submission_files"].tolist()
    assert open(os.path.join(sub, "000000.txt")).read() == str(golden["ev_submission_000000"])


def _kitti_shaped(rng, n_img, n_gt=8, n_dt=40, fixed_dt=None):
    """KITTI-val-shaped synthetic set: ~n_gt GT (with Van / Person_sitting / DontCare) and up to n_dt (or exactly fixed_dt)
    detections per image."""
    types = ["Car", "Car", "Van", "Pedestrian", "Person_sitting", "Cyclist", "Truck", "DontCare"]
    gts, dts = [], []
    for _ in range(n_img):
        g = []
        for _ in range(int(rng.integers(0, 2 * n_gt))):
            h = rng.uniform(10, 120)
            l, t = rng.uniform(0, 1100), rng.uniform(100, 250)
            g.append([str(rng.choice(types)), float(rng.choice([0, 0.2, 0.6])), int(rng.integers(0, 4)), 0.0, l, t, l + h, t + h,
                      rng.uniform(1.4, 1.8), rng.uniform(1.5, 1.9), rng.uniform(3.5, 4.5), rng.uniform(-10, 10), rng.uniform(1, 2), rng.uniform(5, 45),
                      rng.uniform(-3, 3)])
        d = []
        for _ in range(fixed_dt if fixed_dt is not None else int(rng.integers(0, n_dt + 1))):
            src = g[int(rng.integers(0, len(g)))] if g and rng.random() < 0.7 else None
            loc = (np.array(src[11:14]) + rng.normal(0, 0.3, 3)) if src else np.array([rng.uniform(-10, 10), rng.uniform(1, 2), rng.uniform(5, 45)])
            box = (np.array(src[4:8]) + rng.normal(0, 3, 4)) if src else np.array([10.0, 150.0, 60.0, 150 + rng.uniform(10, 100)])
            name = (src[0] if src[0] in CLASSES else "Car") if src and rng.random() < 0.9 else str(rng.choice(CLASSES))
            d.append([name, -1, -1, 0.0] + box.tolist() + [rng.uniform(1.4, 1.8), rng.uniform(1.5, 1.9), rng.uniform(3.5, 4.5)] + loc.tolist()
                     + [rng.uniform(-3, 3), float(np.round(rng.uniform(0, 1), 2))])
        gts.append(pd.DataFrame(g))
        dts.append(pd.DataFrame(d))
    return gts, dts


def test_500_images_counts_match_oracle_on_hip_overlaps(hiplib):
    from dd3d_amd.evaluators import KITTIEvaluationEngine
    rng = np.random.default_rng(500)
    gf, df = _kitti_shaped(rng, 500)
    gt = [KITTIEvaluationEngine._format(i, f, False) for i, f in enumerate(gf)]
    dt = [KITTIEvaluationEngine._format(i, f, True) for i, f in enumerate(df)]
    eng = KITTIEvaluationEngine(ID_TO_NAME)
    p = eng._prepare(gt, dt, THRESHOLDS)
    cd, o, c, d = 1, 0, 0, 1  # Car, Moderate, 0.5
    for metric in ("BOX3D_AP", "BEV_AP"):
        ov = eng._overlap_blocks(p, metric, torch.device("cuda"))
        tps = eng._tp_scores(p, ov)
        ths = eng._thresholds(p, tps)
        counts = eng._pr_counts(p, ov, ths)
        host = ov.cpu().numpy().astype(np.float64)
        blocks = [host[p.ov_off[i]:p.ov_off[i + 1]].reshape(p.nd[i], p.ng[i]) for i in range(500)]
        cleaned = [O.clean_kitti_data(a, b, c, d, ID_TO_NAME) for a, b in zip(gt, dt)]
        per_image = [O.tp_scores(blocks[i], dt[i]["score"], x[1], x[2], THRESHOLDS[o]) for i, x in enumerate(cleaned)]
        want_th = O.get_thresholds([s for q in per_image for s in q], sum(x[0] for x in cleaned))
        assert ths[cd * 2 + o] == want_th and len(want_th) >= 5
        want = np.zeros((len(want_th), 3), dtype=np.int64)
        for t, thr in enumerate(want_th):
            for i, x in enumerate(cleaned):
                want[t] += O.pr_counts(blocks[i], dt[i]["score"], x[1], x[2], THRESHOLDS[o], thr)
        assert np.array_equal(counts[cd, o, :len(want_th)], want)


def test_all_slots_match_oracle_at_topk_and_tta_shapes(hiplib):
    """Up to 100 detections per image (POST_NMS_TOPK) and three images with 390 (the merged TTA detections), so that the matching
    kernels run several chunks per lane in the engine too; 320 images are 50 shards of six and a remainder shard of 20.  Every one
    of the 15 x 2 (class x difficulty, overlap) slots of both metrics is compared: true-positive scores, thresholds, every count,
    and the final dictionary, against the plain-Python oracle run on the HIP overlaps read back."""
    from dd3d_amd.evaluators import KITTIEvaluationEngine
    rng = np.random.default_rng(390)
    n_img = 320
    gf, df = _kitti_shaped(rng, n_img, n_dt=100)
    for i in (10, 161, 319):
        g1, d1 = _kitti_shaped(rng, 1, n_gt=10, fixed_dt=390)
        gf[i], df[i] = g1[0], d1[0]
    gt = [KITTIEvaluationEngine._format(i, f, False) for i, f in enumerate(gf)]
    dt = [KITTIEvaluationEngine._format(i, f, True) for i, f in enumerate(df)]
    eng = KITTIEvaluationEngine(ID_TO_NAME)
    p = eng._prepare(gt, dt, THRESHOLDS)
    assert len(p.shards) == 51 and p.shards[-1][1] - p.shards[-1][0] == 20 and p.max_dt == 390 and (p.nd > 64).sum() > 80
    n_o = len(THRESHOLDS)
    ap = {}
    for metric in ("BOX3D_AP", "BEV_AP"):
        ov = eng._overlap_blocks(p, metric, torch.device("cuda"))
        tps = eng._tp_scores(p, ov)
        ths = eng._thresholds(p, tps)
        counts = eng._pr_counts(p, ov, ths)
        host = ov.cpu().numpy().astype(np.float64)
        blocks = [host[p.ov_off[i]:p.ov_off[i + 1]].reshape(p.nd[i], p.ng[i]) for i in range(n_img)]
        want = O.eval_metric_counts(blocks, gt, dt, ID_TO_NAME, THRESHOLDS)
        curves = 0
        for c in range(len(CLASSES)):
            for d in range(3):
                for o in range(n_o):
                    cd, slot = c * 3 + d, (c, d, o)
                    got_tp = tps[cd, o][tps[cd, o] != -np.inf]
                    assert got_tp.tolist() == [s for q in want["tp_scores"][slot] for s in q], (metric, slot)
                    assert ths[cd * n_o + o] == want["thresholds"][slot], (metric, slot)
                    n = len(want["thresholds"][slot])
                    assert np.array_equal(counts[cd, o, :n], want["counts"][slot]) and not counts[cd, o, n:].any(), (metric, slot)
                    curves += n >= 5
        assert curves >= 10  # a third of the slots have real curves
        recall, precision = eng._curves(p, ths, counts)
        assert np.array_equal(recall, want["recall"], equal_nan=True) and np.array_equal(precision, want["precision"], equal_nan=True)
        ap[metric] = O.mean_ap(want["precision"], want["recall"])
    expect = O.results(ap["BOX3D_AP"], ap["BEV_AP"], ID_TO_NAME, THRESHOLDS)
    same_dict(KITTIEvaluationEngine(ID_TO_NAME).evaluate(gt, dt, THRESHOLDS), list(expect.keys()), np.array([float(v) for v in expect.values()]))


def _rank_main(rank, init_file, golden_path, out_dir):
    import torch.distributed as dist
    from dd3d_amd.evaluators import KITTI3DEvaluator
    dist.init_process_group("gloo", init_method="file://" + init_file, rank=rank, world_size=2)
    try:
        g = dict(np.load(golden_path))
        e, dds = _evaluator_inputs(g)
        half = len(e["inputs"]) // 2
        sl = slice(0, half) if rank == 0 else slice(half, None)
        ev = KITTI3DEvaluator("kitti_3d_val", iou_thresholds=e["thresholds"], output_dir=out_dir, distributed=True, dataset_dicts=dds,
                              class_names=e["class_names"])
        ev.process(e["inputs"][sl], [_instances(r, "cuda") for r in e["outputs"][sl]])
        res = ev.evaluate()
        with open(os.path.join(out_dir, f"rank{rank}.json"), "w") as f:
            json.dump(None if res is None else [[k, float(v)] for k, v in res.items()], f)
    finally:
        dist.destroy_process_group()


def test_distributed_gather_two_ranks(golden, tmp_path, hiplib):
    from tests.test_kitti_ap import GOLDEN
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_rank_main, args=(r, str(tmp_path / "rdv"), GOLDEN, str(tmp_path))) for r in range(2)]
    for pr in procs:
        pr.start()
    for pr in procs:
        pr.join(timeout=600)
    alive = [pr for pr in procs if pr.is_alive()]
    for pr in alive:
        pr.kill()
    assert not alive and [pr.exitcode for pr in procs] == [0, 0]
    r0 = json.load(open(tmp_path / "rank0.json"))
    assert json.load(open(tmp_path / "rank1.json")) is None
    keys, values = golden_dict(golden, "ev_")
    assert [k for k, _ in r0] == keys and np.array_equal(np.array([v for _, v in r0]), values, equal_nan=True)
    assert len(json.load(open(tmp_path / "bbox3d_predictions.json"))) == sum(len(r["scores"]) for r in json.loads(str(golden["ev_json"]))["outputs"])
