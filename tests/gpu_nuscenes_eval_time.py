"""Dev tool (GPU): timing of NuscenesDetectionEval.evaluate (dd3d_amd/evaluators/nuscenes_eval.py) on a nuScenes-val-shaped synthetic
set -- 6019 samples, 500 predictions per sample over the 10 detection classes, ~30 ground-truth boxes per sample with NaN velocities
and empty attributes mixed in, bike racks in some samples -- split into host preparation (validation, filters, sort, segments),
upload, kernel (device events; the wall time of that step includes the read-back of `match`) and host accumulation.

The nuScenes devkit is not installed where this runs, so there is no devkit number.  The CPU stand-in timed instead is the literal
test oracle (tests/nuscenes_eval_oracle.py, the devkit's loops restated one box at a time) on the first 1 % of the samples; the
engine is timed on the same subset and its result compared with the oracle's.

    python tests/gpu_nuscenes_eval_time.py > profiles/nuscenes_eval_time.txt
"""
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

g.build()
from dd3d_amd.evaluators import NuscenesDetectionEval, NuscenesGroundTruth  # noqa: E402
from tests import nuscenes_eval_oracle as O  # noqa: E402
from tests.test_nuscenes_eval import ATTRS, same_metrics  # noqa: E402

CLASSES = O.CLASS_NAMES
FREQ = np.array([0.40, 0.08, 0.02, 0.03, 0.02, 0.18, 0.02, 0.02, 0.10, 0.13])


def val_shaped(rng, n_samples=6019, n_pred=500, n_gt=30):
    results, gt, ego, racks = OrderedDict(), OrderedDict(), {}, {}
    attr_tab = [ATTRS[c] for c in CLASSES]
    for s in range(n_samples):
        tok = f"{s:032x}"
        e = rng.uniform(-2000, 2000, 3)
        ego[tok] = e.tolist()
        k = int(rng.poisson(n_gt))
        gc = rng.choice(10, k, p=FREQ)
        gxy = e[:2] + rng.uniform(-60, 60, (k, 2))
        gt_t = np.concatenate([gxy, e[2] + rng.normal(0, 1, (k, 1))], 1).tolist()
        gs = rng.uniform(0.4, 6, (k, 3))
        gyaw = rng.uniform(-np.pi, np.pi, k)
        gq = np.stack([np.cos(gyaw / 2), 0 * gyaw, 0 * gyaw, np.sin(gyaw / 2)], 1).tolist()
        gv = rng.normal(0, 3, (k, 2))
        gv[rng.random(k) < 0.25] = np.nan
        pts = rng.choice([0, 3, 30], k, p=[0.1, 0.4, 0.5]).tolist()
        ga = rng.integers(0, 12, k).tolist()
        gcl, gsl, gvl = gc.tolist(), gs.tolist(), gv.tolist()
        gt[tok] = [dict(sample_token=tok, translation=gt_t[i], size=gsl[i], rotation=gq[i], velocity=gvl[i], ego_translation=[0.0, 0.0, 0.0],
                        num_pts=pts[i], detection_name=CLASSES[gcl[i]], detection_score=-1.0,
                        attribute_name=attr_tab[gcl[i]][ga[i] % len(attr_tab[gcl[i]])]) for i in range(k)]
        racks[tok] = ([dict(translation=(e + [rng.uniform(-30, 30), rng.uniform(-30, 30), 0.0]).tolist(), size=[3.0, 8.0, 1.5],
                            rotation=[np.cos(0.3), 0.0, 0.0, np.sin(0.3)])] if rng.random() < 0.2 else [])
        near = (rng.random(n_pred) < 0.4) & (k > 0)
        src = rng.integers(0, max(k, 1), n_pred)
        pc = np.where(near, gc[src] if k else 0, rng.choice(10, n_pred, p=FREQ))
        pxy = np.where(near[:, None], (gxy[src] if k else 0) + rng.normal(0, 1.0, (n_pred, 2)), e[:2] + rng.uniform(-60, 60, (n_pred, 2)))
        pt = np.concatenate([pxy, np.full((n_pred, 1), e[2])], 1).tolist()
        ps = np.where(near[:, None], (gs[src] if k else 1) * rng.uniform(0.8, 1.2, (n_pred, 3)), rng.uniform(0.4, 6, (n_pred, 3))).tolist()
        pyaw = rng.uniform(-np.pi, np.pi, n_pred)
        pq = np.stack([np.cos(pyaw / 2), 0 * pyaw, 0 * pyaw, np.sin(pyaw / 2)], 1).tolist()
        pv = rng.normal(0, 3, (n_pred, 2)).tolist()
        score = np.round(rng.uniform(0, 1, n_pred), 3).tolist()
        pa = rng.integers(0, 12, n_pred).tolist()
        pcl = pc.tolist()
        results[tok] = [dict(sample_token=tok, translation=pt[i], size=ps[i], rotation=pq[i], velocity=pv[i], detection_name=CLASSES[pcl[i]],
                             detection_score=score[i], attribute_name=attr_tab[pcl[i]][pa[i] % len(attr_tab[pcl[i]])]) for i in range(n_pred)]
    return results, gt, ego, racks


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    t0 = time.perf_counter()
    results, gt, ego, racks = val_shaped(rng)
    truth = NuscenesGroundTruth(gt, ego, racks)
    n_pred, n_gt = sum(len(v) for v in results.values()), sum(len(v) for v in gt.values())
    print(f"set: {len(results)} samples, {n_pred} predictions, {n_gt} GT ({sum(np.isnan(b['velocity'][0]) for v in gt.values() for b in v)} "
          f"with NaN velocity, {sum(b['attribute_name'] == '' for v in gt.values() for b in v)} with empty attribute), "
          f"{sum(len(r) for r in racks.values())} bike racks; built in {time.perf_counter() - t0:.1f} s")
    eng = NuscenesDetectionEval(truth)
    few = OrderedDict(list(results.items())[:60])
    eng.evaluate(few)  # warm-up: code objects, allocator
    for rep in range(2):
        steps = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.evaluate(results, timings=steps)
        t_all = time.perf_counter() - t0
        print(f"rep {rep}: total {t_all:7.2f} s | host preparation {steps['prepare']:6.2f} s | upload {steps['upload'] * 1e3:6.1f} ms | "
              f"kernel {steps['kernel_events'] * 1e3:6.2f} ms (device events; {steps['kernel'] * 1e3:6.1f} ms with launch and read-back) | "
              f"host accumulation {steps['accumulate'] * 1e3:6.1f} ms")
    print("result:", {k: round(float(res[k]), 6) for k in ("mean_ap", "nd_score")}, {k: round(v, 6) for k, v in res["tp_errors"].items()})
    # CPU stand-in: the literal oracle on 1 % of the samples, and the engine on the same subset
    frac = OrderedDict(list(results.items())[:len(results) // 100])
    t0 = time.perf_counter()
    want = O.evaluate(frac, gt, ego, racks)
    t_oracle = time.perf_counter() - t0
    steps = {}
    t0 = time.perf_counter()
    got = eng.evaluate(frac, timings=steps)
    t_engine = time.perf_counter() - t0
    same_metrics(got, want)
    print(f"1 % of the set ({len(frac)} samples, {sum(len(v) for v in frac.values())} predictions): literal oracle {t_oracle:.2f} s | engine "
          f"{t_engine * 1e3:.1f} ms (kernel {steps['kernel_events'] * 1e3:.3f} ms) | results agree (APs bit-identical, TP errors within 1e-12)")


if __name__ == "__main__":
    main()
