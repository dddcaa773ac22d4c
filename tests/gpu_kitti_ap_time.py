"""Dev tool (GPU): timing of KITTIEvaluationEngine.evaluate (dd3d_amd/evaluators/kitti_ap.py) on a KITTI-val-shaped synthetic set --
3769 images, 5 classes, ~8 ground-truth boxes (Van, Person_sitting, DontCare among them) and up to 100 detections per image,
overlap thresholds [0.5, 0.7] -- split into host preparation, overlaps, pass 1 (with get_thresholds on the host) and pass 2 (with
the curves), each step device-synchronised.  The reference's numba engine cannot run here (no numba, no numba.cuda on ROCm), so
there is no number on its side.

    python tests/gpu_kitti_ap_time.py > profiles/kitti_ap_time.txt
"""
import os
import sys
import time

import numpy as np
import pandas as pd
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

g.build()
from dd3d_amd.evaluators import KITTIEvaluationEngine  # noqa: E402

CLASSES = ["Car", "Pedestrian", "Cyclist", "Van", "Truck"]
TYPES = ["Car", "Car", "Car", "Van", "Pedestrian", "Pedestrian", "Person_sitting", "Cyclist", "Truck", "DontCare"]


def kitti_val_shaped(rng, n_img=3769, n_gt=8, max_dt=100):
    gts, dts = [], []
    for _ in range(n_img):
        k = int(rng.poisson(n_gt))
        h = rng.uniform(12, 150, k)
        l, t = rng.uniform(0, 1100, k), rng.uniform(100, 250, k)
        loc = np.stack([rng.uniform(-15, 15, k), rng.uniform(1, 2.2, k), rng.uniform(5, 60, k)], 1)
        dims = np.stack([rng.uniform(1.4, 1.8, k), rng.uniform(1.5, 1.9, k), rng.uniform(3.5, 4.5, k)], 1)
        ry = rng.uniform(-np.pi, np.pi, k)
        names = rng.choice(TYPES, k)
        g_rows = [[names[i], float(rng.choice([0, 0.2, 0.6])), int(rng.integers(0, 4)), 0.0, l[i], t[i], l[i] + 1.5 * h[i], t[i] + h[i]]
                  + dims[i].tolist() + loc[i].tolist() + [ry[i]] for i in range(k)]
        n = int(rng.integers(0, max_dt + 1))
        src = rng.integers(0, max(k, 1), n)
        near = (rng.random(n) < 0.3) & (k > 0)
        d_rows = []
        for j in range(n):
            if near[j]:
                s = g_rows[src[j]]
                name = s[0] if s[0] in CLASSES else "Car"
                box = (np.array(s[4:8]) + rng.normal(0, 3, 4)).tolist()
                dl = (np.array(s[11:14]) + rng.normal(0, 0.3, 3)).tolist()
                dd, dr = s[8:11], s[14] + rng.normal(0, 0.1)
            else:
                name = str(rng.choice(CLASSES))
                x0, y0 = rng.uniform(0, 1100), rng.uniform(100, 250)
                hh = rng.uniform(10, 120)
                box = [x0, y0, x0 + 1.5 * hh, y0 + hh]
                dl = [rng.uniform(-15, 15), rng.uniform(1, 2.2), rng.uniform(5, 60)]
                dd, dr = [1.6, 1.7, 4.0], rng.uniform(-np.pi, np.pi)
            d_rows.append([name, -1, -1, 0.0] + box + list(dd) + dl + [dr, float(rng.uniform(0, 1))])
        gts.append(pd.DataFrame(g_rows))
        dts.append(pd.DataFrame(d_rows))
    return gts, dts


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    rng = np.random.default_rng(0)
    gf, df = kitti_val_shaped(rng)
    gt = [KITTIEvaluationEngine._format(i, f, False) for i, f in enumerate(gf)]
    dt = [KITTIEvaluationEngine._format(i, f, True) for i, f in enumerate(df)]
    n_gt, n_dt = sum(len(a["name"]) for a in gt), sum(len(a["name"]) for a in dt)
    eng = KITTIEvaluationEngine(dict(enumerate(CLASSES)))
    thresholds = [0.5, 0.7]
    res = eng.evaluate(gt, dt, thresholds)  # warm-up: code objects, allocator
    print(f"set: {len(gt)} images, {n_gt} GT, {n_dt} detections, {len(CLASSES)} classes, thresholds {thresholds}")
    print(f"overlap pairs in image blocks: {int(sum(len(a['name']) * len(b['name']) for a, b in zip(gt, dt)))}")
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.validate_anno_format(gt, dt)
        p = eng._prepare(gt, dt, thresholds)
        t_prep = time.perf_counter() - t0
        steps = {}
        for metric in ("BOX3D_AP", "BEV_AP"):
            eng.eval_metric(gt, dt, metric, thresholds, _prepared=p, timings=steps)
        torch.cuda.synchronize()
        t_all = time.perf_counter() - t0
        print(f"rep {rep}: total {t_all * 1e3:8.1f} ms | host preparation {t_prep * 1e3:7.1f} ms + upload {steps['prepare'] * 1e3:6.1f} ms | "
              f"overlaps {steps['overlaps'] * 1e3:7.1f} ms | pass 1 + get_thresholds {steps['pass1'] * 1e3:7.1f} ms | "
              f"pass 2 + curves {steps['pass2'] * 1e3:7.1f} ms   (both metrics)")
    # the two matching launches alone (device events, inputs resident)
    ov = eng._overlap_blocks(p, "BOX3D_AP", torch.device("cuda"))
    ths = eng._thresholds(p, eng._tp_scores(p, ov))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    import ctypes as C
    from dd3d_amd import hip
    L = hip.lib()
    args = eng._match_args(p, ov)
    tp = torch.empty((p.ign_gt.shape[0], 2, p.ign_gt.shape[1]), dtype=torch.float64, device="cuda")
    t_max = max(len(t) for t in ths)
    th = torch.zeros((p.ign_gt.shape[0] * 2, t_max), dtype=torch.float64)
    for i, t in enumerate(ths):
        th[i, :len(t)] = torch.tensor(t, dtype=torch.float64)
    th = th.cuda()
    nt = torch.tensor([len(t) for t in ths], dtype=torch.int32, device="cuda")
    counts = torch.empty((p.ign_gt.shape[0], 2, t_max, 3), dtype=torch.int64, device="cuda")
    for _ in range(3):
        ev[0].record()
        hip.check(L.dd3d_kitti_tp_scores(C.byref(args), tp.data_ptr(), hip.current_stream()))
        ev[1].record()
        hip.check(L.dd3d_kitti_pr_counts(C.byref(args), th.data_ptr(), nt.data_ptr(), t_max, counts.data_ptr(), hip.current_stream()))
        ev[2].record()
        torch.cuda.synchronize()
    print(f"kernels alone (BOX3D_AP, device events): pass 1 {ev[0].elapsed_time(ev[1]):.3f} ms, pass 2 {ev[1].elapsed_time(ev[2]):.3f} ms "
          f"({sum(len(t) for t in ths)} score thresholds over {len(ths)} curves, t_max {t_max})")
    print("result (first 6):", {k: round(float(v), 6) for k, v in list(res.items())[:6]})


if __name__ == "__main__":
    main()
