"""Plain-Python statement of the nuScenes devkit's detection evaluation (nuscenes-devkit 1.1.x, `eval/detection` with
`detection_cvpr_2019`) as the tests check it: one box at a time, the devkit's loops as written, float64 numpy only where the devkit
itself calls numpy.  Shares no code with dd3d_amd.evaluators.nuscenes_eval.

Input: `results` {sample_token: [box dict]} (the submission's `results`), `gt` {sample_token: [box dict]} (DetectionBox.serialize()
fields), `ego` {sample_token: [x, y, z]}, `racks` {sample_token: [{translation, size, rotation}]}.
"""
import math

import numpy as np

CLASS_RANGE = {"car": 50, "truck": 50, "bus": 50, "trailer": 50, "construction_vehicle": 50, "pedestrian": 40, "motorcycle": 40,
               "bicycle": 40, "traffic_cone": 30, "barrier": 30}
CLASS_NAMES = list(CLASS_RANGE)
DIST_THS = [0.5, 1.0, 2.0, 4.0]
DIST_TH_TP = 2.0
MIN_RECALL = 0.1
MIN_PRECISION = 0.1
MEAN_AP_WEIGHT = 5
TP_METRICS = ["trans_err", "scale_err", "orient_err", "vel_err", "attr_err"]


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def rotation_matrix(q):
    n = math.sqrt(q[0] ** 2 + q[1] ** 2 + q[2] ** 2 + q[3] ** 2)
    w, x, y, z = (c / n for c in q)
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def quaternion_yaw(q):
    R = rotation_matrix(q)
    return math.atan2(R[1][0], R[0][0])


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def point_in_rack(p, rack):
    w, l, h = rack["size"]
    R = rotation_matrix(rack["rotation"])

    def corner(cx, cy, cz):
        c = [cx, cy, cz]
        return [R[r][0] * c[0] + R[r][1] * c[1] + R[r][2] * c[2] + rack["translation"][r] for r in range(3)]

    c0 = corner(l / 2, w / 2, h / 2)
    c1 = corner(l / 2, -w / 2, h / 2)
    c3 = corner(l / 2, w / 2, -h / 2)
    c4 = corner(-l / 2, w / 2, h / 2)
    v = [p[r] - c0[r] for r in range(3)]
    for c in (c4, c1, c3):
        e = [c[r] - c0[r] for r in range(3)]
        ev = dot3(e, v)
        if not (0 <= ev and ev <= dot3(e, e)):
            return False
    return True


def center_distance(g, p):
    dx = p["translation"][0] - g["translation"][0]
    dy = p["translation"][1] - g["translation"][1]
    return math.sqrt(dx * dx + dy * dy)


def velocity_l2(g, p):
    dx = p["velocity"][0] - g["velocity"][0]
    dy = p["velocity"][1] - g["velocity"][1]
    return math.sqrt(dx * dx + dy * dy)


def scale_iou(g, p):
    assert all(s > 0 for s in g["size"]) and all(s > 0 for s in p["size"])
    inter = min(g["size"][0], p["size"][0]) * min(g["size"][1], p["size"][1]) * min(g["size"][2], p["size"][2])
    union = g["size"][0] * g["size"][1] * g["size"][2] + p["size"][0] * p["size"][1] * p["size"][2] - inter
    return inter / union


def angle_diff(x, y, period):
    diff = (x - y + period / 2) % period - period / 2
    if diff > math.pi:
        diff = diff - 2 * math.pi
    return diff


def attr_acc(g, p):
    if g["attribute_name"] == "":
        return math.nan
    return float(g["attribute_name"] == p["attribute_name"])


# ---- loading + filters ------------------------------------------------------------------------------------------------------------
def filter_boxes(boxes_by_sample, ego, racks):
    out = {}
    for token, boxes in boxes_by_sample.items():
        e = ego[token]
        kept = []
        for b in boxes:
            x, y = b["translation"][0] - e[0], b["translation"][1] - e[1]
            if not (math.sqrt(x * x + y * y) < CLASS_RANGE[b["detection_name"]]):
                continue
            kept.append(b)
        kept = [b for b in kept if not b.get("num_pts", -1) == 0]
        final = []
        for b in kept:
            if b["detection_name"] in ("bicycle", "motorcycle"):
                if any(point_in_rack(b["translation"], r) for r in racks.get(token, [])):
                    continue
            final.append(b)
        out[token] = final
    return out


# ---- accumulate -------------------------------------------------------------------------------------------------------------------
def matching_order(confs):
    return [i for (v, i) in sorted((v, i) for (i, v) in enumerate(confs))][::-1]


def greedy_match(pred_list, order, gt, class_name, th):
    """The devkit's loop: [(pred index, matched gt (token, index) or None)] in matching order."""
    taken = set()
    out = []
    for ind in order:
        p = pred_list[ind]
        min_dist, match = math.inf, None
        for gi, g in enumerate(gt.get(p["sample_token"], [])):
            if g["detection_name"] == class_name and (p["sample_token"], gi) not in taken:
                d = center_distance(g, p)
                if d < min_dist:
                    min_dist, match = d, gi
        if min_dist < th:
            taken.add((p["sample_token"], match))
            out.append((ind, (p["sample_token"], match)))
        else:
            out.append((ind, None))
    return out


def cummean(x):
    if sum(np.isnan(x)) == len(x):
        return np.ones(len(x))
    sum_vals = np.nancumsum(x.astype(float))
    count_vals = np.cumsum(~np.isnan(x))
    return np.divide(sum_vals, count_vals, out=np.zeros_like(sum_vals), where=count_vals != 0)


def no_predictions():
    return dict(precision=np.zeros(101), confidence=np.zeros(101), **{m: np.ones(101) for m in TP_METRICS})


def accumulate(pred, gt, class_name, th):
    npos = len([1 for token in gt for g in gt[token] if g["detection_name"] == class_name])
    if npos == 0:
        return no_predictions()
    pred_list = [p for token in pred for p in pred[token] if p["detection_name"] == class_name]
    confs = [p["detection_score"] for p in pred_list]
    tp, fp, conf = [], [], []
    md = {m: [] for m in TP_METRICS}
    md["conf"] = []
    for ind, m in greedy_match(pred_list, matching_order(confs), gt, class_name, th):
        p = pred_list[ind]
        if m is not None:
            g = gt[m[0]][m[1]]
            tp.append(1)
            fp.append(0)
            conf.append(p["detection_score"])
            md["trans_err"].append(center_distance(g, p))
            md["vel_err"].append(velocity_l2(g, p))
            md["scale_err"].append(1 - scale_iou(g, p))
            period = math.pi if class_name == "barrier" else 2 * math.pi
            md["orient_err"].append(abs(angle_diff(quaternion_yaw(g["rotation"]), quaternion_yaw(p["rotation"]), period)))
            md["attr_err"].append(1 - attr_acc(g, p))
            md["conf"].append(p["detection_score"])
        else:
            tp.append(0)
            fp.append(1)
            conf.append(p["detection_score"])
    if len(md["trans_err"]) == 0:
        return no_predictions()
    tp = np.cumsum(tp).astype(float)
    fp = np.cumsum(fp).astype(float)
    conf = np.array(conf)
    prec = tp / (fp + tp)
    rec = tp / float(npos)
    rec_interp = np.linspace(0, 1, 101)
    prec = np.interp(rec_interp, rec, prec, right=0)
    conf = np.interp(rec_interp, rec, conf, right=0)
    out = dict(precision=prec, confidence=conf)
    for key in TP_METRICS:
        tmp = cummean(np.array(md[key]))
        out[key] = np.interp(conf[::-1], md["conf"][::-1], tmp[::-1])[::-1]
    return out


def calc_ap(md):
    prec = np.copy(md["precision"])
    prec = prec[round(100 * MIN_RECALL) + 1:]
    prec -= MIN_PRECISION
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - MIN_PRECISION)


def calc_tp(md, metric):
    first = round(100 * MIN_RECALL) + 1
    nz = np.nonzero(md["confidence"])[0]
    last = 0 if len(nz) == 0 else nz[-1]
    if last < first:
        return 1.0
    return float(np.mean(md[metric][first:last + 1]))


def evaluate(results, gt, ego, racks=None):
    racks = {} if racks is None else racks
    assert set(results).issubset(set(gt))
    gt_sub = {t: gt[t] for t in results}
    pred = filter_boxes(results, ego, racks)
    gt_f = filter_boxes(gt_sub, ego, racks)
    label_aps, label_tp = {}, {}
    for c in CLASS_NAMES:
        label_aps[c] = {}
        for th in DIST_THS:
            label_aps[c][th] = calc_ap(accumulate(pred, gt_f, c, th))
        md = accumulate(pred, gt_f, c, DIST_TH_TP)
        label_tp[c] = {}
        for m in TP_METRICS:
            if c == "traffic_cone" and m in ("attr_err", "vel_err", "orient_err"):
                label_tp[c][m] = np.nan
            elif c == "barrier" and m in ("attr_err", "vel_err"):
                label_tp[c][m] = np.nan
            else:
                label_tp[c][m] = calc_tp(md, m)
    mean_dist_aps = {c: np.mean(list(d.values())) for c, d in label_aps.items()}
    mean_ap = float(np.mean(list(mean_dist_aps.values())))
    tp_errors = {m: float(np.nanmean([label_tp[c][m] for c in CLASS_NAMES])) for m in TP_METRICS}
    tp_scores = {m: max(0.0, 1.0 - tp_errors[m]) for m in TP_METRICS}
    nd = float(MEAN_AP_WEIGHT * mean_ap + np.sum(list(tp_scores.values()))) / float(MEAN_AP_WEIGHT + len(tp_scores))
    return dict(label_aps=label_aps, mean_dist_aps=mean_dist_aps, mean_ap=mean_ap, label_tp_errors=label_tp, tp_errors=tp_errors,
                tp_scores=tp_scores, nd_score=nd)
