"""nuScenes detection metrics (mAP, TP errors, NDS): what tridet/evaluators/nuscenes_evaluator.py:249-312 obtains from the nuScenes
devkit's `DetectionEval` (nuscenes-devkit 1.1.x, `eval/detection`, config `detection_cvpr_2019`), with the devkit's rules restated:

  1. the predictions are validated as `load_prediction` / `DetectionBox` do; the GT is the subset of the prediction samples (the
     reference's `DetectionEval` patch, nuscenes_evaluator.py:103-115);
  2. `add_center_dist` and the three filters of `filter_eval_boxes` (class range, `num_pts == 0`, bicycles / motorcycles inside a
     bike rack), vectorised in numpy;
  3. the greedy centre-distance matching of `accumulate`, the devkit's Python loop over every prediction and every GT of its sample,
     for all classes and distance thresholds in ONE launch (`dd3d_nusc_center_match`, dd3d_amd/csrc/nusc_eval.hip) and one read-back;
  4. precision / recall / TP-error curves, `calc_ap`, `calc_tp` and the summary on the host with the devkit's own float64 numpy calls
     in its order, so the APs are bit-identical once the match decisions agree.

The engine needs the GPU, as KITTIEvaluationEngine does; there is no CPU fallback.  Where the devkit's arithmetic could differ in the
last bits (it computes norms and dot products with np.linalg.norm / np.dot, which may use BLAS, and rotation matrices through
pyquaternion), this module uses plain float64 expressions: the TP errors and a box lying within rounding of a bike-rack face are
the places where bit parity with the devkit is not shown.
"""
import ctypes as C
import json
import time
from collections import OrderedDict

import numpy as np
import torch

from dd3d_amd import hip

# nuscenes/eval/detection/configs/detection_cvpr_2019.json
DETECTION_CVPR_2019 = {
    "class_range": OrderedDict([("car", 50), ("truck", 50), ("bus", 50), ("trailer", 50), ("construction_vehicle", 50), ("pedestrian", 40),
                                ("motorcycle", 40), ("bicycle", 40), ("traffic_cone", 30), ("barrier", 30)]),
    "dist_fcn": "center_distance",
    "dist_ths": [0.5, 1.0, 2.0, 4.0],
    "dist_th_tp": 2.0,
    "min_recall": 0.1,
    "min_precision": 0.1,
    "max_boxes_per_sample": 500,
    "mean_ap_weight": 5,
}
TP_METRICS = ["trans_err", "scale_err", "orient_err", "vel_err", "attr_err"]
# nuscenes/eval/detection/constants.py ATTRIBUTE_NAMES
ATTRIBUTE_NAMES = ["pedestrian.moving", "pedestrian.sitting_lying_down", "pedestrian.standing", "cycle.with_rider", "cycle.without_rider",
                   "vehicle.moving", "vehicle.parked", "vehicle.stopped"]
N_RECALL = 101  # DetectionMetricData.nelem


class NuscenesGroundTruth:
    """The GT side of a nuScenes split, per sample token: the boxes as `DetectionBox.serialize()` writes them (the output of the
    devkit's `load_gt`), the sample's ego translation (the LIDAR_TOP ego pose of `add_center_dist`) and its
    `static_object.bicycle_rack` boxes (translation, size, rotation) for `filter_eval_boxes`.  Extracted once where the devkit and the
    dataset are installed (`from_devkit(...).to_json(path)`), evaluated anywhere (`from_json(path)`)."""
    def __init__(self, boxes, ego_translation, bike_racks=None):
        self.boxes = OrderedDict((str(k), list(v)) for k, v in boxes.items())
        self.ego_translation = {str(k): [float(x) for x in v] for k, v in ego_translation.items()}
        racks = {} if bike_racks is None else bike_racks
        self.bike_racks = {str(k): [dict(translation=list(map(float, r["translation"])), size=list(map(float, r["size"])),
                                         rotation=list(map(float, r["rotation"]))) for r in racks.get(k, [])] for k in self.boxes}
        missing = [k for k in self.boxes if k not in self.ego_translation]
        if missing:
            raise ValueError(f"NuscenesGroundTruth: no ego translation for {len(missing)} sample(s), e.g. {missing[0]}")

    @property
    def sample_tokens(self):
        return list(self.boxes.keys())

    def to_json(self, path):
        """NaN velocities are written as `NaN` (Python's json) and read back as NaN."""
        with open(path, "w") as f:
            json.dump({"boxes": self.boxes, "ego_translation": self.ego_translation, "bike_racks": self.bike_racks}, f)

    @classmethod
    def from_json(cls, path):
        with open(path) as f:
            d = json.load(f, object_pairs_hook=OrderedDict)
        return cls(d["boxes"], d["ego_translation"], d.get("bike_racks"))

    @classmethod
    def from_devkit(cls, nusc, eval_set):
        """The devkit's own `load_gt(nusc, eval_set, DetectionBox)`, plus the ego poses (`add_center_dist`) and bike racks
        (`filter_eval_boxes`) read with `nusc.get` as those functions do."""
        from nuscenes.eval.common.loaders import load_gt
        from nuscenes.eval.detection.data_classes import DetectionBox
        gt = load_gt(nusc, eval_set, DetectionBox, verbose=False)
        boxes, ego, racks = OrderedDict(), {}, {}
        for token in gt.sample_tokens:
            out = []
            for b in gt[token]:
                s = b.serialize()
                for key in ("translation", "size", "rotation", "velocity", "ego_translation"):
                    s[key] = [float(x) for x in s[key]]
                s["num_pts"], s["detection_score"] = int(s["num_pts"]), float(s["detection_score"])
                out.append(s)
            boxes[token] = out
            sample = nusc.get("sample", token)
            sd = nusc.get("sample_data", sample["data"]["LIDAR_TOP"])
            ego[token] = list(nusc.get("ego_pose", sd["ego_pose_token"])["translation"])
            recs = [nusc.get("sample_annotation", ann) for ann in sample["anns"]]
            racks[token] = [dict(translation=r["translation"], size=r["size"], rotation=r["rotation"]) for r in recs
                            if r["category_name"] == "static_object.bicycle_rack"]
        return cls(boxes, ego, racks)


# ---------------------------------------------------------------------------------------------------------------------------
# box geometry (pyquaternion / nuscenes.utils.data_classes.Box restated in float64 numpy, many boxes at once)
# ---------------------------------------------------------------------------------------------------------------------------
def _rotation_matrices(q):
    """[n][4] quaternions (w, x, y, z) -> [n][3][3] rotation matrices of the normalised quaternions."""
    q = q / np.sqrt(np.sum(q * q, axis=1))[:, None]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((len(q), 3, 3))
    R[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R[:, 0, 1] = 2 * (x * y - w * z)
    R[:, 0, 2] = 2 * (x * z + w * y)
    R[:, 1, 0] = 2 * (x * y + w * z)
    R[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R[:, 1, 2] = 2 * (y * z - w * x)
    R[:, 2, 0] = 2 * (x * z - w * y)
    R[:, 2, 1] = 2 * (y * z + w * x)
    R[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R


def _yaw(q):
    """quaternion_yaw: atan2 of the rotated x axis."""
    R = _rotation_matrices(q)
    return np.arctan2(R[:, 1, 0], R[:, 0, 0])


def _in_rack(points, rack_t, rack_s, rack_q):
    """points_in_box(rack, point) for paired rows: [n][3] points against [n] racks (size [w, l, h]).  Inclusive bounds."""
    R = _rotation_matrices(rack_q)
    w, l, h = rack_s[:, 0], rack_s[:, 1], rack_s[:, 2]

    def corner(sx, sy, sz):  # R @ (sx l/2, sy w/2, sz h/2) + centre
        c = np.stack([sx * l / 2, sy * w / 2, sz * h / 2], axis=1)
        return (R[:, :, 0] * c[:, 0:1] + R[:, :, 1] * c[:, 1:2]) + R[:, :, 2] * c[:, 2:3] + rack_t

    c0, c1, c3, c4 = corner(1, 1, 1), corner(1, -1, 1), corner(1, 1, -1), corner(-1, 1, 1)
    v = points - c0
    inside = np.ones(len(points), dtype=bool)
    for e in (c4 - c0, c1 - c0, c3 - c0):
        ev = (e[:, 0] * v[:, 0] + e[:, 1] * v[:, 1]) + e[:, 2] * v[:, 2]
        ee = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        inside &= (0 <= ev) & (ev <= ee)
    return inside


# ---------------------------------------------------------------------------------------------------------------------------
# devkit helpers (eval/common/utils.py, eval/detection/algo.py)
# ---------------------------------------------------------------------------------------------------------------------------
def cummean(x):
    """eval/common/utils.py cummean: running mean ignoring NaN; all NaN -> ones."""
    if sum(np.isnan(x)) == len(x):
        return np.ones(len(x))
    sum_vals = np.nancumsum(x.astype(float))
    count_vals = np.cumsum(~np.isnan(x))
    return np.divide(sum_vals, count_vals, out=np.zeros_like(sum_vals), where=count_vals != 0)


def calc_ap(precision, min_recall, min_precision):
    prec = np.copy(precision)
    prec = prec[round(100 * min_recall) + 1:]
    prec -= min_precision
    prec[prec < 0] = 0
    return float(np.mean(prec)) / (1.0 - min_precision)


def calc_tp(confidence, metric, min_recall):
    first_ind = round(100 * min_recall) + 1
    non_zero = np.nonzero(confidence)[0]
    last_ind = 0 if len(non_zero) == 0 else non_zero[-1]
    if last_ind < first_ind:
        return 1.0
    return float(np.mean(metric[first_ind:last_ind + 1]))


def _no_predictions():
    return dict(precision=np.zeros(N_RECALL), confidence=np.zeros(N_RECALL), **{m: np.ones(N_RECALL) for m in TP_METRICS})


class _Boxes:
    """Boxes of many samples as flat float64 / int arrays (one row per box, samples in order)."""


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("NuscenesDetectionEval needs the MI355X: its matching is a HIP kernel (libdd3d_hip.so); there is no CPU fallback")


class NuscenesDetectionEval:
    """`DetectionEval(...).evaluate()` followed by `metrics.serialize()` minus `cfg` and `eval_time`, on a `NuscenesGroundTruth`."""
    def __init__(self, ground_truth, config=DETECTION_CVPR_2019):
        self.gt = ground_truth
        self.cfg = config
        self.class_names = list(config["class_range"].keys())

    # -- 1. loading ------------------------------------------------------------------------------------------------------
    def _load_predictions(self, results):
        """load_prediction + DetectionBox.deserialize checks: every violation raises."""
        cap = self.cfg["max_boxes_per_sample"]
        cls_id = {c: i for i, c in enumerate(self.class_names)}
        attrs = set(ATTRIBUTE_NAMES) | {""}
        tokens, rows = [], []
        for token, boxes in results.items():
            if len(boxes) > cap:
                raise ValueError(f"Error: Only <= {cap} boxes per sample allowed! (sample {token} has {len(boxes)})")
            tokens.append(token)
            rows.append(boxes)
        b = _Boxes()
        b.tokens = tokens
        b.count = np.array([len(r) for r in rows], dtype=np.int64)
        flat = [box for r in rows for box in r]
        n = len(flat)
        b.sample = np.repeat(np.arange(len(tokens)), b.count)
        try:
            b.t = np.array([box["translation"] for box in flat], dtype=np.float64).reshape(n, 3)
            b.s = np.array([box["size"] for box in flat], dtype=np.float64).reshape(n, 3)
            b.q = np.array([box["rotation"] for box in flat], dtype=np.float64).reshape(n, 4)
            b.v = np.array([box["velocity"] for box in flat], dtype=np.float64).reshape(n, 2)
            b.score = np.array([float(box["detection_score"]) for box in flat], dtype=np.float64)
            b.num_pts = np.array([int(box.get("num_pts", -1)) for box in flat], dtype=np.int64)
            names = [box["detection_name"] for box in flat]
            b.attr = np.array([box["attribute_name"] for box in flat], dtype=object)
        except (KeyError, TypeError, ValueError) as e:
            raise ValueError(f"nuScenes predictions: malformed box ({e!r}); each needs translation[3], size[3], rotation[4], velocity[2], "
                             "detection_name, detection_score, attribute_name") from e
        bad = [x for x in set(names) if x not in cls_id]
        if bad:
            raise ValueError(f"nuScenes predictions: detection_name {bad[0]!r} is not one of {self.class_names}")
        b.cls = np.array([cls_id[x] for x in names], dtype=np.int64)
        bad = [x for x in set(b.attr.tolist()) if x not in attrs]
        if bad:
            raise ValueError(f"nuScenes predictions: attribute_name {bad[0]!r} is not a nuScenes attribute or ''")
        for what, a in (("translation", b.t), ("size", b.s), ("rotation", b.q), ("detection_score", b.score)):
            if np.isnan(a).any():
                raise ValueError(f"nuScenes predictions: NaN in {what}")
        if not (b.s > 0).all():
            raise ValueError("nuScenes predictions: every size must be > 0 (scale_iou asserts it)")
        return b

    def _load_gt(self, tokens):
        """GT of the prediction samples, in the predictions' sample order (nuscenes_evaluator.py:103-115)."""
        missing = [t for t in tokens if t not in self.gt.boxes]
        assert not missing, "Samples in prediction must be a subset of samples in split."
        cls_id = {c: i for i, c in enumerate(self.class_names)}
        rows = [self.gt.boxes[t] for t in tokens]
        flat = [box for r in rows for box in r]
        n = len(flat)
        b = _Boxes()
        b.tokens = tokens
        b.count = np.array([len(r) for r in rows], dtype=np.int64)
        b.sample = np.repeat(np.arange(len(tokens)), b.count)
        b.t = np.array([box["translation"] for box in flat], dtype=np.float64).reshape(n, 3)
        b.s = np.array([box["size"] for box in flat], dtype=np.float64).reshape(n, 3)
        b.q = np.array([box["rotation"] for box in flat], dtype=np.float64).reshape(n, 4)
        b.v = np.array([box["velocity"] for box in flat], dtype=np.float64).reshape(n, 2)
        b.num_pts = np.array([int(box.get("num_pts", -1)) for box in flat], dtype=np.int64)
        b.cls = np.array([cls_id.get(box["detection_name"], -1) for box in flat], dtype=np.int64)
        if (b.cls < 0).any():
            raise ValueError("nuScenes ground truth: a detection_name outside the detection classes")
        b.attr = np.array([box["attribute_name"] for box in flat], dtype=object)
        if not (b.s > 0).all():
            raise ValueError("nuScenes ground truth: every size must be > 0 (scale_iou asserts it)")
        return b

    # -- 2. add_center_dist + filter_eval_boxes ------------------------------------------------------------------------------
    def _keep(self, b):
        """The three filters of filter_eval_boxes, in order, as one mask (filtering keeps the relative order of the rest)."""
        ego = np.array([self.gt.ego_translation[t] for t in b.tokens], dtype=np.float64).reshape(-1, 3)
        e = b.t - ego[b.sample]
        ego_dist = np.sqrt(np.sum(e[:, :2] ** 2, axis=1))
        rng = np.array([self.cfg["class_range"][c] for c in self.class_names], dtype=np.float64)
        keep = ego_dist < rng[b.cls]
        keep &= ~(b.num_pts == 0)
        cyc = np.array([self.class_names.index(c) for c in ("bicycle", "motorcycle") if c in self.class_names])
        cand = np.nonzero(keep & np.isin(b.cls, cyc))[0]
        if len(cand):
            racks = [self.gt.bike_racks.get(t, []) for t in b.tokens]
            n_rack = np.array([len(r) for r in racks], dtype=np.int64)
            if n_rack.sum():
                rack_begin = np.concatenate([[0], np.cumsum(n_rack)])
                flat = [r for rr in racks for r in rr]
                rt = np.array([r["translation"] for r in flat], dtype=np.float64).reshape(-1, 3)
                rs = np.array([r["size"] for r in flat], dtype=np.float64).reshape(-1, 3)
                rq = np.array([r["rotation"] for r in flat], dtype=np.float64).reshape(-1, 4)
                per = n_rack[b.sample[cand]]
                box = np.repeat(cand, per)
                start = np.repeat(rack_begin[b.sample[cand]], per)
                rack = start + (np.arange(len(box)) - np.repeat(np.cumsum(per) - per, per))
                hit = _in_rack(b.t[box], rt[rack], rs[rack], rq[rack])
                keep[box[hit]] = False
        return keep

    # -- 3. segments + the matching launch ---------------------------------------------------------------------------------
    def _segments(self, pred, gt):
        """Per class, the devkit's order (descending score, later prediction first on ties, across samples); then the (class,
        sample) segments: prediction rows in that order, GT rows in the sample's order."""
        n_s = len(pred.tokens)
        order = []
        for c in range(len(self.class_names)):
            idx = np.nonzero(pred.cls == c)[0]
            # sorted((v, i) for (i, v) in enumerate(confs))[::-1]
            o = idx[np.lexsort((np.arange(len(idx)), pred.score[idx]))[::-1]]
            order.append(o)
        seg_pred = [o[np.argsort(pred.sample[o], kind="stable")] for o in order]
        pred_rows = np.concatenate(seg_pred) if seg_pred else np.zeros(0, np.int64)
        pred_key = pred.cls[pred_rows] * n_s + pred.sample[pred_rows]
        gt_rows = np.lexsort((np.arange(len(gt.cls)), gt.sample, gt.cls))
        gt_key = gt.cls[gt_rows] * n_s + gt.sample[gt_rows]
        n_seg = len(self.class_names) * n_s
        pred_begin = np.searchsorted(pred_key, np.arange(n_seg + 1)).astype(np.int32)
        gt_begin = np.searchsorted(gt_key, np.arange(n_seg + 1)).astype(np.int32)
        return order, pred_rows, gt_rows, pred_begin, gt_begin

    def _match(self, pred, gt, pred_rows, gt_rows, pred_begin, gt_begin, clock):
        """match[t][pred box] = matched GT box (index into `gt`) or -1: one launch for every segment and threshold, one read-back."""
        device = torch.device("cuda", torch.cuda.current_device())
        ths = list(self.cfg["dist_ths"])
        n_pred, n_gt = len(pred_rows), len(gt_rows)
        if n_pred == 0 or n_gt == 0:  # nothing can match (and every class has npos == 0 when there is no GT)
            return np.full((len(ths), len(pred.cls)), -1, dtype=np.int64)
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dt)  # noqa: E731
        pred_xy = t(pred.t[pred_rows, :2], torch.float64)
        gt_xy = t(gt.t[gt_rows, :2], torch.float64)
        pb, gb = t(pred_begin, torch.int32), t(gt_begin, torch.int32)
        match = torch.empty((len(ths), n_pred), dtype=torch.int32, device=device)
        clock.lap("upload")
        args = hip.NuscMatchArgs(pred_xy=pred_xy.data_ptr(), gt_xy=gt_xy.data_ptr(), pred_begin=pb.data_ptr(), gt_begin=gb.data_ptr(),
                                 pred_begin_host=pred_begin.ctypes.data_as(C.c_void_p), gt_begin_host=gt_begin.ctypes.data_as(C.c_void_p),
                                 n_seg=len(pred_begin) - 1, n_pred=n_pred, n_gt=n_gt, n_thr=len(ths))
        for i, th in enumerate(ths):
            args.thr[i] = th
        clock.event_start()
        hip.check(hip.lib().dd3d_nusc_center_match(C.byref(args), match.data_ptr(), hip.current_stream()), "nusc_center_match")
        clock.event_stop()
        m = match.cpu().numpy()
        clock.lap("kernel")
        out = np.full((len(ths), len(pred.cls)), -1, dtype=np.int64)
        out[:, pred_rows] = np.where(m >= 0, gt_rows[np.maximum(m, 0)], -1)
        return out

    # -- 4. accumulate + metrics -------------------------------------------------------------------------------------------
    def _accumulate(self, pred, gt, order, npos, match, c, t, want_tp):
        """accumulate(class c, dist_ths[t]) from the match decisions: a dict of the DetectionMetricData curves used downstream."""
        if npos == 0:
            return _no_predictions()
        o = order[c]
        m = match[t, o]
        hit = m >= 0
        if not hit.any():
            return _no_predictions()
        tp = np.cumsum(hit.astype(np.int64)).astype(float)
        fp = np.cumsum((~hit).astype(np.int64)).astype(float)
        conf = pred.score[o]
        prec = tp / (fp + tp)
        rec = tp / float(npos)
        rec_interp = np.linspace(0, 1, N_RECALL)
        md = dict(precision=np.interp(rec_interp, rec, prec, right=0), confidence=np.interp(rec_interp, rec, conf, right=0))
        if not want_tp:
            return md
        p, g = o[hit], m[hit]
        dx, dy = pred.t[p, 0] - gt.t[g, 0], pred.t[p, 1] - gt.t[g, 1]
        dvx, dvy = pred.v[p, 0] - gt.v[g, 0], pred.v[p, 1] - gt.v[g, 1]
        gs, ps = gt.s[g], pred.s[p]
        inter = np.prod(np.minimum(gs, ps), axis=1)
        period = np.pi if self.class_names[c] == "barrier" else 2 * np.pi
        diff = (_yaw(gt.q[g]) - _yaw(pred.q[p]) + period / 2) % period - period / 2
        diff = np.where(diff > np.pi, diff - 2 * np.pi, diff)
        ga = gt.attr[g]
        errs = dict(trans_err=np.sqrt(dx * dx + dy * dy), vel_err=np.sqrt(dvx * dvx + dvy * dvy),
                    scale_err=1 - inter / (np.prod(gs, axis=1) + np.prod(ps, axis=1) - inter), orient_err=np.abs(diff),
                    attr_err=np.where(ga == "", np.nan, 1 - (ga == pred.attr[p]).astype(float)))
        match_conf = conf[hit]
        for key in TP_METRICS:
            tmp = cummean(errs[key])
            md[key] = np.interp(md["confidence"][::-1], match_conf[::-1], tmp[::-1])[::-1]
        return md

    def evaluate(self, results, timings=None):
        """`results`: the submission's `results` dict (sample token -> list of boxes), in the order the devkit reads it.  Returns
        {label_aps, mean_dist_aps, mean_ap, label_tp_errors, tp_errors, tp_scores, nd_score}.  `timings`, when a dict, receives the
        seconds of host preparation, upload, kernel (device events) and host accumulation."""
        _require_gpu()
        clock = _Clock(timings)
        pred = self._load_predictions(results)
        gt = self._load_gt(pred.tokens)
        pred = _subset(pred, self._keep(pred))
        gt = _subset(gt, self._keep(gt))
        order, pred_rows, gt_rows, pred_begin, gt_begin = self._segments(pred, gt)
        clock.lap("prepare")
        match = self._match(pred, gt, pred_rows, gt_rows, pred_begin, gt_begin, clock)
        ths = list(self.cfg["dist_ths"])
        t_tp = ths.index(self.cfg["dist_th_tp"])
        npos = np.bincount(gt.cls, minlength=len(self.class_names))
        label_aps, label_tp_errors = OrderedDict(), OrderedDict()
        for c, name in enumerate(self.class_names):
            label_aps[name] = OrderedDict()
            md_tp = None
            for t, th in enumerate(ths):
                md = self._accumulate(pred, gt, order, int(npos[c]), match, c, t, want_tp=t == t_tp)
                label_aps[name][th] = calc_ap(md["precision"], self.cfg["min_recall"], self.cfg["min_precision"])
                if t == t_tp:
                    md_tp = md
            label_tp_errors[name] = OrderedDict()
            for metric in TP_METRICS:
                if name in ["traffic_cone"] and metric in ["attr_err", "vel_err", "orient_err"]:
                    tp = np.nan
                elif name in ["barrier"] and metric in ["attr_err", "vel_err"]:
                    tp = np.nan
                else:
                    tp = calc_tp(md_tp["confidence"], md_tp[metric], self.cfg["min_recall"])
                label_tp_errors[name][metric] = tp
        out = _summary(label_aps, label_tp_errors, self.class_names, self.cfg["mean_ap_weight"])
        clock.lap("accumulate")
        if timings is not None:
            timings["kernel_events"] = clock.kernel_seconds()
        return out


def _subset(b, keep):
    s = _Boxes()
    s.tokens, s.sample = b.tokens, b.sample[keep]
    for k in ("t", "s", "q", "v", "num_pts", "cls", "attr"):
        setattr(s, k, getattr(b, k)[keep])
    if hasattr(b, "score"):
        s.score = b.score[keep]
    return s


def _summary(label_aps, label_tp_errors, class_names, mean_ap_weight):
    """DetectionMetrics.serialize() minus cfg and eval_time."""
    mean_dist_aps = OrderedDict((c, np.mean(list(d.values()))) for c, d in label_aps.items())
    mean_ap = float(np.mean(list(mean_dist_aps.values())))
    tp_errors = OrderedDict()
    for metric in TP_METRICS:
        tp_errors[metric] = float(np.nanmean([label_tp_errors[c][metric] for c in class_names]))
    tp_scores = OrderedDict((m, max(0.0, 1.0 - tp_errors[m])) for m in TP_METRICS)
    total = float(mean_ap_weight * mean_ap + np.sum(list(tp_scores.values())))
    nd_score = total / float(mean_ap_weight + len(tp_scores.keys()))
    return OrderedDict(label_aps=label_aps, mean_dist_aps=mean_dist_aps, mean_ap=mean_ap, label_tp_errors=label_tp_errors, tp_errors=tp_errors,
                       tp_scores=tp_scores, nd_score=nd_score)


class _Clock:
    def __init__(self, timings):
        self.timings = timings
        self.ev = None
        self.t = self._now()

    def _now(self):
        if self.timings is None:
            return 0.0
        torch.cuda.synchronize()
        return time.perf_counter()

    def lap(self, name):
        if self.timings is None:
            return
        t = self._now()
        self.timings[name] = self.timings.get(name, 0.0) + t - self.t
        self.t = t

    def event_start(self):
        if self.timings is not None:
            self.ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.ev[0].record()

    def event_stop(self):
        if self.ev is not None:
            self.ev[1].record()

    def kernel_seconds(self):
        if self.ev is None:
            return 0.0
        self.ev[1].synchronize()
        return self.ev[0].elapsed_time(self.ev[1]) / 1000.0

