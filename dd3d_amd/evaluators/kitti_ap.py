"""KITTI 3D / BEV AP engine: tridet/evaluators/kitti_3d_evaluator.py `KITTIEvaluationEngine` (:267-632), `clean_kitti_data`
(:635-746) and `get_thresholds` (:813-847) with the reference's names, arguments and results.

Where the reference runs numba CPU loops (one greedy matching per image x class x difficulty x overlap threshold [x score
threshold]), this engine runs two HIP launches per metric (dd3d_amd/csrc/kitti_ap.hip):

  1. overlaps of every shard on the device (`dd3d_rotate_iou_eval` / `dd3d_d3_box_overlap`, :622-632); each image's diagonal block
     is cut into one compact device buffer and the shard matrix is dropped (pairs are independent: the shard size changes no value);
  2. pass 1 (compute_threshold_jit :749-810) for all images, classes, difficulties and overlap thresholds in one launch; the scores
     of the true positives come back to the host once, for get_thresholds;
  3. the thresholds go to the device once; pass 2 (compute_statistics_jit :910-1038, tp / fp / fn only: the other `pr` columns are
     discarded by evaluate) in one launch; the counts come back once;
  4. recall / precision / r40 AP on the host with the reference's float64 operations in the reference's order, so the result is
     bit-identical once the integer counts agree (NaN where a denominator is 0 included).

The engine needs the GPU, as the reference's does (numba.cuda overlaps); there is no CPU fallback.
"""
import ctypes as C
import time
from collections import OrderedDict
from functools import partial

import numpy as np
import torch

from dd3d_amd import hip

DIFFICULTIES = ("Easy", "Moderate", "Hard")


# ---------------------------------------------------------------------------------------------------------------------------
# clean_kitti_data (:635-746), vectorised over every box of every image
# ---------------------------------------------------------------------------------------------------------------------------
def _lower(names):
    return np.array([str(n).lower() for n in names], dtype=object)


def kitti_gt_codes(names_lower, bbox, occluded, truncated, class_name, difficulty, params):
    """ignored_gt of clean_kitti_data (:690-718) for many boxes: int8 -1 (other class), 0 (valid), 1 (ignored: Van for Car,
    Person_sitting for Pedestrian, or too occluded / truncated / small for the difficulty)."""
    cls = class_name.lower()
    valid = np.full(len(names_lower), -1, dtype=np.int8)
    if cls == "pedestrian":
        valid[names_lower == "person_sitting"] = 0
    elif cls == "car":
        valid[names_lower == "van"] = 0
    valid[names_lower == cls] = 1
    height = bbox[:, 3] - bbox[:, 1]
    too_hard = ((occluded > params["max_occlusion"][difficulty]) | (truncated > params["max_truncation"][difficulty])
                | (height <= params["min_height"][difficulty]))
    return np.where((valid == 1) & ~too_hard, 0, np.where((valid == 0) | (too_hard & (valid == 1)), 1, -1)).astype(np.int8)


def kitti_dt_codes(names_lower, bbox, class_name, difficulty, params):
    """ignored_dt of clean_kitti_data (:724-736): 1 when the box is lower than the difficulty's minimum height (whatever its
    class), else 0 for the class and -1 for any other."""
    height = np.abs(bbox[:, 3] - bbox[:, 1])
    return np.where(height < params["min_height"][difficulty], 1, np.where(names_lower == class_name.lower(), 0, -1)).astype(np.int8)


def clean_kitti_data(gt_anno, dt_anno, current_class, difficulty, id_to_name, difficulty_level_to_params=None):
    """kitti_3d_evaluator.py:635-746: (num_valid_gt, ignored_gt, ignored_dt, ignored_bboxes) of one image."""
    params = difficulty_level_to_params
    name = id_to_name[current_class]
    gl = _lower(gt_anno["name"])
    gbox = np.asarray(gt_anno["bbox"], dtype=np.float64).reshape(-1, 4)
    ign_gt = kitti_gt_codes(gl, gbox, np.asarray(gt_anno["occluded"]), np.asarray(gt_anno["truncated"]), name, difficulty, params)
    ign_dt = kitti_dt_codes(_lower(dt_anno["name"]), np.asarray(dt_anno["bbox"], dtype=np.float64).reshape(-1, 4), name, difficulty, params)
    ignored_bboxes = [gt_anno["bbox"][i] for i in np.nonzero(gl == "dontcare")[0]]
    return int((ign_gt == 0).sum()), ign_gt.tolist(), ign_dt.tolist(), ignored_bboxes


# ---------------------------------------------------------------------------------------------------------------------------
# get_thresholds (:813-847)
# ---------------------------------------------------------------------------------------------------------------------------
def get_thresholds(scores, num_gt, num_sample_pts=41):
    """kitti_3d_evaluator.py:813-847, the same float64 operations in the same order.  The reference walks every score; between two
    picks `current_recall` is fixed, so each pick is the first index at or after the previous pick where the reference's skip
    test fails, found with one vector comparison (at most num_sample_pts + 1 of them).  The caller's array is not sorted in place."""
    scores = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
    n = len(scores)
    if n == 0:
        return []
    i = np.arange(n)
    l_recall = (i + 1) / num_gt
    r_recall = np.where(i < n - 1, (i + 2) / num_gt, l_recall)
    last = i == n - 1
    step = 1 / (num_sample_pts - 1.0)
    current_recall = 0
    thresholds = []
    start = 0
    while start < n:
        keep = ~((r_recall[start:] - current_recall) < (current_recall - l_recall[start:])) | last[start:]
        k = start + int(np.argmax(keep))  # the last score is always kept
        thresholds.append(scores[k])
        current_recall += step
        start = k + 1
    return thresholds


def _require_gpu():
    if not torch.cuda.is_available():
        raise RuntimeError("KITTIEvaluationEngine needs the MI355X: its overlaps and matchings are HIP kernels (libdd3d_hip.so), "
                           "as the reference's are numba.cuda ones; there is no CPU fallback")


class _Prepared:
    """Host preparation shared by both metrics: concatenated boxes, prefix offsets, ignore codes, block offsets, shard gathers."""


class KITTIEvaluationEngine:
    """kitti_3d_evaluator.py:267-632."""

    _DEFAULT_KITTI_LEVEL_TO_PARAMETER = {
        "levels": ("easy", "moderate", "hard"),
        "max_occlusion": (0, 1, 2),
        "max_truncation": (0.15, 0.3, 0.5),
        "min_height": (40, 25, 25)
    }

    def __init__(self, id_to_name, num_shards=50, sample_points=41):
        self.id_to_name = id_to_name
        self.sample_points = sample_points
        self.num_shards = num_shards
        self.filter_data_fn = partial(clean_kitti_data, difficulty_level_to_params=self._DEFAULT_KITTI_LEVEL_TO_PARAMETER)

    @staticmethod
    def _format(idx, kitti_format, is_prediction):
        """:282-315: one image's KITTI rows (DataFrame or list of rows) -> annotation dict; dimensions reordered [:, [2, 0, 1]]."""
        if len(kitti_format) == 0:
            return dict(id=f"{idx:06d}", name=[], truncated=np.array([]), occluded=np.array([]), alpha=np.array([]), bbox=np.empty((0, 4)),
                        dimensions=np.empty((0, 3)), location=np.empty((0, 3)), rotation_y=np.array([]), score=np.array([]))
        data = np.array(kitti_format)
        annotations = dict(
            id=f"{idx:06d}",
            name=data[:, 0],
            truncated=data[:, 1].astype(np.float64),
            occluded=data[:, 2].astype(np.int64),
            alpha=data[:, 3].astype(np.float64),
            bbox=data[:, 4:8].astype(np.float64),
            dimensions=data[:, 8:11][:, [2, 0, 1]].astype(np.float64),
            location=data[:, 11:14].astype(np.float64),
            rotation_y=data[:, 14].astype(np.float64),
        )
        if is_prediction:
            annotations["score"] = data[:, 15].astype(np.float64)
        else:
            annotations["score"] = np.zeros([len(annotations["bbox"])])
        return annotations

    def get_shards(self, num, num_shards):
        """:317-340: `num_shards` equal parts, the remainder in one more."""
        assert num_shards > 0, "Invalid number of shards"
        num_per_shard = num // num_shards
        remaining_num = num % num_shards
        full_shards = num_shards * (num_per_shard > 0)
        if remaining_num == 0:
            return [num_per_shard] * full_shards
        return [num_per_shard] * full_shards + [remaining_num]

    def evaluate(self, gt_annos, dt_annos, overlap_thresholds):
        """:342-360: OrderedDict kitti_box3d_r40/{class}_{Easy|Moderate|Hard}_{thresh}, then the same keys under kitti_bev_r40/."""
        gt_annos, dt_annos = self.validate_anno_format(gt_annos, dt_annos)
        prep = self._prepare(gt_annos, dt_annos, overlap_thresholds)
        box3d_pr_curves = self.eval_metric(gt_annos, dt_annos, "BOX3D_AP", overlap_thresholds, _prepared=prep)
        mAP_3d = self.get_mAP(box3d_pr_curves["precision"], box3d_pr_curves["recall"])
        bev_pr_curves = self.eval_metric(gt_annos, dt_annos, "BEV_AP", overlap_thresholds, _prepared=prep)
        mAP_bev = self.get_mAP(bev_pr_curves["precision"], bev_pr_curves["recall"])
        results = OrderedDict()
        for prefix, mAP in (("kitti_box3d_r40", mAP_3d), ("kitti_bev_r40", mAP_bev)):
            for class_i, class_name in self.id_to_name.items():
                for diff_i, diff in enumerate(DIFFICULTIES):
                    for thresh_i, thresh in enumerate(overlap_thresholds):
                        results["{}/{}_{}_{}".format(prefix, class_name, diff, thresh)] = mAP[class_i, diff_i, thresh_i]
        return results

    def get_mAP(self, precision, recall):
        """:362-382."""
        precisions, recall_spacing = self.get_sampled_precision_recall(precision, recall)
        return sum(precisions) / len(recall_spacing)

    def get_sampled_precision_recall(self, precision, recall):
        """:384-414: r40 sampling -- at recall k / (sample_points - 1), k >= 1, the largest precision whose recall reaches it."""
        recall_range = (0.0, 1.0)
        precisions = []
        recall_spacing = [1. / (self.sample_points - 1) * i for i in range(1, self.sample_points)]
        recall_spacing = [r for r in recall_spacing if recall_range[0] <= r <= recall_range[1]]
        for r in recall_spacing:
            precisions.append(((recall >= r) * precision).max(axis=3))
        return precisions, recall_spacing

    @staticmethod
    def validate_anno_format(gt_annos, dt_annos):
        """:416-438."""
        necessary_keys = ["name", "alpha", "bbox", "dimensions", "location", "rotation_y", "score"]
        for i, (gt_anno, dt_anno) in enumerate(zip(gt_annos, dt_annos)):
            for key in necessary_keys:
                assert key in gt_anno, "{} not present in GT {}".format(key, i)
                assert key in dt_anno, "{} not present in prediction {}".format(key, i)
                if key in ["bbox", "dimensions", "location"]:
                    assert len(gt_anno[key].shape) == 2, key
                    assert len(dt_anno[key].shape) == 2, key
            for key in ["truncated", "occluded", "alpha", "rotation_y", "score"]:
                if len(gt_anno[key].shape) == 2:
                    gt_anno[key] = np.squeeze(gt_anno[key], axis=0)
                if len(dt_anno[key].shape) == 2:
                    dt_anno[key] = np.squeeze(dt_anno[key], axis=0)
        return gt_annos, dt_annos

    # -----------------------------------------------------------------------------------------------------------------------
    # the device pipeline
    # -----------------------------------------------------------------------------------------------------------------------
    def _prepare(self, gt_annos, dt_annos, overlap_thresholds):
        """Everything both metrics share, computed once on the host: prefix offsets, ignore codes [class * 3 + difficulty][box],
        valid GT counts, the compact block layout and, per shard, the flat indices of its images' blocks in the shard matrix."""
        assert len(gt_annos) == len(dt_annos), "Must provide a prediction for every ground truth sample"
        p = _Prepared()
        n_img = len(gt_annos)
        ng = np.array([len(a["name"]) for a in gt_annos], dtype=np.int64)
        nd = np.array([len(a["name"]) for a in dt_annos], dtype=np.int64)
        p.n_img, p.ng, p.nd = n_img, ng, nd
        p.gt_begin = np.concatenate([[0], np.cumsum(ng)]).astype(np.int32)
        p.dt_begin = np.concatenate([[0], np.cumsum(nd)]).astype(np.int32)
        cat = lambda annos, key, shape: (np.concatenate([np.asarray(a[key], dtype=np.float64).reshape(shape) for a in annos], 0)  # noqa: E731
                                         if annos else np.zeros((0,) + shape[1:]))
        gbox, dbox = cat(gt_annos, "bbox", (-1, 4)), cat(dt_annos, "bbox", (-1, 4))
        p.dt_score = cat(dt_annos, "score", (-1,))
        occ, trunc = cat(gt_annos, "occluded", (-1,)), cat(gt_annos, "truncated", (-1,))
        gl = _lower([n for a in gt_annos for n in a["name"]])
        dl = _lower([n for a in dt_annos for n in a["name"]])
        params = self._DEFAULT_KITTI_LEVEL_TO_PARAMETER
        n_cls = len(self.id_to_name)
        p.ign_gt = np.stack([kitti_gt_codes(gl, gbox, occ, trunc, self.id_to_name[c], d, params) for c in range(n_cls) for d in range(3)]
                            )
        p.ign_dt = np.stack([kitti_dt_codes(dl, dbox, self.id_to_name[c], d, params) for c in range(n_cls) for d in range(3)])
        p.num_valid_gt = (p.ign_gt == 0).sum(axis=1)
        # boxes (x, y, z, l, h, w, rot_y) as the reference stacks them (:592-615), float32 as its overlap kernels take them
        p.gt7 = np.concatenate([cat(gt_annos, "location", (-1, 3)), cat(gt_annos, "dimensions", (-1, 3)), cat(gt_annos, "rotation_y", (-1, 1))], 1)
        p.dt7 = np.concatenate([cat(dt_annos, "location", (-1, 3)), cat(dt_annos, "dimensions", (-1, 3)), cat(dt_annos, "rotation_y", (-1, 1))], 1)
        # compact blocks: image i's [nd_i][ng_i] block at ov_off[i]
        m = nd * ng
        p.ov_off = np.concatenate([[0], np.cumsum(m)]).astype(np.int64)
        p.n_ov = int(p.ov_off[-1])
        # shards (:520-548) and, for every element of the compact buffer, its flat index in its shard's [N][K] matrix
        p.shards = []
        first = 0
        shard_of = np.zeros(n_img, dtype=np.int64)
        r0 = np.zeros(n_img, dtype=np.int64)
        c0 = np.zeros(n_img, dtype=np.int64)
        kcols = np.zeros(n_img, dtype=np.int64)
        for s, count in enumerate(self.get_shards(n_img, self.num_shards)):
            last = first + count
            rows = (int(p.dt_begin[first]), int(p.dt_begin[last]))
            cols = (int(p.gt_begin[first]), int(p.gt_begin[last]))
            p.shards.append((first, last, rows, cols))
            shard_of[first:last] = s
            r0[first:last] = p.dt_begin[first:last] - rows[0]
            c0[first:last] = p.gt_begin[first:last] - cols[0]
            kcols[first:last] = cols[1] - cols[0]
            first = last
        img = np.repeat(np.arange(n_img), m)
        e = np.arange(p.n_ov, dtype=np.int64) - p.ov_off[:-1][img]
        ngi = np.maximum(ng[img], 1)
        p.gather = (r0[img] + e // ngi) * kcols[img] + c0[img] + e % ngi
        p.min_overlap = np.ascontiguousarray(overlap_thresholds, dtype=np.float64).reshape(-1)
        p.max_dt = int(nd.max()) if n_img else 0
        p.max_gt = int(ng.max()) if n_img else 0
        return p

    def _upload(self, p, device):
        """Host arrays of `_prepare` -> device tensors (once per evaluate)."""
        if getattr(p, "dev", None) is not None:
            return p.dev
        t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a)).to(device=device, dtype=dt)  # noqa: E731
        p.dev = dict(gt7=t(p.gt7, torch.float32), dt7=t(p.dt7, torch.float32), gather=t(p.gather, torch.int64), ov_off=t(p.ov_off[:-1], torch.int64),
                     dt_begin=t(p.dt_begin, torch.int32), gt_begin=t(p.gt_begin, torch.int32), dt_score=t(p.dt_score, torch.float64),
                     ign_dt=t(p.ign_dt, torch.int8), ign_gt=t(p.ign_gt, torch.int8))
        return p.dev

    def _overlap_blocks(self, p, metric, device):
        """Compact float32 buffer of every image's [dt][gt] overlap block for `metric` (:550-632), built shard by shard."""
        L = hip.lib()
        d = self._upload(p, device)
        out = torch.empty(p.n_ov, dtype=torch.float32, device=device)
        bev_cols = [0, 2, 3, 5, 6]  # (x, z, l, w, rot_y): location[:, [0, 2]], dimensions[:, [0, 2]] (:594-601), and the 3D BEV part (:629)
        stream = hip.current_stream()
        for first, last, (ra, rb), (ca, cb) in p.shards:
            N, K = rb - ra, cb - ca
            if N == 0 or K == 0:
                continue
            dt = d["dt7"][ra:rb]
            gt = d["gt7"][ca:cb]
            dtb, gtb = dt[:, bev_cols].contiguous(), gt[:, bev_cols].contiguous()
            m = torch.empty((N, K), dtype=torch.float32, device=device)
            if metric == "BEV_AP":
                hip.check(L.dd3d_rotate_iou_eval(dtb.data_ptr(), gtb.data_ptr(), m.data_ptr(), N, K, -1, stream), "rotate_iou_eval")
            elif metric == "BOX3D_AP":
                hip.check(L.dd3d_rotate_iou_eval(dtb.data_ptr(), gtb.data_ptr(), m.data_ptr(), N, K, 2, stream), "rotate_iou_eval")
                hip.check(L.dd3d_d3_box_overlap(dt.contiguous().data_ptr(), gt.contiguous().data_ptr(), m.data_ptr(), N, K, -1, 1, stream),
                          "d3_box_overlap")
            else:
                raise ValueError("Unknown metric")
            a, b = int(p.ov_off[first]), int(p.ov_off[last])
            if b > a:
                out[a:b] = torch.take(m, d["gather"][a:b])
            del m
        return out

    def _match_args(self, p, ov):
        d = p.dev
        mo = p.min_overlap
        args = hip.KittiMatchArgs(
            ov=ov.data_ptr(), ov_off=d["ov_off"].data_ptr(), dt_begin=d["dt_begin"].data_ptr(), gt_begin=d["gt_begin"].data_ptr(),
            dt_score=d["dt_score"].data_ptr(), ign_dt=d["ign_dt"].data_ptr(), ign_gt=d["ign_gt"].data_ptr(),
            min_overlap=mo.ctypes.data_as(C.c_void_p), n_ov=p.n_ov, n_img=p.n_img, n_dt=len(p.dt_score), n_gt=p.ign_gt.shape[1],
            n_cd=p.ign_gt.shape[0], n_o=len(mo), max_dt=p.max_dt, max_gt=p.max_gt)
        return args

    def _tp_scores(self, p, ov):
        """Pass 1: [n_cd][n_o][n_gt] float64 on the host, -inf where a GT has no true positive."""
        n_cd, n_gt = p.ign_gt.shape
        tp = torch.full((n_cd, len(p.min_overlap), n_gt), float("-inf"), dtype=torch.float64, device=ov.device)
        args = self._match_args(p, ov)
        hip.check(hip.lib().dd3d_kitti_tp_scores(C.byref(args), tp.data_ptr(), hip.current_stream()), "kitti_tp_scores")
        return tp.cpu().numpy()

    def _thresholds(self, p, tp_scores):
        """get_thresholds per (class x difficulty, overlap) -> list of lists."""
        n_cd, n_o, _ = tp_scores.shape
        out = []
        for cd in range(n_cd):
            for o in range(n_o):
                s = tp_scores[cd, o]
                out.append(get_thresholds(s[s != -np.inf], int(p.num_valid_gt[cd]), self.sample_points))
        return out

    def _pr_counts(self, p, ov, thresholds):
        """Pass 2: [n_cd][n_o][t_max][3] int64 (tp, fp, fn) on the host."""
        n_cd, n_o = p.ign_gt.shape[0], len(p.min_overlap)
        t_max = max([len(t) for t in thresholds] + [0])
        if t_max == 0:
            return np.zeros((n_cd, n_o, 0, 3), dtype=np.int64)
        th = np.zeros((n_cd * n_o, t_max), dtype=np.float64)
        for i, t in enumerate(thresholds):
            th[i, :len(t)] = t
        nt = np.array([len(t) for t in thresholds], dtype=np.int32)
        th_d = torch.as_tensor(th).to(ov.device)
        nt_d = torch.as_tensor(nt).to(ov.device)
        counts = torch.empty((n_cd, n_o, t_max, 3), dtype=torch.int64, device=ov.device)
        args = self._match_args(p, ov)
        hip.check(hip.lib().dd3d_kitti_pr_counts(C.byref(args), th_d.data_ptr(), nt_d.data_ptr(), t_max, counts.data_ptr(), hip.current_stream()),
                  "kitti_pr_counts")
        return counts.cpu().numpy()

    def _curves(self, p, thresholds, counts):
        """recall / precision [n_cls][3][n_o][sample_points] from the counts (:505-508), zeros past each curve's thresholds."""
        n_cls, n_o = len(self.id_to_name), len(p.min_overlap)
        recall = np.zeros([n_cls, 3, n_o, self.sample_points])
        precision = np.zeros([n_cls, 3, n_o, self.sample_points])
        with np.errstate(invalid="ignore", divide="ignore"):
            for cd in range(n_cls * 3):
                for o in range(n_o):
                    n = len(thresholds[cd * n_o + o])
                    pr = counts[cd, o, :n].astype(np.float64)
                    recall[cd // 3, cd % 3, o, :n] = pr[:, 0] / (pr[:, 0] + pr[:, 2])
                    precision[cd // 3, cd % 3, o, :n] = pr[:, 0] / (pr[:, 0] + pr[:, 1])
        return recall, precision

    def eval_metric(self, gt_annos, dt_annos, metric, overlap_thresholds, _prepared=None, timings=None):
        """:440-513: {"recall", "precision"} [num_classes][3][num_overlaps][sample_points].  `timings`, when a dict, receives the
        seconds of each step (host preparation, overlaps, pass 1 with get_thresholds, pass 2 with the curves), device-synchronised."""
        _require_gpu()
        device = torch.device("cuda", torch.cuda.current_device())
        clock = _Clock(timings, device)
        p = _prepared if _prepared is not None else self._prepare(gt_annos, dt_annos, overlap_thresholds)
        assert len(p.min_overlap) == len(overlap_thresholds)
        self._upload(p, device)
        clock.lap("prepare")
        ov = self._overlap_blocks(p, metric, device)
        clock.lap("overlaps")
        thresholds = self._thresholds(p, self._tp_scores(p, ov))
        clock.lap("pass1")
        counts = self._pr_counts(p, ov, thresholds)
        recall, precision = self._curves(p, thresholds, counts)
        clock.lap("pass2")
        return {"recall": recall, "precision": precision}


class _Clock:
    def __init__(self, timings, device):
        self.timings, self.device = timings, device
        self.t = self._now()

    def _now(self):
        if self.timings is None:
            return 0.0
        torch.cuda.synchronize(self.device)
        return time.perf_counter()

    def lap(self, name):
        if self.timings is None:
            return
        t = self._now()
        self.timings[name] = self.timings.get(name, 0.0) + t - self.t
        self.t = t
