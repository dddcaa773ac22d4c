"""Result side of tridet/evaluators/kitti_3d_evaluator.py: `convert_3d_box_to_kitti` (:205-264) and `KITTI3DEvaluator.reset /
process / evaluate / prepare_kitti3d_submission` (:55-202) with the same names, arguments and outputs, the box conversion running
batched on the GPU (dd3d_amd.evaluators.formatting) and the AP engine (`KITTIEvaluationEngine` :267-1099) on HIP kernels
(dd3d_amd.evaluators.kitti_ap).
"""
import itertools
import json
import os
from collections import OrderedDict

import numpy as np
import pandas as pd
import torch

from dd3d_amd.evaluators.formatting import format_boxes3d, kitti_tuple, xyxy_to_xywh
from dd3d_amd.evaluators.kitti_ap import KITTIEvaluationEngine

BBOX3D_PREDICTION_FILE = "bbox3d_predictions.json"
KITTI_SUBMISSION_DIR = "kitti_3d_submission"


def convert_3d_box_to_kitti(box):
    """Single box (GenericBoxes3D of length 1, camera frame) -> (W, L, H, x, y, z, rot_y, alpha).  kitti_3d_evaluator.py:205-264."""
    assert len(box) == 1
    return kitti_tuple(format_boxes3d(box.vectorize())[0])


def _xyxy_of(anno):
    """BoxMode.convert(anno['bbox'], anno['bbox_mode'], XYXY_ABS) [ext] for the two modes KITTI dataset dicts use."""
    mode = anno.get("bbox_mode", 0)
    mode = int(getattr(mode, "value", mode))
    a = np.array(anno["bbox"], dtype=np.float64)
    if mode == 0:  # XYXY_ABS
        return a.tolist()
    if mode == 1:  # XYWH_ABS
        a[2] += a[0]
        a[3] += a[1]
        return a.tolist()
    raise NotImplementedError(f"bbox_mode {mode}")


class KITTI3DEvaluator:
    """`dataset_dicts` / `class_names` replace the detectron2 DatasetCatalog / MetadataCatalog lookups of the reference ctor
    (:43-49); when detectron2 is installed and they are omitted the catalogs are used as in the reference.  `id_to_name` replaces
    the catalog's `contiguous_id_to_name`; by default it is dict(enumerate(class_names)), which is what the KITTI dataset registers
    (kitti_3d/build.py:309)."""
    def __init__(self, dataset_name=None, iou_thresholds=None, only_prepare_submission=False, output_dir=None, distributed=False, *,
                 dataset_dicts=None, class_names=None, id_to_name=None):
        if dataset_dicts is None or class_names is None:
            from detectron2.data.catalog import DatasetCatalog, MetadataCatalog  # noqa: deliberate hard dependency of this branch
            dataset_dicts = DatasetCatalog.get(dataset_name) if dataset_dicts is None else dataset_dicts
            class_names = MetadataCatalog.get(dataset_name).thing_classes if class_names is None else class_names
        self._dataset_dicts = {d["file_name"]: d for d in dataset_dicts}
        self._class_names = list(class_names)
        self._id_to_name = dict(enumerate(self._class_names)) if id_to_name is None else dict(id_to_name)
        self._iou_thresholds = iou_thresholds
        self._only_prepare_submission = only_prepare_submission
        self._output_dir = output_dir
        self._distributed = distributed
        self.reset()

    def reset(self):
        self._predictions_as_json = []
        self._predictions_kitti_format = []
        self._groundtruth_kitti_format = []

    def process(self, inputs, outputs):
        """Same records as the reference's per-detection loop (:86-148); every box of the call (predictions and ground-truth
        annotations) goes through one conversion launch."""
        vecs, spans = [], []
        for inp, out in zip(inputs, outputs):
            inst = out["instances"]
            v = inst.pred_boxes3d.vectorize()
            gt = self._dataset_dicts.get(inp["file_name"], {})
            annos = gt.get("annotations") if gt.get("raw_kitti_annotations", None) is None else None
            g = torch.as_tensor(np.array([a["bbox3d"] for a in annos], dtype=np.float32).reshape(-1, 10)) if annos else torch.zeros((0, 10))
            spans.append((len(v), len(g)))
            vecs += [v, g.to(v.device)]
        conv = format_boxes3d(torch.cat(vecs, 0)) if vecs else np.zeros((0, 10))
        row = 0
        for (inp, out), (n_pred, n_gt) in zip(zip(inputs, outputs), spans):
            inst = out["instances"]
            classes = inst.pred_classes.cpu().tolist()
            boxes = inst.pred_boxes.tensor.cpu().tolist()
            vec = inst.pred_boxes3d.vectorize().cpu().numpy()
            scores = inst.scores.cpu().tolist()
            scores_3d = inst.scores_3d.cpu().tolist()
            file_name, image_id = inp["file_name"], inp["image_id"]
            kitti_rows = []
            for i in range(n_pred):
                name = self._class_names[classes[i]]
                self._predictions_as_json.append(OrderedDict(
                    category_id=int(classes[i]), category=name, bbox3d=vec[i].tolist(), bbox=xyxy_to_xywh(boxes[i]), score=float(scores[i]),
                    score_3d=float(scores_3d[i]), file_name=file_name, image_id=image_id))
                W, L, H, x, y, z, rot_y, alpha = kitti_tuple(conv[row + i])
                l, t, r, b = boxes[i]
                kitti_rows.append([name, -1, -1, alpha, l, t, r, b, H, W, L, x, y, z, rot_y, float(scores_3d[i])])
            self._predictions_kitti_format.append(pd.DataFrame(kitti_rows))
            row += n_pred
            gt = self._dataset_dicts[file_name]
            if "annotations" in gt:
                raw = gt.get("raw_kitti_annotations", None)
                if raw is not None:
                    self._groundtruth_kitti_format.append(raw)
                else:
                    gt_rows = []
                    for j, anno in enumerate(gt["annotations"]):
                        W, L, H, x, y, z, rot_y, alpha = kitti_tuple(conv[row + j])
                        l, t, r, b = _xyxy_of(anno)
                        gt_rows.append([self._class_names[anno["category_id"]], -1, -1, alpha, l, t, r, b, H, W, L, x, y, z, rot_y])
                    self._groundtruth_kitti_format.append(pd.DataFrame(gt_rows))
            row += n_gt

    def evaluate(self):
        """kitti_3d_evaluator.py:150-195: OrderedDict kitti_box3d_r40/{class}_{Easy|Moderate|Hard}_{iou} then kitti_bev_r40/..., in
        percent.  With distributed=True in a torch.distributed group of more than one process the three lists are gathered to rank 0
        and every other rank returns None.  The predictions are written to `output_dir`/bbox3d_predictions.json; with output_dir=None
        that file is not written (the reference needs a directory there).  only_prepare_submission writes the KITTI submission
        files under `output_dir`/kitti_3d_submission and returns {}.  The AP engine runs on the GPU (KITTIEvaluationEngine)."""
        if not self._only_prepare_submission and self._iou_thresholds is None:
            raise ValueError("KITTI3DEvaluator.evaluate needs iou_thresholds: the reference passes EVALUATORS.KITTI3D.IOU_THRESHOLDS "
                             "([0.5, 0.7] in configs/evaluators/kitti_3d.yaml)")
        if self._only_prepare_submission and self._output_dir is None:
            raise ValueError("KITTI3DEvaluator: only_prepare_submission writes the submission under output_dir, which is None")
        predictions_as_json = self._predictions_as_json
        predictions_kitti_format = self._predictions_kitti_format
        groundtruth_kitti_format = self._groundtruth_kitti_format
        import torch.distributed as dist
        if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            gathered = []
            for part in (predictions_as_json, predictions_kitti_format, groundtruth_kitti_format):
                dst = [None] * dist.get_world_size() if dist.get_rank() == 0 else None
                dist.gather_object(part, dst, dst=0)
                gathered.append(list(itertools.chain(*dst)) if dst is not None else None)
            if dist.get_rank() != 0:
                return None
            predictions_as_json, predictions_kitti_format, groundtruth_kitti_format = gathered
        if self._output_dir is not None:
            os.makedirs(self._output_dir, exist_ok=True)
            with open(os.path.join(self._output_dir, BBOX3D_PREDICTION_FILE), "w") as f:
                json.dump(predictions_as_json, f, indent=4)
        if self._only_prepare_submission:
            self.prepare_kitti3d_submission(predictions_kitti_format, submission_dir=os.path.join(self._output_dir, KITTI_SUBMISSION_DIR))
            return {}
        assert len(predictions_kitti_format) == len(groundtruth_kitti_format)
        formatted_predictions = [KITTIEvaluationEngine._format(idx, x, True) for idx, x in enumerate(predictions_kitti_format)]
        formatted_groundtruth = [KITTIEvaluationEngine._format(idx, x, False) for idx, x in enumerate(groundtruth_kitti_format)]
        engine = KITTIEvaluationEngine(id_to_name=self._id_to_name)
        results = engine.evaluate(formatted_groundtruth, formatted_predictions, overlap_thresholds=self._iou_thresholds)
        return OrderedDict({k: 100. * v for k, v in results.items()})

    @staticmethod
    def prepare_kitti3d_submission(predictions_kitti_format, submission_dir):
        """kitti_3d_evaluator.py:197-202: one space-separated text file per image."""
        assert not os.path.exists(submission_dir)
        os.makedirs(submission_dir)
        for idx, prediction in enumerate(predictions_kitti_format):
            prediction.to_csv(os.path.join(submission_dir, f"{idx:06d}.txt"), sep=" ", header=False, index=False)
