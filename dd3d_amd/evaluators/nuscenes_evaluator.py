"""Result side of tridet/evaluators/nuscenes_evaluator.py: `NuscenesEvaluator.reset / process / build_nusc_detection / evaluate`
(:138-312) with the same names and outputs; attribute naming on the host, the global velocity of every detection of the call in one
launch (dd3d_amd.evaluators.formatting).  `evaluate` writes the reference's two files and computes the nuScenes detection metrics with
the HIP engine of dd3d_amd.evaluators.nuscenes_eval in place of the devkit's `DetectionEval`.
"""
import itertools
import json
import os
from collections import OrderedDict, defaultdict

from dd3d_amd.evaluators.formatting import format_boxes3d, xyxy_to_xywh
from dd3d_amd.evaluators.nuscenes_eval import NuscenesDetectionEval, NuscenesGroundTruth
from dd3d_amd.modeling.nuscenes_dd3d import get_group_idxs

BBOX3D_PREDICTION_FILE = "bbox3d_predictions.json"
NUSC_SUBMISSION_FILE = "nuscenes_submission.json"

NUM_IMAGES_PER_SAMPLE = 6
# tridet/data/datasets/nuscenes/build.py:50-61 (CATEGORY_IDS order)
NUSCENES_DETECTION_CATEGORIES = ["barrier", "bicycle", "bus", "car", "construction_vehicle", "motorcycle", "pedestrian", "traffic_cone",
                                 "trailer", "truck"]
# nuscenes_evaluator.py:34-43
DEFAULT_ATTRIBUTES = {
    "car": "vehicle.moving", "bus": "vehicle.moving", "construction_vehicle": "vehicle.moving", "trailer": "vehicle.moving",
    "truck": "vehicle.moving", "bicycle": "cycle.with_rider", "motorcycle": "cycle.with_rider", "pedestrian": "pedestrian.moving"
}
# nuscenes_evaluator.py:58-64
VEH_ATTR_CLASSES = ("car", "bus", "construction_vehicle", "trailer", "truck")
PED_ATTR_CLASSES = ("pedestrian", )
CYC_ATTR_CLASSES = ("bicycle", "motorcycle")
VEH_ATTR_ID_TO_NAME = {0: "vehicle.moving", 1: "vehicle.parked", 2: "vehicle.stopped"}
PED_ATTR_ID_TO_NAME = {0: "pedestrian.moving", 1: "pedestrian.standing", 2: "pedestrian.sitting_lying_down"}
CYC_ATTR_ID_TO_NAME = {0: "cycle.with_rider", 1: "cycle.without_rider"}
# tridet/data/datasets/nuscenes/build.py:27-35
DATASET_NAME_TO_VERSION = {
    "nusc_train": "v1.0-trainval", "nusc_val": "v1.0-trainval", "nusc_val-subsample-8": "v1.0-trainval", "nusc_trainval": "v1.0-trainval",
    "nusc_test": "v1.0-test", "nusc_mini_train": "v1.0-mini", "nusc_mini_val": "v1.0-mini"
}
# nuscenes_evaluator.py:45-55
DATASET_NAME_TO_EVAL_SET = {
    "nusc_train": "train", "nusc_val": "val", "nusc_val-subsample-8": "val", "nusc_test": "test", "nusc_mini_train": "mini_train",
    "nusc_mini_val": "mini_val", "nusc_train_detect": "train_detect", "nusc_train_track": "train_track"
}
# nuscenes_evaluator.py:268-274
EVAL_META = {"use_camera": True, "use_lidar": False, "use_radar": False, "use_map": False, "use_external": True}


class NuscenesEvaluationUnavailable(NotImplementedError):
    """evaluate() cannot produce what was asked: the test split without an output_dir, or another split with neither
    `ground_truth=` nor the nuScenes devkit."""


def attribute_name(class_name, attr):
    """nuscenes_evaluator.py:185-193: the attribute id is taken modulo the size of the class family's table."""
    for classes, table in ((VEH_ATTR_CLASSES, VEH_ATTR_ID_TO_NAME), (PED_ATTR_CLASSES, PED_ATTR_ID_TO_NAME), (CYC_ATTR_CLASSES, CYC_ATTR_ID_TO_NAME)):
        if class_name in classes:
            return table[attr % len(table)]
    return ""


def _gather_dict(dikt):
    """tridet/utils/comm.py:71-88 gather_dict: the dicts of every rank merged on rank 0 (keys disjoint across ranks), None elsewhere."""
    import torch.distributed as dist
    dst = [None] * dist.get_world_size() if dist.get_rank() == 0 else None
    dist.gather_object(dikt, dst, dst=0)
    if dst is None:
        return None
    gathered = {}
    for d in dst:
        for k in d.keys():
            assert k not in gathered, f"Dictionary key overlaps: {k}"
        gathered.update(d)
    return gathered


class NuscenesEvaluator:
    """`ground_truth` (a NuscenesGroundTruth or the path of its JSON) replaces the devkit's `load_gt` on the dataset; without it the
    devkit is used when it is installed and `nusc_root` is set, as in the reference.  `distributed=True` gathers to rank 0, as the
    reference does whenever it runs distributed."""
    def __init__(self, nusc_root=None, dataset_name=None, output_dir=None, *, ground_truth=None, distributed=False):
        self._nusc_root = nusc_root
        self._dataset_name = dataset_name
        self._output_dir = output_dir
        self._only_make_submission_file = dataset_name == "nusc_test"
        self._ground_truth = ground_truth
        self._distributed = distributed
        self.reset()

    def reset(self):
        self._predictions_as_json = []
        self._nusc_sample_results = defaultdict(list)

    def process(self, inputs, outputs):
        sample_tokens = [x["sample_token"] for x in inputs]
        idx_to_token = get_group_idxs(sample_tokens, NUM_IMAGES_PER_SAMPLE, inverse=True)
        for token in set(sample_tokens):  # samples with no detections still get an entry
            self._nusc_sample_results[token]  # pylint: disable=pointless-statement
        for image_idx, (inp, out) in enumerate(zip(inputs, outputs)):
            inst = out["instances"]
            n = len(inst)
            glob = inst.pred_boxes3d_global.vectorize()
            conv = format_boxes3d(inst.pred_boxes3d.vectorize(), glob[:, :4], inst.pred_speeds)
            classes = inst.pred_classes.cpu().tolist()
            boxes = inst.pred_boxes.tensor.cpu().tolist()
            vec = inst.pred_boxes3d.vectorize().cpu().numpy()
            glob = glob.cpu().tolist()
            scores, scores_3d = inst.scores.cpu().tolist(), inst.scores_3d.cpu().tolist()
            attrs = inst.pred_attributes.cpu().tolist()
            token = idx_to_token[image_idx]
            for i in range(n):
                name = NUSCENES_DETECTION_CATEGORIES[classes[i]]
                self._predictions_as_json.append(OrderedDict(
                    category_id=int(classes[i]), category=name, bbox3d=vec[i].tolist(), bbox=xyxy_to_xywh(boxes[i]), score=float(scores[i]),
                    score_3d=float(scores_3d[i]), file_name=inp["file_name"], image_id=inp["image_id"]))
                self._nusc_sample_results[token].append({
                    "sample_token": token, "rotation": glob[i][:4], "translation": glob[i][4:7], "size": glob[i][7:],
                    "detection_name": name, "detection_score": scores_3d[i], "attribute_name": attribute_name(name, attrs[i]),
                    "velocity": [float(conv[i, 8]), float(conv[i, 9])]
                })

    @staticmethod
    def build_nusc_detection(sample_token, box3d_global, category, score, attribute=None, velocity=None):
        """nuscenes_evaluator.py:231-247."""
        v = box3d_global.vectorize().tolist()[0]
        return {
            "sample_token": sample_token, "rotation": v[:4], "translation": v[4:7], "size": v[7:], "detection_name": category,
            "detection_score": score.item(), "attribute_name": DEFAULT_ATTRIBUTES.get(category, "") if attribute is None else attribute,
            "velocity": [0., .0] if velocity is None else velocity
        }

    def _load_ground_truth(self):
        gt = self._ground_truth
        if isinstance(gt, NuscenesGroundTruth):
            return gt
        if gt is not None:
            return NuscenesGroundTruth.from_json(os.fspath(gt))
        if self._nusc_root is None:
            return None
        try:
            from nuscenes import NuScenes
        except ImportError:
            return None
        nusc = NuScenes(version=DATASET_NAME_TO_VERSION[self._dataset_name], dataroot=self._nusc_root, verbose=True)
        return NuscenesGroundTruth.from_devkit(nusc, DATASET_NAME_TO_EVAL_SET[self._dataset_name])

    def evaluate(self):
        """nuscenes_evaluator.py:249-312.  Writes `output_dir`/bbox3d_predictions.json and nuscenes_submission.json (with the
        reference's meta block) when output_dir is set; the test split then returns {}.  Otherwise returns what the devkit's
        `DetectionMetrics.serialize()` returns minus cfg and eval_time: label_aps, mean_dist_aps, mean_ap, label_tp_errors, tp_errors,
        tp_scores, nd_score.  With distributed=True in a group of more than one process, ranks other than 0 return None."""
        predictions_as_json, nusc_sample_results = self._predictions_as_json, self._nusc_sample_results
        import torch.distributed as dist
        if self._distributed and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dst = [None] * dist.get_world_size() if dist.get_rank() == 0 else None
            dist.gather_object(predictions_as_json, dst, dst=0)
            nusc_sample_results = _gather_dict(dict(nusc_sample_results))
            if dist.get_rank() != 0:
                return None
            predictions_as_json = list(itertools.chain(*dst))
        if self._output_dir is not None:
            os.makedirs(self._output_dir, exist_ok=True)
            with open(os.path.join(self._output_dir, BBOX3D_PREDICTION_FILE), "w") as f:
                json.dump(predictions_as_json, f, indent=4)
            with open(os.path.join(self._output_dir, NUSC_SUBMISSION_FILE), "w") as f:
                json.dump({"meta": EVAL_META, "results": nusc_sample_results}, f, indent=4)
        if self._only_make_submission_file:
            if self._output_dir is None:
                raise NuscenesEvaluationUnavailable(f"NuscenesEvaluator({self._dataset_name!r}): the test split only makes the submission "
                                                    "file, and output_dir is None")
            return {}
        gt = self._load_ground_truth()
        if gt is None:
            raise NuscenesEvaluationUnavailable(f"NuscenesEvaluator({self._dataset_name!r}): no ground truth: pass ground_truth= (a "
                                                "NuscenesGroundTruth or its JSON), or install the nuScenes devkit and set nusc_root")
        return NuscenesDetectionEval(gt).evaluate(nusc_sample_results)
