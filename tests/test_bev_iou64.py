"""The float64 rotated-IoU helper of the BEV NMS tests (tests/bev_iou64.py) against the oracle's restatement of detectron2's
box_iou_rotated, on random boxes that are not degenerate, plus closed-form cases."""
import math

import numpy as np

from oracle import nuscenes_oracle as N
from tests import bev_iou64


def test_matches_the_oracle_on_random_boxes():
    rng = np.random.default_rng(0)
    worst = 0.0
    for _ in range(2000):
        b1 = [rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(0.5, 6), rng.uniform(0.5, 6), rng.uniform(-180, 180)]
        b2 = [b1[0] + rng.normal(0, 2), b1[1] + rng.normal(0, 2), rng.uniform(0.5, 6), rng.uniform(0.5, 6), rng.uniform(-180, 180)]
        b1, b2 = np.float32(b1).astype(np.float64), np.float32(b2).astype(np.float64)
        worst = max(worst, abs(bev_iou64.iou(b1, b2) - N.box_iou_rotated_single(b1, b2)))
    assert worst < 2e-5, worst  # the oracle rounds its centres and trig to float32, as detectron2 does


def test_closed_form_cases():
    assert abs(bev_iou64.iou((0, 0, 2, 1, 30), (0, 0, 2, 1, 30)) - 1.0) < 1e-12  # identical
    assert abs(bev_iou64.iou((0, 0, 2, 2, 0), (0, 0, 2, 2, 90)) - 1.0) < 1e-12  # a square rotated by 90 degrees
    assert abs(bev_iou64.iou((0, 0, 2, 2, 0), (1, 0, 2, 2, 0)) - 1.0 / 3.0) < 1e-12  # half overlap: 2 / (4 + 4 - 2)
    assert bev_iou64.iou((0, 0, 2, 2, 0), (2, 0, 2, 2, 0)) == 0.0  # shared edge
    assert abs(bev_iou64.iou((0, 0, 4, 4, 0), (0, 0, 2, 2, 17)) - 0.25) < 1e-12  # containment
    # two unit squares crossed at 45 degrees: a regular octagon of area 2 (sqrt 2 - 1)
    oct_area = 2.0 * (math.sqrt(2.0) - 1.0)
    assert abs(bev_iou64.iou((0, 0, 1, 1, 0), (0, 0, 1, 1, 45)) - oct_area / (2 - oct_area)) < 1e-12
    assert bev_iou64.iou((0, 0, 0, 2, 0), (0, 0, 2, 2, 0)) == 0.0  # zero area
