"""Evaluator-side overlap kernels: the oracle vs the golden vectors produced by the reference's own functions."""
import os

import numpy as np
import pytest

from oracle import rotate_iou_oracle as R

G = np.load(os.path.join(os.path.dirname(__file__), "golden", "rotate_iou.npz"))


@pytest.mark.parametrize("crit", [-1, 0, 1, 2])
def test_rotate_iou_oracle_matches_reference(crit):
    got = R.rotate_iou_eval(G["boxes"], G["qboxes"], crit)
    ref = G[f"riou_{crit}"]
    assert (got > 0).sum() == (ref > 0).sum() > 150
    assert np.allclose(got, ref, rtol=2e-5, atol=2e-6)
    if crit == -1:  # known answers: identical boxes, contained box, edge-touching boxes, far apart
        assert abs(ref[0, 0] - 1.0) < 1e-5 and abs(ref[1, 2] - 1.0 / 16.0) < 1e-5 and ref[2, 3] < 1e-4 and ref[0, 4] == 0.0


@pytest.mark.parametrize("crit,cam", [(-1, True), (-1, False), (0, True), (1, False)])
def test_d3_overlap_oracle_matches_reference(crit, cam):
    got = R.d3_box_overlap(G["boxes3d"], G["qboxes3d"], G["riou_2"], crit, cam)
    assert np.allclose(got, G[f"d3_{crit}_{int(cam)}"], rtol=2e-5, atol=2e-6)


@pytest.mark.parametrize("crit", [-1, 0, 1])
def test_image_overlap_oracle_matches_reference(crit):
    assert np.allclose(R.image_box_overlap(G["iboxes"], G["iqboxes"], crit), G[f"image_{crit}"], rtol=1e-6, atol=1e-7)


# ---- the oracle against a float64 statement of the geometry, family by family (tests/eval_overlap_cases.py) -------------------------
from tests import eval_overlap_cases as C  # noqa: E402


@pytest.mark.parametrize("family", C.STABLE_FAMILIES)
def test_family_is_stable_and_oracle_is_within_its_measured_bound(family):
    """At most 1 % of a stable-by-construction family may fail `stable()` (a family that exceeds it gets another generator, not
    another cap), and on the stable pairs the oracle is within the committed E_FAMILY of the float64 truth, times 1.25 for a
    different libm."""
    m = C.measured(family)
    s = m["stable"]
    e_int, e_iou = m["e_int"][s].max(), m["e_iou"][s].max()
    print(f"{family}: unstable {int((~s).sum())} / {len(s)}, e_int {e_int:.3e}, e_iou {e_iou:.3e}, E_FAMILY {C.E_FAMILY[family]:.3e}")
    assert (~s).sum() <= C.MAX_UNSTABLE_SHARE * len(s)
    assert e_int <= 1.25 * C.E_FAMILY[family] and e_iou <= 1.25 * C.E_FAMILY[family]
    assert (m["truth"][s] > 0).mean() > 0.75 or family.endswith("yaw0")  # the pairs do overlap (touching ones: exactly 0)


@pytest.mark.parametrize("family", C.ZERO_FAMILIES)
def test_disjoint_and_dontcare_pairs_are_exactly_zero(family):
    m = C.measured(family)
    assert m["stable"].all() and not m["oracle"].any() and not m["truth"].any()
    b, q = C.pairs(family)
    for crit in (-1, 0, 1, 2):
        out = R.rotate_iou_eval(b[:20], q[:20], crit)
        assert not out.any() and np.isfinite(out).all()


@pytest.mark.parametrize("family", C.D3_FAMILIES)
def test_d3_oracle_is_within_its_measured_bound(family):
    for camera in (True, False):
        e = C.measured_3d(family, camera)
        print(f"{family} camera={camera}: e_3d {e:.3e}, E_3D {C.E_3D[family]:.3e}")
        assert e <= 1.25 * C.E_3D[family]


def test_unstable_families_are_what_the_documents_say_and_math_is_restored():
    """Nothing is asserted about values in the ill-conditioned regime (nearly parallel, nearly coincident edges): only that the
    committed generators do reach it, so that the GPU test of that regime and the figures in DESIGN.md mean something."""
    import math
    for family in C.UNSTABLE_FAMILIES:
        m = C.measured(family)
        print(f"{family}: unstable {int((~m['stable']).sum())} / {len(m['stable'])}, recorded {C.UNSTABLE_MEASURED[family]}")
        assert (~m["stable"]).sum() > C.MAX_UNSTABLE_SHARE * len(m["stable"])
    assert R.math is math
    with pytest.raises(ZeroDivisionError):
        with C.perturbed_trig(1, 1):
            assert R.math is not math
            1 / 0
    assert R.math is math


def test_truth_adapter_turns_the_right_way():
    """bev_iou64 takes degrees, counter-clockwise: a 4 x 1 box at yaw +0.3 (clockwise) and the same box at -0.3 differ, and the
    adapter pairs each with the oracle's reading of the same numbers."""
    b = np.array([0, 0, 4, 1, 0.3], dtype=np.float32)
    for yaw in (0.3, -0.3, 1.2):
        q = np.array([0.5, 0.2, 3, 1, yaw], dtype=np.float32)
        assert abs(float(R.intersection_area(q, b)) - C.truth_intersection(b, q)) < 1e-5
    assert abs(C.truth_intersection(b, np.array([0, 0, 4, 1, -0.3], dtype=np.float32)) - 4.0) > 0.5
