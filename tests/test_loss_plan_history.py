"""The batch sequences of tests/loss_plan_history_cases.py are what they claim, without a GPU: the float64 oracle's assignment
(tests.loss_oracle, as tests/whole_model_grad_oracle.py calls it) of every batch says that a plan replayed over a sequence meets other
pixels, other positives on at least three pyramid levels, locations that turn from positive to negative and back, a batch without any
positive, a shrinking GT record count and images smaller than the canvas -- the conditions under which a value left in a plan buffer
by the previous batch differs from the value the current batch should have written there."""
import functools

import pytest
import torch

from tests import loss_grad_oracle as GO
from tests import loss_plan_history_cases as HC
from tests import whole_model_grad_oracle as WO


@functools.lru_cache(maxsize=None)
def _sequence(seq):
    """Per distinct label of a sequence: (batch, canvas, positive mask, positives per level, GT records)."""
    model = HC.cpu_model(seq)
    out, hw = {}, None
    for label in dict.fromkeys(HC.SEQUENCES[seq]["steps"]):
        b = HC.batch(seq, label, model)
        hw = hw or HC.level_hw(model, b)
        out[label] = (b, model.canvas_size(b)) + HC.positives(model, b, hw)
    return out


@pytest.mark.parametrize("seq", list(HC.SEQUENCES))
def test_consecutive_batches_differ_where_a_replayed_plan_could_keep_something(seq):
    spec, got = HC.SEQUENCES[seq], _sequence(seq)
    steps = spec["steps"]
    assert steps[0] == steps[-1] and len(set(steps)) >= 2  # the sequence returns to its first batch
    shrinks = smaller = 0
    for a, b in zip(steps, steps[1:]):
        (xa, _, pa, la, na), (xb, _, pb, lb, nb) = got[a], got[b]
        for ia, ib in zip(xa, xb):  # other pixels in every image (on the common corner, where the sizes differ)
            h, w = min(ia["image"].shape[1], ib["image"].shape[1]), min(ia["image"].shape[2], ib["image"].shape[2])
            assert float((ia["image"][:, :h, :w] != ib["image"][:, :h, :w]).float().mean()) > 0.9, (seq, a, b)
        differ = sum(1 for u, v in zip(la, lb) if u != v)
        print(f"[loss_plan_history] {seq} {a} -> {b}: positives per level {la} -> {lb}, GT records {na} -> {nb}, "
              f"{int((pa & ~pb).sum())} locations turn negative, {int((~pa & pb).sum())} positive")
        assert differ >= 3, (seq, a, b, la, lb)
        # a batch with positives loses some of them to the next batch, and a batch with positives gains some over the one before (a step
        # into or out of the batch without positives can only go one way)
        assert bool((pa & ~pb).any()) == bool(pa.any()) and bool((~pa & pb).any()) == bool(pb.any()), (seq, a, b)
        shrinks += nb < na
    for label, (x, canvas, pos, _, _) in got.items():
        n = int(pos.sum())
        assert (n == 0) == (label in spec["zero_positives"]), (seq, label, n)
        assert n >= 50 or label not in spec["many_positives"], (seq, label, n)
        case = HC.case_of(seq)
        assert canvas == got[steps[0]][1] and canvas[0] == case["B"] and canvas[1] >= case["H"] and canvas[2] >= case["W"]  # one canvas: one plan
        assert tuple(x[0]["image"].shape[1:]) == (case["H"], case["W"])  # the first image spans it
        smaller += any(tuple(i["image"].shape[1:]) != (case["H"], case["W"]) for i in x)
    assert shrinks >= 1  # stage_gt ships a shorter prefix over a longer one's records
    assert smaller >= 1 or seq == "kitti_v99"  # stage_inputs leaves old pixels in the padding (one image per batch: nothing to pad)


@pytest.mark.parametrize("seq", [s for s, v in HC.SEQUENCES.items() if "case" in v["batches"].values()])
def test_a_reused_pinned_seed_is_the_whole_model_cases_batch_unchanged(seq):
    case, model = HC.case_of(seq), HC.cpu_model(seq)
    inputs, gt = WO.case_inputs(case, model)
    x, _, pos, _, _ = _sequence(seq)["A"]
    assert int(pos.sum()) == case["positives"]
    for a, b, g in zip(x, inputs, gt):
        assert torch.equal(a["image"], b["image"]) and torch.equal(a["intrinsics"], b["intrinsics"])
        i = a["instances"]
        assert torch.equal(i.gt_boxes.tensor, g.gt_boxes.tensor) and torch.equal(i.gt_classes, g.gt_classes)
        for f in ("quat", "proj_ctr", "depth", "size"):
            assert torch.equal(getattr(i.gt_boxes3d, f), getattr(g.gt_boxes3d, f))
    for label, spec in HC.SEQUENCES[seq]["batches"].items():  # no other batch carries the pinned seed with the case's box count
        assert spec == "case" or (spec["gt_seed"], spec["n_per_image"]) != (case["gt_seed"], case["n_per_image"]), label


def test_the_guard_case_has_positives_and_none_on_a_kink():
    """Part 4's batch (1 x 128 x 256): at least 50 positives; the pinned seed leaves no positive within the kink margin on the float64
    oracle's head maps of the unscaled weights (scaled_between leaves the network function as it is; the GPU test asserts the same on the
    scaled weights it compares)."""
    c = HC.GUARD_CASE
    model = WO.case_model(c)
    b = HC.guard_batch(model)
    assert model.canvas_size(b) == (1, 128, 256)
    ex = {}
    WO.whole_model_grads(model, model.cfg, b, [x["instances"] for x in b], torch.float64, extras=ex, backward=False)
    assert ex["targets"]["pos_inds"].numel() == c["positives"] >= 50
    assert int(GO.near_kink(ex["maps"], ex["targets"], ex["inv_K"], ex["p"]).sum()) == 0
    sd = model.state_dict()
    assert all(n + ".running_var" in sd for n in HC.GUARD_NORMS)
    assert [r[2] for r in HC.GUARD_ROWS] == [dict(math=None, act_scale=4.0), dict(math=None, act_scale=1.0)] + [dict(math="bf16x3", act_scale=None)] * 2


def test_levels_name_every_flag_of_compute_losses_in_order():
    import inspect
    from dd3d_amd.modeling.dd3d import DD3D
    flags = [k for k in inspect.signature(DD3D.compute_losses).parameters if k.endswith("_grads")]
    assert flags == [f for f, _ in HC.LEVELS[1:]]
    known = set(inspect.signature(DD3D.get_loss_plan).parameters)
    assert all(p in known for _, p in HC.LEVELS[1:])
    # the V2-99 ladder: the shared levels up to the FPN, then the two flags compute_losses takes from **branch
    assert HC.V99_LEVELS[:5] == HC.LEVELS[:5] and [f for f, _ in HC.V99_LEVELS[5:]] == ["vovnet_grads", "vovnet_stem_grads"]
    assert "vovnet_grads" in known and "vovnet_stem_grads" in known and "batch_stats" in known
    assert all(HC.PLAN_FLAG[f] == p for f, p in HC.LEVELS + HC.V99_LEVELS)


def test_the_new_sequences_are_what_the_gpu_tests_take_them_for():
    """The batch-statistics sequences are the DLA sequences batch for batch; the two-image V2-99 sequences share their batches, have GT
    in both images of A and in image 0 of B alone, and their smaller image is no multiple of any stride."""
    S = HC.SEQUENCES
    for seq in ("kitti_dla34", "nusc_dla34"):
        twin = S[seq + "_bn"]
        assert twin["extra"] == dict(batch_stats=True) and "extra" not in S[seq]
        assert all(twin[k] is S[seq][k] for k in ("case", "deepest", "steps", "batches"))
    a, b = S["kitti_v99_b2"], S["kitti_v99_b2_bn"]
    assert b["extra"] == dict(batch_stats=True) and "extra" not in a and all(b["batches"][k] is a["batches"][k] for k in b["batches"])
    assert a["steps"] == ["A", "B", "C", "A"] and b["steps"] == ["A", "B", "A"] and a["deepest"] == b["deepest"] == "vovnet_stem_grads"
    case = HC.case_of("kitti_v99_b2")
    assert (case["exp"], case["B"], case["H"], case["W"]) == ("dd3d_kitti_v99", 2, 128, 256)
    model = HC.cpu_model("kitti_v99_b2")
    counts = {k: [len(x["instances"].gt_classes) for x in HC.batch("kitti_v99_b2", k, model)] for k in "ABC"}
    assert counts == {"A": [24, 24], "B": [24, 0], "C": [0, 0]}
    h, w = a["batches"]["B"]["sizes"][1]
    strides = [s.stride for s in model.backbone_output_shape]
    assert all(h % s and w % s for s in [2] + strides) and h < case["H"] and w < case["W"]
    assert HC.levels_of("kitti_v99_b2") == [f for f, _ in HC.V99_LEVELS] and HC.levels_of("kitti_dla34_bn") == [f for f, _ in HC.LEVELS]
    for seq in ("kitti_dla34_bn", "nusc_dla34_bn", "kitti_v99_b2_bn"):  # the plan will have batch-statistics layers to run
        from tests import tower_bn_oracle as TB
        assert len(TB.bn_prefixes(HC.cpu_model(seq))) > 0
