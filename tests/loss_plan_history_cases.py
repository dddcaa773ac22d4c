"""Batch sequences for the tests that replay ONE LossPlan on differing batches (tests/test_loss_plan_history.py proves on the CPU that
the sequences are what they claim, tests/test_loss_plan_history_gpu.py runs them): every other plan-level test builds a fresh plan and
runs it on one batch, so a value the previous batch left behind in a plan buffer equals the value that should have been written.

A sequence is a list of step labels over a dict of batches; a label that returns is the same batch again.  Every batch's FIRST image
has the canvas' size, so the canvas (and with it the plan) never changes; later images may be smaller -- DD3D.stage_inputs then leaves
the previous batch's pixels in the padding -- and the GT record count shrinks at least once -- LossPlan.stage_gt ships only the prefix
in use.  Where a batch reuses the pinned GT seed of a case of tests/whole_model_grad_oracle.CASES it is that case's batch, unchanged."""
import functools

import torch

from tests import loss_grad_cases as GC
from tests import whole_model_grad_oracle as WO

# compute_losses' flags, shallowest first, with the flag DD3D.get_loss_plan knows the same plan by
LEVELS = [(None, None), ("head_grads", "grads"), ("predictor_grads", "pred_grads"), ("tower_grads", "tower_grads"), ("fpn_grads", "fpn_grads"),
          ("backbone_grads", "backbone_grads"), ("stem_grads", "stem_grads")]
# a VoVNet-V2 model's ladder: the shared levels up to the FPN, then the two flags compute_losses takes from **branch
V99_LEVELS = LEVELS[:5] + [("vovnet_grads", "vovnet_grads"), ("vovnet_stem_grads", "vovnet_stem_grads")]
PLAN_FLAG = dict(LEVELS + V99_LEVELS)

# `case`: the case of WO.CASES whose model, weights, canvas and first batch the sequence uses, or a dict of that form of the sequence's
# own; `deepest`: the flag the references are computed at; `steps`: the labels in order; `batches`: label -> dict(pixels: make_inputs'
# seed, sizes: per-image (h, w) or None for the canvas', gt_seed, n_per_image, empty: images without GT), or "case" for the whole-model
# case's own batch; `extra`: further keywords of compute_losses and get_loss_plan (batch_stats), for the replayed model and the fresh
# references alike.
_V99_B2 = dict(WO.CASES["kitti_v99"], B=2)  # two images on the 128 x 256 canvas: the eSE mean and the ceil_mode pool read the padding
# GT seeds of the V2-99 batches: scanned on the CPU (2100 .. 2105 for A and for B: every pair but (2105, 2101) meets
# the conditions tests/test_loss_plan_history.py asserts; on this canvas positives fall on the three finest levels only)
_V99_B2_BATCHES = {
    "A": dict(pixels=1000, sizes=[None, None], gt_seed=2100, n_per_image=24, empty=()),                              # 24 boxes per image
    "B": dict(pixels=1100, sizes=[None, (101, 189)], gt_seed=2103, n_per_image=24, empty=(1, )),                    # no stride divides 101 x 189
    "C": dict(pixels=1200, sizes=[None, None], gt_seed=2000, n_per_image=0, empty=(0, 1)),                          # num_pos = 0
}
SEQUENCES = {
    "kitti_dla34": dict(
        case="kitti_dla34", deepest="stem_grads", steps=["A", "B", "C", "D", "A"], zero_positives=("C", ), many_positives=("A", "D"),
        batches={
            "A": "case",                                                                                            # seed 2004, 150 positives
            "B": dict(pixels=1100, sizes=[None, (115, 362)], gt_seed=2103, n_per_image=2, empty=(1, )),             # two boxes in image 0
            "C": dict(pixels=1200, sizes=[None, None], gt_seed=2000, n_per_image=0, empty=(0, 1)),                  # num_pos = 0
            "D": dict(pixels=1300, sizes=[None, (96, 200)], gt_seed=2011, n_per_image=24, empty=()),                # boxes in both images
        }),
    "nusc_dla34": dict(
        case="nusc_dla34", deepest="stem_grads", steps=["A", "B", "A"], zero_positives=(), many_positives=("A", ),
        batches={
            "A": "case",                                                                                            # seed 2007, six boxes per image
            "B": dict(pixels=1100, sizes=[None, None, None, (100, 190), None, None], gt_seed=2020, n_per_image=3, empty=(0, 4)),
        }),
    "kitti_v99": dict(
        case="kitti_v99", deepest="fpn_grads", steps=["A", "B", "A"], zero_positives=("B", ), many_positives=("A", ),
        batches={
            "A": "case",                                                                                            # seed 2000
            "B": dict(pixels=1100, sizes=[None], gt_seed=2000, n_per_image=0, empty=(0, )),
        }),
    # the VoVNet backward (OSA, eSE, 3x3 pool, stem_1) with a second image to pad
    "kitti_v99_b2": dict(case=_V99_B2, deepest="vovnet_stem_grads", steps=["A", "B", "C", "A"], zero_positives=("C", ), many_positives=("A", "B"),
                         batches=_V99_B2_BATCHES),
    "kitti_v99_b2_bn": dict(case=_V99_B2, deepest="vovnet_stem_grads", extra=dict(batch_stats=True), steps=["A", "B", "A"], zero_positives=(),
                            many_positives=("A", "B"), batches={k: _V99_B2_BATCHES[k] for k in "AB"}),
}
# batch statistics in the towers sum over the whole padded canvas: the DLA sequences again, batch for batch
SEQUENCES["kitti_dla34_bn"] = dict(SEQUENCES["kitti_dla34"], extra=dict(batch_stats=True))
SEQUENCES["nusc_dla34_bn"] = dict(SEQUENCES["nusc_dla34"], extra=dict(batch_stats=True))
# part 4 (the range guard's retry loop inside compute_losses): dd3d_kitti_dla34 on 1 x 128 x 256 with GT
# GT seed: scanned like the whole-model cases' for a batch without a positive near a non-smooth point of the loss (seeds 2000, 2001 and
# 2004 .. 2006 have one such positive on this canvas, 2002 and 2003 none); tests/test_loss_plan_history.py pins it.
GUARD_CASE = dict(WO.CASES["kitti_dla34"], B=1, H=128, W=256, gt_seed=2002, n_per_image=24, positives=78)
GUARD_NORMS = ("backbone.bottom_up.level3.tree1.tree1.conv1.norm", "backbone.bottom_up.level3.tree1.tree1.conv2.norm")  # as tests/test_full_size_gpu.py
# (largest activation between the two norms, the guard's message, the state a model on the default arithmetic ends in)
GUARD_ROWS = [(6000.0, "half range", dict(math=None, act_scale=4.0)), (40000.0, "half range", dict(math=None, act_scale=1.0)),
              (2.0e5, "half range", dict(math="bf16x3", act_scale=None)), (1e-6, "useful part", dict(math="bf16x3", act_scale=None))]


def case_of(seq):
    case = SEQUENCES[seq]["case"]
    return case if isinstance(case, dict) else WO.CASES[case]


def extra_of(seq):
    return dict(SEQUENCES[seq].get("extra", {}))


def levels_of(seq):
    """The flags of compute_losses a sequence's model takes, shallowest first, down to the sequence's deepest."""
    ladder = [f for f, _ in (LEVELS if WO.is_dla(cpu_model(seq)) else V99_LEVELS)]
    return ladder[:ladder.index(SEQUENCES[seq]["deepest"]) + 1]


def _gt(model, inputs, seed, n_per_image, empty):
    from dd3d_amd.synthetic import make_gt_instances
    return make_gt_instances(inputs, model.num_classes, model.cfg.DD3D.FCOS3D.CANONICAL_BOX3D_SIZES, seed=seed, n_per_image=n_per_image,
                             num_attributes=model.attr_logits.out_channels if hasattr(model, "attr_logits") else None, empty_images=tuple(empty))


def batch(seq, label, model):
    """The batch `label` of sequence `seq` as compute_losses takes it: make_inputs' dicts with `instances`.  `model`: any model of the
    sequence's configuration (class count, canonical sizes, attributes)."""
    case, spec = case_of(seq), SEQUENCES[seq]["batches"][label]
    if spec == "case":
        inputs, gt = WO.case_inputs(case, model)
    else:
        from dd3d_amd.synthetic import make_inputs
        inputs = make_inputs(case["B"], case["H"], case["W"], dataset=case["ds"], seed=spec["pixels"])
        for x, hw in zip(inputs, spec["sizes"]):
            if hw is not None:
                x["image"] = x["image"][:, :hw[0], :hw[1]].contiguous()
                x["height"], x["width"] = hw
        gt = _gt(model, inputs, spec["gt_seed"], spec["n_per_image"], spec["empty"])
    for x, g in zip(inputs, gt):
        x["instances"] = g
    return inputs


def guard_batch(model):
    """Part 4's batch: one 128 x 256 KITTI image with 24 boxes."""
    from dd3d_amd.synthetic import make_inputs
    c = GUARD_CASE
    inputs = make_inputs(c["B"], c["H"], c["W"], dataset=c["ds"])
    for x, g in zip(inputs, _gt(model, inputs, c["gt_seed"], c["n_per_image"], ())):
        x["instances"] = g
    return inputs


@functools.lru_cache(maxsize=None)
def _case_model(exp, weights):
    return WO.case_model(dict(exp=exp, weights=weights, overrides=None))


def cpu_model(seq):
    """The sequence's CPU model with its synthetic weights; sequences of one configuration share it."""
    case = case_of(seq)
    assert case["overrides"] is None
    return _case_model(case["exp"], case["weights"])


def level_hw(model, inputs):
    """The pyramid's (h, w) per level on the batch's canvas, off a dry-run plan."""
    from dd3d_amd.engine.losses import LossPlan
    plan = LossPlan(model, *model.canvas_size(inputs), device="cpu", dry_run=True)
    return [(f.H, f.W) for f in plan.features]


def positives(model, inputs, hw):
    """The float64 oracle's assignment of a batch (tests.loss_oracle through loss_grad_cases.oracle_targets): (boolean [N] over the
    targets in the kernels' order -- level, then image, then location --, positives per level, GT records in the batch)."""
    t = GC.oracle_targets(model, hw, [x["instances"] for x in inputs])
    B = len(inputs)
    pos = torch.zeros(t["labels"].numel(), dtype=torch.bool)
    pos[t["pos_inds"]] = True
    sizes = [B * h * w for h, w in hw]
    return pos, [int(p.sum()) for p in torch.split(pos, sizes)], sum(len(x["instances"].gt_classes) for x in inputs)
