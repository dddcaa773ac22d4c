"""ONE LossPlan replayed on differing batches, on the MI355X (the sequences: tests/loss_plan_history_cases.py; what they exercise:
tests/test_loss_plan_history.py).  Every other plan-level test builds a fresh plan and runs it on one batch; a training loop replays one
captured plan on other images and other GT every step.  The reference of a batch is a FRESH model on that batch alone -- a new DD3D with
the same state dict, arithmetic and plane scale, hence a new plan with newly allocated, zero-filled buffers -- and the bar is bit
equality everywhere: the kernels promise a fixed summation order and no float atomics.

  1. sequences on one plan, at every flag level and on the other arithmetics: DLA-34 on KITTI and nuScenes, on running statistics and with
     batch_stats (tower_batch_stats() after every step, the model's own buffers at the end), V2-99 on one image down to the FPN and on
     two images down to stem_1, with and without batch_stats;
  2. other plans of the same model (inference on two canvases, a shallower loss plan, the running-statistics twin of a batch-statistics
     plan) in between, with and without an eviction;
  3. every floating-point tensor the backward's ops write -- under batch_stats also the statistics tensors and the scratch rows the
     forward's reduction shares with the norm's backward -- overwritten with the seam tests' sentinel between two runs;
  4. the range guard's retry loop inside compute_losses, and plane scale 4 -- which only the guard reaches -- against the whole-model
     oracle of tests/test_whole_model_grads_gpu.py.
"""
import fnmatch
import functools
import warnings

import pytest
import torch

from tests import loss_grad_cases as GC
from tests import loss_plan_history_cases as HC
from tests.util import scaled_between

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0  # the seam tests' (tests/test_predictor_grads_gpu.py, test_backbone_grads_gpu.py, test_stem_grads_gpu.py)
_REFS, _REF_STATS = {}, {}


@pytest.fixture(autouse=True)
def _default_arithmetic(monkeypatch):
    monkeypatch.delenv("DD3D_MATH", raising=False)
    monkeypatch.delenv("DD3D_F16_ACT_SCALE", raising=False)


def _fresh(seq, math=None, act_scale=None, use_graph=True, sd=None):
    """A new model of the sequence's configuration on the GPU: nothing of it has run yet."""
    case = HC.case_of(seq)
    m = GC.cpu_model(case["exp"], case["overrides"])
    m.load_state_dict(sd if sd is not None else HC.cpu_model(seq).state_dict())
    m = m.to("cuda").eval()
    m.math, m.act_scale, m.use_graph = math, act_scale, use_graph
    return m


@functools.lru_cache(maxsize=None)
def _batch(seq, label):
    return HC.batch(seq, label, HC.cpu_model(seq))


def _split(res):
    """compute_losses' three result forms as (losses, grads, param_grads)."""
    if isinstance(res, dict):
        return res, {}, {}
    return (res[0], res[1], {}) if len(res) == 2 else tuple(res)


def _reference(seq, label, math=None, act_scale=None):
    """(losses, grads, param_grads) of a fresh model on batch `label` alone at the sequence's deepest flag and with its `extra`, once per
    configuration; with batch_stats the fresh plan's tower_batch_stats() is kept beside them (_reference_stats)."""
    key = (seq, label, math, act_scale)
    if key not in _REFS:
        model = _fresh(seq, math, act_scale)
        extra = HC.extra_of(seq)
        _REFS[key] = _split(model.compute_losses(_batch(seq, label), **{HC.SEQUENCES[seq]["deepest"]: True}, **extra))
        if extra.get("batch_stats"):
            _REF_STATS[key] = _plan(model, seq, HC.SEQUENCES[seq]["deepest"]).tower_batch_stats()
        torch.cuda.synchronize()
        del model
    return _REFS[key]


def _reference_stats(seq, label, math=None, act_scale=None):
    _reference(seq, label, math, act_scale)
    return _REF_STATS[(seq, label, math, act_scale)]


def _assert_stats_are(plan, seq, label, what, math=None, act_scale=None):
    """plan.tower_batch_stats() after a step against the fresh plan's: every key of tower_bn_oracle.batch_stats_names, bit for bit."""
    from tests import tower_bn_oracle as TB
    got, want = plan.tower_batch_stats(), _reference_stats(seq, label, math, act_scale)
    assert sorted(got) == sorted(want) == TB.batch_stats_names(HC.cpu_model(seq)) and len(got) > 0, (what, len(got), len(want))
    bad = [(k, float((got[k].double() - want[k].double()).abs().max())) for k in got if not torch.equal(got[k], want[k])]
    assert not bad, (what, f"{len(bad)} of {len(got)} statistics differ", " ".join(f"{k}:{d:.1e}" for k, d in bad[:24]))


def _assert_buffers_kept(model, seq, what):
    """The docstring of compute_losses: the model's own running statistics are never written."""
    sd, loaded = model.state_dict(), HC.cpu_model(seq).state_dict()
    keys = [k for k in sd if k.endswith("running_mean") or k.endswith("running_var")]
    assert keys and all(torch.equal(sd[k].cpu(), loaded[k]) for k in keys), what


def _assert_is(res, ref, what):
    """Everything `res` holds equals the reference bit for bit; the loss dict has the reference's keys in its order."""
    for part, got, want in zip(("losses", "grads", "param_grads"), _split(res), ref):
        if part == "losses":
            assert list(got) == list(want), (what, list(got), list(want))
        missing = [k for k in got if k not in want]
        assert not missing, (what, part, missing)
        bad = [(k, float((got[k].double() - want[k].double()).abs().max())) for k in got if not torch.equal(got[k], want[k])]
        assert not bad, (what, part, f"{len(bad)} of {len(got)} entries differ", " ".join(f"{k}:{d:.1e}" for k, d in bad[:48]))


def _flags(level, seq=None):
    return dict({level: True} if level else {}, **(HC.extra_of(seq) if seq else {}))


def _plan(model, seq, level):
    return model.get_loss_plan(*model.canvas_size(_batch(seq, HC.SEQUENCES[seq]["steps"][0])), **({HC.PLAN_FLAG[level]: True} if level else {}),
                               **HC.extra_of(seq))


def _run_sequence(seq, level, math=None, act_scale=None, use_graph=True):
    spec = HC.SEQUENCES[seq]
    model = _fresh(seq, math, act_scale, use_graph)
    plan = _plan(model, seq, level)  # built here; every step below must find it
    first, bs = None, bool(HC.extra_of(seq).get("batch_stats"))
    assert plan.batch_stats == bs and bool(plan.tower_bn) == bs
    for i, label in enumerate(spec["steps"]):
        res = model.compute_losses(_batch(seq, label), **_flags(level, seq))
        assert (isinstance(res, dict) if level is None else len(res) == (2 if level == "head_grads" else 3)), (seq, level, type(res))
        _assert_is(res, _reference(seq, label, math, act_scale), (seq, level, i, label))
        if level == spec["deepest"]:
            assert all(set(a) == set(b) for a, b in zip(_split(res), _reference(seq, label, math, act_scale)))
        first = first or res
        assert _plan(model, seq, level) is plan and len(model._plans) == 1, (seq, level, i)  # one plan throughout, no rebuild
        if bs:
            _assert_stats_are(plan, seq, label, (seq, level, i, label), math, act_scale)
    # what the first step returned was never cloned here: the values are copies, not views of plan buffers four batches later
    _assert_is(first, _reference(seq, spec["steps"][0], math, act_scale), (seq, level, "the first step's tensors after the last step"))
    if bs:
        _assert_buffers_kept(model, seq, (seq, level))
    return plan


# ---------------------------------------------------------------------------------------------------------- 1. sequences on one plan
def test_fresh_references_of_the_kitti_sequence(hiplib):
    """The references themselves (computed here, cached for the module): the deepest level returns every named parameter; the batch
    without positives has the other key order and exact zeros as regression gradients; the batches differ."""
    from dd3d_amd.engine.losses import LOSS_KEYS_2D, LOSS_KEYS_3D, LOSS_KEYS_3D_EMPTY
    refs = {label: _reference("kitti_dla34", label) for label in "ABCD"}
    named = dict(HC.cpu_model("kitti_dla34").named_parameters())
    for label, (losses, grads, params) in refs.items():
        assert sorted(params) == sorted(named) and all(params[k].shape == named[k].shape for k in named)
        assert list(losses) == list(LOSS_KEYS_2D) + list(LOSS_KEYS_3D_EMPTY if label == "C" else LOSS_KEYS_3D)
        assert all(bool(torch.isfinite(v).all()) for d in (losses, grads, params) for v in d.values())
    _, gC, pC = refs["C"]
    for k, v in gC.items():
        if k.rstrip("0123456789") in ("box2d_reg", "quat", "ctr", "depth", "size"):
            assert not bool(v.any()), k
    assert any(bool(v.any()) for k, v in gC.items() if k.startswith("logits")) and bool(pC["backbone.bottom_up.base_layer.weight"].any())
    for a, b in ("AB", "BC", "CD", "DA"):
        assert not torch.equal(refs[a][2]["backbone.bottom_up.base_layer.weight"], refs[b][2]["backbone.bottom_up.base_layer.weight"])


@pytest.mark.parametrize("level", [f for f, _ in HC.LEVELS], ids=lambda f: f or "losses")
def test_kitti_sequence_on_one_plan_at_every_flag_level(hiplib, level):
    _run_sequence("kitti_dla34", level)


@pytest.mark.parametrize("how", ["bf16x3", "plane_scale_1", "launch_by_launch"])
def test_kitti_sequence_on_one_plan_other_arithmetics_and_no_graph(hiplib, how):
    """bf16x3: the launch-by-launch stem reads its own f32 buffers, not the KEEP launch's; plane scale 1; no captured graph."""
    from dd3d_amd import hip
    kw = dict(bf16x3=dict(math="bf16x3"), plane_scale_1=dict(act_scale=1.0), launch_by_launch=dict(use_graph=False))[how]
    plan = _run_sequence("kitti_dla34", "stem_grads", **kw)
    buf = plan.bufs["level5.cat"]
    if how == "bf16x3":
        assert plan.math == hip.MATH_BF16X3 and buf.np == 3 and not buf.f16
    else:
        assert buf.f16 and buf.plane_scale == (1.0 if how == "plane_scale_1" else 16.0)
    assert (plan.graph is None) == (how == "launch_by_launch")


def test_forty_replays_of_the_deepest_plan_keep_their_bits(hiplib):
    """What this file found: DD3D.compute_losses' plan cleared the renormalisation trigger word of the allocentric decode with a
    hipMemsetAsync captured into the graph; replayed a dozen times, the memset node of the stem_grads graph wrote 0x20202020 or
    0xF0F0F0F0 instead of 0 for thirteen replays at a time, every positive then took the renormalised decode and the 3D gradients moved
    by a few ulps.  A kernel clears the word now.  Forty replays span three of those periods."""
    seq = "kitti_dla34"
    model = _fresh(seq)
    ref = _reference(seq, "A")
    for i in range(40):
        losses, grads, _ = model.compute_losses(_batch(seq, "A"), stem_grads=True)
        plan = _plan(model, seq, "stem_grads")
        assert int(plan.targets.flags[0]) == 0, (i, hex(int(plan.targets.flags[0]) & 0xFFFFFFFF))
        _assert_is((losses, grads), ref, (seq, "replay", i))


def test_nuscenes_sequence_on_one_plan(hiplib):
    plan = _run_sequence("nusc_dla34", "stem_grads")
    assert plan.nusc and plan.B == 6


def test_v99_sequence_on_one_plan(hiplib):
    _run_sequence("kitti_v99", "fpn_grads")


@pytest.mark.parametrize("level", [f for f, _ in HC.V99_LEVELS], ids=lambda f: f or "losses")
def test_two_image_v99_sequence_on_one_plan_at_every_flag_level(hiplib, level):
    """V2-99 with a second image to pad (A, B, C, A; B's second image is 101 x 189, C has no GT): the eSE gate's per-image mean and the
    ceil_mode pool read every pixel of the padded canvas, the VoVNet backward reads what they stored."""
    plan = _run_sequence("kitti_v99_b2", level)
    assert plan.B == 2 and (plan.Hp, plan.Wp) == (128, 256) and level in HC.levels_of("kitti_v99_b2")
    assert hasattr(plan, "vovnet_layers") == (level in ("vovnet_grads", "vovnet_stem_grads"))
    assert hasattr(plan, "vovnet_stem_layers") == (level == "vovnet_stem_grads")


@pytest.mark.parametrize("how", ["bf16x3", "launch_by_launch"])
def test_two_image_v99_sequence_on_one_plan_other_arithmetic_and_no_graph(hiplib, how):
    from dd3d_amd import hip
    kw = dict(bf16x3=dict(math="bf16x3"), launch_by_launch=dict(use_graph=False))[how]
    plan = _run_sequence("kitti_v99_b2", "vovnet_stem_grads", **kw)
    assert (plan.math == hip.MATH_BF16X3) == (how == "bf16x3") and (plan.graph is None) == (how == "launch_by_launch")


@pytest.mark.parametrize("level", ["tower_grads", "fpn_grads", "stem_grads"])
def test_kitti_batch_statistics_sequence_on_one_plan(hiplib, level):
    """kitti_dla34's five steps with the towers' BatchNorm on the batch's statistics: they sum over the whole padded canvas, so a stale
    pixel in the padding of B and D or a stale row of the shared scratch moves every tower output.  tower_batch_stats() is compared
    after every step, the model's own running statistics after the last."""
    plan = _run_sequence("kitti_dla34_bn", level)
    assert len(plan.tower_bn) == 8 and plan.bn_part is not None


@pytest.mark.parametrize("how", ["bf16x3", "plane_scale_1", "launch_by_launch"])
def test_kitti_batch_statistics_sequence_on_one_plan_other_arithmetics_and_no_graph(hiplib, how):
    from dd3d_amd import hip
    kw = dict(bf16x3=dict(math="bf16x3"), plane_scale_1=dict(act_scale=1.0), launch_by_launch=dict(use_graph=False))[how]
    plan = _run_sequence("kitti_dla34_bn", "stem_grads", **kw)
    buf = plan.bufs["level5.cat"]
    if how == "bf16x3":
        assert plan.math == hip.MATH_BF16X3 and buf.np == 3 and not buf.f16
    else:
        assert buf.f16 and buf.plane_scale == (1.0 if how == "plane_scale_1" else 16.0)
    assert (plan.graph is None) == (how == "launch_by_launch")


def test_nuscenes_batch_statistics_sequence_on_one_plan(hiplib):
    plan = _run_sequence("nusc_dla34_bn", "stem_grads")
    assert plan.nusc and plan.B == 6 and plan.batch_stats


def test_two_image_v99_batch_statistics_sequence_on_one_plan(hiplib):
    plan = _run_sequence("kitti_v99_b2_bn", "vovnet_stem_grads")
    assert plan.batch_stats and plan.with_vovnet_stem_grads and plan.B == 2


def test_forty_replays_of_the_v99_batch_statistics_plan_keep_their_bits(hiplib):
    """The forty-replay test's argument on a graph several times longer: the V2-99 backward down to stem_1 behind batch-statistics
    towers.  Every replay equals the fresh reference, the statistics included, and the renormalisation trigger word stays 0."""
    seq = "kitti_v99_b2_bn"
    model = _fresh(seq)
    ref = _reference(seq, "A")
    for i in range(40):
        res = model.compute_losses(_batch(seq, "A"), vovnet_stem_grads=True, batch_stats=True)
        plan = _plan(model, seq, "vovnet_stem_grads")
        assert int(plan.targets.flags[0]) == 0, (i, hex(int(plan.targets.flags[0]) & 0xFFFFFFFF))
        _assert_is(res, ref, (seq, "replay", i))
        _assert_stats_are(plan, seq, "A", (seq, "replay", i))
    assert len(model._plans) == 1
    _assert_buffers_kept(model, seq, seq)


# ------------------------------------------------------------------------------------------------------ 2. other plans in between
@pytest.mark.parametrize("max_cached_plans", [None, 2], ids=["cached", "evicted"])
def test_other_plans_of_the_model_run_in_between(hiplib, max_cached_plans):
    """A, B, A at stem_grads; between the steps an inference on the same canvas, an inference on a 128 x 256 canvas and a compute_losses
    at predictor_grads.  All plans share the model's weight store.  With a cache of two plans the stem_grads plan is evicted and
    rebuilt in mid-sequence."""
    from dd3d_amd.synthetic import make_inputs
    seq = "kitti_dla34"
    model = _fresh(seq)
    if max_cached_plans is not None:
        model.max_cached_plans = max_cached_plans
    other = make_inputs(1, 128, 256, seed=1400)
    plans = []
    for i, label in enumerate(["A", "B", "A"]):
        res = model.compute_losses(_batch(seq, label), stem_grads=True)
        _assert_is(res, _reference(seq, label), (seq, max_cached_plans, i, label))
        plans.append(_plan(model, seq, "stem_grads"))  # (a cache hit: the plan that just ran)
        if i < 2:
            assert len(model(_batch(seq, label))) == 2
            assert len(model(other)) == 1
            res = model.compute_losses(_batch(seq, "D"), predictor_grads=True)
            _assert_is(res, _reference(seq, "D"), (seq, max_cached_plans, i, "D at predictor_grads"))
    if max_cached_plans is None:
        assert plans[1] is plans[0] and plans[2] is plans[0] and len(model._plans) == 4
    else:
        assert plans[1] is not plans[0] and plans[2] is not plans[1] and len(model._plans) == 2  # rebuilt: new buffers, the same bits


def _detections(out):
    """An inference result as plain CPU tensors per image."""
    rows = []
    for o in out:
        i = o["instances"]
        rows.append([t.detach().cpu().clone() for t in (i.pred_boxes.tensor, i.scores, i.scores_3d, i.pred_classes, i.pred_boxes3d.vectorize())])
    return rows


def _inference_reference(seq, label):
    key = (seq, label, "inference")
    if key not in _REFS:
        model = _fresh(seq)
        _REFS[key] = _detections(model(_batch(seq, label)))
        torch.cuda.synchronize()
        del model
    return _REFS[key]


@pytest.mark.parametrize("max_cached_plans", [None, 2], ids=["cached", "evicted"])
def test_batch_and_running_statistics_forwards_share_one_weight_store(hiplib, max_cached_plans):
    """A, B, A on ONE model: compute_losses(stem_grads, batch_stats), compute_losses(stem_grads) on the running statistics, an inference.
    The batch-statistics towers run the model's packed filters through a raw epilogue with scale ones, the other two through the
    folded norm; the `descaled` vectors and the term planes live in the model's shared weight store.  Each result equals its own
    fresh reference.  With a cache of two plans each of the three is rebuilt in every round: new buffers, the same bits."""
    seq, bn = "kitti_dla34", "kitti_dla34_bn"
    model = _fresh(seq)
    if max_cached_plans is not None:
        model.max_cached_plans = max_cached_plans
    plans = []
    for i, label in enumerate(["A", "B", "A"]):
        res = model.compute_losses(_batch(seq, label), stem_grads=True, batch_stats=True)
        _assert_is(res, _reference(bn, label), (bn, max_cached_plans, i, label))
        plan = _plan(model, bn, "stem_grads")  # (a cache hit: the plan that just ran)
        _assert_stats_are(plan, bn, label, (bn, max_cached_plans, i, label))
        res = model.compute_losses(_batch(seq, label), stem_grads=True)
        _assert_is(res, _reference(seq, label), (seq, max_cached_plans, i, label))
        other = _plan(model, seq, "stem_grads")
        assert other is not plan and not other.batch_stats and plan.batch_stats
        got, want = _detections(model(_batch(seq, label))), _inference_reference(seq, label)
        assert len(got) == len(want) == 2 and all(len(g[1]) > 0 for g in want)
        assert all(torch.equal(a, b) for g, w in zip(got, want) for a, b in zip(g, w)), (seq, max_cached_plans, i, label, "inference")
        plans.append((plan, other))
    if max_cached_plans is None:
        assert all(p is plans[0][0] and o is plans[0][1] for p, o in plans) and len(model._plans) == 3
    else:
        assert plans[1][0] is not plans[0][0] and plans[2][0] is not plans[1][0] and plans[1][1] is not plans[0][1] and len(model._plans) == 2
    _assert_buffers_kept(model, bn, (bn, max_cached_plans))


# ------------------------------------------------------------------------------------------------------------ 3. poisoned outputs
# Floating-point tensors on the backward side that NO kernel writes: build-time constants the ops only read.  Nothing here may be
# written by any op; the test asserts that a run leaves every one of them unchanged.  (name pattern, reason)
EXCLUDED = [
    ("upstream", "the vector of ones dd3d_loss_backward reads as the gradient of the sum of the loss dict; filled once when the plan is built"),
    ("fpn_layers.*.g[*]", "the zero gradient standing in for an FPN output that DD3D.IN_FEATURES does not select: torch.zeros when the plan is "
                          "built, read by the FPN backward, written by nothing (the released configs select every output)"),
    ("tower_ones[*]", "the all-ones f32 tensor per level that the batch-statistics layers' two GEMMs read as the stored output whose sign "
                      "masks the gradient (the norm's backward has applied the real mask already); torch.ones when the plan is built"),
]
NEW_CALLS = ("EseGrads", "Pool3Grads", "SumGrads", "VovnetConvGrads", "VovnetStemGrads")  # what the VoVNet stages contribute


def _backward_outputs(plan):
    """({name: tensor} of every floating-point tensor an op of the plan writes on the backward side -- and, under batch statistics, the
    forward-side tensors that are no named buffers: every tower layer's statistics and the scratch rows they share with the norm's
    backward --, {name: tensor} of the constants)."""
    out = {}
    groups = [(g, getattr(plan, g)) for g in ("pred_groups", "tower_layers", "fpn_layers")]
    groups += [(g, getattr(plan, g, {})) for g in ("backbone_layers", "stem_layers", "vovnet_layers", "vovnet_stem_layers")]  # by backbone and depth
    for gname, group in groups:
        for key, lay in group.items():
            for j, (t, _) in enumerate(lay._raw):
                out[f"{gname}.{key}.raw{j}"] = t
    for key, lay in plan.tower_layers.items():  # the norm's backward of a batch-statistics layer: qp and gc
        for j, (t, _) in enumerate(lay.bn._raw if lay.bn is not None else ()):
            out[f"tower_layers.{key}.bn.raw{j}"] = t
    for (_, i), rec in plan.tower_bn.items():  # one statistics tensor per tower depth, shared by its towers
        if all(rec["stats"].data_ptr() != t.data_ptr() for t in out.values()):
            out[f"tower_bn.{i}.stats"] = rec["stats"]
    if plan.tower_bn:
        out["bn_part"] = plan.bn_part
    out["tower_slab.part"], out["tower_slab.qpart"] = plan.tower_slab
    for name, maps in (("d_cls", plan.d_cls), ("d_b2d", plan.d_b2d), ("d_b3d", plan.d_b3d or [])):
        for l, t in enumerate(maps):
            out[f"{name}[{l}]"] = t
    out["partials"], out["loss_out"], out["grad_denoms"] = plan.partials, plan.loss_out, plan.grad_denoms
    assert all(t.is_floating_point() for t in out.values())
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in out.values()]
    owned = lambda t: any(a <= t.data_ptr() < b for a, b in spans)
    const = {"upstream": plan.upstream}
    for key, lay in plan.fpn_layers.items():
        for l, g in enumerate(lay.keep[0]):
            if not owned(g):
                const[f"fpn_layers.{key}.g[{l}]"] = g
    for l, t in enumerate(plan.tower_ones or ()):
        const[f"tower_ones[{l}]"] = t
    assert not any(owned(t) for t in const.values())
    return out, const


def _grad_calls_in_the_ops(plan):
    """Every GradCall a launch of the plan is bound to, found by walking plan.ops -- not through the plan's layer dicts."""
    from dd3d_amd.engine.losses import GradCall
    calls = []
    for op in plan.ops:
        fn = getattr(op, "fn", None)
        bound = list(getattr(fn, "__defaults__", None) or ()) + [c.cell_contents for c in getattr(fn, "__closure__", None) or ()]
        calls += [b for b in bound if isinstance(b, GradCall) and all(b is not c for c in calls)]
    return calls


def _assert_structural_coverage(plan, outputs, seq):
    """The poisoned tensors are every `_raw` tensor of every gradient call among the plan's launches, whatever stage it belongs to; the
    VoVNet stages and the batch-statistics norms contributed."""
    calls = _grad_calls_in_the_ops(plan)
    want = {(t.data_ptr(), t.numel()) for c in calls for t, _ in c._raw}
    got = {(t.data_ptr(), t.numel()) for n, t in outputs.items() if ".raw" in n}
    assert got == want and len(want) > 100, (seq, len(got), len(want), len(got ^ want))
    kinds = {type(c).__name__ for c in calls}
    if hasattr(plan, "vovnet_stem_layers"):
        assert set(NEW_CALLS) <= kinds, (seq, sorted(kinds))
        by_group = {type(lay).__name__ for g in ("vovnet_layers", "vovnet_stem_layers") for lay in getattr(plan, g).values()}
        assert by_group == set(NEW_CALLS), (seq, sorted(by_group))
    spans = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in outputs.values()]
    owned = lambda t: any(a <= t.data_ptr() and t.data_ptr() + t.numel() * t.element_size() <= b for a, b in spans)
    if plan.batch_stats:
        assert "TowerBnGrads" in kinds and len(plan.tower_bn) > 0 and owned(plan.bn_part)
        for key, rec in plan.tower_bn.items():
            bn = plan.tower_layers[key].bn
            assert owned(bn.qp) and all(owned(g) for g in bn.gc) and owned(rec["stats"]), (seq, key)
    else:
        assert not plan.tower_bn and plan.tower_ones is None


POISON = ["kitti_dla34", "nusc_dla34", "kitti_dla34_bn", "kitti_v99_b2", "kitti_v99_b2_bn"]


@pytest.mark.parametrize("seq", POISON)
def test_poisoned_backward_outputs_change_no_bit(hiplib, seq):
    """Step A, then every tensor the backward's ops write holds the sentinel, then step A again: the same bits.  A kernel that skips a
    store it owes -- an all-zero block, a slice whose units were all skipped -- would hand the sentinel on.  Under batch statistics the
    statistics tensors and the scratch rows of the forward's reduction are written too and hold the sentinel as well.  Integer and index
    tensors, the forward's named activation buffers (towerraw* among them), the staged inputs and the parameter-derived constants are
    not touched (the sequences cover them)."""
    level, flags = HC.SEQUENCES[seq]["deepest"], _flags(HC.SEQUENCES[seq]["deepest"], seq)
    bs = bool(flags.get("batch_stats"))
    model = _fresh(seq)
    batch = _batch(seq, "A")
    first = _split(model.compute_losses(batch, **flags))
    _assert_is(first, _reference(seq, "A"), (seq, "before"))
    plan = _plan(model, seq, level)
    outputs, const = _backward_outputs(plan)
    matches = lambda name: any(fnmatch.fnmatchcase(name, pat.replace("[", "[[]")) for pat, _ in EXCLUDED)
    assert all(matches(n) for n in const) and not any(matches(n) for n in outputs)
    if seq in ("kitti_dla34", "nusc_dla34"):
        assert len(outputs) > 200 and sum(t.numel() for t in outputs.values()) > 5_000_000
    _assert_structural_coverage(plan, outputs, seq)
    assert bs == any(n.startswith("tower_ones") for n in const)
    print(f"[loss_plan_history] poisoned {seq}: {len(outputs)} tensors, {sum(t.numel() for t in outputs.values())} words, {len(const)} constants")
    torch.cuda.synchronize()
    before = {n: t.clone() for n, t in const.items()}
    stats = plan.tower_batch_stats() if bs else {}
    for t in outputs.values():
        t.fill_(SENTINEL)
    second = _split(model.compute_losses(batch, **flags))
    assert _plan(model, seq, level) is plan
    _assert_is(second, first, (seq, "after the sentinel"))
    assert all(set(a) == set(b) for a, b in zip(second, first))
    assert all(torch.equal(const[n], before[n]) for n in const)  # no op writes what the list excludes
    assert not any(bool((v == SENTINEL).any()) for d in second for v in d.values())
    if bs:
        after = plan.tower_batch_stats()
        assert sorted(after) == sorted(stats) and all(torch.equal(after[k], stats[k]) for k in stats)
        assert not any(bool((v == SENTINEL).any()) for v in after.values())
        _assert_stats_are(plan, seq, "A", (seq, "after the sentinel"))


# ------------------------------------------------------------------------------------- 4. the guard's retry loop in compute_losses
@functools.lru_cache(maxsize=None)
def _guard_setup():
    """(state dict, batch, a0): a0 is the largest sampled activation between the two norms on the unscaled weights, read off an
    inference plan on explicit f16x2 as tests/test_full_size_gpu.py reads it."""
    from tests import whole_model_grad_oracle as WO
    cpu = WO.case_model(HC.GUARD_CASE)
    sd = {k: v.clone() for k, v in cpu.state_dict().items()}
    batch = HC.guard_batch(cpu)
    base = _fresh("kitti_dla34", math="f16x2", use_graph=False, sd=sd)
    base(batch)
    plan = next(iter(base._plans.values()))
    a0 = float(plan.amax_values()[plan.amax_names.index("level3.tree1.tree1.conv1")]) / plan.act_scale
    assert a0 > 0
    return sd, batch, a0


def _range_messages(w):
    return [str(x.message) for x in w if "dd3d_amd" in str(x.message)]


@pytest.mark.parametrize("target,what,end", HC.GUARD_ROWS, ids=["6000", "40000", "2e5", "1e-6"])
def test_range_guard_retry_loop_of_compute_losses(hiplib, target, what, end):
    from dd3d_amd import hip
    sd, batch, a0 = _guard_setup()
    sd_x = scaled_between(sd, *HC.GUARD_NORMS, target / a0)
    explicit = _fresh("kitti_dla34", math="f16x2", sd=sd_x)
    res = None
    with pytest.raises(FloatingPointError, match=what):
        res = explicit.compute_losses(batch, stem_grads=True)
    assert res is None
    model = _fresh("kitti_dla34", sd=sd_x)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = _split(model.compute_losses(batch, stem_grads=True))
    msgs = _range_messages(w)
    assert (model.math, model.act_scale) == (end["math"], end["act_scale"]), (target, model.math, model.act_scale, msgs)
    if end["math"] == "bf16x3":
        assert any("switching this model to math='bf16x3'" in m for m in msgs), msgs
    else:
        assert any("plane scale lowered" in m for m in msgs) and not any("switching this model" in m for m in msgs), msgs
    plan = model.get_loss_plan(*model.canvas_size(batch), stem_grads=True)
    assert len(model._plans) == 1  # the plan of the arithmetic that overflowed is gone
    if end["math"] == "bf16x3":
        assert plan.math == hip.MATH_BF16X3
    else:
        assert plan.math == hip.MATH_F16X2 and plan.act_scale == end["act_scale"] and plan.bufs["level5.cat"].plane_scale == end["act_scale"]
    # a fresh model built explicitly in the end state, on the same state dict: the same bits
    there = _fresh("kitti_dla34", math=end["math"], act_scale=end["act_scale"], sd=sd_x)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        want = _split(there.compute_losses(batch, stem_grads=True))
    assert not any("lowered" in m or "switching" in m for m in _range_messages(w))
    _assert_is(got, want, (target, "through the guard against the end state built explicitly"))
    assert all(set(a) == set(b) for a, b in zip(got, want)) and len(got[2]) == len(dict(model.named_parameters()))
    # a second call: no further warning, the same bits
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        again = _split(model.compute_losses(batch, stem_grads=True))
    assert not _range_messages(w), _range_messages(w)
    _assert_is(again, got, (target, "second call"))
    # the inference forward runs on the relaxed arithmetic and does not trip the guard again
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        out = model(batch)
    assert not any("lowered" in m or "switching" in m for m in _range_messages(w)), _range_messages(w)
    assert (model.math, model.act_scale) == (end["math"], end["act_scale"]) and len(out) == 1
    fwd = model.get_plan(*model.canvas_size(batch))
    assert fwd.math == plan.math and (end["math"] == "bf16x3" or fwd.act_scale == end["act_scale"])


def test_plane_scale_4_is_the_whole_model_gradient(hiplib):
    """Plane scale 4 is what the guard picks for activations up to 16376 and nothing else sets: the whole-model comparison of
    tests/test_whole_model_grads_gpu.py (its bar, 8 * max(d32, 2^-23 * max|g64|), and its sign conditions) on the state dict scaled to
    about 6000 between the two norms, at backbone_grads, on the model the guard itself moved to plane scale 4.
    Measured (profiles/loss_plan_history.txt): every family inside the bar, the worst use of the factor 8 is 2.20 (the depth map
    gradient); no stored ReLU sign differs from the float64 forward's."""
    from tests import whole_model_grad_oracle as WO
    from tests.test_whole_model_grads_gpu import compare_with_whole_model_oracle
    sd, batch, a0 = _guard_setup()
    sd_x = scaled_between(sd, *HC.GUARD_NORMS, 6000.0 / a0)
    model = _fresh("kitti_dla34", sd=sd_x)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        model.compute_losses(batch, stem_grads=True)
    assert (model.math, model.act_scale) == (None, 4.0) and any("plane scale lowered 16 -> 4" in m for m in _range_messages(w))
    cpu = WO.case_model(HC.GUARD_CASE)
    cpu.load_state_dict(sd_x)
    case = dict(HC.GUARD_CASE, ref="kitti_dla34_guard_plane_scale_4", math=None, act_scale=4.0, grads="backbone_grads")
    worst, _, _, _ = compare_with_whole_model_oracle("kitti_dla34_guard_plane_scale_4", case, model, cpu, batch, [x["instances"] for x in batch])
    assert (model.math, model.act_scale) == (None, 4.0)
    print(f"[loss_plan_history] plane scale 4 against the whole-model oracle: the worst family uses {worst:.2f} of the factor 8")
