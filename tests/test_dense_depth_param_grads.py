"""DD3DDenseDepth's backward chain, the parts that need no GPU: dry-run DenseDepthLossPlans on the CPU (key sets, op lists, the predictor
call's bindings, the plan cache, the refusals) and the oracle of tests/test_dense_depth_param_grads_gpu.py checked against itself
(tests/dense_depth_param_grad_oracle.py).  The HIP path is that GPU file."""
import inspect

import pytest
import torch

from tests import dense_depth_param_grad_oracle as PO
from tests import loss_grad_cases as GC
from tests.golden import make_dense_depth_loss_golden as G

B, H, W = 2, 128, 256
V99 = PO.case_overrides(PO.CASES["v99"])


def _dla(norm="FrozenBN", use_scale=True, **fe):
    over = G._merge(G.BASE_OVERRIDES, {"DD3D": {"FCOS3D": {"NORM": norm, "USE_SCALE": use_scale}}})
    return GC.cpu_model("dd3d_kitti_dla34", G._merge(over, fe) if fe else over)


def _v99(**fe):
    return GC.cpu_model("dd3d_kitti_v99", G._merge(V99, fe) if fe else V99)


def _plan(model, b=B, h=H, w=W, **flags):
    from dd3d_amd.engine import DenseDepthLossPlan
    return DenseDepthLossPlan(model, b, h, w, device="cpu", dry_run=True, **flags)


def _read(plan, *names):
    tens, params = {}, {}
    for n in names:
        t, p = getattr(plan, n)()
        assert not set(t) & set(tens) and not set(p) & set(params), n  # no stage returns another stage's key
        tens.update(t), params.update(p)
    return tens, params


# ------------------------------------------------------------------------------------------------ key sets
@pytest.mark.parametrize("use_scale", [True, False], ids=["scale", "noscale"])
@pytest.mark.parametrize("norm", ["BN", "FrozenBN", ""], ids=["BN", "FrozenBN", "nonorm"])
def test_param_grads_keys_are_named_parameters_dla34(hiplib, norm, use_scale):
    model = _dla(norm, use_scale)
    plan = _plan(model, stem_grads=True)
    _, params = _read(plan, "predictor_grads", "tower_grads", "fpn_grads", "backbone_grads", "stem_grads")
    named = dict(model.named_parameters())
    assert sorted(params) == sorted(named)
    assert all(params[k].shape == named[k].shape and params[k].dtype == torch.float32 for k in named)
    assert params["fcos3d_head.dense_depth.0.weight"].shape == (1, 256, 3, 3)
    assert ("fcos3d_head.dense_depth.0.bias" in params) == (not use_scale) and ("fcos3d_head.scales_depth.0.scale" in params) == use_scale
    assert ("fcos3d_head.box3d_tower.0.norm.0.weight" in params) == (norm == "BN") and ("fcos3d_head.box3d_tower.0.bias" in params) == (norm == "")


def test_param_grads_keys_are_named_parameters_v99(hiplib):
    model = _v99()
    plan = _plan(model, vovnet_stem_grads=True)
    tens, params = _read(plan, "predictor_grads", "tower_grads", "fpn_grads", "vovnet_grads", "vovnet_stem_grads")
    named = dict(model.named_parameters())
    assert sorted(params) == sorted(named) and all(params[k].shape == named[k].shape for k in named)
    assert sorted(k for k in tens if k.startswith("backbone_")) == ["backbone_stage2", "backbone_stage3", "backbone_stage4", "backbone_stage5", "backbone_stem_1"]


def test_each_depth_adds_exactly_its_keys(hiplib):
    model = _dla("BN")
    L = range(5)
    pre = "fcos3d_head."
    ladder = [
        ("pred_grads", "predictor_grads", [f"box3d_tower_out{l}" for l in L],
         lambda k: k.startswith((pre + "dense_depth.", pre + "scales_depth.", pre + "offsets_depth."))),
        ("tower_grads", "tower_grads", [f"feature{l}" for l in L], lambda k: k.startswith(pre + "box3d_tower.")),
        ("fpn_grads", "fpn_grads", ["backbone_level3", "backbone_level4", "backbone_level5"],
         lambda k: k.startswith("backbone.") and not k.startswith("backbone.bottom_up.")),
        ("backbone_grads", "backbone_grads", ["backbone_level1"], lambda k: k.startswith(tuple(f"backbone.bottom_up.level{n}." for n in (2, 3, 4, 5)))),
        ("stem_grads", "stem_grads", ["backbone_level0", "backbone_base_layer"],
         lambda k: k.startswith(("backbone.bottom_up.base_layer.", "backbone.bottom_up.level0.", "backbone.bottom_up.level1."))),
    ]
    named = [k for k, _ in model.named_parameters()]
    readers = []
    for flag, reader, tens_keys, owns in ladder:
        plan = _plan(model, **{flag: True})
        readers.append(reader)
        t, p = getattr(plan, reader)()
        assert sorted(t) == sorted(tens_keys), flag
        assert sorted(p) == sorted(k for k in named if owns(k)), flag
        _read(plan, *readers)  # every shallower read-out exists on the deeper plan
        for later in [r for _, r, _, _ in ladder if r not in readers]:
            with pytest.raises(RuntimeError, match="built without"):
                getattr(plan, later)()
    v99 = _v99()
    t, p = _plan(v99, vovnet_grads=True).vovnet_grads()
    assert sorted(t) == ["backbone_stem_1"] and sorted(p) == sorted(k for k, _ in v99.named_parameters()
                                                                  if k.startswith("backbone.bottom_up.") and ".stem.stem_1/" not in k)
    t, p = _plan(v99, vovnet_stem_grads=True).vovnet_stem_grads()
    assert t == {} and sorted(p) == ["backbone.bottom_up.stem.stem_1/conv.weight"]
    assert sorted(_plan(v99, fpn_grads=True).fpn_grads()[0]) == ["backbone_stage2", "backbone_stage3", "backbone_stage4", "backbone_stage5"]


# ------------------------------------------------------------------------------------------------ op lists: recorded from the parent commit
TRUNK_OPS = ["preprocess", "stem"] + [
    f"{t}.{op}" for t, ops in (
        ("level2", ["pool", "project", "tree1.conv1", "tree1.conv2", "tree2.conv1", "tree2.conv2", "root"]),
        ("level3", ["pool", "tree1.project", "tree1.tree1.conv1", "tree1.tree1.conv2", "tree1.tree2.conv1", "tree1.tree2.conv2", "tree1.root",
                    "tree2.tree1.conv1", "tree2.tree1.conv2", "tree2.tree2.conv1", "tree2.tree2.conv2", "tree2.root"]),
        ("level4", ["pool", "tree1.project", "tree1.tree1.conv1", "tree1.tree1.conv2", "tree1.tree2.conv1", "tree1.tree2.conv2", "tree1.root",
                    "tree2.tree1.conv1", "tree2.tree1.conv2", "tree2.tree2.conv1", "tree2.tree2.conv2", "tree2.root"]),
        ("level5", ["pool", "project", "tree1.conv1", "tree1.conv2", "tree2.conv1", "tree2.conv2", "root"])) for op in ops
] + ["fpn_lateral5", "fpn_lateral4", "fpn_lateral3", "fpn_outputs", "top_block.p6", "top_block.p7"]
HEAD_OPS = ["dd_tower.0", "dd_tower.1", "dd_tower.2", "dd_tower.3", "dd_predictors"]
PREDICT_OPS = TRUNK_OPS + HEAD_OPS + [f"dd_upsample.{l}" for l in range(5)]
LOSS_OPS = TRUNK_OPS + HEAD_OPS + ["dense_depth_loss"]
HEAD_GRAD_OPS = LOSS_OPS + ["dense_depth_loss_backward"]
HEAD_BUFS = [f"dd{p}.{l}" for p in "AB" for l in range(5)] + [f"dd_raw.{l}" for l in range(5)]


def test_plans_without_the_new_flags_keep_their_ops_and_buffers(hiplib):
    from dd3d_amd.engine import DenseDepthPlan
    model = _dla()
    assert len(PREDICT_OPS) == 56 and len(LOSS_OPS) == 52
    assert [op.name for op in DenseDepthPlan(model, B, H, W, device="cpu", dry_run=True).ops] == PREDICT_OPS
    assert [op.name for op in _plan(model).ops] == LOSS_OPS
    plan = _plan(model, head_grads=True)
    assert [op.name for op in plan.ops] == HEAD_GRAD_OPS and list(plan.bufs)[-15:] == HEAD_BUFS
    # the predictor stage reads the last tower layer's output in its ping / pong buffer: same forward launches, same buffers
    pred = _plan(model, pred_grads=True)
    assert [op.name for op in pred.ops] == HEAD_GRAD_OPS + ["predictor_grads.dd_raw"] and list(pred.bufs) == list(plan.bufs)
    # from tower_grads on every tower layer keeps its output
    tower = _plan(model, tower_grads=True)
    assert [op.name for op in tower.ops] == HEAD_GRAD_OPS + ["predictor_grads.dd_raw"] + [f"tower_grads.box3d.{i}" for i in (3, 2, 1, 0)]
    assert list(tower.bufs)[-25:] == [f"ddL{i}.{l}" for i in range(4) for l in range(5)] + [f"dd_raw.{l}" for l in range(5)]
    deep = _plan(model, stem_grads=True)
    names = [op.name for op in deep.ops]
    kinds = [n.split(".")[0] for n in names if n.split(".")[0].endswith("_grads")]
    assert list(dict.fromkeys(kinds)) == ["predictor_grads", "tower_grads", "fpn_grads", "backbone_grads", "stem_grads"]
    assert deep.tower_slab[0] is deep.fpn_layers["outputs"].part is deep.stem_layers["base_layer"].part  # ONE slab of partials


def test_batch_stats_lowering(hiplib):
    """NORM: BN under batch_stats: raw convolution, statistics and apply per tower layer, the norm's backward in front of each layer's
    gradient call; FrozenBN and norm-less towers keep the fused launches."""
    bn = _plan(_dla("BN"), tower_grads=True, batch_stats=True)
    names = [op.name for op in bn.ops]
    fwd = [x for i in range(4) for x in (f"dd_tower.{i}.raw", f"dd_tower.{i}.bn_stats", f"dd_tower.{i}.bn_apply")]
    assert names[len(TRUNK_OPS):len(TRUNK_OPS) + 13] == fwd + ["dd_predictors"]
    assert names[-8:] == [x for i in (3, 2, 1, 0) for x in (f"tower_bn_grads.box3d.{i}", f"tower_grads.box3d.{i}")]
    assert sorted(bn.tower_bn) == [("box3d", i) for i in range(4)] and all(f"ddraw{i}.{l}" in bn.bufs for i in range(4) for l in range(5))
    stats = bn.tower_batch_stats()
    assert len(stats) == 4 * 5 * 4 and "fcos3d_head.box3d_tower.2.norm.3.running_var" in stats and "fcos3d_head.box3d_tower.0.norm.0.batch_mean" in stats
    shared = _plan(_dla("BN"), batch_stats=True)  # no backward: one raw buffer per level serves every layer
    assert [n for n in shared.bufs if n.startswith("ddraw")] == [f"ddraw.{l}" for l in range(5)]
    for norm in ("FrozenBN", ""):
        plan = _plan(_dla(norm), tower_grads=True, batch_stats=True)
        assert not plan.tower_bn and [op.name for op in plan.ops] == [op.name for op in _plan(_dla(norm), tower_grads=True).ops]
        assert plan.tower_batch_stats() == {}
    with pytest.raises(RuntimeError, match="built without batch_stats"):
        _plan(_dla("BN"), tower_grads=True).tower_batch_stats()


# ------------------------------------------------------------------------------------------------ the predictor call's bindings
@pytest.mark.parametrize("use_scale", [True, False], ids=["scale", "noscale"])
def test_predictor_group_bindings(hiplib, use_scale):
    from dd3d_amd import hip
    model = _dla("FrozenBN", use_scale)
    plan = _plan(model, pred_grads=True)
    assert list(plan.pred_groups) == ["dd_raw"]
    grp = plan.pred_groups["dd_raw"]
    a = grp.args
    assert (a.n, a.g_pitch, a.num_levels, a.B, a.Cin) == (1, 4, 5, B, 256) and grp.tower == "box3d"
    assert not a.lo  # no clamp
    g, maps, w, bias, scale, lo, slot = grp.keep
    assert len({t.data_ptr() for t in w}) == 5 and grp.owners == [0, 1, 2, 3, 4] and all(tuple(t.shape) == (1, 3, 3, 256) for t in w)  # a filter per level
    assert [a.w[l] for l in range(5)] == [t.data_ptr() for t in w]
    assert slot.tolist() == ([0] if use_scale else [-1]) and slot.dtype == torch.int32
    assert all(g[l] is plan.d_raw[l] and a.g[l] == plan.d_raw[l].data_ptr() and a.map[l] == plan.dd_raw[l].t.data_ptr() for l in range(5))
    assert [(a.H[l], a.W[l]) for l in range(5)] == [(f.H, f.W) for f in plan.features] == [(16, 32), (8, 16), (4, 8), (2, 4), (1, 2)]
    head = model.fcos3d_head
    for l in range(5):
        want = float(head.scales_depth[l].scale) if use_scale else 1.0
        assert scale[l].tolist() == [want] and bias[l].tolist() == ([0.0] if use_scale else [float(head.dense_depth[l].bias)])
    assert bool((plan.upstream == 1).all())
    assert a.act_mode == hip.PG_ACT_F16X2  # the default arithmetic's planes of the last tower layer


# ------------------------------------------------------------------------------------------------ the public interface
def _dry_loss_plans(monkeypatch):
    """get_loss_plan on a CPU model: the plans it builds are dry-run plans."""
    import dd3d_amd.engine as E
    real = E.DenseDepthLossPlan
    built = []

    def dry(model, b, h, w, **flags):
        built.append(flags)
        return real(model, b, h, w, device="cpu", dry_run=True, **flags)

    monkeypatch.setattr(E, "DenseDepthLossPlan", dry)
    return built


def test_one_cached_plan_per_deepest_flag(hiplib, monkeypatch):
    built = _dry_loss_plans(monkeypatch)
    model = _dla("BN")
    model.use_graph = False
    plain, head = model.get_loss_plan(B, H, W), model.get_loss_plan(B, H, W, head_grads=True)
    assert list(model._plans) == [("dense_depth_loss", B, H, W, None), ("dense_depth_loss_grads", B, H, W, None)]  # the two keys of before
    assert built == [{}, {"head_grads": True}] and not plain.grads and head.grads and not head.pred_grads
    ladder = ["pred_grads", "tower_grads", "fpn_grads", "backbone_grads", "stem_grads"]
    plans = [model.get_loss_plan(B, H, W, **{f: True}) for f in ladder]
    assert len(model._plans) == 7 and len({id(p) for p in plans + [plain, head]}) == 7
    assert built[2:] == [{f: True} for f in ladder]
    # shallower flags beside a deeper one name the deeper one's plan; the existing two stay the plans they are
    assert model.get_loss_plan(B, H, W, head_grads=True, pred_grads=True, stem_grads=True) is plans[-1]
    assert model.get_loss_plan(B, H, W, tower_grads=True, pred_grads=True) is plans[1]
    assert model.get_loss_plan(B, H, W) is plain and model.get_loss_plan(B, H, W, head_grads=True) is head and len(built) == 7
    bs = model.get_loss_plan(B, H, W, tower_grads=True, batch_stats=True)
    assert bs is not plans[1] and bs.batch_stats and built[-1] == {"tower_grads": True, "batch_stats": True}
    assert model.get_loss_plan(B, H, W, tower_grads=True, batch_stats=True) is bs
    assert model.get_loss_plan(B, H, W, batch_stats=True) is not plain and built[-1] == {"batch_stats": True}
    with pytest.raises(TypeError, match="batch_stat"):
        model.get_loss_plan(B, H, W, batch_stat=True)
    sig = inspect.signature(type(model).get_loss_plan).parameters
    assert all(sig[f].default is False for f in ["head_grads"] + ladder + ["vovnet_grads", "vovnet_stem_grads"])


def _labelled(case_name="dla34_frozenbn_none"):
    case = PO.CASES[case_name]
    inputs = PO.case_images(case)
    for x, (h, w) in zip(inputs, case["sizes"]):
        x["depth"] = torch.zeros(h, w)
    return inputs


def test_compute_losses_keywords(hiplib, monkeypatch):
    from dd3d_amd.modeling.dense_depth import DD3DDenseDepth
    sig = inspect.signature(DD3DDenseDepth.compute_losses).parameters
    assert [k for k in sig if k.endswith("_grads")] == ["head_grads", "predictor_grads", "tower_grads", "fpn_grads", "backbone_grads", "stem_grads"]
    assert all(sig[k].default is False for k in sig if k.endswith("_grads")) and "vovnet_grads" not in sig  # (those two come through **branch)
    model = _dla()
    for bad in ("vovnet_stem_grad", "predictor_grad", "grads", "pred_grads"):
        with pytest.raises(TypeError, match=bad):
            model.compute_losses(_labelled(), **{bad: True})
    # the flags reach the plan builder with their implications, deepest first
    built = _dry_loss_plans(monkeypatch)
    model.use_graph = False

    class Stop(Exception):
        pass

    def stop(*a, **k):
        raise Stop()

    monkeypatch.setattr(DD3DDenseDepth, "_stage", lambda self, inputs, get_plan: (get_plan(B, H, W), stop())[0])
    for flags, want in ((dict(), {}), (dict(head_grads=True), {"head_grads": True}), (dict(predictor_grads=True), {"pred_grads": True}),
                        (dict(tower_grads=True, head_grads=True), {"tower_grads": True}), (dict(stem_grads=True, fpn_grads=True), {"stem_grads": True}),
                        (dict(fpn_grads=True, batch_stats=True), {"fpn_grads": True, "batch_stats": True})):
        with pytest.raises(Stop):
            model.compute_losses(_labelled(), **flags)
        assert built[-1] == want, flags
    with pytest.raises(NotImplementedError, match="stem_grads=True"):  # a DLA model has its own flags
        model.compute_losses(_labelled(), vovnet_grads=True)
    with pytest.raises(NotImplementedError, match="inference math only"):
        model.train()


# ------------------------------------------------------------------------------------------------ refusals: LossPlan's cases and wording
def test_unsupported_combinations_raise(hiplib, monkeypatch):
    for variant, word in (("DLA-60", "Bottleneck"), ("DLA-X-60-C", "BottleneckX")):
        m = _dla(FE={"BACKBONE": {"NAME": variant}})
        for flag in ("backbone_grads", "stem_grads"):
            with pytest.raises(NotImplementedError, match=word):
                _plan(m, **{flag: True})
        _plan(m, fpn_grads=True)
    model = _dla()
    model.force_generic_dla = True
    with pytest.raises(NotImplementedError, match="force_generic_dla"):
        _plan(model, backbone_grads=True)
    model.force_generic_dla = False
    with pytest.raises(NotImplementedError, match="stem_grads=True"):  # vovnet_grads on a DLA model
        _plan(model, vovnet_grads=True)
    with pytest.raises(NotImplementedError, match="stem_grads=True"):
        _plan(model, vovnet_stem_grads=True)
    for hw in ((127, 256), (128, 254 + 1)):
        with pytest.raises(NotImplementedError, match="even canvas"):
            _plan(model, h=hw[0], w=hw[1], stem_grads=True)
    for math in ("bf16x2", "bf16"):  # the reduced arithmetic modes have no loader: from the predictor stage on
        model.math = math
        for flag in ("pred_grads", "tower_grads", "stem_grads"):
            with pytest.raises(NotImplementedError, match=math):
                _plan(model, **{flag: True})
        _plan(model, head_grads=True)
    model.math = None
    v99 = _v99()
    with pytest.raises(NotImplementedError, match="V2-99"):  # backbone_grads on a VoVNet model
        _plan(v99, backbone_grads=True)
    with pytest.raises(NotImplementedError, match="V2-99"):
        _plan(v99, stem_grads=True)
    for name, word in (("V-19-slim-eSE", "multiple of 32"), ("V-19-dw-eSE", "depthwise"), ("V-19-slim-dw-eSE", "depthwise")):
        m = _v99(FE={"BACKBONE": {"NAME": name}})
        for flag in ("vovnet_grads", "vovnet_stem_grads"):
            with pytest.raises(NotImplementedError, match=word):
                _plan(m, **{flag: True})
    for math in ("bf16x2", "bf16"):
        v99.math = math
        with pytest.raises(NotImplementedError, match=math):
            _plan(v99, vovnet_grads=True)
    # DD3D_PLANES=0 (the three-term arithmetic on f32 NHWC tensors): the predictor, tower and FPN stages build, the VoVNet's refuses
    monkeypatch.setenv("DD3D_PLANES", "0")
    v99.math = "bf16x3"
    _plan(v99, fpn_grads=True)
    with pytest.raises(NotImplementedError, match="split-plane"):
        _plan(v99, vovnet_stem_grads=True)
    monkeypatch.delenv("DD3D_PLANES")
    v99.math = None
    # batch statistics: a level with one value per channel, and trunk norms that would need them too
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        _plan(_dla("BN"), b=1, h=128, w=128, batch_stats=True)  # P7 is 1 x 1
    _plan(_dla("BN"), b=1, h=128, w=128)
    for key, fe in (("FE.BACKBONE.NORM", {"BACKBONE": {"NORM": "BN"}}), ("FE.FPN.NORM", {"FPN": {"NORM": "BN"}})):
        with pytest.raises(NotImplementedError, match=key):
            _plan(_dla("BN", FE=fe), batch_stats=True)
        _plan(_dla("BN", FE=fe), stem_grads=True)


# ------------------------------------------------------------------------------------------------ the oracle against itself
@pytest.fixture(scope="module")
def forwards():
    """The float64 forward of every distinct (model, batch) of the GPU test's cases, once."""
    out = {}
    for name in ("dla34_frozenbn_none", "dla34_frozenbn_half", "dla34_bn_batch_stats", "v99"):
        case = PO.CASES[name]
        model, inputs, ex = PO.cpu_model(case), PO.case_images(case), {}
        pre = PO.param_grads(model, inputs, [torch.zeros(h, w) for h, w in case["sizes"]], PO.F64, extras=ex, backward=False,
                             batch_stats=case["batch_stats"])[2]
        out[name] = (case, model, inputs, ex, pre)
    return out


@pytest.mark.parametrize("name", ["dla34_frozenbn_none", "dla34_frozenbn_half", "dla34_bn_batch_stats", "v99"])
def test_the_seeds_keep_the_fixture_under_the_cap(forwards, name):
    """The float64 oracle alone, with KINK_MARGIN + 1e-2 as the margin: the removed share stays under the cap, both signs of the
    derivative occur, and no kept pixel is within beta of a prediction (the linear branch everywhere: see the oracle's docstring)."""
    case, model, inputs, ex, pre = forwards[name]
    s = PO.loss_settings(model)
    assert len(pre) == {True: 3 + 30 + 1 + 20, False: 119}[PO.is_dla(model)]
    depths = PO.ground_truth(inputs, ex["maps"], s, case["gt_seed"])
    assert [tuple(d.shape) for d in depths] == case["sizes"]
    kept, removed, quad = PO.remove_kinks(depths, ex["maps"], s, case["H"], case["W"], PO.CPU_SCAN_EXTRA)
    valid = sum(int(((k >= s["min_depth"]) & (k <= s["max_depth"])).sum()) for k in kept)
    print(f"[dense_depth_param_grads] {name} seed {case['gt_seed']}: removed {100 * removed:.3f} % (cap 2 %), quadratic share {quad}, {valid} valid pixels")
    assert removed <= PO.KINK_CAP and quad == 0.0 and valid > 0.3 * sum(h * w for h, w in case["sizes"])
    gt = torch.stack([torch.nn.functional.pad(k, (0, case["W"] - k.shape[1], 0, case["H"] - k.shape[0])) for k in kept])
    M = (gt >= s["min_depth"]) & (gt <= s["max_depth"])
    below = float((ex["maps"][0][M] > gt[M]).double().mean())
    assert 0.3 < below < 0.7  # ground truth on either side of the predictions


def test_float32_and_float64_passes_agree(forwards):
    """The DLA-34 fixture under the float64 forward's own masks: the float32 pass is within 2e-5 of the float64 one relative to each
    family's largest gradient (measured: at most 1.4e-6), every family is nonzero, every parameter and tensor has its shape."""
    case, model, inputs, ex, pre = forwards["dla34_frozenbn_none"]
    s = PO.loss_settings(model)
    depths, _, _ = PO.remove_kinks(PO.ground_truth(inputs, ex["maps"], s, case["gt_seed"]), ex["maps"], s, case["H"], case["W"], PO.CPU_SCAN_EXTRA)
    masks = [v > 0 for v in pre]
    p64, a64, _ = PO.param_grads(model, inputs, depths, PO.F64, masks=masks)
    p32, a32, _ = PO.param_grads(model, inputs, depths, PO.F32, masks=masks)
    named = dict(model.named_parameters())
    assert sorted(p64) == sorted(named) and all(p64[k].shape == named[k].shape and p64[k].dtype == PO.F64 and p32[k].dtype == PO.F32 for k in named)
    fams = {}
    for k in p64:
        fams.setdefault(PO.stage_and_family(k), []).append(k)
    assert {st for st, _ in fams} == {"predictors", "towers", "fpn", "stem"} | {f"backbone level{n}" for n in (2, 3, 4, 5)}
    for (st, fam), ks in sorted(fams.items()):
        a, b = torch.cat([p64[k].reshape(-1) for k in ks]), torch.cat([p32[k].reshape(-1).double() for k in ks])
        gmax, d32 = float(a.abs().max()), float((a - b).abs().max())
        print(f"[dense_depth_param_grads] oracle {st} {fam}: max|g64| {gmax:.3e} d32 {d32:.3e} ({d32 / gmax:.1e} of max)")
        assert gmax > 0 and d32 <= 2e-5 * gmax, (st, fam)
    want = [f"{k}{l}" for k in ("dense_depth", "box3d_tower_out", "feature") for l in range(5)] + \
        ["backbone_level3", "backbone_level4", "backbone_level5", "backbone_base_layer", "backbone_level0", "backbone_level1"]
    assert list(a64) == want
    for k in a64:
        gmax, d32 = float(a64[k].abs().max()), float((a64[k] - a32[k].double()).abs().max())
        assert gmax > 0 and d32 <= 2e-5 * gmax, k
    assert a64["dense_depth4"].shape == (2, 1, 1, 2) and a64["feature0"].shape == (2, 256, 16, 32) and a64["backbone_base_layer"].shape == (2, 16, 128, 256)
    # the loss dict of the pass is the loss oracle's on the forward's maps
    from tests import dense_depth_loss_oracle as DO
    e32 = {}
    PO.param_grads(model, inputs, depths, PO.F32, masks=masks, extras=e32, backward=False)
    ref, count, _ = DO.dense_depth_loss(e32["maps"], DO.pad_depth(depths, case["H"], case["W"]), s["min_depth"], s["max_depth"], s["beta"], s["weight"])
    assert count > 0 and all(abs(float(v) - float(w)) <= 2e-6 * abs(float(w)) for v, w in zip(e32["losses"], ref.values()))
