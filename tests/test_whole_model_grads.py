"""The composed backward's reference without a GPU (tests/whole_model_grad_oracle.py): the whole-model autograd pass equals the five stage
oracles chained on the float64 forward's own activations; the GT seeds of the GPU cases are pinned to batches without a positive on a
non-smooth point of the loss; the float32 and the float64 forward disagree on ReLU signs only within the conditions the GPU test holds
the kernels to; forcing the natural masks changes no bit; a forced mask is honoured."""
import copy
import functools

import pytest
import torch

from oracle import dd3d_oracle as O
from tests import backbone_grad_cases as BC
from tests import backbone_grad_oracle as BO
from tests import fpn_grad_oracle as FO
from tests import loss_grad_cases as GC
from tests import loss_grad_oracle as GO
from tests import predictor_grad_oracle as PO
from tests import tower_grad_oracle as TO
from tests import whole_model_grad_oracle as WO

F64 = torch.float64


class Reference:
    """A reference of WO.REFERENCES: the CPU model, the batch, and the natural (unforced) float64 pass, computed once."""
    def __init__(self, name):
        self.case = next(c for c in WO.CASES.values() if c["ref"] == name)
        self.model = WO.case_model(self.case)
        self.inputs, self.gt = WO.case_inputs(self.case, self.model)
        self.extras = {}
        self.batch_stats = bool(self.case.get("batch_stats"))
        self.params, self.at, self.pre = WO.whole_model_grads(self.model, self.model.cfg, self.inputs, self.gt, F64, extras=self.extras,
                                                              batch_stats=self.batch_stats)

    @functools.cached_property
    def pre32(self):
        return WO.whole_model_grads(self.model, self.model.cfg, self.inputs, self.gt, torch.float32, batch_stats=self.batch_stats)[2]

    @functools.cached_property
    def sites(self):
        from dd3d_amd.engine.losses import LossPlan
        return WO.relu_sites(LossPlan(self.model, *self.model.canvas_size(self.inputs), device="cpu", dry_run=True, batch_stats=self.batch_stats,
                                      **{self.case["grads"]: True}))


@functools.lru_cache(maxsize=None)
def reference(name):
    return Reference(name)


@pytest.mark.parametrize("name", WO.REFERENCES)
def test_gt_seeds_are_pinned_to_batches_without_kink_positives(name):
    ref = reference(name)
    ex = ref.extras
    assert ex["targets"]["pos_inds"].numel() == ref.case["positives"] >= 50
    assert int(GO.near_kink(ex["maps"], ex["targets"], ex["inv_K"], ex["p"]).sum()) == 0
    # every named parameter receives a gradient; the ReLU calls are those the plan's mapping lists
    named = dict(ref.model.named_parameters())
    assert sorted(ref.params) == sorted(named) and all(ref.params[k].shape == named[k].shape for k in named)
    assert len(ref.sites) == len(ref.pre) == ref.case["relus"]
    free = WO.free_relus(ref.model)
    assert [s is None for s in ref.sites] == [True] * free + [False] * (len(ref.pre) - free) and free == (3 if WO.is_dla(ref.model) else 99)
    for site, pre in zip(ref.sites, ref.pre):  # the dry-run plan's buffers have the oracle's shapes, call by call
        if site is not None:
            _, buf, c0, n, _ = site
            assert (buf.B, buf.pitch - c0 if n is None else n, buf.H, buf.W) == tuple(pre.shape), site[0]


@pytest.mark.parametrize("name", WO.REFERENCES)
def test_reference_sign_disagreements_stay_within_the_conditions(name):
    """float32 against float64 oracle forward: a sign may differ only where |pre64| <= 2^-16 of its tensor's largest magnitude, and on at
    most 1e-4 of all ReLU elements (measured on the KITTI case: 1 of 15.39 M; 1240 elements are candidates)."""
    ref = reference(name)
    total = bad = far = near = 0
    for a, b in zip(ref.pre, ref.pre32):
        d = (a > 0) != (b > 0)
        small = a.abs() <= WO.SIGN_NEAR * float(a.abs().max())
        total, bad, far, near = total + a.numel(), bad + int(d.sum()), far + int((d & ~small).sum()), near + int((small & (a != 0)).sum())
    print(f"[whole_model_grads] {name}: {total} ReLU elements, {near} nonzero within 2^-16 of their tensor's maximum, {bad} float32 sign disagreements")
    assert far == 0 and bad <= WO.SIGN_CAP * total


def test_forcing_the_natural_masks_changes_no_bit():
    ref = reference("kitti_dla34")
    params, at, pre = WO.whole_model_grads(ref.model, ref.model.cfg, ref.inputs, ref.gt, F64, masks=WO.natural_masks(ref.pre))
    assert all(torch.equal(params[k], ref.params[k]) for k in ref.params) and all(torch.equal(at[k], ref.at[k]) for k in ref.at)
    assert all(torch.equal(a, b) for a, b in zip(pre, ref.pre))
    with pytest.raises(ValueError, match="ReLU call 98"):
        WO.whole_model_grads(ref.model, ref.model.cfg, ref.inputs, ref.gt, F64, masks=WO.natural_masks(ref.pre)[:-1])


def test_a_forced_mask_is_honoured():
    """One element of level4.tree1.tree1.mid (conv1 of a BasicBlock) switched off: that output channel's filter row changes, the
    layer's other rows do not, the forward (the recorded pre-activations, the loss) does not."""
    ref = reference("kitti_dla34")
    k = next(i for i, s in enumerate(ref.sites) if s is not None and s[0] == "level4.tree1.tree1.mid")
    masks = WO.natural_masks(ref.pre)
    flat = int(ref.pre[k].argmax())  # an element the natural mask lets through
    masks[k] = masks[k].clone()
    assert bool(masks[k].view(-1)[flat])
    masks[k].view(-1)[flat] = False
    ch = (flat // (ref.pre[k].shape[2] * ref.pre[k].shape[3])) % ref.pre[k].shape[1]
    ex = {}
    params, _, pre = WO.whole_model_grads(ref.model, ref.model.cfg, ref.inputs, ref.gt, F64, masks=masks, extras=ex)
    assert all(torch.equal(a, b) for a, b in zip(pre, ref.pre)) and all(torch.equal(ex["losses"][n], ref.extras["losses"][n]) for n in ex["losses"])
    w, w0 = params["backbone.bottom_up.level4.tree1.tree1.conv1.weight"], ref.params["backbone.bottom_up.level4.tree1.tree1.conv1.weight"]
    rest = torch.arange(w.shape[0]) != ch
    assert not torch.equal(w[ch], w0[ch]) and torch.equal(w[rest], w0[rest])
    assert not torch.equal(params["backbone.bottom_up.level2.tree1.conv1.weight"], ref.params["backbone.bottom_up.level2.tree1.conv1.weight"])  # everything upstream moves
    assert torch.equal(params["backbone.bottom_up.level5.root.conv.weight"], ref.params["backbone.bottom_up.level5.root.conv.weight"])  # nothing downstream does


def test_batch_statistics_switch_is_the_train_mode_tower_forward_and_its_autograd():
    """whole_model_grads(batch_stats=True) -- the batch_norm method of the intercepting functional -- against tower_bn_oracle's own
    switch, which replaces the oracle's norm function: the head maps on the pass' own FPN features are tower_bn_oracle.head_maps, and
    the gradients are plain autograd of the whole forward under that other switch.  Every norm of the two BN towers takes the
    batch's statistics (four layers, one norm per level: the call count is checked against bn_prefixes), the state dict's running
    statistics stay, and the running-statistics forward is another function."""
    from tests import tower_bn_oracle as TB
    ref, base = reference("kitti_dla34_batch_stats"), reference("kitti_dla34")
    assert ref.batch_stats and not base.batch_stats and ref.case["gt_seed"] == base.case["gt_seed"]
    model, ex = ref.model, ref.extras
    prefixes = TB.bn_prefixes(model)
    L = ex["p"]["num_levels"]
    assert len(prefixes) == 8 * L  # cls and box2d towers, four layers each, one norm per level
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        maps = TB.head_maps(model, ex["features"], F64)
    assert sorted(maps) == sorted(ex["maps"]) and all(torch.equal(maps[k], ex["maps"][k]) for k in maps)
    assert not torch.equal(ex["maps"]["logits0"], base.extras["maps"]["logits0"]) and all(torch.equal(a, b) for a, b in zip(ex["features"], base.extras["features"]))
    with TB.batch_statistics(prefixes):
        params, at, pre = WO.whole_model_grads(model, model.cfg, ref.inputs, ref.gt, F64)
    assert sorted(params) == sorted(ref.params) and sorted(at) == sorted(ref.at) and len(pre) == len(ref.pre)
    assert all(torch.equal(params[k], ref.params[k]) for k in params) and all(torch.equal(at[k], ref.at[k]) for k in at)
    assert all(torch.equal(a, b) for a, b in zip(pre, ref.pre))
    moved = {k for k in params if not torch.equal(ref.params[k], base.params[k])}  # (the FrozenBN box3d tower and its predictors stay)
    cls = [p for p in prefixes if "cls_tower" in p]  # the classification loss reaches every location of every level
    assert len(cls) == 4 * L and all(p + ".weight" in moved and p + ".bias" in moved for p in cls)
    assert any("box2d_tower" in k for k in moved) and "backbone.bottom_up.level2.tree1.conv1.weight" in moved
    assert all(torch.equal(v, sd0[k]) for k, v in model.state_dict().items())  # the statistics in the state dict are never written
    with pytest.raises(ValueError, match="batch-statistics norm calls"):  # a switch that reaches no norm is an error, not a silent eval forward
        with TB.batch_statistics(prefixes):
            WO.whole_model_grads(model, model.cfg, ref.inputs, ref.gt, F64, backward=False, batch_stats=True)


# ------------------------------------------------------------------------------------------------------------ the stages compose
def _towers_with_exact_norm_scales(model):
    """A float64 copy of `model` whose tower norms carry weight * rstd as their weight, variance 1 and eps 0.  tower_grad_oracle folds a
    norm as layers.fold_norm does, the reciprocal root in FLOAT32 (what the kernels multiply by); the oracle forward evaluates it in the
    working precision.  The two differ by 6e-8 relative, far above float64 rounding; with variance 1 the float32 root is exact and the
    copy computes what the float64 forward computes.  Returns (copy, {norm weight's name: rstd}): d / d weight = rstd * d / d (weight * rstd)."""
    m = copy.deepcopy(model).double()
    names = {id(p): k for k, p in m.named_parameters()}
    rstd = {}
    with torch.no_grad():
        for convs in TO.tower_modules(m).values():
            for conv in convs:
                for l in range(len(conv.norm) if isinstance(conv.norm, torch.nn.ModuleList) else 1):
                    n = TO.level_norm(conv, l)
                    if n is None or id(n) in rstd:
                        continue
                    s = torch.rsqrt(n.running_var + n.eps)
                    n.weight.mul_(s)
                    n.running_var.fill_(1.0)
                    n.eps = 0.0
                    rstd[id(n)] = True
                    if id(n.weight) in names:
                        rstd[names[id(n.weight)]] = s
    return m, {k: v for k, v in rstd.items() if isinstance(k, str)}


def composed_stage_oracles(model, ex, sites):
    """loss_grad_oracle.head_grads, then the predictor, tower-chain, FPN-chain and backbone-chain oracles in float64, each fed the
    previous one's output and the float64 forward's own activations (`ex`: the extras of a natural whole_model_grads pass).  Returns
    ({parameter name: gradient}, {tensor key: gradient}) under whole_model_grads' names."""
    out, p = ex["relu_out"], ex["p"]
    idx = {s[0]: k for k, s in enumerate(sites) if s is not None}
    L = p["num_levels"]
    G = GO.head_grads(ex["maps"], ex["targets"], ex["inv_K"], p, None, F64)
    depth = {t: len(convs) for t, convs in TO.tower_modules(model).items()}
    y = lambda t, i, l: out[idx[f"{t}_tower.{i}[{l}]"]]
    towers = {t: [y(t, depth[t] - 1, l) for l in range(L)] for t in depth}
    params, tg = PO.model_grads(model, towers, G, ex["maps"], F64)
    stored = {t: [([ex["features"][l] if i == 0 else y(t, i - 1, l) for l in range(L)], [y(t, i, l) for l in range(L)]) for i in range(depth[t])] for t in depth}
    m64, rstd = _towers_with_exact_norm_scales(model)
    tp, fg, _ = TO.chain_grads(m64, stored, {t: [tg[f"{t}_tower_out{l}"] for l in range(L)] for t in depth}, F64)
    params.update({k: (v * rstd[k] if k in rstd else v) for k, v in tp.items()})
    sd = {k: (v.detach().double() if v.is_floating_point() else v) for k, v in model.state_dict().items()}
    sp, sel = FO.spec(model), list(model.in_features)
    feats = ex["bottom_up"]
    fp, bg, _ = FO.chain_grads(model, FO.stored_activations(sd, feats, sp), feats, {n: fg[f"feature{sel.index(n)}"] for n in model.backbone._out_features if n in sel}, F64)
    params.update(fp)
    dla = model.backbone.bottom_up
    S = BO.stored_activations(dla, out[WO.stem_relus(model) - 1])
    bp, g1, _ = BO.chain_grads(dla, S, {n: bg[f"backbone_{n}"] for n in model.backbone.in_features}, F64)
    params.update(bp)
    return params, dict(G, **fg, **bg, backbone_level1=g1)


def _assert_composes(model, params, at, ex, sites, what):
    cp, ct = composed_stage_oracles(model, ex, sites)
    assert sorted(cp) == sorted(k for k in params if WO.stage_and_family(k) is not None)
    assert sorted(ct) == sorted(at)
    fams = {}
    for k in cp:
        fams.setdefault(WO.stage_and_family(k), []).append((cp[k], params[k]))
    for k in ct:
        fams.setdefault(("tensors", WO.tensor_family_of(k)), []).append((ct[k], at[k]))
    for fam, pairs in sorted(fams.items()):
        gmax = max(float(b.abs().max()) for _, b in pairs)
        dev = max(float((a - b).abs().max()) for a, b in pairs)
        print(f"[whole_model_grads] {what} {fam[0]} {fam[1]}: max|g64| {gmax:.3e} composed-minus-whole {dev:.3e} ({dev / gmax if gmax else 0.0:.1e} relative)")
        assert gmax > 0.0 and dev <= 1e-9 * gmax, (what, fam, dev, gmax)


def test_stage_oracles_compose_to_the_whole_model_dla34():
    ref = reference("kitti_dla34_bn")  # every norm owns a weight and a bias: the read-out formulas take part
    _assert_composes(ref.model, ref.params, ref.at, ref.extras, ref.sites, "dla34")


def test_stage_oracles_compose_to_the_whole_model_mini(monkeypatch):
    """The mini DLA of backbone_grad_cases (a depth-2 level_root tree WITHOUT a project among its levels) under the KITTI heads."""
    from dd3d_amd.engine.losses import LossPlan
    from dd3d_amd.modeling import dla as D
    from dd3d_amd.synthetic import make_state_dict
    monkeypatch.setitem(D.DLA_NAME_TO_BUILDER, "DLA-mini", lambda cfg: D.DLA(BC.MINI_LEVELS, BC.MINI_CHANNELS, out_features=list(cfg.OUT_FEATURES), norm=cfg.NORM))
    monkeypatch.setitem(O.DLA_SPECS, "DLA-mini", (BC.MINI_LEVELS, BC.MINI_CHANNELS, O._basic_block, False))
    case = WO.CASES["kitti_dla34"]
    model = GC.cpu_model(case["exp"], GC.merged(WO.BN_EVERYWHERE, {"FE": {"BACKBONE": {"NAME": "DLA-mini"}}}))
    model.load_state_dict(make_state_dict(model))
    BC.randomize(model.backbone.bottom_up)
    inputs, gt = WO.case_inputs(case, model)
    ex = {}
    params, at, pre = WO.whole_model_grads(model, model.cfg, inputs, gt, F64, extras=ex)
    sites = WO.relu_sites(LossPlan(model, *model.canvas_size(inputs), device="cpu", dry_run=True, backbone_grads=True))
    assert len(sites) == len(pre)
    _assert_composes(model, params, at, ex, sites, "mini")
