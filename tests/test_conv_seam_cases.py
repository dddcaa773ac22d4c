"""The case tables of the convolution seam tests (tests/conv_seam_cases.py) exercise what they claim -- shown on the float64 reference and
on dry-run ConvOps, without a GPU.  tests/test_conv_seam_gpu.py runs the same tables on the device."""
import pytest
import torch
import torch.nn.functional as F

from dd3d_amd import hip
from tests import conv_seam_cases as S


def _tile_grid(tile):
    from dd3d_amd.engine.tiling import PLANE_TILE_ALIAS, TILE_WAVE_GRID
    return TILE_WAVE_GRID[PLANE_TILE_ALIAS.get(tile, tile)]


def test_m_table_meets_every_tile_edge():
    """Group A: for the BM of every tile it names, the 3 x 3 / stride 1 launch has a segment smaller than a tile, one that fills its tiles
    exactly, one whose last tile holds one pixel, the 1 x 3 map, a batch of three tiny images; at least 5 segments, at least two filters,
    no map larger than 24 x 40."""
    seen = set()
    for L in S.group_a():
        assert len(L["segs"]) >= 5 and len({s["filt"] for s in L["segs"]}) >= 2
        assert len({s["tag"] for s in L["segs"]}) == len(L["segs"])  # every segment its own input, scale and bias
        assert all(s["H"] <= 24 and s["W"] <= 40 for s in L["segs"]) and L["Cin"] in (32, 64, 96, 128)
        if L["name"] not in ("a_s1", "a_sk"):
            continue
        bm = hip.TILE_SHAPES[L["tile"]][0]
        seen.add(bm)
        ms = [S.seg_m(L, s) for s in L["segs"]]
        assert 3 in ms and any(m < bm for m in ms if m > 3) and any(m % bm == 0 for m in ms) and any(m % bm == 1 for m in ms), (bm, ms)
        assert any(s["B"] == 3 and S.seg_m(L, s) < bm for s in L["segs"])
    assert seen == {64, 128, 192, 256}
    for L in S.group_a():
        if L["name"] == "a_s2":
            assert L["stride"] == 2 and all(s["H"] % 2 == 1 and s["W"] % 2 == 1 for s in L["segs"])


def test_group_a_names_a_representative_tile_set():
    """Per family and mode: an 8-wave tile, a 4-wave tile, a T42 / T24 tile and, where the mode has them, the 8-wave 256-column tiles; the
    split-K variation has a row-kernel split and one that falls back to the per-tap kernel."""
    by = {}
    for L in S.group_a():
        if L["name"] == "a_s1":
            by.setdefault((L["family"], L["mode"]), set()).add(L["tile"])
    assert set(by) == {("f32", None), ("x3f32", None)} | {(f, m) for f in S.PLANE_FAMILIES for m in S.MODES}
    for (fam, mode), tiles in by.items():
        if fam == "f32":
            assert {hip.TILE_SHAPES[t] for t in tiles} >= {(128, 128), (64, 64), (64, 128)}
            continue
        waves = {_tile_grid(t)[2] * _tile_grid(t)[3] for t in tiles}
        assert waves == {4, 8}, (fam, mode, waves)
        if fam == "x3f32":
            assert hip.TILE_128x64_K2 in tiles  # two K-tiles per barrier
            continue
        assert hip.TILE_256x128_T42 in tiles and hip.TILE_128x256_T24 in tiles
        two_term = hip.MATH_PLANES[S.MODES[mode][0]] <= 2
        assert (hip.TILE_256x256_W8 in tiles) == two_term and (hip.TILE_192x256_W8 in tiles) == (two_term and fam == "row")
    sk = [L for L in S.group_a() if L["name"] == "a_sk" and L["family"] == "row"]
    assert {L["splitk"] for L in sk} == {2, 3}
    assert {S.row_kernel_runs(L) for L in sk if L["splitk"] == 3} == {True} and {S.row_kernel_runs(L) for L in sk if L["splitk"] == 2} == {False}


def test_n_limit_table():
    assert {n % 4 for n in S.N_LIMITS} == {0, 1, 2, 3} and 33 in S.N_LIMITS and set(S.N_LIMITS) == {3, 5, 20, 33, 55, 110}
    per_family = {}
    for L in S.group_d():
        per_family.setdefault(L["family"], set()).update(s["n_limit"] for s in L["segs"])
        assert all(s["n_limit"] and s["lo"] == "mixed" for s in L["segs"])
        assert len({s["n_limit"] for s in L["segs"]}) >= 3  # groups of different stored widths in one launch
    assert set().union(*per_family.values()) == set(S.N_LIMITS)
    for fam in ("f32", "pertap", "row"):
        assert per_family[fam] == set(S.N_LIMITS), fam
    narrow = {(L["family"], L["tile"]) for L in S.group_d() if L["name"] == "d_narrow"}
    assert narrow == {("f32", hip.TILE_128x32), ("pertap", hip.TILE_128x32_W4), ("row", hip.TILE_128x32_W4)}
    for fam in S.FAMILIES:
        cols = {None if L["tile"] is None else hip.TILE_SHAPES[L["tile"]][1] for L in S.group_d() if L["name"] == "d_wide" and L["family"] == fam}
        assert cols >= {64, 128, None}, (fam, cols)
        assert any(L["splitk"] == 2 for L in S.group_d() if L["family"] == fam)


@pytest.mark.parametrize("L", S.group_d(), ids=S.case_id)
def test_clamp_cases_sit_on_both_sides_of_lo(L):
    """Groups D: with and without the launch's relu, every channel with a finite lo' has 20 .. 80 % of its reference outputs below lo' by
    more than the bar and every other output above it by more than the bar -- a kernel that reads another channel's lo, or drops
    max(lo, 0), moves outputs by far more than the bar.  The lo vector of every segment mixes -inf, 0, a positive and a negative bound."""
    for relu in (False, True):
        Lr = dict(L, relu=relu)
        for i, s in enumerate(Lr["segs"]):
            n = s["n_limit"]
            lo_raw = S.seg_data(Lr, i)["lo"][:n]
            if n >= 4:
                assert {float(v) for v in lo_raw} == set(S.LO_CYCLE)
            ref, lo, y = S.reference(Lr, i)
            tol = S.bar(Lr, ref)
            finite = torch.isfinite(lo)
            assert bool(finite.any()) or n < 4
            assert torch.equal(finite, torch.isfinite(lo_raw) | torch.tensor(relu))
            below = (y < lo.view(1, -1, 1, 1) - tol)[:, finite]
            above = (y > lo.view(1, -1, 1, 1) + tol)[:, finite]
            assert bool((below | above).all()), (S.case_id(Lr), i, "an output within the bar of lo'")
            frac = below.float().mean((0, 2, 3))
            assert float(frac.min()) >= 0.2 and float(frac.max()) <= 0.8, (S.case_id(Lr), i, frac)


def test_in_relu_cases_need_the_rectifier():
    for L in S.group_e():
        assert L["in_relu"] and L["family"] == "x3f32" and (L["k"], L["pad"]) == (3, 1)
        for i, s in enumerate(L["segs"]):
            d = S.seg_data(L, i)
            assert float((d["x"] < 0).float().mean()) >= 0.6
            ref, _, _ = S.reference(L, i)
            plain, _, _ = S.reference(dict(L, in_relu=False), i)
            assert float((ref - plain).abs().max()) > 100 * S.bar(L, ref)
    assert {(L["stride"], len(L["segs"])) for L in S.group_e()} == {(2, 1), (2, 2), (1, 1), (1, 2)}
    assert all(s["H"] % 2 == 1 and s["W"] % 2 == 1 for L in S.group_e() if L["stride"] == 2 for s in L["segs"])


def test_range_guard_cases():
    """Group F: the baseline sits a factor of four inside the half range; in the raised launch ONLY the chosen channel of the chosen segment
    leaves it (all of that channel's values do); no output is clamped (relu 0, no lo)."""
    scale = 16.0  # PlanBase.act_scale's default, asserted on the GPU
    chans = set()
    for base, raised in S.group_f_overflow():
        assert base["mode"] == "f16x2" and not base["relu"] and all(s["lo"] is None and s["out"] in ("planes", "both") for s in base["segs"])
        si, ch, val = raised["raise_bias"]
        assert dict(raised, raise_bias=None) == base
        chans.add(ch)
        for i in range(len(base["segs"])):
            ref, lo, _ = S.reference(base, i)
            assert not bool(torch.isfinite(lo).any())
            assert float(ref.abs().max()) * scale < 65504.0 / 4
            hot, _, _ = S.reference(raised, i)
            over = (hot.abs() * scale > 65504.0)
            if i != si:
                assert not bool(over.any())
            else:
                assert bool(over[:, ch].all()) and int(over.sum()) == int(over[:, ch].sum())
    assert 90 in chans and 64 <= 90 < 96  # the last, partly filled, 64-column block of N = 96
    names = {L["name"] for L in S.group_f_amax()}
    assert names == {"f_amax_m3n5", "f_amax_multi", "f_amax_sk", "f_amax_randn", "f_amax_rowfb", "f_amax_colfb"}
    # the fallback of the reporting wave: an entry that ONLY a tile whose rotating wave holds no stored value reports into (an entry that a
    # full tile feeds as well would hide a reporting wave that stayed on rows >= M / columns >= N)
    for nm in ("f_amax_rowfb", "f_amax_colfb"):
        L = next(L for L in S.group_f_amax() if L["name"] == nm)
        feeders = S.amax_feeders(L, L["tile"])
        assert any(all(moved) for moved in feeders.values()), (nm, feeders)
        assert sorted(feeders) == S.amax_slots(L, *hip.TILE_SHAPES[L["tile"]]) and len(L["segs"]) > 1
    for L in S.group_f_amax():
        if L["data"] == "zero_w":
            for i in range(len(L["segs"])):
                ref, _, _ = S.reference(L, i)
                assert torch.all(ref == 1.5)
        if L["name"] == "f_amax_m3n5":
            assert [S.seg_m(L, s) for s in L["segs"]] == [3] and L["N"] == 5
    # one-row last tiles: the reporting wave of that tile (wave row seed % WM != 0) holds rows >= M only
    L = next(L for L in S.group_f_amax() if L["name"] == "f_amax_multi" and L["tile"] == hip.TILE_64x64_W4)
    assert 65 in [S.seg_m(L, s) for s in L["segs"]] and _tile_grid(L["tile"])[2] == 2
    assert S.amax_slots(L, 64, 64) == [0, 1, 2]


def test_group_b_and_c_shapes():
    for _, places in S.group_b():
        assert set(places) == {"alone", "first", "middle", "last"}
        tgt = [[s for s in L["segs"] if s["tag"] == "tgt"] for L in places.values()]
        assert all(len(t) == 1 and t[0] == tgt[0][0] for t in tgt)
        assert len(places["alone"]["segs"]) == 1 and all(len(places[p]["segs"]) == 4 for p in ("first", "middle", "last"))
        assert [places[p]["segs"].index(tgt[0][0]) for p in ("first", "middle", "last")] == [0, 2, 3]
        assert len({(L["tile"], L["splitk"], L["family"], L["mode"]) for L in places.values()}) == 1
    assert {p["alone"]["splitk"] for _, p in S.group_b()} == {1, 3}
    for L in S.group_c():
        assert {s["res"] for s in L["segs"]} == {None, "f32", "planes", "planes_up"} and {s["out"] for s in L["segs"]} == {"f32", "planes", "both"}
    assert {L["N"] for L in S.group_c()} == {64, 96, 160} and {L["tile"] for L in S.group_c()} == {hip.TILE_128x64_W4, None}


def test_every_launch_is_one_convop_accepts(hiplib):
    """Every (family, mode, tile, splitk) the tables name, built as a dry-run ConvOp: the kernel family is the one the case says, the
    forced tile and split-K are kept (no silent substitution), and the library's own restrictions hold: the 8-wave 256-column tiles carry
    no residual, no split-K and exist for the one- and two-term modes, 192 x 256 for the row-shared kernel only."""
    from dd3d_amd.engine.tiling import MATH_TILES, PLANE_TILES
    ids = set()
    launches = S.all_launches() + [dict(L, relu=True) for L in S.group_d()]
    for L in launches:
        R = S.build(L, device="cpu", dry_run=True)
        op, math = R.op, S.math_of(L)
        planes = L["family"] in S.PLANE_FAMILIES
        assert op.math == math and op.in_planes == planes, S.case_id(L)
        if L["tile"] is not None:
            assert L["tile"] in (PLANE_TILES if planes else MATH_TILES[math])
            assert op.info["tile_name"] == hip.TILE_NAMES[L["tile"]] and op.info["splitk"] == L["splitk"], (S.case_id(L), op.info)
        if op.L.tile_cfg in S.W8_TILES:
            assert hip.MATH_PLANES[math] <= 2 and op.L.splitk == 1 and all(s["res"] is None for s in L["segs"]), S.case_id(L)
        if op.L.tile_cfg == hip.TILE_192x256_W8:
            assert L["family"] == "row" and S.row_kernel_runs(L)
        assert op.res_forms == [s["res"] for s in L["segs"]], (S.case_id(L), op.res_forms)
        want_forms = [(s["out"] if planes and not s["n_limit"] else "f32") for s in L["segs"]]
        assert op.out_forms == [(f != "planes", f != "f32") for f in want_forms], (S.case_id(L), op.out_forms)
        assert op.L.nsegs == len(L["segs"]) and op.L.ntiles == sum(-(-S.seg_m(L, s) // op.info["tile"][0]) for s in L["segs"])
        ids.add((S.case_id(L), L["relu"], L["raise_bias"]))
    assert len(ids) == len(launches)  # no case is a duplicate of another


def test_reference_agrees_with_the_plan_emulator(hiplib):
    """The float64 statement against tests/plan_emulator.py, which states the same contract from op.desc (a cross-check of the two
    statements, one launch per group that the emulator can express: f32 residuals, lo, n_limit, in_relu)."""
    from tests.plan_emulator import emulate
    picks = [next(L for L in S.group_a() if L["family"] == "f32"), dict(next(L for L in S.group_d() if L["family"] == "row" and L["name"] == "d_wide"), relu=True),
             S.group_e()[1]]
    for L in picks:
        R = S.build(L, device="cpu", dry_run=True)
        emulate(R.plan)
        for i, (yb, vout, n, form) in enumerate(R.outs):
            ref, _, _ = S.reference(L, i)
            got = yb.t[..., vout.c0:vout.c0 + n].permute(0, 3, 1, 2).double()
            assert float((got - ref).abs().max()) <= 2e-5 * max(1.0, float(ref.abs().max())), (S.case_id(L), i)
