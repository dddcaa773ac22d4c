"""dd3d_conv2d_igemm_f32 at its seam, through ConvOp / PlanBase as the model drives it, on the paths the single-segment tests of
test_conv_gpu.py / test_conv_planes_gpu.py never reach: the device-side tile table and segment descriptors (a single-segment ConvOp
launch carries its descriptor by value and computes m0 = mt * BM), forced tiles and split-K with many unequal segments, residual and
output forms mixed inside one launch, and the epilogue options of the predictors and of LastLevelP6P7 -- `lo`, `n_limit`, `in_relu` --
plus the half-range guard raised by the convolution epilogue (overflow bit, sampled maxima).

Reference: tests/conv_seam_cases.py::reference, float64 on the CPU, per segment.  Bars: the project's per-mode bars
(test_conv_planes_gpu.py::MODES, 2e-5 for the f32-input kernels, plus the output rounding step for a value read back from planes), applied
PER SEGMENT relative to max(1, max |ref|) of that segment; where the reference is below the clamp lo' by more than the bar the output
must equal lo' bit for bit.  tests/test_conv_seam_cases.py shows without a GPU that the tables reach the edges they name.

The largest error seen per group, kernel family and mode is printed at the end of the module (and written to the file
DD3D_SEAM_ERRORS_OUT names: profiles/conv_seam_errors.txt is such a run)."""
import os

import pytest
import torch

from dd3d_amd import hip
from tests import conv_seam_cases as S

pytestmark = pytest.mark.gpu

ERRORS = {}  # (group, family, mode, storage) -> [largest err / max(1, max |ref|), its bar (relative)]


@pytest.fixture(scope="module", autouse=True)
def _error_report():
    yield
    lines = ["# tests/test_conv_seam_gpu.py: largest |got - float64 ref| / max(1, max |ref|) per segment, and the bar it is held to",
             "# group family mode storage max_rel_err bar"]
    lines += [f"{g} {f} {m} {st} {e:.3e} {b:.3e}" for (g, f, m, st), (e, b) in sorted(ERRORS.items())]
    print("\n" + "\n".join(lines))
    path = os.environ.get("DD3D_SEAM_ERRORS_OUT")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def _run(L, monkeypatch, launches=None):
    """Build launch L, run it (twice with split-K: the arrival counters must be zero again after every launch)."""
    monkeypatch.setenv("DD3D_CONV_ROW", "1" if L["family"] == "row" else "0")
    R = S.build(L)
    op = R.op
    assert op.math == S.math_of(L) and op.in_planes == (L["family"] in S.PLANE_FAMILIES), op.info
    if L["tile"] is not None:  # no silent substitution: the case runs the tile and split-K it names
        assert op.info["tile_name"] == hip.TILE_NAMES[L["tile"]] and op.info["splitk"] == L["splitk"], (S.case_id(L), op.info)
    assert op.info["nsegs"] == len(L["segs"])
    for _ in range(launches or (2 if op.info["splitk"] > 1 else 1)):
        R.plan.launch()
        torch.cuda.synchronize()
        if op.counters is not None:
            assert int(op.counters.abs().sum()) == 0, (S.case_id(L), "split-K arrival counters not back at zero")
    return R


def _stored(R, i):
    """{storage: [B, n, Ho, Wo] value} of segment i, after checking the sentinels around its slice."""
    yb, vout, n, form = R.outs[i]
    what = f"{S.case_id(R.L)} segment {i} ({R.L['segs'][i]['tag']})"
    out = {}
    if form != "planes":
        t = yb.t.cpu()
        out["f32"] = t[..., vout.c0:vout.c0 + n].permute(0, 3, 1, 2)
        assert torch.all(t[..., :vout.c0] == S.SENT_F32), what + ": f32 channels before the slice written"
        assert torch.all(t[..., vout.c0 + n:] == S.SENT_F32), what + ": f32 channels past the last stored one written"
    if form != "f32":
        p = yb.p.cpu()
        k0, k1 = vout.c0 // 32, (vout.c0 + S.pad32(n)) // 32
        assert torch.all(p[:k0] == S.SENT_PLANE) and torch.all(p[k1:] == S.SENT_PLANE), what + ": plane chunks outside the slice written"
        dec = S.decode_planes(p[k0:k1], yb.f16, yb.plane_scale).view(yb.B, yb.H, yb.W, -1).permute(0, 3, 1, 2)
        assert torch.all(dec[:, n:] == 0), what + ": channels past N inside the last chunk are not zero planes"
        out["planes"] = dec[:, :n]
    return out


def _residual_value(R, i):
    """What the kernel adds: the generated f32 map, or -- for a plane residual -- the value the source's planes hold."""
    s, rb = R.L["segs"][i], R.ress[i]
    if s["res"] in (None, "f32"):
        return None
    cp = S.pad32(R.L["N"])
    dec = S.decode_planes(rb.p[1:1 + cp // 32].cpu(), rb.f16, rb.plane_scale)
    return dec.view(rb.B, rb.H, rb.W, cp).permute(0, 3, 1, 2)[:, :R.L["N"]]


def _check(R, group, storages=("f32", "planes")):
    L = R.L
    for i, s in enumerate(L["segs"]):
        what = f"{S.case_id(L)} relu={int(L['relu'])} segment {i} ({s['tag']}, M={S.seg_m(L, s)}, n_limit={s['n_limit']}, res={s['res']})"
        ref, lo, y = S.reference(L, i, _residual_value(R, i))
        for st, got in _stored(R, i).items():
            if st not in storages:
                continue
            tol = S.bar(L, ref, planes_only=st == "planes")
            scale = max(1.0, float(ref.abs().max()))
            err = float((got.double() - ref).abs().max())
            key = (group, L["family"], L["mode"] or "-", st)
            if key not in ERRORS or err / scale > ERRORS[key][0]:
                ERRORS[key] = [err / scale, tol / scale]
            print(f"{what} {st}: max abs err {err:.3e} (bar {tol:.3e})")
            assert err <= tol, f"{what} {st}: max abs err {err:.3e} > {tol:.3e} (info {R.op.info})"
            clamped = (y < lo.view(1, -1, 1, 1) - tol)
            want = lo.float().view(1, -1, 1, 1).expand_as(got)
            if st == "f32":  # bit for bit
                same = got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)
            else:  # (0 and +-0.25 are exact in every plane format)
                same = got == want
            assert bool(same[clamped].all()), f"{what} {st}: an output whose reference is below lo' by more than the bar is not lo' exactly"
    for arena in (R.arena_t, R.arena_p):
        if arena is not None:
            mem, guard = arena
            sent = S.SENT_F32 if mem.dtype == torch.float32 else S.SENT_PLANE
            assert bool((mem.cpu()[guard] == sent).all()), f"{S.case_id(L)}: a guard frame between / after the segments' output storages was written"


# ------------------------------------------------------------------------------------------------ A
@pytest.mark.parametrize("L", S.group_a(), ids=S.case_id)
def test_many_unequal_segments_through_the_tile_table(hiplib, L, monkeypatch):
    """One launch, >= 5 segments of unequal size (1 x 3, BM - 1, BM, BM + 1 pixels, three tiny images), forced tile, per-segment scale /
    bias, two filters: every segment matches, sentinels and guard frames intact.  Variations: split-K 2 / 3 (counters zero after each of
    two launches), 1 x 1, 3 x 3 / stride 2 on odd maps."""
    _check(_run(L, monkeypatch), "A")


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize("places", [p for _, p in S.group_b()], ids=[n for n, _ in S.group_b()])
def test_a_segment_does_not_depend_on_its_company(hiplib, places, monkeypatch):
    """The same segment alone (descriptor by value, m0 = mt * BM) and first / in the middle / last of a four-segment launch (descriptor
    and tile origin read from device memory), same tile and split-K: bit-identical f32 and plane storages.  Tile origins and the K order
    are the same, and the split-K slices are summed in slice order by the last arriver."""
    raw = {}
    for place, L in places.items():
        R = _run(L, monkeypatch)
        _check(R, "B")
        i = [s["tag"] for s in L["segs"]].index("tgt")
        yb = R.outs[i][0]
        raw[place] = (yb.t.cpu().clone(), None if yb.p is None else yb.p.cpu().clone())
    for place in ("first", "middle", "last"):
        assert torch.equal(raw[place][0].view(torch.int32), raw["alone"][0].view(torch.int32)), f"f32 output differs: alone vs {place}"
        if raw["alone"][1] is not None:
            assert torch.equal(raw[place][1], raw["alone"][1]), f"plane output differs: alone vs {place}"


# ------------------------------------------------------------------------------------------------ C
@pytest.mark.parametrize("L", S.group_c(), ids=S.case_id)
def test_mixed_residual_and_output_forms_in_one_launch(hiplib, L, monkeypatch):
    """No residual, an f32 residual (a 32-aligned slice, res_pitch > channels), a same-pixel plane residual and a half-resolution plane
    residual, with f32-only / planes-only / both outputs, in ONE launch of the split-plane kernels; Cout 64, 96, 160."""
    R = _run(L, monkeypatch)
    assert R.op.res_forms == [s["res"] for s in L["segs"]]
    _check(R, "C")
    assert int(R.plan.status.cpu()) == 0


# ------------------------------------------------------------------------------------------------ D
@pytest.mark.parametrize("L", S.group_d(), ids=S.case_id)
def test_lo_relu_and_n_limit(hiplib, L, monkeypatch):
    """The predictor launches (forward.py::_heads): groups of different stored widths zero-padded to one N, n_limit per segment, a lo
    vector mixing -inf / 0 / +0.25 / -0.25, with the launch's relu off and on (lo' = max(lo, 0)); channels [n_limit, pitch) of the
    output rows keep their sentinel."""
    for relu in (False, True):
        _check(_run(dict(L, relu=relu), monkeypatch), "D")


# ------------------------------------------------------------------------------------------------ E
@pytest.mark.parametrize("L", S.group_e(), ids=S.case_id)
def test_in_relu(hiplib, L, monkeypatch):
    """dd3d_conv_launch.in_relu: conv2d(relu(x)) on a mostly negative input, which stays as it was."""
    R = _run(L, monkeypatch)
    assert R.op.L.in_relu == 1
    _check(R, "E")
    for i, xin in enumerate(R.ins):
        t = xin.t.cpu()
        assert torch.equal(t[..., 4:4 + L["Cin"]], R.data[i]["x"].permute(0, 2, 3, 1)) and torch.all(t[..., :4] == 0) and torch.all(t[..., 4 + L["Cin"]:] == 0)


# ------------------------------------------------------------------------------------------------ F
@pytest.mark.parametrize("pair", S.group_f_overflow(), ids=lambda p: S.case_id(p[1]) + f"-ch{p[1]['raise_bias'][1]}")
def test_conv_epilogue_raises_the_overflow_bit(hiplib, pair, monkeypatch):
    """DD3D_MATH_F16X2, plane outputs: inside the half range the status word stays 0; ONE bias entry raised so that one channel's scaled
    values pass 65504 sets DD3D_STATUS_F16_OVERFLOW, and the f32 output is still right."""
    base, raised = pair
    R = _run(base, monkeypatch)
    assert R.plan.act_scale == 16.0
    assert int(R.plan.status.cpu()) == 0
    _check(R, "F")
    R = _run(raised, monkeypatch)
    assert int(R.plan.status.cpu()) & hip.STATUS_F16_OVERFLOW
    si, ch, _ = raised["raise_bias"]
    for i in range(len(raised["segs"])):
        ref, _, _ = S.reference(raised, i)
        got = _stored_f32_only(R, i)
        if got is None:
            continue
        keep = [c for c in range(raised["N"]) if not (i == si and c == ch)]
        for chans in (keep, [ch] if i == si else []):  # the raised channel at its own magnitude, the others at theirs
            if chans:
                err = float((got[:, chans].double() - ref[:, chans]).abs().max())
                assert err <= S.bar(raised, ref[:, chans]), (S.case_id(raised), i, chans[:1], err)
    R.plan.status.zero_()


def _stored_f32_only(R, i):
    yb, vout, n, form = R.outs[i]
    return None if form == "planes" else yb.t[..., vout.c0:vout.c0 + n].permute(0, 3, 1, 2).cpu()


@pytest.mark.parametrize("L", S.group_f_amax(), ids=S.case_id)
def test_conv_epilogue_samples_the_largest_stored_value(hiplib, L, monkeypatch):
    """dd3d_conv_launch.amax, a [16][32] float array: only entries amax[32 j] change.  With zero filters and bias 1.5 every stored value is
    1.5, so every tile's reporting wave reports exactly 1.5 x plane scale into entry (m0 / BM + n0 / BN) & 15 -- also the tiles whose
    rotating reporting wave would sit on rows >= M (a one-row last tile; the single tile of an M = 3, N = 5 launch) -- and no other entry
    moves.  With real data: 0 < max <= max |stored value| x plane scale.  ConvOp points the launch at the slot it takes from the plan."""
    monkeypatch.setenv("DD3D_CONV_ROW", "1" if L["family"] == "row" else "0")
    R = S.build(L)
    plan, op = R.plan, R.op
    assert plan.amax_names == [L["name"]] and op.L.amax == plan.amax[0].data_ptr() and plan.act_scale == 16.0
    plan.amax.zero_()  # (the plan's own start-of-forward zeroing)
    plan.amax[0, :, 1:] = S.SENT_F32
    for _ in range(2 if op.info["splitk"] > 1 else 1):
        plan.launch()
        torch.cuda.synchronize()
    a = plan.amax.cpu()
    assert torch.all(a[0, :, 1:] == S.SENT_F32) and torch.all(a[1:] == 0), "an entry other than amax[32 j] of the launch's own slot changed"
    vals = a[0, :, 0]
    assert float(plan.amax_values()[0]) == float(vals.max()) > 0
    if L["tile"] is not None:
        assert op.info["tile_name"] == hip.TILE_NAMES[L["tile"]] and op.info["splitk"] == L["splitk"]
    if L["data"] == "zero_w":
        want = torch.zeros(16)
        want[S.amax_slots(L, *op.info["tile"])] = 1.5 * plan.act_scale
        assert torch.equal(vals, want), (S.case_id(L), vals, want)
    else:
        stored = max(float(_stored_f32_only(R, i).abs().max()) for i in range(len(L["segs"])))
        assert 0 < float(vals.max()) <= stored * plan.act_scale
    assert int(plan.status.cpu()) == 0
    _check(R, "F")
