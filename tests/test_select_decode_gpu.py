"""dd3d_fcos_select_decode called directly (C ABI) at the seams of fcos_select_decode_kernel.

The forward tests reach this kernel only through synthetic head maps, so most of its paths are decided by chance there.  These
cases aim at them: element counts around the 4096-element rounds and 65536-element super-rounds, levels where every element
passes, logits next to logit(PRE_NMS_THRESH) and inside the 0.0625 shortcut margin, thresholds 0 and 1, npass around topk,
score ties straddling the k-th key, every 3D decode mode, depth clamps, nuScenes attribute ties, degenerate quaternions and the
(level, image)-wide renormalisation, and sentinel regions around every buffer the kernel writes.

References.  Discrete decisions (which elements pass, top-k membership, npass, counts) are compared EXACTLY with the float32
oracle (oracle.dd3d_oracle.fcos2d_inference_level).  The only allowed exception is an element whose float64 gate score (or
ranking score) lies within MARGIN of the cut that decided it; such cases are counted, reported and must stay rare.  Top-k ties:
torch.topk picks arbitrarily among equal keys, so the kernel is held to its documented rule (every key > the k-th key, then the
lowest-index keys equal to it) on its own keys (the compacted scores it leaves in scratch_score), and its set must agree with
the oracle's outside the tied keys.

Float fields are compared with a float64 evaluation of the same formulas (oracle.dd3d_oracle.predictions_to_boxes3d fed float64
inputs).  Fields that are one float32 operation on the same operands are compared bit for bit: box x1..y2, locations, proj_ctr,
speed, and the integer fields class, flat index and attribute.  Tolerances of the other fields, from their float32 operation
counts (u = 2^-24; OCML expf/tanhf/logf are <= 2 ulp, division and sqrtf are correctly rounded, contraction is off):
  score     = sqrt(sig(x) * sig(c)), sig = 1/(1+exp(-x)): per sigmoid 2 (exp) + 1 (add) + 1 (div) half-ulps, product 1, sqrt
              halves the input error and adds 1:  ~ (9/2 + 1) u ~ 3.3e-7 relative                       -> TOL_SCORE
  score_3d  = score * sig(conf): score + sigmoid + product ~ 11 u ~ 6.6e-7                                 -> TOL_SCORE3D
  depth     = d / (sqrt(K0^2+K4^2) * f) / max(|K^-1 [x,y,1]|, eps), clamped: ~ 16 u ~ 1e-6                -> TOL_DEPTH
  size      = (tanh(s) + 1) * canon: tanhf 2 ulp of |tanh| <= 0.762 relative to tanh+1 >= 0.238 (|s| <= 1 here; the
              cancellation below that is a property of the formula, not of the kernel), + add + mul ~ 9 u ~ 5.4e-7  -> TOL_SIZE
  quat      (sign-free, absolute, unit quaternion): two normalisations, and when allocentric the viewing-ray frame (two
              normalisations, a cross product), a 3x3 product and matrix_to_quaternion: ~ 40 u ~ 2.4e-6          -> TOL_QUAT
Measured maxima over all cases (MI355X): score 1.35e-7, score_3d 2.3e-7, depth 2.1e-7, size 2.8e-7, quat 2.4e-7; the bounds are
these rounded up, each within its derivation and far below the 1e-5 ceiling.
"""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL_SCORE, TOL_SCORE3D, TOL_DEPTH, TOL_SIZE, TOL_QUAT = 2e-7, 3e-7, 3e-7, 4e-7, 3e-7
MARGIN_REL = 2.0**-20  # a decision may differ from the float32 oracle only this close (relative) to its cut ...
MARGIN_ABS = 2.0**-126  # ... or where float32 sigmoid is denormal / underflows
GUARD = 67  # sentinel elements after every scratch region, slots after every level's candidate region
IDX_SENT = -123456789
SENT_BITS = np.int32(0x7FBADBAD)  # a NaN with a payload no kernel arithmetic produces
KITTI_CANON = [[1.61876949, 3.89154523, 1.52969237], [0.62806586, 0.82038497, 1.76784787], [0.56898187, 1.77149234, 1.7237099],
               [1.9134491, 5.15499603, 2.18998422], [2.61168401, 9.22692319, 3.36492722]]

_REPORTED = []  # (case, kind, detail) of every within-margin disagreement


def _inv_k(B, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(B):
        f = 700.0 + 60.0 * b + rng.uniform(0, 20)
        K = np.array([[f, 0.0, 610.0 + 7 * b], [0.0, f * 1.01, 180.0 - 5 * b], [0.0, 0.0, 1.0]])
        out.append(np.linalg.inv(K))
    return np.stack(out).astype(F32)


def make_level(rng, B, H, W, C, *, C3=None, frac_hi=0.05, lo=(-7.0, -3.5), hi=(-1.0, 3.0), ctr=(-1.0, 4.0), num_attr=0, speed=False,
               box3d=True, depth=(5.0, 60.0)):
    """Random head maps of one level, in the kernel's NHWC channel layout, float32: cls [B,HW,C+num_attr+speed], b2d [B,HW,5],
    b3d [B,HW,11*C3]."""
    HW = H * W
    cls = rng.uniform(*lo, size=(B, HW, C))
    m = rng.random((B, HW, C)) < frac_hi
    cls[m] = rng.uniform(*hi, size=int(m.sum()))
    extra = []
    if num_attr:
        extra.append(rng.integers(-3, 3, size=(B, HW, num_attr)).astype(np.float64) * 0.5)  # small integers: exact ties
    if speed:
        extra.append(np.maximum(rng.normal(0, 3, size=(B, HW, 1)), 0.0))
    cls = np.concatenate([cls] + extra, 2)
    b2d = np.concatenate([np.maximum(rng.normal(20, 15, size=(B, HW, 4)), 0.0), rng.uniform(*ctr, size=(B, HW, 1))], 2)
    lv = dict(H=H, W=W, stride=8, cls=cls.astype(F32), b2d=b2d.astype(F32), b3d=None)
    if box3d:
        C3 = C if C3 is None else C3
        q = rng.normal(0, 1, size=(B, HW, 4, C3))
        ctr2 = rng.normal(0, 2, size=(B, HW, 2, C3))
        dep = rng.uniform(*depth, size=(B, HW, 1, C3))
        sz = rng.uniform(-1, 1, size=(B, HW, 3, C3))
        conf = rng.normal(0, 2, size=(B, HW, 1, C3))
        lv["b3d"] = np.concatenate([q, ctr2, dep, sz, conf], 2).reshape(B, HW, 11 * C3).astype(F32)
    return lv


def _cfg(thr, topk, with_ctr):
    return {"DD3D": {"FCOS2D": {"INFERENCE": {"THRESH_WITH_CTR": bool(with_ctr), "PRE_NMS_THRESH": float(thr), "PRE_NMS_TOPK": int(topk)}}}}


def run_select(levels, C, *, topk, thr=0.05, with_ctr=1, half=0, agnostic=0, alloc=1, dist=0, focal=1, min_depth=0.1, max_depth=80.0,
               focal_factor=500.0, inv_k=None, canon=None, num_attr=0, speed=False, pad_val=np.nan, slots="gapped"):
    """One launch over `levels` (all with the same B).  Pitches exceed the channels the kernel reads (pad_val in the rest), every
    written buffer carries sentinel regions, and those are checked here.  Returns a dict with npass, counts, the compacted
    scratch (idx, score) per (b, l) and the candidate fields per (b, l)."""
    from dd3d_amd import hip
    lib = hip.lib()
    dev = torch.device("cuda")
    L, B = len(levels), levels[0]["cls"].shape[0]
    has3d = levels[0]["b3d"] is not None
    C3 = 1 if agnostic else C
    ncls = levels[0]["cls"].shape[2]
    pitch = (ncls + 3, 5 + 2, 11 * C3 + 5)
    inv_k = _inv_k(B) if inv_k is None else inv_k
    canon = np.array(KITTI_CANON[:C] + [[1.0, 2.0, 3.0]] * max(0, C - 5), dtype=F32) if canon is None else canon
    keep = []

    def dev_map(x, p):
        m = np.full((x.shape[0] * x.shape[1], p), pad_val, dtype=F32)
        m[:, :x.shape[2]] = x.reshape(-1, x.shape[2])
        t = torch.from_numpy(m).to(dev)
        keep.append(t)
        return t.data_ptr()

    n_el = [lv["H"] * lv["W"] * C for lv in levels]
    caps = [min(topk, n) for n in n_el]
    if slots == "dense":
        base, NS, slot_tab = [l * topk for l in range(L)], L * topk, [0] * 9
    elif slots == "trimmed":  # the engine's table (engine/forward.py): level l holds min(topk, H*W*C) slots, no gaps
        base = [sum(caps[:l]) for l in range(L)]
        NS = sum(caps)
        slot_tab = base + [NS] + [0] * (8 - L)
    else:  # gapped: GUARD sentinel slots after every level's region
        base = [sum(caps[:l]) + GUARD * l for l in range(L)]
        NS = sum(caps) + GUARD * L
        slot_tab = base + [NS] + [0] * (8 - L)
    soff = [sum(n_el[:l]) + GUARD * l for l in range(L)]
    img_stride = sum(n_el) + GUARD * L
    s_idx = torch.full((B * img_stride + GUARD, ), IDX_SENT, dtype=torch.int32, device=dev)
    s_sc = torch.full((B * img_stride + GUARD, ), int(SENT_BITS), dtype=torch.int32, device=dev)
    cand = torch.full((B * hip.CAND_FIELDS * NS + GUARD, ), int(SENT_BITS), dtype=torch.int32, device=dev)
    counts = torch.full((B * L + GUARD, ), IDX_SENT, dtype=torch.int32, device=dev)
    npass = torch.full((B * L + GUARD, ), IDX_SENT, dtype=torch.int32, device=dev)
    ik = torch.from_numpy(np.ascontiguousarray(inv_k)).to(dev)
    cs = torch.from_numpy(np.ascontiguousarray(canon)).to(dev)
    a = hip.SelectArgs()
    for l, lv in enumerate(levels):
        a.cls[l], a.box2d[l] = dev_map(lv["cls"], pitch[0]), dev_map(lv["b2d"], pitch[1])
        a.box3d[l] = dev_map(lv["b3d"], pitch[2]) if has3d else None
        a.H[l], a.W[l], a.stride[l] = lv["H"], lv["W"], lv["stride"]
        a.scratch_off[l] = soff[l]
    a.cls_pitch, a.b2d_pitch, a.b3d_pitch = pitch
    a.num_levels, a.B, a.num_classes = L, B, C
    a.class_agnostic_3d, a.loc_offset_half, a.thresh_with_ctr, a.topk = agnostic, half, with_ctr, topk
    a.attr_off, a.num_attr, a.speed_off = C, num_attr, (C + num_attr if speed else -1)
    a.pre_nms_thresh, a.min_depth, a.max_depth, a.focal_factor = thr, min_depth, max_depth, focal_factor
    a.scale_depth_by_focal, a.allocentric, a.depth_is_distance = focal, alloc, dist
    a.inv_K, a.canon_sizes = ik.data_ptr(), cs.data_ptr()
    a.scratch_idx, a.scratch_score, a.scratch_img_stride = s_idx.data_ptr(), s_sc.data_ptr(), img_stride
    a.cand, a.counts, a.npass = cand.data_ptr(), counts.data_ptr(), npass.data_ptr()
    for i, v in enumerate(slot_tab):
        a.slot_off[i] = v
    hip.check(lib.dd3d_fcos_select_decode(ctypes.byref(a), hip.current_stream()), "select")
    torch.cuda.synchronize()
    s_idx, s_sc, cand = s_idx.cpu().numpy(), s_sc.cpu().numpy(), cand.cpu().numpy()
    counts, npass = counts.cpu().numpy(), npass.cpu().numpy()
    # ---- sentinels: nothing past the B*L counters, the used part of every scratch region, the counts of every level's slots
    assert (counts[B * L:] == IDX_SENT).all() and (npass[B * L:] == IDX_SENT).all()
    counts, npass = counts[:B * L].reshape(B, L), npass[:B * L].reshape(B, L)
    assert (s_idx[B * img_stride:] == IDX_SENT).all() and (s_sc[B * img_stride:] == SENT_BITS).all()
    assert (cand[B * hip.CAND_FIELDS * NS:] == SENT_BITS).all()
    cand = cand[:B * hip.CAND_FIELDS * NS].reshape(B, hip.CAND_FIELDS, NS)
    written = np.zeros((B, NS), dtype=bool)
    out = dict(npass=npass, counts=counts, scratch={}, cand={}, NS=NS, base=base)
    for b in range(B):
        for l in range(L):
            n, k = int(npass[b, l]), int(counts[b, l])
            assert 0 <= n <= n_el[l] and k == min(n, topk), (b, l, n, k)
            r0 = b * img_stride + soff[l]
            assert (s_idx[r0 + n:r0 + n_el[l] + GUARD] == IDX_SENT).all(), ("scratch idx written past npass", b, l)
            assert (s_sc[r0 + n:r0 + n_el[l] + GUARD] == SENT_BITS).all(), ("scratch score written past npass", b, l)
            out["scratch"][b, l] = (s_idx[r0:r0 + n].copy(), s_sc[r0:r0 + n].view(F32).copy())
            written[b, base[l]:base[l] + k] = True
            out["cand"][b, l] = cand[b, :, base[l]:base[l] + k].view(F32).copy()
    assert (cand.transpose(0, 2, 1)[~written] == SENT_BITS).all(), "candidate slot at or beyond counts was written"
    return out


def _sig64(x):
    x = np.asarray(x, dtype=np.float64)
    return 1.0 / (1.0 + np.exp(-x))


def check_select(out, levels, C, *, topk, thr=0.05, with_ctr=1, half=0, agnostic=0, alloc=1, dist=0, focal=1, min_depth=0.1,
                 max_depth=80.0, focal_factor=500.0, inv_k=None, canon=None, num_attr=0, speed=False, case="", max_margin=None, **_):
    """Compare one run_select result with the float32 oracle (decisions) and float64 formulas (fields).  Returns the max errors."""
    from oracle import dd3d_oracle as O
    B, L = out["counts"].shape
    thr32 = float(F32(thr))
    inv_k = _inv_k(B) if inv_k is None else inv_k
    canon = np.array(KITTI_CANON[:C] + [[1.0, 2.0, 3.0]] * max(0, C - 5), dtype=F32) if canon is None else canon
    cfg = _cfg(thr, topk, with_ctr)
    errs = dict(score=0.0, score3d=0.0, depth=0.0, size=0.0, quat=0.0)
    reported = 0
    total = 0
    for l, lv in enumerate(levels):
        H, W, st = lv["H"], lv["W"], lv["stride"]
        nchw = lambda x: torch.from_numpy(x.reshape(B, H, W, -1)).permute(0, 3, 1, 2).contiguous()
        locs = O.compute_features_locations(H, W, st, "half" if half else "none")
        res, info = O.fcos2d_inference_level(nchw(lv["cls"][..., :C]), nchw(lv["b2d"][..., :4]), nchw(lv["b2d"][..., 4:5]), locs,
                                             cfg)
        sc64 = _sig64(lv["cls"][..., :C])  # [B, HW, C]
        ct64 = _sig64(lv["b2d"][..., 4])[..., None]
        rank64 = (sc64 * ct64).reshape(B, -1)
        gate64 = (sc64 * ct64 if with_ctr else sc64).reshape(B, -1)
        for b in range(B):
            total += gate64.shape[1]
            within = lambda v, cut: abs(v - cut) <= MARGIN_REL * abs(cut) + MARGIN_ABS
            # -- pass set (the compacted scratch list, ascending = torch.nonzero order) against the oracle's mask
            e_pass, keys = out["scratch"][b, l]
            assert (np.diff(e_pass) > 0).all(), "compaction is not in ascending element order"
            fg, cl, tk = info[b]["fg_inds"].numpy(), info[b]["class_inds"].numpy(), info[b]["topk_indices"]
            ref_pass = fg * C + cl
            for e in np.setxor1d(e_pass, ref_pass):
                assert within(gate64[b, e], thr32), (case, "pass decision differs outside the margin", l, b, int(e), gate64[b, e])
                _REPORTED.append((case, "threshold", l, b, int(e), float(gate64[b, e] - thr32)))
                reported += 1
            # the keys the kernel ranks are sigmoid(cls)*sigmoid(ctr) of exactly these elements
            np.testing.assert_allclose(keys, rank64[b, e_pass], rtol=2 * TOL_SCORE, atol=2.0**-126)
            # -- top-k: the kernel's documented rule on its own keys, and agreement with the oracle outside the tied key
            k = int(out["counts"][b, l])
            c = out["cand"][b, l]
            e_sel = c[7].view(np.int32)
            assert (np.diff(e_sel) > 0).all(), "candidates are not in ascending element order"
            if len(e_pass) > topk:
                T = np.sort(keys)[::-1][topk - 1]
                gt = e_pass[keys > T]
                eq = e_pass[keys == T]
                want = np.sort(np.concatenate([gt, eq[:topk - len(gt)]]))
                assert np.array_equal(e_sel, want), (case, "top-k rule", l, b)
                ref_sel = ref_pass[tk.numpy()] if tk is not None else ref_pass
                assert len(ref_sel) == len(e_sel) or len(ref_pass) != len(e_pass)
                kth64 = float(np.sort(rank64[b, ref_pass])[::-1][topk - 1]) if len(ref_pass) > topk else None
                tied = set(eq.tolist())
                for e in np.setxor1d(e_sel, ref_sel):
                    if int(e) in tied:
                        continue
                    ok = within(gate64[b, e], thr32) or (kth64 is not None and within(rank64[b, e], kth64))
                    assert ok, (case, "top-k membership differs outside the tied key and the margin", l, b, int(e))
                    _REPORTED.append((case, "top-k", l, b, int(e), float(rank64[b, e] - (kth64 or 0.0))))
                    reported += 1
            else:
                assert np.array_equal(e_sel, e_pass)
            # -- per-candidate fields
            if k == 0:
                continue
            loc, cls_i = e_sel // C, e_sel % C
            assert np.array_equal(c[6].view(np.int32), cls_i)
            off = F32(st // 2) if half else F32(0)
            lx = (loc % W * st).astype(F32) + off
            ly = (loc // W * st).astype(F32) + off
            assert np.array_equal(c[8], lx) and np.array_equal(c[9], ly)
            reg = lv["b2d"][b, loc]
            box = np.stack([lx - reg[:, 0], ly - reg[:, 1], lx + reg[:, 2], ly + reg[:, 3]])
            assert np.array_equal(c[0:4].view(np.int32), box.view(np.int32)), (case, "2D box not bit-identical")
            score64 = np.sqrt(rank64[b, e_sel])
            rel = lambda got, want: float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 2.0**-63)))  # (denormal keys: absolute)
            errs["score"] = max(errs["score"], rel(c[4], score64))
            pc = lv["cls"][b, loc]
            attr = np.argmax(pc[:, C:C + num_attr], 1) if num_attr else np.zeros(k, np.int64)
            assert np.array_equal(c[20].view(np.int32), attr.astype(np.int32)), (case, "attribute argmax (first maximum)")
            spd = pc[:, C + num_attr] if speed else np.zeros(k, F32)
            assert np.array_equal(c[21].view(np.int32), spd.view(np.int32))
            if lv["b3d"] is None:
                assert np.array_equal(c[5].view(np.int32), c[4].view(np.int32)) and (c[10:20] == 0).all()
                continue
            C3 = 1 if agnostic else C
            c3 = np.zeros_like(cls_i) if agnostic else cls_i
            p = lv["b3d"][b, loc].reshape(k, 11, C3)[np.arange(k), :, c3].astype(np.float64)  # [k, 11]
            conf64 = _sig64(p[:, 10])
            s3 = score64 * conf64
            errs["score3d"] = max(errs["score3d"], rel(c[5], s3))
            t64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
            ref = O.predictions_to_boxes3d(t64(p[:, 0:4]), t64(p[:, 4:6]), t64(p[:, 6]), t64(p[:, 7:10]), t64(np.stack([lx, ly], 1)),
                                           t64(inv_k[b])[None].expand(k, 3, 3), t64(canon[cls_i]), float(F32(min_depth)),
                                           float(F32(max_depth)), float(F32(focal_factor)), bool(focal), bool(alloc), bool(dist))
            pctr = np.stack([p[:, 4].astype(F32) + lx, p[:, 5].astype(F32) + ly])
            assert np.array_equal(c[14:16].view(np.int32), pctr.view(np.int32)), (case, "proj_ctr not bit-identical")
            d64 = ref["depth"][:, 0].numpy()
            errs["depth"] = max(errs["depth"], float(np.max(np.abs(c[16] - d64) / d64)))
            assert (c[16] >= F32(min_depth)).all() and (c[16] <= F32(max_depth)).all()
            sz = ref["size"].numpy().T
            errs["size"] = max(errs["size"], float(np.max(np.abs(c[17:20] - sz) / sz)))
            q64 = ref["quat"].numpy().T
            nan_ref, nan_got = np.isnan(q64).any(0), np.isnan(c[10:14]).any(0)
            assert np.array_equal(nan_ref, nan_got), (case, "NaN quaternions differ from the oracle's")
            ok = ~nan_ref
            if ok.any():
                dq = np.minimum(np.abs(c[10:14, ok] - q64[:, ok]).max(0), np.abs(c[10:14, ok] + q64[:, ok]).max(0))
                errs["quat"] = max(errs["quat"], float(dq.max()))
    assert errs["score"] <= TOL_SCORE and errs["score3d"] <= TOL_SCORE3D, (case, errs)
    assert errs["depth"] <= TOL_DEPTH and errs["size"] <= TOL_SIZE and errs["quat"] <= TOL_QUAT, (case, errs)
    cap = max(8, total // 100) if max_margin is None else max_margin
    assert reported <= cap, (case, "too many within-margin disagreements", reported)
    if reported:
        warnings.warn(f"{case}: {reported} within-margin disagreement(s) with the float32 oracle: {_REPORTED[-reported:][:8]}")
    print(f"[select-decode] {case}: max errors {errs}, within-margin disagreements {reported}")
    return errs


def select_case(levels, C, case, **kw):
    out = run_select(levels, C, **kw)
    check_select(out, levels, C, case=case, **kw)
    return out


# ------------------------------------------------------------------------------------------------------------------------ cases
ELEMENT_COUNTS = [  # (H, W, C): n_el = 1, 3, 4095, 4096, 4097, 65535, 65536, 65537, ~4*65536+3; rows misaligned with 4-vectors
    (1, 1, 1), (1, 1, 3), (1, 3, 1), (21, 39, 5), (64, 64, 1), (17, 241, 1), (3, 4369, 5), (256, 256, 1), (1, 65537, 1),
    (5, 5243, 10), (7, 13, 10), (9, 1457, 3)
]


@pytest.mark.parametrize("H,W,C", ELEMENT_COUNTS)
def test_element_counts_around_rounds_and_super_rounds(hiplib, H, W, C):
    rng = np.random.default_rng(H * 1000 + W * 10 + C)
    lv = make_level(rng, 2, H, W, C, frac_hi=0.01 if H * W * C > 20000 else 0.2)
    select_case([lv], C, f"n_el={H * W * C} C={C}", topk=1000)
    # the same map with every element passing: every round and every packed 16-bit counter full
    lv["cls"][..., :C] = rng.uniform(0.0, 4.0, size=lv["cls"][..., :C].shape).astype(F32)
    lv["b2d"][..., 4] = rng.uniform(1.0, 5.0, size=lv["b2d"][..., 4].shape).astype(F32)
    out = select_case([lv], C, f"n_el={H * W * C} C={C} all pass", topk=1024, thr=0.05)
    assert (out["npass"] == H * W * C).all()


@pytest.mark.parametrize("thr", [0.05, 0.5, 0.0, 1.0])
@pytest.mark.parametrize("with_ctr", [0, 1])
def test_thresholds_ulps_and_shortcut_margin(hiplib, thr, with_ctr):
    rng = np.random.default_rng(int(thr * 100) + with_ctr)
    B, H, W, C = 2, 40, 53, 3
    lv = make_level(rng, B, H, W, C, frac_hi=0.02)
    cls = lv["cls"][..., :C].reshape(B, -1).copy()
    ctr = lv["b2d"][..., 4].copy()  # [B, HW]
    n = cls.shape[1]
    thr32 = float(F32(thr))
    if 0.0 < thr < 1.0:
        lg = F32(math.log(thr32 / (1.0 - thr32)))
        # a few ulps on either side of logit(thr), large centerness (their gate decides with or without it)
        ulps = [lg]
        for _ in range(6):
            ulps = [np.nextafter(ulps[0], F32(-np.inf))] + ulps + [np.nextafter(ulps[-1], F32(np.inf))]
        pick = rng.choice(n, size=(B, 3 * len(ulps)), replace=False)
        for b in range(B):
            cls[b, pick[b]] = np.tile(np.array(ulps, F32), 3)
        # just inside the 0.0625 shortcut margin, below and above logit(thr), centerness logits large and small
        inside = np.concatenate([lg + np.linspace(-0.0624, -0.0005, 24, dtype=F32), lg + np.linspace(0.0005, 0.0624, 24, dtype=F32)])
        pick = rng.choice(n, size=(B, len(inside)), replace=False)
        for b in range(B):
            cls[b, pick[b]] = inside.astype(F32)
            ctr[b, pick[b] // C] = np.where(np.arange(len(inside)) % 2 == 0, F32(12.0), F32(-0.5))
    if thr == 0.0:  # sigmoid goes denormal or underflows in float32
        pick = rng.choice(n, size=(B, 200), replace=False)
        for b in range(B):
            cls[b, pick[b]] = rng.uniform(-110.0, -80.0, size=200).astype(F32)
    lv["cls"][..., :C] = cls.reshape(B, H * W, C)
    lv["b2d"][..., 4] = ctr
    select_case([lv], C, f"thr={thr} with_ctr={with_ctr}", topk=1024 if thr else 1000, thr=thr, with_ctr=with_ctr)


@pytest.mark.parametrize("topk", [1, 7, 1024])
def test_topk_around_npass_and_ties(hiplib, topk):
    rng = np.random.default_rng(topk)
    B, C = 1, 3
    for delta in (-1, 0, 1):  # npass = topk - 1, topk, topk + 1
        H, W = 30, 41
        lv = make_level(rng, B, H, W, C, frac_hi=0.0)
        n = H * W * C
        on = rng.choice(n, size=topk + delta, replace=False) if topk + delta > 0 else np.zeros(0, np.int64)
        lv["cls"][0, :, :C].reshape(-1)[on] = rng.uniform(0.0, 3.0, size=len(on)).astype(F32)
        out = select_case([lv], C, f"topk={topk} npass=topk{delta:+d}", topk=topk)
        assert out["npass"][0, 0] == topk + delta
    # many equal scores straddling the k-th key: one round, and spread over several rounds / super-rounds
    for spread, (H, W) in (("one round", (8, 100)), ("across rounds", (300, 301))):
        lv = make_level(rng, 2, H, W, C, frac_hi=0.0)
        n = H * W * C
        for b in range(2):
            lim = min(n, 2400) if spread == "one round" else n
            on = rng.choice(lim, size=topk + 600, replace=False)
            vals = rng.uniform(0.5, 3.0, size=len(on)).astype(F32)
            vals[topk // 2:] = F32(0.25)  # topk // 2 keys above, the rest tied: the tied key sits at the cut
            lv["cls"][b, :, :C].reshape(-1)[on] = vals
            lv["b2d"][b, :, 4] = F32(2.0)  # one centerness: equal logits => equal keys bit for bit
        select_case([lv], C, f"topk={topk} ties {spread}", topk=topk)


def test_level_smaller_than_topk_with_trimmed_slots(hiplib):
    rng = np.random.default_rng(9)
    C = 3
    levels = [make_level(rng, 2, 48, 60, C, frac_hi=0.2), make_level(rng, 2, 12, 15, C, frac_hi=0.6),
              make_level(rng, 2, 3, 4, C, frac_hi=1.0), make_level(rng, 2, 1, 2, C, frac_hi=1.0)]
    for i, lv in enumerate(levels):
        lv["stride"] = 8 << i
    for slots in ("trimmed", "gapped", "dense"):
        select_case(levels, C, f"H*W*C < topk, {slots} slots", topk=1000, slots=slots)


@pytest.mark.parametrize("alloc", [0, 1])
@pytest.mark.parametrize("agnostic", [0, 1])
@pytest.mark.parametrize("dist", [0, 1])
@pytest.mark.parametrize("focal", [0, 1])
def test_decode_modes(hiplib, alloc, agnostic, dist, focal):
    rng = np.random.default_rng(alloc * 8 + agnostic * 4 + dist * 2 + focal)
    C, B = 5, 3  # B = 3 images with different intrinsics
    C3 = 1 if agnostic else C
    levels = [make_level(rng, B, 24, 40, C, C3=C3, frac_hi=0.1), make_level(rng, B, 12, 20, C, C3=C3, frac_hi=0.2)]
    levels[1]["stride"] = 16
    # depths that clamp at both ends (the focal / distance scalings divide by ~1 and ~sqrt(1 + r^2) here)
    for lv in levels:
        d = lv["b3d"].reshape(B, -1, 11, C3)[:, :, 6, :]
        m = rng.random(d.shape)
        d[m < 0.1] = rng.uniform(-5.0, 0.05, size=int((m < 0.1).sum())).astype(F32)
        d[m > 0.9] = rng.uniform(200.0, 400.0, size=int((m > 0.9).sum())).astype(F32)
    select_case(levels, C, f"alloc={alloc} agnostic={agnostic} dist={dist} focal={focal}", topk=300, alloc=alloc, agnostic=agnostic,
                dist=dist, focal=focal)


def test_half_offset_two_d_only_and_pad_values(hiplib):
    rng = np.random.default_rng(21)
    C = 3
    lv = make_level(rng, 2, 20, 33, C, frac_hi=0.2)
    lv["stride"] = 16
    for pad in (np.nan, 1e30, -1e30):
        select_case([lv], C, f"half offset pad={pad}", topk=200, half=1, pad_val=pad)
    lv2 = make_level(rng, 2, 20, 33, C, frac_hi=0.2, box3d=False)
    select_case([lv2], C, "2D only", topk=200, pad_val=1e30)


def test_nuscenes_attribute_ties_and_speed(hiplib):
    rng = np.random.default_rng(33)
    C = 10
    lv = make_level(rng, 2, 16, 29, C, frac_hi=0.1, num_attr=9, speed=True)
    a = lv["cls"][..., C:C + 9]
    a[:, ::3, :] = F32(0.5)  # every attribute equal: the first one wins
    a[:, 1::3, 4:] = F32(2.5)  # tie between attributes 4..8
    select_case([lv], C, "nuScenes attributes + speed", topk=500, num_attr=9, speed=True, pad_val=1e30)


def test_degenerate_quaternions_and_block_renormalisation(hiplib):
    rng = np.random.default_rng(44)
    C, B = 3, 2
    levels = [make_level(rng, B, 20, 30, C, frac_hi=0.1), make_level(rng, B, 10, 15, C, frac_hi=0.2)]
    levels[1]["stride"] = 16
    kw = dict(topk=400, alloc=1)
    clean = select_case(levels, C, "clean", **kw)
    # a candidate of (level 0, image 1): tiny quaternion (norm < QEPS, no NaN), of (level 1, image 0): all-zero quaternion (NaN)
    poisoned = [dict(lv, b3d=lv["b3d"].copy()) for lv in levels]
    e_tiny = int(clean["cand"][1, 0][7].view(np.int32)[3])
    e_zero = int(clean["cand"][0, 1][7].view(np.int32)[5])
    q = poisoned[0]["b3d"]
    for comp, v in enumerate((3e-9, -2e-9, 1e-9, 4e-9)):
        q[1, e_tiny // C, comp * C + e_tiny % C] = F32(v)
    q = poisoned[1]["b3d"]
    for comp in range(4):
        q[0, e_zero // C, comp * C + e_zero % C] = F32(0.0)
    bad = select_case(poisoned, C, "degenerate quaternions", **kw)
    for b in range(B):
        for l in range(2):
            cq, bq = clean["cand"][b, l], bad["cand"][b, l]
            assert np.array_equal(np.delete(cq, [10, 11, 12, 13], 0).view(np.int32), np.delete(bq, [10, 11, 12, 13], 0).view(np.int32))
            if (b, l) != (0, 1):
                if (b, l) == (1, 0):  # the tiny quaternion is normalised through the QEPS clamp and stays finite
                    j = 3
                    assert np.isfinite(bq[10:14, j]).all()
                    cq, bq = np.delete(cq, j, 1), np.delete(bq, j, 1)
                assert np.array_equal(cq.view(np.int32), bq.view(np.int32)), ("renormalisation leaked into another block", b, l)
                continue
            # the poisoned block: NaN at the zero quaternion, every other quaternion = clean / float32 norm of itself
            j = 5
            assert np.isnan(bq[10:14, j]).any()  # (which components are NaN was compared with the oracle above)
            others = np.delete(np.arange(cq.shape[1]), j)
            q0, q1, q2, q3 = cq[10:14, others]
            nrm = np.sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
            want = cq[10:14, others] / np.maximum(nrm, F32(1e-7))
            assert want.dtype == F32
            assert np.array_equal(bq[10:14, others].view(np.int32), want.view(np.int32)), "block renormalisation is not q / |q|_f32"

