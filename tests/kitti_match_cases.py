"""Synthetic inputs for the two KITTI matching kernels (dd3d_kitti_tp_scores / dd3d_kitti_pr_counts), built by hand: overlap
blocks, scores and ignore codes, no boxes and no geometry.  Plain module, no GPU: tests/test_kitti_match_gpu.py launches the
kernels on what is built here and compares with `expected`, which runs the sequential state machines of tests/kitti_ap_oracle.py
image by image, slot by slot, threshold by threshold.

An image is a tuple (ov [nd][ng] float32, score [nd] float64, ign_dt [n_cd][nd] int8, ign_gt [n_cd][ng] int8).
"""
import numpy as np

from tests import kitti_ap_oracle as O

F32 = np.float32
FILL = 123.25  # what the caller leaves in tp_score before the launch: a kernel that skips an image leaves it there
SCORES = np.array([0.2, 0.4, 0.6, 0.8])  # four values: ties on the score everywhere
# overlap levels around both shipped cuts.  float32(0.7) < 0.7 and float32(0.5) == 0.5 in float64: neither passes `>`.
LEVELS = np.array([0.0, 0.0, 0.0, 0.3, 0.5, np.nextafter(F32(0.5), F32(1)), 0.6, 0.7, np.nextafter(F32(0.7), F32(1)), 0.9], dtype=F32)
MIN_OVERLAP = [0.5, 0.7]  # the shipped (overlap) slots
assert float(F32(0.7)) < 0.7 and float(F32(0.5)) == 0.5 and float(LEVELS[8]) > 0.7 and float(LEVELS[5]) > 0.5


def pack(images):
    """Concatenate images into the flat arrays and offsets of `dd3d_kitti_match_args` (host numpy)."""
    n_cd = images[0][2].shape[0]
    nd = np.array([im[0].shape[0] for im in images], dtype=np.int64)
    ng = np.array([im[0].shape[1] for im in images], dtype=np.int64)
    for ov, sc, igd, igg in images:
        assert ov.dtype == F32 and sc.dtype == np.float64 and igd.dtype == np.int8 and igg.dtype == np.int8
        assert sc.shape == (ov.shape[0],) and igd.shape == (n_cd, ov.shape[0]) and igg.shape == (n_cd, ov.shape[1])
    return dict(
        ov=np.concatenate([im[0].reshape(-1) for im in images]), ov_off=np.concatenate([[0], np.cumsum(nd * ng)])[:-1].astype(np.int64),
        dt_begin=np.concatenate([[0], np.cumsum(nd)]).astype(np.int32), gt_begin=np.concatenate([[0], np.cumsum(ng)]).astype(np.int32),
        dt_score=np.concatenate([im[1] for im in images]), ign_dt=np.ascontiguousarray(np.concatenate([im[2] for im in images], axis=1)),
        ign_gt=np.ascontiguousarray(np.concatenate([im[3] for im in images], axis=1)), n_ov=int((nd * ng).sum()), n_img=len(images),
        n_dt=int(nd.sum()), n_gt=int(ng.sum()), n_cd=n_cd, max_dt=int(nd.max()), max_gt=int(ng.max()))


def expected(images, min_overlap, thresh, n_thresh, skip=()):
    """-> (tp_score [n_cd][n_o][n_gt] float64, tp_fp_fn [n_cd][n_o][t_max][3] int64) from the oracle's state machines.  Images in
    `skip` contribute nothing: their tp_score entries keep FILL.  Slots of one image that see the same ignore codes and overlap
    cut share one oracle call (the codes of many class x difficulty rows coincide)."""
    n_cd, n_o = images[0][2].shape[0], len(min_overlap)
    thresh = np.asarray(thresh, dtype=np.float64).reshape(n_cd * n_o, -1)
    t_max = thresh.shape[1]
    n_gt = sum(im[0].shape[1] for im in images)
    tp = np.full((n_cd, n_o, n_gt), FILL, dtype=np.float64)
    counts = np.zeros((n_cd, n_o, t_max, 3), dtype=np.int64)
    g0 = 0
    for i, (ov, sc, igd, igg) in enumerate(images):
        ng = ov.shape[1]
        if i not in skip:
            ovl, scl = ov.astype(np.float64).tolist(), sc.tolist()
            seen1, seen2 = {}, {}
            for cd in range(n_cd):
                d, g = igd[cd].tolist(), igg[cd].tolist()
                for o, mo in enumerate(min_overlap):
                    key = (igd[cd].tobytes(), igg[cd].tobytes(), float(mo))
                    if key not in seen1:
                        seen1[key] = O.tp_scores(ovl, scl, g, d, mo, per_gt=True)
                    tp[cd, o, g0:g0 + ng] = seen1[key]
                    for t in range(int(n_thresh[cd * n_o + o])):
                        k2 = key + (float(thresh[cd * n_o + o, t]),)
                        if k2 not in seen2:
                            seen2[k2] = O.pr_counts(ovl, scl, g, d, mo, k2[-1])
                        counts[cd, o, t] += seen2[k2]
        g0 += ng
    return tp, counts


def codes(rng, n_cd, n, p=(0.15, 0.65, 0.2)):
    """[n_cd][n] int8 ignore codes, -1 / 0 / 1 with probabilities `p`, drawn independently per class x difficulty row."""
    return rng.choice(np.array([-1, 0, 1], dtype=np.int8), size=(n_cd, n), p=p)


def dense_image(rng, nd, ng, n_cd, levels=LEVELS, scores=SCORES, zeros=0):
    """Every (detection, GT) overlap drawn from `levels` (and `zeros` more zeros: fewer candidates per GT), every score from `scores`
    (None: distinct uniform draws, so that the recorded scores tell the picks apart): many GT compete for the same detections."""
    ov = rng.choice(np.concatenate([levels, np.zeros(zeros, dtype=F32)]), size=(nd, ng)).astype(F32)
    sc = rng.uniform(0.05, 0.95, size=nd) if scores is None else rng.choice(scores, size=nd).astype(np.float64)
    return ov, sc, codes(rng, n_cd, nd), codes(rng, n_cd, ng)


def sparse_image(rng, nd, ng, n_cd, n_cand=12):
    """`n_cand` detections spread over the whole index range overlap every GT (levels above both cuts, tied scores); all the
    others overlap nothing.  The picks land in random chunks, so the flags of late chunks decide the later GT."""
    ov = np.zeros((nd, ng), dtype=F32)
    sc = rng.choice(SCORES, size=nd).astype(np.float64)
    if nd and ng:
        cand = rng.choice(nd, size=min(n_cand, nd), replace=False)
        ov[cand] = rng.choice(np.array([0.6, 0.75, 0.9], dtype=F32), size=(len(cand), ng))
        sc[cand] = rng.choice(SCORES[2:], size=len(cand))
    igd = codes(rng, n_cd, nd, p=(0.1, 0.7, 0.2))
    return ov, sc, igd, codes(rng, n_cd, ng, p=(0.1, 0.8, 0.1))


def thresholds_from_scores(rng, n_cdo, t_max, n_thresh, values=SCORES):
    """thresh [n_cdo][t_max]: the first n_thresh[s] entries of row s are score values, one float64 step below / above them, or values
    in between; the rest is a nonzero filler that the kernel must not use."""
    pool = np.concatenate([values, np.nextafter(values, -np.inf), np.nextafter(values, np.inf), values + 0.1, [0.0, 1.0]])
    th = np.full((n_cdo, t_max), 0.123)
    for s in range(n_cdo):
        th[s, :n_thresh[s]] = rng.choice(pool, size=n_thresh[s])
    return th


# --- hand-placed ties -----------------------------------------------------------------------------------------------------------
TIE_PAIRS = [(5, 69), (63, 127), (6, 69), (63, 64), (0, 8191), (4095, 4096), (4000, 4200), (70, 134), (4160, 4224), (6200, 6264)]
# (j, j + 64): one lane, neighbouring chunks (chunks 0 / 1, 1 / 2, and 65 / 66 and 96 / 97 of the `hi` word); (6, 69): the lower index sits in the
# higher lane (lane 6 of chunk 0 against lane 5 of chunk 1); (63, 64): last lane of chunk 0 against first lane of chunk 1; (0, 8191):
# the first and the last detection a wave can hold; (4095, 4096) and (4000, 4200): across the lo / hi flag words.
TIE_DT_CODES = [(0, 0), (0, 1), (1, 0)]  # ign_dt of (a, b)
TIE_GT_CODES = [(0, 0), (1, 0), (0, 1)]  # ign_gt of (GT 0, GT 1)
TIE_SCORES = [(0.5, 0.5), (0.4, 0.6), (0.6, 0.4)]
TIE_THRESH = [0.3, 0.4, 0.5, 0.6, 0.7]
TIE_N_CD = len(TIE_DT_CODES) * len(TIE_GT_CODES)


def tie_images(a, b):
    """Detections a < b are the only candidates of GT 0 and overlap it equally (0.8, above both cuts).  GT 1 overlaps both, only a,
    or only b, so which of the two GT 0 consumed decides what GT 1 finds: the wrong tie-break changes tp_score or a count.  One
    image per (GT 1 variant, score pair); the n_cd rows run every combination of TIE_DT_CODES x TIE_GT_CODES.  Every other
    detection has a higher score and a zero overlap (a kernel that ignored the overlap would pick it)."""
    nd = b + 1
    out = []
    for second in ("both", "a", "b"):
        for sa, sb in TIE_SCORES:
            ov = np.zeros((nd, 2), dtype=F32)
            ov[[a, b], 0] = 0.8
            ov[a, 1] = 0.8 if second in ("both", "a") else 0.0
            ov[b, 1] = 0.8 if second in ("both", "b") else 0.0
            sc = np.full(nd, 0.95)
            sc[a], sc[b] = sa, sb
            igd = np.full((TIE_N_CD, nd), -1, dtype=np.int8)
            igd[:, ::7] = 0  # bystanders that are valid but overlap nothing: false positives at every threshold
            igg = np.zeros((TIE_N_CD, 2), dtype=np.int8)
            for r in range(TIE_N_CD):
                igd[r, [a, b]] = TIE_DT_CODES[r // len(TIE_GT_CODES)]
                igg[r] = TIE_GT_CODES[r % len(TIE_GT_CODES)]
            out.append((ov, sc, igd, igg))
    return out
