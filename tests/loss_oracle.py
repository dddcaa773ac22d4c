"""Torch-CPU statement of the reference's training targets and losses, for the tests of the loss engine (csrc/losses.hip).

Restated from tridet (TRI-ML/dd3d), single process:
  prepare_targets   DD3DTargetPreparer (tridet/modeling/dd3d/prepare_targets.py:28-235), NuscenesDD3DTargetPreparer
                    (nuscenes_dd3d.py:24-196)
  losses            FCOS2DLoss (fcos2d.py:159-239), FCOS3DLoss (fcos3d.py:191-299), DisentangledBox3DLoss
                    (disentangled_box3d_loss.py:27-54), NuscenesLoss (nuscenes_dd3d.py:199-265), tridet smooth_l1_loss
                    (layers/smooth_l1_loss.py:57-80) for the corners, [ext] fvcore smooth_l1_loss for the speed, IOULoss (layers/iou_loss.py:20-71), [ext] fvcore sigmoid_focal_loss.
Head maps are the reference's NCHW per-level tensors; the 3D decode and the corners come from the forward oracle (oracle/dd3d_oracle.py).
"""
import torch
import torch.nn.functional as F

from oracle import dd3d_oracle as O

INF = 100000000.


def sizes_of_interest(sizes):
    """prepare_targets.py:19-25."""
    soi, prev = [], -1
    for s in sizes:
        soi.append([prev, s])
        prev = s
    soi.append([prev, INF])
    return soi


def sample_region(boxes, num_loc_list, xs, ys, strides, radius):
    """prepare_targets.py:179-212 get_sample_region, including the all-false return when the FIRST box has x1 + x2 == 0 (:190)."""
    center_x = boxes[..., [0, 2]].sum(dim=-1) * 0.5
    center_y = boxes[..., [1, 3]].sum(dim=-1) * 0.5
    K, G = len(xs), boxes.shape[0]
    if center_x.numel() == 0 or center_x[0].expand(K).sum() == 0:
        return torch.zeros((K, G), dtype=torch.bool)
    cg = torch.zeros((K, G, 4))
    beg = 0
    for level, n in enumerate(num_loc_list):
        end = beg + n
        s = strides[level] * radius
        xmin, ymin, xmax, ymax = center_x - s, center_y - s, center_x + s, center_y + s
        cg[beg:end, :, 0] = torch.where(xmin > boxes[:, 0], xmin, boxes[:, 0])
        cg[beg:end, :, 1] = torch.where(ymin > boxes[:, 1], ymin, boxes[:, 1])
        cg[beg:end, :, 2] = torch.where(xmax > boxes[:, 2], boxes[:, 2], xmax)
        cg[beg:end, :, 3] = torch.where(ymax > boxes[:, 3], boxes[:, 3], ymax)
        beg = end
    left = xs[:, None] - cg[..., 0]
    right = cg[..., 2] - xs[:, None]
    top = ys[:, None] - cg[..., 1]
    bottom = cg[..., 3] - ys[:, None]
    return torch.stack((left, top, right, bottom), -1).min(-1)[0] > 0


def prepare_targets(locations, gt, strides, num_classes, sizes, center_sample=True, radius=1.5, box3d=True, nusc=False, num_attr=3):
    """locations: per-level (HW, 2); gt: per image dict(boxes (n,4), classes (n,), and for box3d quat, proj_ctr, depth, size, inv_K
    (n,3,3) float32; nusc: attributes, speeds).  Returns the flattened targets (level-first, image, H*W; prepare_targets.py:49-63) with
    box3d as one (N, 19) tensor [quat, proj_ctr, depth, size, K^-1], plus the per-target centerness target `ctr` (0 off the positives)."""
    num_loc_list = [len(l) for l in locations]
    soi = sizes_of_interest(sizes)
    size_ranges = torch.cat([torch.tensor(soi[l], dtype=torch.float32)[None].expand(n, -1) for l, n in enumerate(num_loc_list)])
    loc = torch.cat(locations)
    xs, ys = loc[:, 0], loc[:, 1]
    N1 = len(loc)
    per = {k: [] for k in ("labels", "reg", "inds", "box3d", "attr", "speed")}
    num_targets = 0
    for g in gt:
        boxes = g["boxes"]
        if boxes.numel() == 0:  # :111-127
            per["labels"].append(torch.full((N1, ), num_classes, dtype=torch.long))
            per["reg"].append(torch.zeros((N1, 4)))
            per["inds"].append(torch.full((N1, ), -1, dtype=torch.long))
            per["box3d"].append(torch.zeros((N1, 19)))
            per["attr"].append(torch.full((N1, ), num_attr, dtype=torch.long))  # (the reference appends nothing here: see DESIGN)
            per["speed"].append(torch.full((N1, ), float("nan")))
            continue
        area = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
        l_ = xs[:, None] - boxes[:, 0][None]
        t_ = ys[:, None] - boxes[:, 1][None]
        r_ = boxes[:, 2][None] - xs[:, None]
        b_ = boxes[:, 3][None] - ys[:, None]
        reg = torch.stack([l_, t_, r_, b_], dim=2)
        inside = sample_region(boxes, num_loc_list, xs, ys, strides, radius) if center_sample else reg.min(dim=2)[0] > 0
        mx = reg.max(dim=2)[0]
        cared = (mx >= size_ranges[:, [0]]) & (mx <= size_ranges[:, [1]])
        a2 = area[None].repeat(N1, 1)
        a2[~inside] = INF
        a2[~cared] = INF
        min_area, inds = a2.min(dim=1)  # first index among equal minima
        per["reg"].append(reg[range(N1), inds])
        per["inds"].append(inds + num_targets)
        num_targets += len(boxes)
        lab = g["classes"].long()[inds]
        lab[min_area == INF] = num_classes
        per["labels"].append(lab)
        if box3d:
            per["box3d"].append(torch.cat([g["quat"][inds], g["proj_ctr"][inds], g["depth"].reshape(-1, 1)[inds], g["size"][inds],
                                           g["inv_K"].reshape(-1, 9)[inds]], 1))
        if nusc:
            per["attr"].append(g["attributes"].long()[inds])
            per["speed"].append(g["speeds"].float()[inds])

    def level_first(lst):  # _transpose (:214-235) + flatten
        return torch.cat([torch.cat([t.split(num_loc_list)[l] for t in lst]) for l in range(len(num_loc_list))])

    B = len(gt)
    out = {"labels": level_first(per["labels"]), "box2d_reg_targets": level_first(per["reg"]), "target_inds": level_first(per["inds"])}
    out["locations"] = torch.cat([locations[l].repeat(B, 1) for l in range(len(locations))])
    out["im_inds"] = torch.cat([torch.arange(B).repeat_interleave(n) for n in num_loc_list])
    out["fpn_levels"] = torch.cat([torch.full((B * n, ), l, dtype=torch.long) for l, n in enumerate(num_loc_list)])
    out["pos_inds"] = torch.nonzero(out["labels"] != num_classes).squeeze(1)
    if box3d:
        out["box3d"] = level_first(per["box3d"])
    if nusc:
        out["attributes"], out["speeds"] = level_first(per["attr"]), level_first(per["speed"])
    ctr = torch.zeros(len(out["labels"]))
    p = out["pos_inds"]
    if len(p):
        ctr[p] = ctrness_targets(out["box2d_reg_targets"][p])
    out["ctr"] = ctr
    out["num_classes"] = num_classes
    return out


def ctrness_targets(reg):
    """fcos2d.py:20-27."""
    lr, tb = reg[:, [0, 2]], reg[:, [1, 3]]
    return torch.sqrt((lr.min(dim=-1)[0] / lr.max(dim=-1)[0]) * (tb.min(dim=-1)[0] / tb.max(dim=-1)[0]))


def sigmoid_focal_loss(inputs, targets, alpha=0.25, gamma=2.0):
    """[ext] fvcore.nn.sigmoid_focal_loss, reduction "sum"; BCE with logits in its stable form."""
    p = torch.sigmoid(inputs)
    ce = F.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce * ((1 - p_t)**gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss.sum()


def smooth_l1_loss(x, y, beta):
    """tridet/layers/smooth_l1_loss.py:57-74: 0.5 n^2 below beta (not / beta: the loss jumps at n = beta); plain L1 for beta < 1e-5."""
    n = torch.abs(x - y)
    if beta < 1e-5:
        return n
    return torch.where(n < beta, 0.5 * n**2, n - 0.5 * beta)


def smooth_l1_loss_fvcore(x, y, beta):
    """[ext] fvcore.nn.smooth_l1_loss (reduction "none"), which NuscenesLoss imports for the speed term (nuscenes_dd3d.py:4, :261):
    0.5 n^2 / beta below beta, n - 0.5 beta above; plain L1 for beta < 1e-5."""
    n = torch.abs(x - y)
    if beta < 1e-5:
        return n
    return torch.where(n < beta, 0.5 * n**2 / beta, n - 0.5 * beta)


def giou_loss(pred, target, weight):
    """iou_loss.py:20-71, loc_loss_type 'giou', with the +1 smoothing of :57."""
    pl, pt, pr, pb = pred.unbind(1)
    tl, tt, tr, tb = target.unbind(1)
    target_area = (tl + tr) * (tt + tb)
    pred_area = (pl + pr) * (pt + pb)
    w_i = torch.min(pl, tl) + torch.min(pr, tr)
    h_i = torch.min(pb, tb) + torch.min(pt, tt)
    g_w = torch.max(pl, tl) + torch.max(pr, tr)
    g_h = torch.max(pb, tb) + torch.max(pt, tt)
    ac = g_w * g_h
    inter = w_i * h_i
    union = target_area + pred_area - inter
    ious = (inter + 1.0) / (union + 1.0)
    gious = ious - (ac - union) / ac
    return ((1 - gious) * weight).sum()


def _corners(quat, proj_ctr, depth, size, inv_K):
    tvec = O.unproject_points2d(proj_ctr, inv_K) * depth.reshape(-1, 1)
    return O.boxes3d_corners(quat, tvec, size)


def flat(maps, key, L, k):
    """cat([x.permute(0, 2, 3, 1).reshape(-1, k) for x in per-level maps]) -- the flattening of fcos2d.py:179-181 / fcos3d.py:234-238."""
    return torch.cat([maps[f"{key}{l}"].permute(0, 2, 3, 1).reshape(-1, k) for l in range(L)])


def losses(maps, targets, inv_K, p):
    """The loss dict of core.py:95-112 (+ nuscenes_dd3d.py:385-397) from head maps `maps` ({logits<l>, box2d_reg<l>, centerness<l>,
    quat<l>, ctr<l>, depth<l>, size<l>, conf<l>, attr<l>, speed<l>} NCHW), targets of prepare_targets, the images' K^-1 (B,3,3) and
    settings `p` (num_classes, num_levels, alpha, gamma, box3d, nusc, class_agnostic, canon, min_depth, max_depth, focal_factor,
    scale_depth, allocentric, depth_is_distance, beta, temperature, w_box3d, w_conf3d, w_attr, w_speed, num_attr)."""
    C, L = p["num_classes"], p["num_levels"]
    labels, reg_t, pos = targets["labels"], targets["box2d_reg_targets"], targets["pos_inds"]
    logits = flat(maps, "logits", L, C)
    reg_p = flat(maps, "box2d_reg", L, 4)
    ctr_p = flat(maps, "centerness", L, 1).reshape(-1)
    num_pos_avg = max(float(pos.numel()), 1.0)
    cls_t = torch.zeros_like(logits)
    cls_t[pos, labels[pos]] = 1
    out = {"loss_cls": sigmoid_focal_loss(logits, cls_t, p["alpha"], p["gamma"]) / num_pos_avg}
    if pos.numel() == 0:
        out["loss_box2d_reg"] = reg_p.sum() * 0.
        out["loss_centerness"] = ctr_p.sum() * 0.
        if p["box3d"]:
            for k in ("quat", "ctr", "depth", "size", "conf"):
                out[{"ctr": "loss_box3d_proj_ctr", "conf": "loss_conf3d"}.get(k, "loss_box3d_" + k)] = flat(maps, k, L, 1).sum() * 0.
        if p["nusc"]:
            out["loss_attr"] = flat(maps, "attr", L, 1).sum() * 0.
            out["loss_speed"] = flat(maps, "speed", L, 1).sum() * 0.
        return out
    ct = ctrness_targets(reg_t[pos])
    loss_denom = max(float(ct.sum()), 1e-6)
    out["loss_box2d_reg"] = giou_loss(reg_p[pos], reg_t[pos], ct) / loss_denom
    out["loss_centerness"] = F.binary_cross_entropy_with_logits(ctr_p[pos], ct, reduction="sum") / num_pos_avg
    if p["box3d"]:
        C3 = 1 if p["class_agnostic"] else C
        get = lambda key, k: flat(maps, key, L, k * C3).reshape(-1, k, C3)[pos]
        lab = labels[pos]
        I = torch.zeros_like(lab) if p["class_agnostic"] else lab
        pick = lambda t: torch.gather(t, 2, I[:, None, None].expand(-1, t.shape[1], 1)).squeeze(-1)
        q, c2, d, s, cf = pick(get("quat", 4)), pick(get("ctr", 2)), pick(get("depth", 1)), pick(get("size", 3)), pick(get("conf", 1))
        locs = targets["locations"][pos]
        iK = inv_K[targets["im_inds"][pos]]
        canon = torch.tensor(p["canon"], dtype=torch.float32)[lab]
        b = O.predictions_to_boxes3d(q, c2, d.reshape(-1), s, locs, iK, canon, p["min_depth"], p["max_depth"], p["focal_factor"],
                                     p["scale_depth"], p["allocentric"], p["depth_is_distance"])
        t = targets["box3d"][pos]
        tq, tc, td, ts, tK = t[:, 0:4], t[:, 4:6], t[:, 6:7], t[:, 7:10], t[:, 10:19].reshape(-1, 3, 3)
        target_corners = _corners(tq, tc, td, ts, tK)
        fields = {"quat": (b["quat"], tc, td, ts), "proj_ctr": (tq, b["proj_ctr"], td, ts), "depth": (tq, tc, b["depth"], ts),
                  "size": (tq, tc, td, b["size"])}
        for key in ("quat", "proj_ctr", "depth", "size"):
            qq, cc, dd, ss = fields[key]
            l1 = smooth_l1_loss(_corners(qq, cc, dd, ss, tK), target_corners, p["beta"])  # (the clamp of :42 discards its result)
            out["loss_box3d_" + key] = p["w_box3d"] * torch.sum(l1.reshape(-1, 24).mean(dim=1) * ct) / loss_denom
        pred_corners = _corners(b["quat"], b["proj_ctr"], b["depth"], b["size"], iK)
        err = (target_corners - pred_corners).abs().reshape(-1, 24).mean(dim=1)
        conf_t = torch.exp(-1. / p["temperature"] * err)
        bce = F.binary_cross_entropy_with_logits(cf.reshape(-1), conf_t, reduction="none")
        out["loss_conf3d"] = p["w_conf3d"] * (bce * ct).sum() / loss_denom
        out = {k: out[k] for k in ["loss_cls", "loss_box2d_reg", "loss_centerness", "loss_conf3d", "loss_box3d_quat", "loss_box3d_proj_ctr",
                                   "loss_box3d_depth", "loss_box3d_size"]}
    if p["nusc"]:
        A = p["num_attr"]
        attr_l = flat(maps, "attr", L, A)[pos]
        spd = flat(maps, "speed", L, 1).reshape(-1)[pos]
        ta, ts_ = targets["attributes"][pos], targets["speeds"][pos]
        valid = ta != A
        w = ct[valid]
        denom = max(float(w.sum()), 1e-6)
        if valid.sum() == 0:
            out["loss_attr"] = attr_l.sum() * 0.
        else:
            xent = F.cross_entropy(attr_l[valid], ta[valid])  # mean over the valid attributes (nuscenes_dd3d.py:237)
            out["loss_attr"] = p["w_attr"] * (xent * w).sum() / denom
        vs = ~torch.isnan(ts_)
        w = ct[vs]
        denom = max(float(w.sum()), 1e-6)
        if vs.sum() == 0:
            out["loss_speed"] = spd.sum() * 0.
        else:
            out["loss_speed"] = p["w_speed"] * (smooth_l1_loss_fvcore(spd[vs], ts_[vs], 0.05) * w).sum() / denom
    return out


def settings(model):
    """The `p` of losses() for a dd3d_amd model."""
    cfg = model.cfg
    c3 = cfg.DD3D.FCOS3D
    nusc = hasattr(model, "attr_logits")
    return dict(num_classes=model.num_classes, alpha=float(cfg.DD3D.FCOS2D.LOSS.ALPHA), gamma=float(cfg.DD3D.FCOS2D.LOSS.GAMMA),
                box3d=not model.only_box2d, nusc=nusc, class_agnostic=bool(c3.CLASS_AGNOSTIC_BOX3D), canon=[list(r) for r in c3.CANONICAL_BOX3D_SIZES],
                min_depth=float(c3.MIN_DEPTH), max_depth=float(c3.MAX_DEPTH), focal_factor=float(c3.SCALE_DEPTH_BY_FOCAL_LENGTHS_FACTOR),
                scale_depth=bool(c3.SCALE_DEPTH_BY_FOCAL_LENGTHS), allocentric=bool(c3.PREDICT_ALLOCENTRIC_ROT),
                depth_is_distance=bool(c3.PREDICT_DISTANCE), beta=float(c3.LOSS.SMOOTH_L1_BETA), temperature=float(c3.LOSS.CONF_3D_TEMPERATURE),
                w_box3d=float(c3.LOSS.WEIGHT_BOX3D), w_conf3d=float(c3.LOSS.WEIGHT_CONF3D),
                w_attr=float(cfg.DD3D.NUSC.LOSS.WEIGHT_ATTR) if nusc else 0.0, w_speed=float(cfg.DD3D.NUSC.LOSS.WEIGHT_SPEED) if nusc else 0.0,
                num_attr=int(model.attr_logits.out_channels) if nusc else 0)


def gt_dicts(instances, box3d=True, nusc=False):
    """Instances (make_gt_instances / the reference's mapper) -> the per-image dicts of prepare_targets (float32 K^-1)."""
    out = []
    for inst in instances:
        g = {"boxes": inst.gt_boxes.tensor.float(), "classes": inst.gt_classes}
        if box3d:
            b = inst.gt_boxes3d
            g.update(quat=b.quat.float(), proj_ctr=b.proj_ctr.float(), depth=b.depth.float(), size=b.size.float(), inv_K=b.inv_intrinsics.float())
        if nusc:
            g.update(attributes=inst.gt_attributes, speeds=inst.gt_speeds)
        out.append(g)
    return out
