"""Reference gradients of the training losses for the tests of the loss backward (csrc/loss_grads.hip): torch autograd through the CPU
oracle of the losses (tests/loss_oracle.py, plain torch), and the mask of the positives that sit at a point where the loss is not
differentiable or jumps, which are compared for finiteness only.
"""
import torch

from oracle import dd3d_oracle as O
from tests import loss_oracle as LO

FAMILIES = ("logits", "box2d_reg", "centerness", "quat", "ctr", "depth", "size", "conf", "attr", "speed")
OUT_INDEX = {"loss_cls": 0, "loss_box2d_reg": 1, "loss_centerness": 2, "loss_box3d_quat": 3, "loss_box3d_proj_ctr": 4, "loss_box3d_depth": 5,
             "loss_box3d_size": 6, "loss_conf3d": 7, "loss_attr": 8, "loss_speed": 9}  # the words of dd3d_loss_args.out
KINK_MARGIN = 1e-4
FLOAT_TARGETS = ("box2d_reg_targets", "locations", "box3d", "speeds", "ctr")


def families(p):
    return [k for k in FAMILIES if (k in FAMILIES[:3]) or (k in FAMILIES[3:8] and p["box3d"]) or (k in FAMILIES[8:] and p["nusc"])]


def channels(p, key):
    C3 = 1 if p.get("class_agnostic") else p["num_classes"]
    return {"logits": p["num_classes"], "box2d_reg": 4, "centerness": 1, "quat": 4 * C3, "ctr": 2 * C3, "depth": C3, "size": 3 * C3, "conf": C3,
            "attr": p.get("num_attr", 0), "speed": 1}[key]


def _cast(targets, dtype):
    return {k: (v.to(dtype) if k in FLOAT_TARGETS and torch.is_tensor(v) else v) for k, v in targets.items()}


def summed_loss(leaf, targets, inv_K, p, upstream=None, dtype=torch.float64):
    """sum_k upstream[k] * loss_k of LO.losses on the maps `leaf` in `dtype` (`upstream`: 10 weights in the order of OUT_INDEX; None:
    ones), the conf target detached as in the reference.  Returns (the sum, the loss dict).  The one statement of the scalar every
    gradient oracle differentiates: head_grads with the head maps as leaves, whole_model_grad_oracle with the model's parameters."""
    out = LO.losses(leaf, _cast(targets, dtype), inv_K.to(dtype), p)
    if "loss_conf3d" in out and targets["pos_inds"].numel():
        # LO.losses leaves the entangled corner error attached to the graph; the reference detaches it before it becomes the conf
        # target (disentangled_box3d_loss.py:52), so loss_conf3d reaches the conf logits only: take it from a second evaluation whose
        # decode inputs are constants
        cut = {k: (v.detach() if k[:-1] in ("quat", "ctr", "depth", "size") else v) for k, v in leaf.items()}
        out["loss_conf3d"] = LO.losses(cut, _cast(targets, dtype), inv_K.to(dtype), p)["loss_conf3d"]
    w = torch.ones(10, dtype=dtype) if upstream is None else torch.as_tensor(upstream).to(dtype)
    return sum(w[OUT_INDEX[k]] * v for k, v in out.items()), out


def head_grads(maps, targets, inv_K, p, upstream=None, dtype=torch.float64):
    """d (sum_k upstream[k] * loss_k) / d maps by autograd through LO.losses in `dtype` (the conf target detached, as in the reference); `upstream`: 10 weights in the order of
    OUT_INDEX (None: ones).  Returns {key<l>: NCHW gradient in `dtype`} for every head map of the case (zeros where the loss does not
    reach a map)."""
    fam = families(p)
    L = p["num_levels"]
    leaf = {f"{k}{l}": maps[f"{k}{l}"].detach().to(dtype).clone().requires_grad_(True) for k in fam for l in range(L)}
    total, _ = summed_loss(leaf, targets, inv_K, p, upstream, dtype)
    g = torch.autograd.grad(total, list(leaf.values()), allow_unused=True)
    return {k: (torch.zeros_like(v) if gi is None else gi) for (k, v), gi in zip(leaf.items(), g)}


def flat_family(grads, key, p):
    """A family's gradient over all levels as (N, channels) rows in target order (level-first, image, H*W)."""
    return LO.flat(grads, key, p["num_levels"], channels(p, key))


def near_kink(maps, targets, inv_K, p, margin=KINK_MARGIN):
    """Boolean mask over the positives (the order of targets["pos_inds"]): True where the positive lies within `margin` of a point
    where the loss is not differentiable or jumps -- a disentangled corner residual at beta (at 0 for beta < 1e-5, plain L1; only a
    residual the prediction can move counts: a corner's z does not depend on the projected centre when the third row of K^-1 is
    (0, 0, 1), so the proj_ctr group's z residuals are 0 whatever the prediction, with a zero tangent), the speed residual at 0.05, a GIoU side
    equal to its target, the decoded depth on a clamp bound (relative), the two largest q_abs of matrix_to_quaternion equal.
    Evaluated in float64 on the float32 inputs."""
    f64 = torch.float64
    L, C = p["num_levels"], p["num_classes"]
    pos, labels = targets["pos_inds"], targets["labels"]
    n = pos.numel()
    mask = torch.zeros(n, dtype=torch.bool)
    if n == 0:
        return mask
    t = _cast(targets, f64)
    m = {k: v.to(f64) for k, v in maps.items()}
    reg_p, reg_t = LO.flat(m, "box2d_reg", L, 4)[pos], t["box2d_reg_targets"][pos]
    mask |= ((reg_p - reg_t).abs() <= margin).any(1)
    if p["box3d"]:
        C3 = 1 if p["class_agnostic"] else C
        lab = labels[pos]
        I = torch.zeros_like(lab) if p["class_agnostic"] else lab
        get = lambda key, k: LO.flat(m, key, L, k * C3).reshape(-1, k, C3)[pos]
        pick = lambda x: torch.gather(x, 2, I[:, None, None].expand(-1, x.shape[1], 1)).squeeze(-1)
        q, c2, d, s = pick(get("quat", 4)), pick(get("ctr", 2)), pick(get("depth", 1)), pick(get("size", 3))
        locs, iK = t["locations"][pos], inv_K.to(f64)[targets["im_inds"][pos]]
        canon = torch.tensor(p["canon"], dtype=f64)[lab]
        b = O.predictions_to_boxes3d(q, c2, d.reshape(-1), s, locs, iK, canon, p["min_depth"], p["max_depth"], p["focal_factor"], p["scale_depth"],
                                     p["allocentric"], p["depth_is_distance"])
        tb = t["box3d"][pos]
        tq, tc, td, ts, tK = tb[:, 0:4], tb[:, 4:6], tb[:, 6:7], tb[:, 7:10], tb[:, 10:19].reshape(-1, 3, 3)
        target_corners = LO._corners(tq, tc, td, ts, tK)
        kink_at = p["beta"] if p["beta"] >= 1e-5 else 0.0
        ctr_moves_z = (tK[:, 2, :2] != 0).any(1)  # tvec z = (K20 u + K21 v + K22) * depth
        for grp, (qq, cc, dd, ss) in enumerate(((b["quat"], tc, td, ts), (tq, b["proj_ctr"], td, ts), (tq, tc, b["depth"], ts), (tq, tc, td, b["size"]))):
            res = (LO._corners(qq, cc, dd, ss, tK) - target_corners).abs().reshape(n, 8, 3)
            near = (res - kink_at).abs() <= margin
            if grp == 1:
                near[:, :, 2] &= ctr_moves_z[:, None]
            mask |= near.reshape(n, 24).any(1)
        # the depth before its clamp (fcos3d.py:36-42)
        dep = d.reshape(-1)
        if p["scale_depth"]:
            dep = dep / (torch.norm(torch.stack([iK[:, 0, 0], iK[:, 1, 1]], dim=-1), dim=-1) * p["focal_factor"])
        if p["depth_is_distance"]:
            dep = dep / O.unproject_points2d(locs, iK).norm(dim=1).clamp(min=1e-7)
        for bound in (p["min_depth"], p["max_depth"]):
            mask |= (dep - bound).abs() <= margin * abs(bound)
        if p["allocentric"]:  # the candidate choice of matrix_to_quaternion (geometry.py:30-46)
            qn = q / q.norm(dim=1, keepdim=True).clamp(min=1e-7)
            qn = qn / qn.norm(dim=1, keepdim=True)
            ray = O.unproject_points2d(c2 + locs, iK)
            z = ray / ray.norm(dim=1, keepdim=True)
            y = z.new_tensor([[0., 1., 0.]]) - z[:, 1:2] * z
            y = y / y.norm(dim=1, keepdim=True)
            R = torch.bmm(torch.stack([torch.cross(y, z, dim=1), y, z], dim=-1), O.quaternion_to_matrix(qn))
            m00, m11, m22 = R[:, 0, 0], R[:, 1, 1], R[:, 2, 2]
            q_abs = O._sqrt_positive_part(torch.stack([1.0 + m00 + m11 + m22, 1.0 + m00 - m11 - m22, 1.0 - m00 + m11 - m22, 1.0 - m00 - m11 + m22], -1))
            top = q_abs.topk(2, dim=1).values
            mask |= (top[:, 0] - top[:, 1]) <= margin
    if p["nusc"]:
        spd = LO.flat(m, "speed", L, 1).reshape(-1)[pos]
        ts_ = t["speeds"][pos]
        mask |= (~torch.isnan(ts_)) & (((spd - ts_).abs() - 0.05).abs() <= margin)
    return mask


def bar(g64, g32, keep):
    """The acceptance bound of one family: 8 * max(d32, 2^-23 * max|g64|), d32 the float32 autograd's own deviation from the float64 one
    over the rows `keep` (the reference's rounding, not the kernel's)."""
    gmax = float(g64.abs().max()) if g64.numel() else 0.0
    d32 = float((g32.to(torch.float64) - g64)[keep].abs().max()) if bool(keep.any()) and g64.numel() else 0.0
    return 8.0 * max(d32, 2.0**-23 * gmax), d32, gmax
