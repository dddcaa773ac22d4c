"""CPU tests of the loss backward's host side and of the reference it is tested against (tests/loss_grad_oracle.py): the oracle's float64
autograd against central differences, the oracle against the gradients of the reference's own loss modules
(tests/golden/loss_grads_*.npz), the kink counts of the GPU cases, the C / ctypes layout of dd3d_loss_grad_args, the op list of
LossPlan(grads=True) and the argument checks of FusedDD3DLoss."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import loss_grad_cases as GC
from tests import loss_grad_oracle as GO
from tests import loss_oracle as LO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small_nusc_case():
    """The 4 x 4 single-level nuScenes case of tests/test_losses.py, with a valid attribute and speed and a depth inside the clamp."""
    model = GC.cpu_model("dd3d_nusc_dla34")
    p = dict(LO.settings(model), num_levels=1, beta=0.05)
    g = torch.Generator().manual_seed(0)
    C_, H, W = 10, 4, 4
    maps = {"logits0": torch.randn(1, C_, H, W, generator=g), "box2d_reg0": torch.rand(1, 4, H, W, generator=g) * 20,
            "centerness0": torch.randn(1, 1, H, W, generator=g), "quat0": torch.randn(1, 4 * C_, H, W, generator=g),
            "ctr0": torch.randn(1, 2 * C_, H, W, generator=g), "depth0": torch.randn(1, C_, H, W, generator=g) * 1000,
            "size0": torch.randn(1, 3 * C_, H, W, generator=g), "conf0": torch.randn(1, C_, H, W, generator=g),
            "attr0": torch.randn(1, 3, H, W, generator=g), "speed0": torch.rand(1, 1, H, W, generator=g)}
    loc = [torch.tensor([[x * 8.0, y * 8.0] for y in range(H) for x in range(W)])]
    K = torch.tensor([[700.0, 0, 16], [0, 700.0, 16], [0, 0, 1]])
    iK = torch.linalg.inv(K)[None]
    px = float(torch.sqrt(iK[0, 0, 0]**2 + iK[0, 1, 1]**2)) * p["focal_factor"]
    maps["depth0"][0, 4, 1:3] = torch.tensor([[20.0, 35.0, 50.0, 5.0], [60.0, 9.0, 70.0, 11.0]]) * px  # class 4: inside [MIN, MAX]
    gt = {"boxes": torch.tensor([[0.0, 0.0, 30.0, 30.0]]), "classes": torch.tensor([4]), "quat": torch.tensor([[1.0, 0, 0, 0]]),
          "proj_ctr": torch.tensor([[15.0, 15.0]]), "depth": torch.tensor([[30.0]]), "size": torch.tensor([[1.0, 2.0, 1.5]]),
          "inv_K": iK, "attributes": torch.tensor([1]), "speeds": torch.tensor([0.4])}
    t = LO.prepare_targets(loc, [gt], [8], C_, [], True, 1.5, True, True, 3)
    return maps, t, iK, p


def test_oracle_autograd_matches_central_differences():
    maps, t, iK, p = _small_nusc_case()
    assert t["pos_inds"].numel() >= 4
    g = GO.head_grads(maps, t, iK, p)
    kink = GO.near_kink(maps, t, iK, p)
    masked = set(t["pos_inds"][kink].tolist())
    w = torch.ones(10, dtype=torch.float64)
    m64 = {k: v.double().clone() for k, v in maps.items()}
    t64 = GO._cast(t, torch.float64)

    base = {k: v.clone() for k, v in m64.items()}

    def total():
        # the function the reference differentiates: loss_conf3d sees the entangled error as a constant (its detach), so its conf
        # target comes from the unperturbed decode inputs
        out = LO.losses(m64, t64, iK.double(), p)
        frozen = {k: (base[k] if k[:-1] in ("quat", "ctr", "depth", "size") else v) for k, v in m64.items()}
        out["loss_conf3d"] = LO.losses(frozen, t64, iK.double(), p)["loss_conf3d"]
        return float(sum(w[GO.OUT_INDEX[k]] * v for k, v in out.items()))

    rng = np.random.default_rng(0)
    checked = nonzero = 0
    for key, gk in g.items():
        gmax = float(gk.abs().max())
        flat, gf = m64[key].view(-1), gk.reshape(-1)
        cand = torch.nonzero(gf).reshape(-1).tolist()
        cand = [int(i) for i in rng.permutation(cand)[:24]] + [int(i) for i in rng.integers(0, flat.numel(), 4)]
        HW = 16
        for i in cand:
            if (i % HW) in masked:  # (one image, one level: the target index is the location)
                continue
            x0 = float(flat[i])
            h = 1e-6 * max(1.0, abs(x0))
            flat[i] = x0 + h
            up = total()
            flat[i] = x0 - h
            dn = total()
            flat[i] = x0
            fd = (up - dn) / (2 * h)
            assert abs(fd - float(gf[i])) <= 1e-6 * max(gmax, 1e-12) + 1e-4 * abs(float(gf[i])), (key, i, fd, float(gf[i]))
            checked += 1
            nonzero += float(gf[i]) != 0.0
    assert checked > 150 and nonzero > 120
    for fam in ("quat", "ctr", "depth", "size", "conf", "attr", "speed", "box2d_reg", "centerness"):
        assert float(g[fam + "0"].abs().max()) > 0.0, fam  # every family carries a gradient in this case


@pytest.mark.parametrize("name", list(GC.REFERENCE_CASES))
def test_oracle_matches_reference_modules_gradients(name):
    """The oracle's float32 autograd against torch autograd through the reference's own FCOS2DLoss / FCOS3DLoss / NuscenesLoss."""
    case = GC.reference_case(name)
    z = case.golden
    pos = torch.from_numpy(z["pos_inds"])
    assert torch.equal(pos, case.targets["pos_inds"])
    g32, g64, keep = case.ref(torch.float32), case.ref(torch.float64), case.keep_rows()
    for fam in GO.families(case.p):
        a = GO.flat_family(g32, fam, case.p)
        bar, d32, gmax = GO.bar(GO.flat_family(g64, fam, case.p), a, keep)
        if fam == "logits":
            mine, ref, kp = a, torch.from_numpy(z["dense_logits"]), keep
        else:
            mine, ref, kp = a[pos], torch.from_numpy(z["pos_" + fam]), keep[pos]
            rest = torch.ones(a.shape[0], dtype=torch.bool)
            rest[pos] = False
            assert float(a[rest].abs().max()) == 0.0
        if mine.numel():
            # two float32 autograds of the same function in different operation orders: each within d32 of the float64 gradient
            assert float((mine - ref)[kp].abs().max()) <= 2 * max(d32, 2.0**-23 * gmax), (name, fam)
            assert bool(np.isfinite(ref.numpy()).all())
        if case.num_pos and fam != "logits":
            assert float(ref.abs().max()) > 0.0, (name, fam)  # (the quaternion path is attached: the shim's scipy conversion is replaced)


def test_kink_counts_of_the_gpu_cases_stay_under_the_cap():
    from tests.test_losses_gpu import GOLDEN_CASES
    for name in GOLDEN_CASES:
        case = GC.golden_case(name)
        n, k = case.num_pos, int(case.kink.sum())
        assert n > 20 and k <= GC.KINK_CAP * n, (name, n, k)
        assert all(bool(torch.isfinite(v).all()) for v in case.ref().values())
    for hw in ((4, 4), (1, 257)):
        case = GC.handmade_case(*hw)
        assert case.num_pos == len(case.specs)
        tie = [i for i, s in enumerate(case.specs) if s.get("reg") == "tie"][0]
        exact = [i for i, s in enumerate(case.specs) if "depth_exact" in s][0]
        assert bool(case.kink[tie]) and bool(case.kink[exact])  # on a non-smooth point by construction


def _finite(d):
    return all(bool(torch.isfinite(v).all()) for v in d.values())


@pytest.mark.parametrize("name,key", GC.SETTINGS_ROWS)
def test_settings_rows_are_not_vacuous(name, key):
    """Pins the GT seed of every (case, settings row) the GPU tests run: enough positives, few of them under the kink mask, finite
    float64 / float32 reference gradients and a finite loss dict."""
    case = GC.settings_case(name, key)
    n, k = case.num_pos, int(case.kink.sum())
    fin64, fin32, finl = _finite(case.ref(torch.float64)), _finite(case.ref(torch.float32)), _finite(case.losses()) and _finite(case.losses(torch.float64))
    print(f"[settings] {name} {key}: positives {n}, masked {k} ({100.0 * k / max(n, 1):.2f} %), finite g64 {fin64} g32 {fin32} losses {finl}")
    assert n > 20 and k <= GC.KINK_CAP * n, (name, key, n, k)
    assert fin64 and fin32 and finl
    over = GC.SETTINGS[key]["DD3D"]
    if "FCOS2D" in over:  # the row's values reached the oracle's settings
        assert (case.p["alpha"], case.p["gamma"]) == (over["FCOS2D"]["LOSS"].get("ALPHA", 0.25), over["FCOS2D"]["LOSS"]["GAMMA"])
    if "nusc" in name:
        assert (case.p["w_attr"], case.p["w_speed"]) == (0.4, 2.5)


def test_proj_ctr_z_residuals_do_not_count_as_kinks():
    """Plain L1 (beta < 1e-5) has its kink at residual 0, and the proj_ctr group's eight z residuals are 0 whatever the prediction:
    counting them would mask every positive.  With them skipped the row is under the cap; moving a z residual by hand still masks."""
    case = GC.settings_case(GC.SETTINGS_KITTI, "beta_tiny")
    assert case.p["beta"] < 1e-5 and int(case.kink.sum()) <= GC.KINK_CAP * case.num_pos
    # the structural zeros are there: the group's z residuals of every positive are exactly 0
    t, pos = GO._cast(case.targets, torch.float64), case.targets["pos_inds"]
    tb = t["box3d"][pos]
    tq, tc, td, ts, tK = tb[:, 0:4], tb[:, 4:6], tb[:, 6:7], tb[:, 7:10], tb[:, 10:19].reshape(-1, 3, 3)
    moved = LO._corners(tq, tc + 3.0, td, ts, tK) - LO._corners(tq, tc, td, ts, tK)
    assert float(moved[..., 2].abs().max()) == 0.0 and float(moved[..., :2].abs().min()) > 0.0
    # a K^-1 whose third row reaches the centre makes those residuals count again
    skew = case.inv_K.clone()
    skew[:, 2, 0] = 1e-9
    t2 = dict(case.targets)
    t2["box3d"] = case.targets["box3d"].clone()
    t2["box3d"][:, 10:19] = skew[case.targets["im_inds"]].reshape(-1, 9)
    assert int(GO.near_kink(case.maps, t2, case.inv_K, case.p).sum()) > GC.KINK_CAP * case.num_pos


def test_saturated_and_poisoned_cases_on_the_cpu():
    for hw in ((4, 4), (1, 257)):
        for gamma in GC.SATURATED_GAMMAS:
            case = GC.handmade_case(*hw, gamma=gamma)
            assert case.num_pos == len(case.specs) == 6 and case.p["gamma"] == gamma
            lg = LO.flat(case.maps, "logits", 1, case.p["num_classes"])
            bg = case.targets["labels"] == case.p["num_classes"]
            assert int((lg[bg] == -60.0).all(1).sum()) == 2 and int((lg[~bg] == 60.0).sum()) == 2 and int((lg[~bg] == -60.0).sum()) == 1
            assert _finite(case.ref(torch.float64)) and _finite(case.ref(torch.float32)) and _finite(case.losses(torch.float64))
    for name in GC.POISONED_CASES:
        case, clean = GC.poisoned_case(name), GC.golden_case(name)
        j = case.poisoned
        n = int(case.targets["pos_inds"][j])
        assert not bool(clean.kink[j]) and 64 <= n % 256 < 192 and ("nusc" not in name or int(case.targets["im_inds"][n]) != 0)
        ref = case.losses(torch.float64)
        nan = {k for k, v in ref.items() if bool(torch.isnan(v))}
        assert nan == {"loss_conf3d", "loss_box3d_quat"}, nan
        g64 = case.ref(torch.float64)
        for fam in GO.families(case.p):
            g = GO.flat_family(g64, fam, case.p)
            rest = torch.ones(g.shape[0], dtype=torch.bool)
            rest[n] = False
            assert bool(torch.isfinite(g[rest]).all()), (name, fam)
            assert bool(torch.isnan(g[n]).any()) == (fam in ("quat", "ctr", "conf")), (name, fam)


def test_loss_grad_args_layout_matches_header(hiplib, tmp_path):
    from dd3d_amd import hip
    cls = hip.LossGradArgs
    names = ["d_cls", "d_box2d", "d_box3d", "upstream", "denoms"]
    out = (C.c_int64 * 8)()
    n = hiplib.dd3d_loss_grad_layout(out, 8)
    assert n == len(names) + 1 and [f[0] for f in cls._fields_] == names and out[0] == C.sizeof(cls)
    assert [out[i + 1] for i in range(len(names))] == [getattr(cls, f).offset for f in names] and out[6] == -1
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "dd3d_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(dd3d_loss_grad_args));', '  printf("ndenoms %d\\n", DD3D_LOSS_GRAD_DENOMS);']
    lines += [f'  printf("{f} %zu\\n", offsetof(dd3d_loss_grad_args, {f}));' for f in names] + ['  return 0;', '}']
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines))
    exe = str(tmp_path / "abi")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True)
    got = dict(l.split(" ", 1) for l in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) and int(got["ndenoms"]) == hip.LOSS_GRAD_DENOMS
    for f in names:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert "dd3d_loss_backward" in hip.EXPORTS and "dd3d_loss_grad_layout" in hip.EXPORTS and hip.ABI_VERSION == 7


def test_loss_plan_ops_with_and_without_grads():
    from dd3d_amd.engine.losses import LossPlan
    model = GC.cpu_model("dd3d_nusc_dla34")
    plain = LossPlan(model, 2, 128, 224, device="cpu", dry_run=True)
    with_g = LossPlan(model, 2, 128, 224, device="cpu", dry_run=True, grads=True)
    names = [op.name for op in plain.ops]
    assert names[-2:] == ["loss_assign", "loss_terms"] and "loss_backward" not in names
    assert [op.name for op in with_g.ops] == names + ["loss_backward"]
    assert [tuple(t.shape) for t in with_g.d_cls] == [tuple(m.t.shape) for m in with_g.cls_maps]
    assert [tuple(t.shape) for t in with_g.d_b3d] == [tuple(m.t.shape) for m in with_g.b3d_maps]
    assert with_g.upstream.tolist() == [1.0] * 16 and with_g.grad_denoms.numel() == 4
    g = with_g.head_grads()
    L = len(with_g.features)
    assert set(g) == {f"{k}{l}" for k in GO.FAMILIES for l in range(L)}
    assert tuple(g["quat0"].shape) == (2, 40, with_g.features[0].H, with_g.features[0].W) and tuple(g["speed0"].shape)[1] == 1
    with pytest.raises(RuntimeError, match="grads=True"):
        plain.head_grads()
    import inspect
    assert inspect.signature(model.compute_losses).parameters["head_grads"].default is False


def test_fused_loss_argument_errors():
    from dd3d_amd.losses import FusedDD3DLoss, check_head_maps
    case = GC.golden_case("dla34_kitti_variant_egocentric_agnostic")
    f = FusedDD3DLoss(case.model)
    with pytest.raises(ValueError, match="cpu"):
        f(case.maps, case.inv_K, case.gt)  # CPU tensors
    missing = {k: v for k, v in case.maps.items() if k != "conf2"}
    with pytest.raises(ValueError, match="conf2"):
        f(missing, case.inv_K, case.gt)
    with pytest.raises(ValueError, match="dict"):
        f([1, 2], case.inv_K, case.gt)
    meta = {k: v.to("meta") for k, v in case.maps.items()}
    with pytest.raises(ValueError, match="meta"):
        check_head_maps(case.model, meta)
    # shapes and dtypes are checked before the device: use a stand-in whose device reads "cuda"
    class Fake(torch.Tensor):
        @property
        def device(self):
            return torch.device("cuda")

    fake = {k: v.as_subclass(Fake) for k, v in case.maps.items()}
    fams, level_hw, B = check_head_maps(case.model, fake)
    assert fams == ["logits", "box2d_reg", "centerness", "quat", "ctr", "depth", "size", "conf"] and B == 1 and level_hw == case.level_hw
    bad = dict(fake)
    bad["quat1"] = fake["quat1"][:, :3]
    with pytest.raises(ValueError, match="quat1 has shape"):
        check_head_maps(case.model, bad)
    bad = dict(fake)
    bad["depth0"] = fake["depth0"].double().as_subclass(Fake)
    with pytest.raises(ValueError, match="float32"):
        check_head_maps(case.model, bad)
    bad = dict(fake)
    bad["size0"] = fake["size0"][0]
    with pytest.raises(ValueError, match="4-d"):
        check_head_maps(case.model, bad)
