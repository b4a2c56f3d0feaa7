"""--camloss_version v2 | v3 on the host: the float64 restatement (tests/camloss_ref.py) against the golden vectors the
reference wrote (tests/golden/camloss.npz) and, where the reference tree is present, against the live reference; the closed-form
gradients against autograd; the torch compositions of cosa_amd.utils.seg_helper; the trainer's two new fields."""
import numpy as np
import pytest
import torch

import camloss_ref as R
from cosa_amd.utils import seg_helper as sh

t64 = lambda a: torch.from_numpy(np.asarray(a)).double()


@pytest.fixture(scope="module")
def gold(golden):
    return golden("camloss")


def _targets(gold):
    return R.resize(t64(gold["seg_ps"])[:, 1:], *gold["cam"].shape[-2:])


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if want.ndim == 0:
        err = abs(got - want) / abs(want)
    else:
        err = np.abs(got - want).max() / np.abs(want).max()
    print(f"{what}: {err:.3e}")
    assert err <= 1e-10, (what, err)


def test_golden_inputs_hold_the_special_planes(gold):
    cam, lab = gold["cam"], gold["v3_label_50"]
    assert cam[0, 0].min() > 0 and cam[0, 1].max() <= 0
    assert (cam[1, 0] == cam[1, 0].max()).sum() == 2 and cam[1, 0].max() > 0
    assert cam[1, :, 0, 0].max() <= 0
    for share in ((lab == 255).mean(), (lab == 0).mean(), ((lab != 0) & (lab != 255)).mean()):
        assert 0.05 <= share <= 0.90, share


def test_restatement_against_golden(gold):
    x, seg = t64(gold["cam"]), t64(gold["seg_ps"])
    y = _targets(gold)
    _close(R.v2_loss(x, y), gold["v2_loss"], "v2 loss")
    _close(R.v2_grad(x, y), gold["v2_grad"], "v2 grad")
    for tag, thre in (("25", 0.25), ("50", 0.5)):
        lab = R.label_of(seg, thre)
        assert np.array_equal(lab.numpy().astype(np.uint8), gold["v3_label_" + tag])
        _close(R.v3_loss(x, lab), gold["v3_loss_" + tag], "v3 loss " + tag)
        _close(R.v3_grad(x, lab), gold["v3_grad_" + tag], "v3 grad " + tag)
    # the two positions of the doubled maximum are told apart (the first takes the maximum's share); the all-non-positive plane and the dead cell get none
    g = gold["v3_grad_25"]
    first, second = np.flatnonzero(gold["cam"][1, 0].reshape(-1) == gold["cam"][1, 0].max())
    assert g[1, 0].reshape(-1)[first] != g[1, 0].reshape(-1)[second]
    assert not g[0, 1].any() and not g[1, :, 0, 0].any() and not gold["v2_grad"][0, 1].any()


def test_restatement_against_live_reference(gold):
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip("reference tree not present")
    ref = ref_loader.seg_helper()
    seg = t64(gold["seg_ps"])
    for name, fn, mine in (("v2", lambda x: ref.cam_lossv2(x, seg), lambda x: R.v2_loss(x, _targets(gold))),
                           ("v3", lambda x: ref.cam_lossv3_wrap(x, seg, 0.5), lambda x: R.v3_loss(x, R.label_of(seg, 0.5)))):
        xa, xb = (t64(gold["cam"]).requires_grad_(True) for _ in range(2))
        la, lb = fn(xa), mine(xb)
        la.backward()
        lb.backward()
        _close(lb.item(), la.item(), name + " loss (live)")
        _close(xb.grad, xa.grad, name + " grad (live)")


@pytest.mark.parametrize("shape", [(2, 5, 4, 4), (2, 3, 5, 7)])
def test_closed_form_gradients_against_autograd(shape):
    rng = np.random.default_rng(3)
    B, C, h, w = shape
    S = 8 * max(h, w)
    x = t64(R.special_cam(rng, B, C, h, w))
    y = t64(rng.uniform(0, 1, shape))
    lab = torch.from_numpy(rng.choice([0, 1, C, 255], size=(B, S, S)))
    for loss, grad, tgt in ((R.v2_loss, R.v2_grad, y), (R.v3_loss, R.v3_grad, lab)):
        xa = x.clone().requires_grad_(True)
        loss(xa, tgt).backward()
        err = (grad(x, tgt) - xa.grad).abs().max() / xa.grad.abs().max()
        assert err <= 1e-12, (loss.__name__, float(err))


def test_torch_compositions_against_golden(gold):
    """the op-by-op path of seg_helper (fused_losses=False, host tensors) in float64, through the public names"""
    seg = t64(gold["seg_ps"])
    for name, fn in (("v2", lambda x: sh.cam_lossv2(x, seg)), ("v3_25", lambda x: sh.cam_lossv3_wrap(x, seg, 0.25)),
                     ("v3_50", lambda x: sh.cam_lossv3_wrap(x, seg, seg_confident_thre=0.5))):
        x = t64(gold["cam"]).requires_grad_(True)
        loss = fn(x)
        loss.backward()
        # (the compositions compute in fp32, as cam_loss does: the reference's own fp32 error is 3e-8 / 3e-7)
        k = name.partition("_")
        lw, gw = gold[f"{k[0]}_loss" + ("_" + k[2] if k[2] else "")], gold[f"{k[0]}_grad" + ("_" + k[2] if k[2] else "")]
        assert abs(loss.item() - lw) <= 1e-5 * abs(lw), name
        assert np.abs(x.grad.numpy() - gw).max() <= 1e-4 * np.abs(gw).max(), name
    assert np.array_equal(sh._cam_label_torch(seg, 0.5).numpy().astype(np.uint8), gold["v3_label_50"])
    # the reference's signatures
    import inspect
    assert list(inspect.signature(sh.cam_lossv2).parameters) == ["cam", "seg_ps", "detach"]
    assert list(inspect.signature(sh.cam_lossv3).parameters) == ["cam", "seg_label", "detach", "cambgmax"]
    assert list(inspect.signature(sh.cam_lossv3_wrap).parameters) == ["cam", "seg_ps", "seg_confident_thre"]
    x = t64(gold["cam"])
    assert torch.isfinite(sh.cam_lossv2(x, seg, detach=True)) and torch.isfinite(sh.cam_lossv3(x, sh._cam_label_torch(seg, 0.5), True, False))


def test_dropin_exposes_the_three_functions():
    import importlib
    import os
    import sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_dropin_seg_helper", os.path.join(here, "dropin", "utils", "seg_helper.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in ("cam_lossv2", "cam_lossv3", "cam_lossv3_wrap"):
        assert getattr(mod, name) is getattr(sh, name)


def test_label_cases_on_the_host():
    """the label kernel's committed cases: the float64 label's ignore share at (1.0, 0.5), and the fp32 restatement inside the excusal cap"""
    scales, cls = R.label_case()
    for T, thre in R.LABEL_SETTINGS:
        for after in (False, True):
            lab64, excus = R.label_from_scales([t64(s) for s in scales], t64(cls), R.LABEL_S, T, thre, after)
            lab32, _ = R.label_from_scales([torch.from_numpy(s) for s in scales], torch.from_numpy(cls), R.LABEL_S, np.float32(T), np.float32(thre), after)
            diff = lab32 != lab64
            share = float((lab64 == 255).float().mean())
            print(f"T {T} thre {thre} after {after}: ignore {share:.3f}, excusable {float(excus.float().mean()):.2e}, fp32 differs at {int(diff.sum())}")
            if (T, thre) == (1.0, 0.5):
                assert 0.10 <= share <= 0.90, share
            assert not bool((diff & ~excus).any())
            assert float(excus.float().mean()) <= R.LABEL_EXCUSED_MAX
            assert bool((lab64[0] == 0).all()) or after      # image 0 has no class: background everywhere unless the softmax saw them


def test_default_args_and_unknown_version():
    from cosa_amd import train_step as ts
    a = ts.default_args()
    assert a.camloss_version == "v1" and a.segconf_thre == 0.25
    assert ts.default_args(camloss_version="v3", segconf_thre=0.5).segconf_thre == 0.5
    assert ts.camloss_version(ts.default_args(camloss_version="v2")) == "v2"
    with pytest.raises(ValueError, match="camloss_version"):
        ts.CoSATrainer(ts.default_args(camloss_version="v4", crop_size=64, compute_dtype=torch.float32), torch.device("cpu"))
    with pytest.raises(ValueError, match="segconf_thre"):
        ts.CoSATrainer(ts.default_args(camloss_version="v3", segconf_thre=float("nan")), torch.device("cpu"))
