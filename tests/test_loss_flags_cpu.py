"""CPU suite of the loss-flag settings (--segfg_alpha, --aux_cam2seg_alpha, --aux_cam2seg, --after_softmax): the oracle functions the GPU
tests compare against are pinned to the reference's own outputs (tests/golden/loss_flags.npz, written by tools/gen_loss_flags_golden.py),
and the table of blend weights the fused kernels take is pinned to the reference's expression."""
import numpy as np
import pytest
import torch

from oracle import torch_oracle as to


@pytest.mark.parametrize("tag,alpha", [("a0", 0.0), ("a03", 0.3), ("a1", 1.0)])
def test_oracle_seg_loss_at_other_fg_alphas_vs_reference_golden(golden, tag, alpha):
    """utils/seg_helper.py:800-813 at fg_alpha 0 / 0.3 / 1: fp32 sums over 2 x 64 x 64 pixels in another order than the reference's -- 1e-6
    relative (measured when the file was written: 8e-8)"""
    g = golden("loss_flags")
    pred, mask = torch.from_numpy(g["segloss_pred"]), torch.from_numpy(g["segloss_mask"].astype(np.float32))
    assert float(to.seg_loss(pred, mask, fg_alpha=alpha)) == pytest.approx(float(g["segloss_" + tag]), rel=1e-6)


def test_product_seg_loss_at_other_fg_alphas_vs_reference_golden(golden):
    """the torch path's seg_loss (what `fused_losses=False` trainers run) against the same vectors"""
    from cosa_amd.utils import seg_helper
    g = golden("loss_flags")
    pred, mask = torch.from_numpy(g["segloss_pred"]), torch.from_numpy(g["segloss_mask"].astype(np.float32))
    for tag, alpha in (("a0", 0.0), ("a03", 0.3), ("a1", 1.0)):
        assert float(seg_helper.seg_loss(pred, mask, fg_alpha=alpha)) == pytest.approx(float(g["segloss_" + tag]), rel=1e-6)


def test_oracle_after_softmax_refine_and_cam_loss_vs_reference_golden(golden):
    """utils/seg_helper.py:558-561 (softmax over all channels, then absent classes zeroed) and cam_loss on it (:593-602); image 0 has no
    class present, image 1 two"""
    g = golden("loss_flags")
    seg, labels = torch.from_numpy(g["refine_seg"]), torch.from_numpy(g["refine_labels"])
    assert labels.sum(1).tolist() == [0.0, 2.0]
    out = to.seg_refine_by_label(seg, labels, float(g["temp"]), after_softmax=True)
    assert torch.equal(out, torch.from_numpy(g["refine_after"]))
    assert float(out[0, 1:].abs().max()) == 0.0 and float(out[1, 1:].max()) > 0.5
    cam = torch.from_numpy(g["camloss_cam"])
    assert float(to.cam_loss(cam, out)) == pytest.approx(float(g["camloss_after"]), rel=1e-6)
    # the other branch on the same input is a different function: the vectors cannot pass by accident
    assert not torch.allclose(to.seg_refine_by_label(seg, labels, float(g["temp"])), out, atol=1e-3)


@pytest.mark.parametrize("a", [0.0, 0.3, 0.5, 0.7, 1.0])
@pytest.mark.parametrize("b", [0.0, 0.25, 0.5, 1.0])
def test_blend_weight_table(a, b):
    """(wA_bg, wA_fg, wB_bg, wB_fg) = ((1-b)(1-a), (1-b) a, b (1-a), b a)  (main.py:200-203 x seg_helper.py:813): applied to any four
    terms it is the reference's two-level blend; the weights are in [0, 1] and sum to 1"""
    from cosa_amd.utils import seg_helper
    w = seg_helper.seg_blend_weights(a, b)
    assert w == ((1 - b) * (1 - a), (1 - b) * a, b * (1 - a), b * a)
    assert all(0.0 <= x <= 1.0 for x in w) and sum(w) == pytest.approx(1.0, abs=1e-15)
    bgA, fgA, bgB, fgB = 1.25, 0.5, 3.0, 0.125
    ref = (1 - b) * ((1 - a) * bgA + a * fgA) + b * ((1 - a) * bgB + a * fgB)
    assert w[0] * bgA + w[1] * fgA + w[2] * bgB + w[3] * fgB == pytest.approx(ref, rel=1e-14)


def test_blend_weight_table_edges():
    from cosa_amd.utils import seg_helper
    assert seg_helper.seg_blend_weights() == (0.25, 0.25, 0.25, 0.25)              # the defaults, exactly
    assert seg_helper.seg_blend_weights(0.0, 0.0) == (1.0, 0.0, 0.0, 0.0)
    assert seg_helper.seg_blend_weights(1.0, 1.0) == (0.0, 0.0, 0.0, 1.0)
    assert seg_helper.seg_blend_weights(1.0, 0.0) == (0.0, 1.0, 0.0, 0.0)
    assert seg_helper.seg_blend_weights(0.0, 1.0) == (0.0, 0.0, 1.0, 0.0)
    # no auxiliary label map: b = 0 whatever --aux_cam2seg_alpha says
    assert seg_helper.seg_blend_weights(0.3, 0.5, has_aux=False) == (0.7, 0.3, 0.0, 0.0)
    assert seg_helper.seg_blend_weights(0.5, 0.9, has_aux=False) == (0.5, 0.5, 0.0, 0.0)
    for bad in ((-0.1, 0.5), (1.5, 0.5), (0.5, -0.25), (0.5, 1.01), (float("nan"), 0.5), (0.5, float("inf"))):
        with pytest.raises(ValueError):
            seg_helper.seg_blend_weights(*bad)
