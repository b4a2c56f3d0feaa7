"""A float64 restatement of the reliability-weighted seg loss -- not a test.  What tests/test_seg_reliability_cpu.py
and tests/test_seg_reliability_gpu.py compare the product against:

  weight_f32 / weight_f64   the per-pixel weight of cosa_label_reliability: numpy float32 in the kernel's exact operation order, and float64
  weight_stats              the fixed-point counters {Sum_bg rint(w 2^32), n_bg, Sum_fg rint(w 2^32), n_fg}
  ratio_f64                 the clamped distance r itself (the tests' own input checks)
  weighted_ce_f64           utils/seg_helper.py:823-835 on the bilinearly up-sampled logits, in float64, with its gradient w.r.t. the
                            low-resolution logits (F.interpolate and autograd in float64)
"""
import numpy as np
import torch
import torch.nn.functional as F


def _gather(cam, y, mask, C, dt):
    """-> (l int64 [b,S,S], m = max_c y[c] cam[c], v = y[l-1] cam[l-1] (0 where l is no class), bg, fg) in dtype dt"""
    cam = cam.astype(dt) * y.astype(dt)[:, :, None, None]
    l = mask.astype(np.float32).astype(np.int64)
    bg, fg = l == 0, (l >= 1) & (l <= C)
    with np.errstate(invalid="ignore"):
        m = cam.max(axis=1)                                            # (np.max keeps a NaN, as the kernel's maximum does)
    v = np.take_along_axis(cam, np.clip(l - 1, 0, C - 1)[:, None], axis=1)[:, 0]
    return l, m, v, bg, fg


def _weight(cam, y, mask, hi, lo, beta, floor, dt):
    C = cam.shape[1]
    l, m, v, bg, fg = _gather(cam, y, mask, C, dt)
    hi, lo, one = dt(np.float32(hi)), dt(np.float32(lo)), dt(1)
    beta, floor = dt(np.float32(beta)), dt(np.float32(floor))
    omf = dt(np.float32(1) - np.float32(floor))                        # (formed once in fp32, as the entry point forms it)
    with np.errstate(all="ignore"):
        r = np.where(bg, (lo - m) / lo, (v - hi) / (one - hi)).astype(dt)
        r = np.where(r != r, dt(0), np.minimum(np.maximum(r, dt(0)), dt(1))).astype(dt)
        if beta == 0:
            u = np.ones_like(r)
        elif beta == 1:
            u = r
        else:
            u = np.where(r == 0, dt(0), np.exp2(beta * np.log2(np.where(r == 0, dt(1), r)))).astype(dt)
        w = (floor + (omf * u).astype(dt)).astype(dt)
    return np.where(bg | fg, w, dt(0)).astype(dt), r, bg, fg


def weight_f32(cam, y, mask, hi, lo, beta, floor):
    """numpy float32, one rounding per operation, in the kernel's order -> w float32 [b,S,S]"""
    return _weight(np.asarray(cam, np.float32), np.asarray(y, np.float32), np.asarray(mask), hi, lo, beta, floor, np.float32)[0]


def weight_f64(cam, y, mask, hi, lo, beta, floor):
    """the same formula on the same fp32 inputs and settings, evaluated in float64 -> w float64 [b,S,S]"""
    return _weight(np.asarray(cam, np.float32), np.asarray(y, np.float32), np.asarray(mask), hi, lo, beta, floor, np.float64)[0]


def ratio_f64(cam, y, mask, hi, lo):
    """-> (r float64 [b,S,S] after the clamp, labelled bool [b,S,S])"""
    _, r, bg, fg = _weight(np.asarray(cam, np.float32), np.asarray(y, np.float32), np.asarray(mask), hi, lo, 1.0, 0.0, np.float64)
    return r, bg | fg


def weight_stats(w, mask, C):
    """w [b,S,S] (any float dtype) -> int64 [4] = {Sum_bg rint(w 2^32), n_bg, Sum_fg rint(w 2^32), n_fg}"""
    l = np.asarray(mask).astype(np.float32).astype(np.int64)
    bg, fg = l == 0, (l >= 1) & (l <= C)
    q = np.rint(np.asarray(w, np.float64) * 4294967296.0).astype(np.int64)
    return np.array([q[bg].sum(), bg.sum(), q[fg].sum(), fg.sum()], dtype=np.int64)


def _wce(up, mask, w, a, ignore_index=255):
    """seg_weightloss in float64 on full-resolution logits `up` [b,K,S,S]"""
    K = up.shape[1]
    lab = mask.long()
    logp = F.log_softmax(up, dim=1)
    ce = -logp.gather(1, lab.clamp(0, K - 1).unsqueeze(1)).squeeze(1)
    bg, fg = lab == 0, (lab != 0) & (lab != ignore_index)
    assert int(((lab >= K) & (lab != ignore_index)).sum()) == 0, "labels outside the classes are not part of this restatement"
    wd = w.double()
    bg_loss = (ce * wd * bg).sum() / (bg.sum() + 1e-6)
    fg_loss = (ce * wd * fg).sum() / (fg.sum() + 1e-6)
    return (1 - a) * bg_loss + a * fg_loss


def weighted_ce_f64(seg_lr, mA, mB, relA, relB, S, a, b):
    """(1 - b) seg_weightloss(up, mA, relA, a) + b seg_weightloss(up, mB, relB, a) of the bilinearly up-sampled logits (mB None: the first
    term alone) -> (loss float, d loss / d seg_lr float64)"""
    lr = seg_lr.double().clone().requires_grad_(True)
    up = F.interpolate(lr, size=(S, S), mode="bilinear", align_corners=False)
    l = _wce(up, mA, relA, a)
    if mB is not None:
        l = (1 - b) * l + b * _wce(up, mB, relB, a)
    (g,) = torch.autograd.grad(l, lr)
    return float(l.detach()), g


def weighted_ce_full_f64(pred, mask, w, a):
    """seg_weightloss on full-resolution logits in float64 -> (loss float, d loss / d pred float64): the golden vectors' restatement"""
    p = pred.double().clone().requires_grad_(True)
    l = _wce(p, mask, w, a)
    (g,) = torch.autograd.grad(l, p)
    return float(l.detach()), g
