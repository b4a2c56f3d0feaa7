"""The soft-label seg loss restated in float64 for the tests: the target from F.interpolate and flips, summed exactly
as the reference's multi_scale_camseg sums the teacher's passes (utils/seg_helper.py:553-568 of the reference: up(seg) + flip(up(seg_flip)) per
scale, scale after scale); the loss written the way the reference's seg_softloss writes it (boolean row selection, :837-861) with the
(count + 1e-6) denominators; its gradient from autograd.  Nothing here calls cosa_amd."""
import numpy as np
import torch
import torch.nn.functional as F


def targets_f64(seg_scales, cls_label, S, temp):
    """seg_scales: list of [2B,K,h_i,w_i] (original batch, then the flipped one), any float dtype -> q float64 [B,K,S,S]"""
    B = seg_scales[0].shape[0] // 2
    z = None
    for s in seg_scales:
        up = F.interpolate(s.double().cpu(), size=(S, S), mode="bilinear", align_corners=False)
        v = up[:B] + torch.flip(up[B:], dims=[-1])
        z = v if z is None else z + v
    z = z / (2.0 * len(seg_scales) * float(temp))
    present = torch.cat([torch.ones(B, 1, dtype=torch.bool), cls_label.cpu() != 0], dim=1)
    q = torch.zeros_like(z)
    for b in range(B):
        keys = torch.nonzero(present[b])[:, 0]
        q[b, keys] = torch.softmax(z[b, keys], dim=0)
    return q


def sets(q, boxes, conf):
    """-> (bg, fg) bool [B,S,S]: inside the box, max q > conf, first argmax == 0 / != 0"""
    B, _, S, _ = q.shape
    value, label = torch.max(q, dim=1)
    inside = torch.zeros(B, S, S, dtype=torch.bool)
    for b, (y0, y1, x0, x1) in enumerate(torch.as_tensor(boxes).tolist()):
        inside[b, y0:y1, x0:x1] = True
    keep = inside & ~(value <= conf)
    return keep & (label == 0), keep & (label != 0)


def loss_full_f64(up, q, bg, fg, alpha):
    """the loss on full-resolution float64 logits `up` [B,K,S,S], seg_softloss's way: rows selected by the set, -log_softmax * q summed over
    the classes, summed over the rows and divided by (rows + 1e-6)"""
    rows, qr = up.permute(0, 2, 3, 1), q.permute(0, 2, 3, 1)

    def one(sel):
        per = -(F.log_softmax(rows[sel], dim=1) * qr[sel]).sum(dim=1)
        return per.sum() / (per.shape[0] + 1e-6)
    return (1 - alpha) * one(bg) + alpha * one(fg)


def loss_and_grad_f64(seg_lr, seg_scales, cls_label, boxes, S, temp, conf, alpha):
    """-> (loss float, grad float64 [B,K,h,w], n_bg, n_fg, q): the whole term on the student's low-res logits"""
    q = targets_f64(seg_scales, cls_label, S, temp)
    bg, fg = sets(q, boxes, conf)
    x = seg_lr.detach().double().cpu().requires_grad_(True)
    loss = loss_full_f64(F.interpolate(x, size=(S, S), mode="bilinear", align_corners=False), q, bg, fg, alpha)
    loss.backward()
    return float(loss.detach()), x.grad.clone(), int(bg.sum()), int(fg.sum()), q


def full_f64(pred, probs, alpha):
    """seg_softloss on full-resolution inputs in float64 -> (loss, grad): the golden vectors' restatement"""
    x = torch.as_tensor(pred).double().requires_grad_(True)
    q = torch.as_tensor(probs).double()
    label = q.argmax(dim=1)
    loss = loss_full_f64(x, q, label == 0, label != 0, alpha)
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def touched(S, n, lo, hi, mirror=False):
    """bool [n]: the low-res indices the bilinear taps (align_corners=False) of full-resolution positions lo..hi-1 read -- of the mirrored
    positions S-1-x with mirror"""
    m = np.zeros(n, dtype=bool)
    for d in range(lo, hi):
        d = S - 1 - d if mirror else d
        src = max(np.float32(n) / np.float32(S) * (np.float32(d) + np.float32(0.5)) - np.float32(0.5), np.float32(0))
        i0 = min(int(src), n - 1)
        m[i0] = m[min(i0 + 1, n - 1)] = True
    return m
