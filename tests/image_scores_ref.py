"""numpy restatement of the per-image counter row of cosa_image_scores (include/cosa_hip.h), for the tests:
row = [n, n_valid, then for map m, class c: I, P, G, A].  A pixel is counted for map m when gt < nc and, as cosa_confusion_hist drops it
otherwise, pred < nc; with pseudo[m] a prediction of 255 drops it too (the same pixels at nc <= 255)."""
import numpy as np


def ref_row(gt, preds, pseudo, nc):
    gt = np.asarray(gt, np.uint8).reshape(-1).astype(np.int64)
    row = np.zeros(2 + len(preds) * nc * 4, np.int64)
    row[0], row[1] = gt.size, int((gt < nc).sum())
    cnt = row[2:].reshape(len(preds), nc, 4)
    for m, (p, ps) in enumerate(zip(preds, pseudo)):
        p = np.asarray(p, np.uint8).reshape(-1).astype(np.int64)
        assert p.size == gt.size
        counted = (gt < nc) & (p < nc)
        if ps:
            counted &= p != 255
        cnt[m, :, 0] = np.bincount(gt[counted & (gt == p)], minlength=nc)[:nc]
        cnt[m, :, 1] = np.bincount(p[counted], minlength=nc)[:nc]
        cnt[m, :, 2] = np.bincount(gt[counted], minlength=nc)[:nc]
        cnt[m, :, 3] = np.bincount(p[p < nc], minlength=nc)[:nc]
    return row


def ref_counts(seg, gt, nc):
    """what assist_seg reads of (seg, gt): per class id I = #{seg == c and gt == c}, A = #{seg == c}, G_all = #{gt == c}, and n"""
    seg, gt = np.asarray(seg).reshape(-1), np.asarray(gt).reshape(-1)
    ids = np.arange(nc)[:, None]
    return ((seg == ids) & (gt == ids)).sum(axis=1), (seg == ids).sum(axis=1), (gt == ids).sum(axis=1), gt.size


def confusion(gt, pred, nc, pseudo=False):
    """the matrix cosa_confusion_hist accumulates (row = truth)"""
    gt, p = np.asarray(gt, np.uint8).reshape(-1).astype(np.int64), np.asarray(pred, np.uint8).reshape(-1).astype(np.int64)
    keep = (gt < nc) & (p < nc)
    if pseudo:
        keep &= p != 255
    return np.bincount(nc * gt[keep] + p[keep], minlength=nc * nc).reshape(nc, nc)
