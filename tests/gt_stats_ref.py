"""Tests-side yardstick of --gt_stats: `reference`, the rules of cosa_gt_stats in numpy on the C oracle's
`resize_bilinear` (spec R) and a first-maximum arg-max, returning the counter vector in the documented order; `pillow_crop`, what the
reference does to a label map that travels with its image; `gather`, the two-table gather; and `draw`, the seeded inputs the CPU and GPU
tests share.  A helper, not a test."""
import numpy as np
from PIL import Image

import label_stats_ref as LR

IGNORE = 255


def layout(K):
    """the documented order: steps, pix, valid, gt_other, main[K][K+1], aux[K][K+1], student[K][K] -> ({name: offset}, n)"""
    off, o = {}, 0
    for name, n in (("steps", 1), ("pix", 1), ("valid", 1), ("gt_other", 1), ("main", K * (K + 1)), ("aux", K * (K + 1)), ("student", K * K)):
        off[name] = o
        o += n
    return off, o


def reference(oracle_c, gt, mask_main, mask_aux, seg, cls, boxes, ignore=IGNORE):
    """-> int64 [4 + 2K(K+1) + K^2]: what ONE call adds to a zeroed counter vector"""
    B, K = seg.shape[:2]
    S = mask_main.shape[-1]
    off, n = layout(K)
    out = np.zeros(n, np.int64)
    inside = LR.inside_boxes(boxes, S)
    valid = inside & (gt < K)
    out[off["steps"]] = 1
    out[off["pix"]] = inside.sum()
    out[off["valid"]] = valid.sum()
    out[off["gt_other"]] = (inside & (gt >= K) & (gt != 255)).sum()
    for name, mask in (("main", mask_main), ("aux", mask_aux)):
        if mask is None:
            continue
        m = out[off[name]:off[name] + K * (K + 1)].reshape(K, K + 1)
        for t in range(K):
            v = mask[valid & (gt == t)]
            for k in range(K):
                m[t, k] = (v == k).sum()
            m[t, K] = (v == ignore).sum()
    student = np.argmax(LR.resized_logits(oracle_c, seg, cls, S), axis=1)          # numpy: the first maximum
    m = out[off["student"]:off["student"] + K * K].reshape(K, K)
    for t in range(K):
        m[t] = np.bincount(student[valid & (gt == t)], minlength=K)
    return out


def pillow_crop(gt, p, S):
    """dataloaders/transforms.py:61-77,101-114,145-202 for a label: resize NEAREST, fliplr when drawn, pad with 255, crop"""
    lab = np.asarray(Image.fromarray(gt).resize((p["new_w"], p["new_h"]), Image.NEAREST))
    if p["flip"]:
        lab = np.fliplr(lab)
    H, W = max(S, p["new_h"]), max(S, p["new_w"])
    pad = np.full((H, W), 255, np.uint8)
    pad[p["H_pad"]:p["H_pad"] + p["new_h"], p["W_pad"]:p["W_pad"] + p["new_w"]] = lab
    return pad[p["H_start"]:p["H_start"] + S, p["W_start"]:p["W_start"] + S]


def gather(gt, src_y, src_x):
    """gt_crop[y][x] = gt[src_y[y]][src_x[x]], 255 where either entry is -1"""
    out = gt[np.maximum(src_y, 0)[:, None], np.maximum(src_x, 0)[None, :]].copy()
    out[(src_y < 0)[:, None] | (src_x < 0)[None, :]] = 255
    return out


def random_map(rng, h, w, K=21):
    """a map of 8 x 8 patches with values in {0..K-1, 255}, off the pixel grid of any resize"""
    cells = rng.choice(np.concatenate([np.arange(K), [255]]), size=(h // 8 + 2, w // 8 + 2)).astype(np.uint8)
    m = np.kron(cells, np.ones((8, 8), np.uint8))[3:h + 3, 5:w + 5].copy()
    noise = rng.random((h, w)) < 0.1                                              # single pixels too: a resize off by one shows
    m[noise] = rng.choice(np.concatenate([np.arange(K), [255]]), size=int(noise.sum())).astype(np.uint8)
    return m


def draw(oracle_c, B, K, S, h, seed, box_kinds, label_kinds, integer_logits=False, margin=None, gt_kinds=None):
    """label_stats_ref.draw's inputs plus `gt` uint8 [B,S,S].  gt_kinds: per image "mixed" (patches of the classes, runs of 255 and, in
    image 0, a few pixels of the value 200 -- no class, not 255), "all255", or "mask" (the main mask's own values as uint8)."""
    d = LR.draw(oracle_c, B, K, S, h, seed, box_kinds, label_kinds, integer_logits=integer_logits, margin=margin)
    d.pop("cam"), d.pop("cam_aux")
    rng = np.random.default_rng([seed, 77])
    gt = np.zeros((B, S, S), np.uint8)
    for b, kind in enumerate(gt_kinds or ("mixed",) * B):
        if kind == "all255":
            gt[b] = 255
        elif kind == "mask":
            gt[b] = d["mask_main"][b].astype(np.uint8)
        else:
            cells = rng.integers(0, K, size=(S // 4 + 1, S // 4 + 1))
            gt[b] = np.kron(cells, np.ones((4, 4)))[2:S + 2, 1:S + 1].astype(np.uint8)
            for _ in range(S // 4):
                y, x0 = int(rng.integers(0, S)), int(rng.integers(0, S))
                gt[b, y, x0:x0 + int(rng.integers(1, S // 2))] = 255
            if b == 0 and K <= 200:
                gt[b, rng.integers(0, S, 9), rng.integers(0, S, 9)] = 200
    d["gt"] = gt
    return d
