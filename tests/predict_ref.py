"""Restatements in numpy of the two kernels of label-free export, for tests/test_predict_classes_cpu.py (which pins
them on hand-written cases) and tests/test_predict_classes_gpu.py (which holds the kernels to them, exactly)."""
import numpy as np

MEAN = (123.675, 116.28, 103.53)                    # dataloaders.train_loader.normalize_img
STD = (58.395, 57.12, 57.375)


def threshold_logit(t):
    """float32(log(t / (1 - t))), formed in float64"""
    assert 0.0 < t < 1.0
    return np.float32(np.log(np.float64(t) / (np.float64(1.0) - np.float64(t))))


def predict_classes_ref(logits, t=0.5, cls_min=1):
    """logits [G, C] (or [C]) float32 -> (rows [G, C] float32 in {0, 1}, k_live [G] int32, nonfinite [G] int32).
    Class c is present iff logit_c >= L (never a NaN).  While fewer than cls_min are present, the largest logit among the absent ones
    that are neither NaN nor -inf is added, the lowest index among equal ones; nothing addable left ends the fill.  nonfinite counts the
    NaN and +-inf logits."""
    x = np.asarray(logits, dtype=np.float32)
    x = x.reshape(-1, x.shape[-1])
    L = threshold_logit(t)
    G, C = x.shape
    rows = np.zeros((G, C), np.float32)
    k_live, nonfinite = np.zeros(G, np.int32), np.zeros(G, np.int32)
    for g in range(G):
        with np.errstate(invalid="ignore"):
            present = x[g] >= L
        while present.sum() < cls_min:
            addable = ~present & ~np.isnan(x[g]) & (x[g] != -np.inf)
            if not addable.any():
                break
            best = x[g][addable].max()
            present[int(np.nonzero(addable & (x[g] == best))[0][0])] = True
        rows[g], k_live[g], nonfinite[g] = present, present.sum(), (~np.isfinite(x[g])).sum()
    return rows, k_live, nonfinite


def alpha256(alpha):
    return int(round(float(alpha) * 256))


def overlay_ref(image, seg, palette, alpha):
    """image uint8 [H, W, 3], seg uint8 [H, W], palette uint8 [256, 3] -> uint8 [H, W, 3]: label 0 keeps the image's byte, label l > 0
    gives (a pal[l][c] + (256 - a) img + 128) >> 8 with a = round(alpha 256)"""
    img = np.asarray(image).astype(np.int64)
    seg = np.asarray(seg)
    a = alpha256(alpha)
    blend = (a * np.asarray(palette).astype(np.int64)[seg] + (256 - a) * img + 128) >> 8
    return np.where((seg > 0)[..., None], blend, img).astype(np.uint8)


def classification_ref(predicted, given):
    """rows [N, C] in {0, 1} -> (exact-match count, tp, fp, fn) as Python ints"""
    p, g = np.asarray(predicted) != 0, np.asarray(given) != 0
    return int((p == g).all(axis=1).sum()), int((p & g).sum()), int((p & ~g).sum()), int((~p & g).sum())


CRAFTED_C = 6
NAN, INF = float("nan"), float("inf")
# (logits, t, cls_min) -> (present classes 0-based, nonfinite), written out by hand
CRAFTED = [
    (([-1.0, 2.0, -3.0, 2.0, 0.0, -0.5], 0.5, 1), ([1, 3, 4], 0)),            # a value equal to L = 0 is present
    (([-1.0, -2.0, -1.0, -3.0, -1.0, -9.0], 0.5, 0), ([], 0)),                # nothing above the threshold, cls_min 0: the empty row
    (([-1.0, -2.0, -1.0, -3.0, -1.0, -9.0], 0.5, 1), ([0], 0)),               # ... cls_min 1: the tie at -1 goes to the lowest index
    (([-1.0, -2.0, -1.0, -3.0, -1.0, -9.0], 0.5, 3), ([0, 2, 4], 0)),         # ... cls_min 3: the three -1s, nothing else
    (([-4.0, -2.0, -1.0, -3.0, -1.0, -9.0], 0.5, 3), ([1, 2, 4], 0)),         # ... then the next largest
    (([NAN, -INF, INF, -5.0, NAN, -6.0], 0.5, 3), ([2, 3, 5], 4)),            # +inf present; NaN and -inf never added
    (([NAN, -INF, NAN, -INF, NAN, -INF], 0.5, 2), ([], 6)),                   # nothing addable: the fill ends short of cls_min
    (([NAN, -INF, INF, -5.0, NAN, -6.0], 0.5, 6), ([2, 3, 5], 4)),            # cls_min = C: everything addable, no more
    (([-0.9, -0.8, 0.5, 2.0, 2.3, -0.84729785], 0.3, 1), ([1, 2, 3, 4, 5], 0)),     # t 0.3: L = float32(log(3/7)) = -0.84729785 (equal: present)
    (([-0.9, -0.8, 0.5, 2.0, 2.3, 2.1972246], 0.9, 1), ([4, 5], 0)),          # t 0.9: L = float32(log 9) = 2.1972246 (equal: present)
    (([-0.9, -0.8, 0.5, 2.0, 2.1, 2.1972244], 0.9, 2), ([4, 5], 0)),          # one float32 below L: absent, then added as the largest, then 2.1
    (([0.0, -0.0, -1.0, -1.0, -1.0, -1.0], 0.5, 1), ([0, 1], 0)),             # -0.0 >= 0
]
