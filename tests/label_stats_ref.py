"""Tests-side yardstick of the per-step pseudo-label statistics: `reference`, the rules of cosa_label_stats in
numpy on the C oracle's `resize_bilinear` (spec R) and a first-maximum arg-max, returning the counter vector in the documented order;
and `draw`, the seeded inputs the CPU and GPU tests share.  A helper, not a test."""
import numpy as np

IGNORE = 255
BOX_KINDS = ("full", "interior", "row", "empty")
LABEL_KINDS = ("none", "all", "some")


def layout(K):
    """the documented order: steps, pix, main[K+1], aux[K+1], agree, inter[K], pred[K], bad_cam, bad_cam_aux -> ({name: offset}, n)"""
    off, o = {}, 0
    for name, n in (("steps", 1), ("pix", 1), ("main", K + 1), ("aux", K + 1), ("agree", 1), ("inter", K), ("pred", K), ("bad_cam", 1),
                    ("bad_cam_aux", 1)):
        off[name] = o
        o += n
    return off, o


def resized_logits(oracle_c, seg, cls, S):
    """[B,K,S,S]: spec R resize of every plane, absent classes replaced by -1e5 afterwards (background always live)"""
    B, K = seg.shape[:2]
    out = np.empty((B, K, S, S), np.float32)
    for b in range(B):
        out[b] = oracle_c.resize_bilinear(seg[b], S, S)
        for c in range(1, K):
            if cls[b, c - 1] == 0:
                out[b, c] = np.float32(-1e5)
    return out


def top_two_margin(resized):
    """the smallest difference between the largest and second largest logit over all pixels"""
    s = np.sort(resized, axis=1)
    return float((s[:, -1] - s[:, -2]).min())


def inside_boxes(boxes, S):
    ar = np.arange(S)
    return np.stack([((ar[:, None] >= y0) & (ar[:, None] < y1) & (ar[None, :] >= x0) & (ar[None, :] < x1)) for y0, y1, x0, x1 in boxes])


def reference(oracle_c, mask_main, mask_aux, seg, cls, boxes, cam, cam_aux, ignore=IGNORE):
    """-> int64 [4K+7]: what ONE call adds to a zeroed counter vector"""
    B, K = seg.shape[:2]
    S = mask_main.shape[-1]
    off, n = layout(K)
    out = np.zeros(n, np.int64)
    inside = inside_boxes(boxes, S)
    out[off["steps"]] = 1
    out[off["pix"]] = inside.sum()

    def hist(mask):
        h = np.zeros(K + 1, np.int64)
        v = mask[inside]
        for k in range(K):
            h[k] = (v == k).sum()
        h[K] = (v == ignore).sum()
        return h

    out[off["main"]:off["main"] + K + 1] = hist(mask_main)
    if mask_aux is not None:
        out[off["aux"]:off["aux"] + K + 1] = hist(mask_aux)
        out[off["agree"]] = (inside & (mask_main == mask_aux)).sum()
    student = np.argmax(resized_logits(oracle_c, seg, cls, S), axis=1)          # numpy: the first maximum
    labelled = inside & (mask_main >= 0) & (mask_main < K) & (mask_main == np.floor(mask_main))     # a label 0..K-1, nothing else
    for k in range(K):
        out[off["pred"] + k] = (labelled & (student == k)).sum()
        out[off["inter"] + k] = (labelled & (student == k) & (mask_main == k)).sum()
    present = cls != 0
    for name, c in (("bad_cam", cam), ("bad_cam_aux", cam_aux)):
        if c is not None:
            out[off[name]] = (~np.isfinite(c) & present[:, :, None, None] & inside[:, None]).sum()
    return out


def make_box(kind, S, rng):
    if kind == "full":
        return (0, S, 0, S)
    if kind == "interior":
        y0, x0 = int(rng.integers(1, S // 4)), int(rng.integers(1, S // 4))
        return (y0, S - int(rng.integers(1, S // 4)), x0, S - int(rng.integers(2, S // 4)) - 1)       # (an odd width now and then)
    if kind == "row":
        y = int(rng.integers(0, S))
        return (y, y + 1, 3, S - 2)
    if kind == "empty":
        return (S // 2, S // 2, 0, S)
    raise ValueError(kind)


def draw(oracle_c, B, K, S, h, seed, box_kinds, label_kinds, integer_logits=False, margin=None):
    """Seeded inputs of one call as float32 / int32 numpy arrays: dict(mask_main, mask_aux, seg, cls, boxes, cam, cam_aux).
    box_kinds / label_kinds: one entry per image.  Masks hold the present classes, background and runs of IGNORE; the auxiliary map is
    the main one with every seventh row redrawn.  integer_logits: small integers, so that ties occur between classes.  margin: the
    top-two resized logits must differ by more than this at every pixel (the logits are redrawn from the next sub-seed until they
    do, and the property is asserted): an ulp between two bilinear resizes then cannot flip a label."""
    assert len(box_kinds) == B and len(label_kinds) == B
    rng = np.random.default_rng(seed)
    cls = np.zeros((B, K - 1), np.float32)
    for b, kind in enumerate(label_kinds):
        if kind == "all":
            cls[b] = 1
        elif kind == "some":
            cls[b, rng.choice(K - 1, size=min(3, K - 1), replace=False)] = 1
    boxes = np.array([make_box(k, S, rng) for k in box_kinds], np.int32)

    def mask():
        m = np.zeros((B, S, S), np.float32)
        for b in range(B):
            values = np.concatenate([[0], 1 + np.nonzero(cls[b])[0]])
            cells = rng.choice(values, size=(S // 4 + 1, S // 4 + 1))
            m[b] = np.kron(cells, np.ones((4, 4)))[1:S + 1, 2:S + 2]                 # 4 x 4 patches, off the thread's 4-pixel grid
            for _ in range(S // 2):                                                  # runs of ignore
                y, x0 = int(rng.integers(0, S)), int(rng.integers(0, S))
                m[b, y, x0:x0 + int(rng.integers(1, S // 2))] = IGNORE
        return m

    mask_main = mask()
    mask_aux = mask_main.copy()
    mask_aux[:, ::7] = mask()[:, ::7]
    for sub in range(64):
        r2 = np.random.default_rng([seed, sub])
        if integer_logits:
            seg = r2.integers(-2, 3, size=(B, K, h, h)).astype(np.float32)
        else:
            seg = (r2.standard_normal((B, K, h, h)) * 4).astype(np.float32)
        if margin is None or top_two_margin(resized_logits(oracle_c, seg, cls, S)) > margin:
            break
    if margin is not None:
        assert top_two_margin(resized_logits(oracle_c, seg, cls, S)) > margin
    cam = rng.random((B, K - 1, S, S), dtype=np.float32)
    cam_aux = rng.random((B, K - 1, S, S), dtype=np.float32)
    return dict(mask_main=mask_main, mask_aux=mask_aux, seg=seg, cls=cls, boxes=boxes, cam=cam, cam_aux=cam_aux)
