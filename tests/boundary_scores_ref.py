"""numpy restatement of the boundary row of cosa_boundary_scores (include/cosa_hip.h), for the tests.

A label map is uint8 [H, W]; a value < nc is a class.  A class pixel is interior iff its whole (2d+1) x (2d+1) window lies inside the image
and every pixel of it holds the pixel's label; a class pixel that is not interior is a band pixel of its class.  Two routes that share no
code: `band` by the window definition itself, pixel by pixel, and `band_by_erosion` by d iterations of 3x3 erosion of each class's mask on
a one-pixel border of zeros (the `mask_to_boundary` of the Boundary IoU paper's code, written in numpy).
row = [n, n_valid, then for map m, class c: I, P, G, A]: a pixel is counted for map m when gt < nc and pred_m < nc (on the maps themselves);
over counted pixels I = #{gt band c and pred band c}, P = #{pred band c}, G = #{gt band c}; A = #{pred band c} over all pixels."""
import numpy as np


def band(L, d, nc):
    """-> bool [H, W]: the pixel is a band pixel of its own class.  The literal definition: no separability, no run lengths."""
    L = np.asarray(L, np.uint8)
    H, W = L.shape
    out = np.zeros((H, W), bool)
    for y in range(H):
        for x in range(W):
            c = int(L[y, x])
            if c >= nc:
                continue
            inside = y - d >= 0 and y + d < H and x - d >= 0 and x + d < W
            out[y, x] = not (inside and bool((L[y - d:y + d + 1, x - d:x + d + 1] == c).all()))
    return out


def band_by_erosion(L, d, nc):
    """the second route: per class, mask minus the mask eroded d times by a 3x3 square, positions outside the image being zero"""
    L = np.asarray(L, np.uint8)
    H, W = L.shape
    out = np.zeros((H, W), bool)
    for c in np.unique(L):
        if c >= nc:
            continue
        mask = L == c
        er = mask.copy()
        for _ in range(d):
            if not er.any():
                break
            p = np.zeros((H + 2, W + 2), bool)
            p[1:-1, 1:-1] = er
            er = np.ones((H, W), bool)
            for dy in (0, 1, 2):
                for dx in (0, 1, 2):
                    er &= p[dy:dy + H, dx:dx + W]
        out |= mask & ~er
    return out


def row(gt, preds, d, nc, band_fn=band):
    gt = np.asarray(gt, np.uint8)
    H, W = gt.shape
    out = np.zeros(2 + len(preds) * nc * 4, np.int64)
    out[0], out[1] = H * W, int((gt < nc).sum())
    cnt = out[2:].reshape(len(preds), nc, 4)
    gb = band_fn(gt, d, nc)
    g = gt.astype(np.int64)
    for m, p in enumerate(preds):
        p = np.asarray(p, np.uint8)
        assert p.shape == gt.shape
        pb = band_fn(p, d, nc)
        q = p.astype(np.int64)
        counted = (g < nc) & (q < nc)
        cnt[m, :, 0] = np.bincount(g[counted & gb & pb & (g == q)], minlength=nc)[:nc]
        cnt[m, :, 1] = np.bincount(q[counted & pb], minlength=nc)[:nc]
        cnt[m, :, 2] = np.bincount(g[counted & gb], minlength=nc)[:nc]
        cnt[m, :, 3] = np.bincount(q[pb], minlength=nc)[:nc]
    return out


def run_map(rng, H, W, values, blocks=6):
    """a label map made of runs: rectangles of `values` thrown over a background of values[0]"""
    L = np.full((H, W), values[0], np.uint8)
    for _ in range(blocks):
        y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        h, w = int(rng.integers(1, max(2, H // 2 + 1))), int(rng.integers(1, max(2, W // 2 + 1)))
        L[y0:y0 + h, x0:x0 + w] = values[int(rng.integers(0, len(values)))]
    return L
