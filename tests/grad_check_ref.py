"""The --grad_check_iters figure restated in float64 NumPy: what the two kernels of csrc/grad_check_kernels.hip
compute over a list of (w, g, dir) tensors, and the host maths on the record.  Written from the definition, not from the kernels: plain
sums over whole tensors, no chunks."""
import math

import numpy as np

RECORD = 36
G2, W2, S, FLAGS, T, LOSS, BAD_G, BAD_W = 0, 1, 2, 3, 4, 8, 33, 34
STEPS = (1.0, -1.0, 0.5, -0.5)
CHUNK = 16384


def norms(ws, gs, dirs, n_dirs, rho):
    """-> rows [n_dirs, RECORD] with G2, W2, s, flags and the non-finite counts filled in"""
    rows = np.zeros((n_dirs, RECORD), dtype=np.float64)
    for d in range(n_dirs):
        g2 = w2 = 0.0
        bad_g = bad_w = 0
        with np.errstate(all="ignore"):
            for w, g, k in zip(ws, gs, dirs):
                if k != d:
                    continue
                g2 += float(np.sum(g.astype(np.float64) ** 2))
                w2 += float(np.sum(w.astype(np.float64) ** 2))
                bad_g += int(np.sum(~np.isfinite(g)))
                bad_w += int(np.sum(~np.isfinite(w)))
        flags = (1 if g2 == 0 else 0) | (2 if (not math.isfinite(g2) or bad_g) else 0) | (4 if (not math.isfinite(w2) or bad_w) else 0)
        s = 0.0
        if not flags:
            with np.errstate(all="ignore"):
                s = float(np.float32(rho * math.sqrt(w2 / g2)))
            if not math.isfinite(s) or s == 0.0:
                s, flags = 0.0, flags | 8
        rows[d, [G2, W2, S, FLAGS, BAD_G, BAD_W]] = [g2, w2, s, flags, bad_g, bad_w]
    return rows


def perturb(ws, gs, dirs, d, c, s):
    """-> ([w' per tensor], t_c): w' = w + fl32(fl32(c s) g) in direction d (two float32 roundings), w elsewhere or with s = 0"""
    cs = np.float32(c) * np.float32(s)
    out, t = [], 0.0
    for w, g, k in zip(ws, gs, dirs):
        if k == d and float(s) != 0.0:
            wp = (w + (cs * g).astype(np.float32)).astype(np.float32)
            t += float(np.sum((wp.astype(np.float64) - w.astype(np.float64)) * g.astype(np.float64)))
        else:
            wp = w.copy()
        out.append(wp)
    return out, t


def make_case(seed=0):
    """the tensors both suites run: sizes 1, 3, chunk - 1, chunk, chunk + 1 and 3 chunk + 5 over two interleaved directions (0, 1), a tensor
    whose views sit 4 bytes off a 16-byte boundary (`off4`: the tests allocate it so), one in no direction with a gradient and one without,
    a direction whose gradient is zero (2), one with a planted inf and NaN (3) and an empty one (4)
    -> dict(ws, gs, dirs, n_dirs, off4: indices of the tensors to allocate 4 bytes off)"""
    rng = np.random.default_rng(seed)
    sizes = [1, 3, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 1003, 777, 500, 2048, 300]
    dirs = [0, 1, 0, 1, 0, 1, 0, -1, -1, 2, 3]
    ws = [rng.standard_normal(n).astype(np.float32) * np.float32(0.05) for n in sizes]
    gs = [rng.standard_normal(n).astype(np.float32) * np.float32(1e-3) for n in sizes]
    gs[8] = None
    gs[9][:] = 0
    gs[10][7], gs[10][200] = np.inf, np.nan
    return dict(ws=ws, gs=gs, dirs=dirs, n_dirs=5, off4=[6])


def figures(L, t, s, g2):
    """L: the objective at (w, +1, -1, +1/2, -1/2); t: the four realised steps -> (r1, r_half, r_star, rough, curv)"""
    r1 = (L[1] - L[2]) / (t[0] - t[1])
    rh = (L[3] - L[4]) / (t[2] - t[3])
    return r1, rh, (4 * rh - r1) / 3, abs(r1 - rh), (L[1] + L[2] - 2 * L[0]) / (s * s * g2)
