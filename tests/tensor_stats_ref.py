"""The yardstick of the per-tensor diagnostics in numpy float64: the six slots of a tensor's row and the summary
formulas, written from the slot definitions and not from the code under test."""
import math

import numpy as np

SLOTS = ("g_sq", "w_sq", "gap_sq", "g_absmax", "g_nonfinite", "w_nonfinite")
ROW_BYTES = 48


def row(p, tp, g):
    """one tensor: fp32 arrays p (student master), tp (teacher master), g (gradient, or None: frozen) -> the six slots as Python numbers"""
    p, tp = np.asarray(p, np.float32).reshape(-1), np.asarray(tp, np.float32).reshape(-1)
    pf, tf = np.isfinite(p), np.isfinite(tp)
    p64, t64 = p.astype(np.float64), tp.astype(np.float64)
    out = {"g_sq": 0.0, "g_absmax": 0.0, "g_nonfinite": 0}
    out["w_sq"] = float(np.sum(np.square(p64[pf])))
    both = pf & tf
    out["gap_sq"] = float(np.sum(np.square(t64[both] - p64[both])))
    out["w_nonfinite"] = int(np.sum(~both))
    if g is not None:
        g = np.asarray(g, np.float32).reshape(-1)
        gf = np.isfinite(g)
        out["g_sq"] = float(np.sum(np.square(g[gf].astype(np.float64))))
        out["g_absmax"] = float(np.max(np.abs(g[gf]))) if gf.any() else 0.0
        out["g_nonfinite"] = int(np.sum(~gf))
    return out


def table(ps, tps, gs):
    """[T][6] rows in slot order"""
    return [[row(p, tp, g)[k] for k in SLOTS] for p, tp, g in zip(ps, tps, gs)]


def decode(raw):
    """an int64 [T, 6] table as the device writes it -> float64 [T, 6] values"""
    raw = np.ascontiguousarray(np.asarray(raw, np.int64))
    return np.concatenate([raw[:, :4].copy().view(np.float64), raw[:, 4:].astype(np.float64)], axis=1)


def figures(rows, sizes, blamed):
    """the figures of a set of rows: one tensor, a group, or all"""
    g_sq, w_sq, gap_sq = (math.fsum(r[k] for r in rows) for k in range(3))
    wn, gap = math.sqrt(w_sq), math.sqrt(gap_sq)
    return {"n": sum(sizes), "grad_norm": math.sqrt(g_sq), "grad_absmax": max([r[3] for r in rows], default=0.0), "weight_norm": wn,
            "ema_gap": gap, "ema_gap_rel": gap / (wn + 1e-12) if wn > 0 else 0.0, "g_nonfinite": sum(int(r[4]) for r in rows),
            "w_nonfinite": sum(int(r[5]) for r in rows), "blamed": sum(blamed)}


def summary(rows, blame, names, group_idx, sizes):
    T = len(rows)
    blame = [0] * T if blame is None else [int(b) for b in blame]
    out = {"tensors": {n: figures([rows[i]], [sizes[i]], [blame[i]]) for i, n in enumerate(names)}, "groups": {}}
    for gi in sorted(set(group_idx)):
        idx = [i for i in range(T) if group_idx[i] == gi]
        out["groups"][str(gi)] = figures([rows[i] for i in idx], [sizes[i] for i in idx], [blame[i] for i in idx])
    out["global"] = figures(rows, sizes, blame)
    best = max(range(T), key=lambda i: (blame[i], int(rows[i][4]), -i))
    out["worst"] = names[best] if (blame[best], int(rows[best][4])) > (0, 0) else None
    return out


def sum_bound(n):
    """relative bound of a double sum of n non-negative terms, in any order: n * 2^-52 (the worst case of n - 1 roundings of 2^-53 each,
    doubled; not a measured figure)"""
    return max(int(n), 1) * 2.0 ** -52
