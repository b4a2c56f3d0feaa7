"""The supervised-contrastive token loss restated in numpy float64: token labels, loss, M and the gradient, written
from the definition with plain loops over images.  Nothing here imports cosa_amd."""
import math

import numpy as np

IGNORE = 255
EPS = 1e-12


def need_of(patch, purity=1.0):
    return int(math.ceil(purity * patch * patch))


def token_labels(mask, patch, purity=1.0):
    """mask int [B,S,S] -> uint8 [B,(S/patch)^2]: the class whose pixel count in the cell is >= need, else 255"""
    mask = np.asarray(mask)
    B, S = mask.shape[0], mask.shape[-1]
    g, need = S // patch, need_of(patch, purity)
    out = np.full((B, g * g), IGNORE, dtype=np.uint8)
    for b in range(B):
        for r in range(g):
            for c in range(g):
                cell = mask[b, r * patch:(r + 1) * patch, c * patch:(c + 1) * patch].reshape(-1)
                vals, cnts = np.unique(cell, return_counts=True)
                for v, k in zip(vals, cnts):
                    if int(v) != IGNORE and k >= need:
                        out[b, r * g + c] = v
    return out


def _sets(y):
    """-> (A [n,n] bool: j in A(i), P [n,n] bool: j in P(i), anchors [n] bool)"""
    n = y.shape[0]
    valid = y != IGNORE
    off = ~np.eye(n, dtype=bool)
    A = np.broadcast_to(valid[None, :], (n, n)) & off
    P = A & valid[:, None] & (y[:, None] == y[None, :])
    return A, P, P.sum(1) >= 1


def loss_and_grad(x, y, tau, want_grad=True):
    """x float [B,n,D] (taken as float64), y int [B,n] -> (L, M, dL/dx float64 [B,n,D] | None)"""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y).astype(np.int64)
    B, n, D = x.shape
    per_image = []
    M = 0
    for b in range(B):
        A, P, anc = _sets(y[b])
        M += int(anc.sum())
        per_image.append((A, P, anc))
    total = 0.0
    grad = np.zeros_like(x) if want_grad else None
    for b in range(B):
        A, P, anc = per_image[b]
        if not anc.any():
            continue
        nrm = np.maximum(np.sqrt((x[b] * x[b]).sum(1)), EPS)
        z = x[b] / nrm[:, None]
        s = z @ z.T / tau
        sm = np.where(A, s, -np.inf)
        mx = sm[anc].max(1)
        lse = np.zeros(n)
        lse[anc] = mx + np.log(np.exp(sm[anc] - mx[:, None]).sum(1))
        npos = P.sum(1)
        li = np.zeros(n)
        li[anc] = lse[anc] - (s * P).sum(1)[anc] / npos[anc]
        total += li.sum()
        if want_grad:
            G = np.zeros((n, n))
            G[anc] = (np.exp(sm[anc] - lse[anc, None]) - P[anc] / npos[anc, None]) / M
            dz = (G + G.T) @ z / tau
            grad[b] = (dz - (dz * z).sum(1, keepdims=True) * z) / nrm[:, None]
    L = total / M if M > 0 else 0.0
    return L, M, grad


def loss_only(x, y, tau):
    return loss_and_grad(x, y, tau, want_grad=False)[0]
