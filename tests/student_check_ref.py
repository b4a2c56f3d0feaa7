"""A NumPy restatement of cosa_student_check's counter rules (include/cosa_hip.h), written from the rules and not from
the kernel or from seg_helper.student_check_torch: loops over cells where the rule speaks of a cell, fp32 arithmetic where the rule says
fp32, np.rint (half to even) of the term times a power of two in float64 for the fixed-point sums.  Every counter is an integer, so the
tests compare with exact equality."""
import numpy as np

TENSORS = ("seg", "cam", "cam_aux", "cls", "cls_aux")
FIELDS = ("n", "nonfinite_a", "nonfinite_b", "max_abs", "range", "sum_d2", "sum_b2")
LOSSES = ("cls_loss", "cls_loss_aux", "seg_loss", "cam_loss")
LOSS_FIELDS = ("sum_d", "sum_b", "max_abs", "n")
HEAD = 62
D2, B2, LOSS = (32, 10), (20, 22), (32, 10)            # (fractional bits, a term must be < 2^int)
EDGES = (np.float32(1e-3), np.float32(1e-2), np.float32(1e-1))


def layout(K):
    off = {"checks": 0, "flags": 1}
    for t, name in enumerate(TENSORS):
        for f, field in enumerate(FIELDS):
            off[f"{name}.{field}"] = 2 + 7 * t + f
    off.update({"cells": 37, "differ": 38, "flip_hist": 39, "cls.sign_flips": 43, "cls_aux.sign_flips": 44, "cls_cols": 45})
    for j, name in enumerate(LOSSES):
        for f, field in enumerate(LOSS_FIELDS):
            off[f"{name}.{field}"] = 46 + 4 * j + f
    off["labelled"], off["agree"] = HEAD, HEAD + K
    return off, HEAD + 2 * K


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _fixed(term, spec):
    """a non-negative fp32 term -> its fixed-point integer, or None when it is not representable (>= 2^int, NaN, inf)"""
    frac, bits = spec
    if not term < np.float32(2.0 ** bits):
        return None
    return int(np.rint(np.float64(term) * 2.0 ** frac))


def _tensor_stats(c, off, t, name, a, b):
    """a, b: flat fp32 arrays of the elements compared"""
    bad = False
    c[off[name + ".n"]] += a.size
    for x, y in zip(a, b):
        fa, fb = np.isfinite(x), np.isfinite(y)
        c[off[name + ".nonfinite_a"]] += int(not fa)
        c[off[name + ".nonfinite_b"]] += int(not fb)
        if fb:
            c[off[name + ".range"]] = max(c[off[name + ".range"]], _bits(abs(y)))
        if not (fa and fb):
            bad = True
            continue
        with np.errstate(over="ignore"):
            d = np.float32(x - y)
            d2, b2 = np.float32(d * d), np.float32(y * y)
        if np.isfinite(d):
            c[off[name + ".max_abs"]] = max(c[off[name + ".max_abs"]], _bits(abs(d)))
        for term, spec, slot in ((d2, D2, ".sum_d2"), (b2, B2, ".sum_b2")):
            v = _fixed(term, spec)
            if v is None:
                bad = True
            else:
                c[off[name + slot]] += v
    if bad:
        c[off["flags"]] |= 1 << t


def _argmax(v, allowed):
    """(index, top value, second value) over the allowed channels: NaN read as -inf, the lowest index among equals; second: the largest
    allowed value outside the argmax channel, -inf when there is none"""
    best, idx = -np.inf, None
    for k in range(len(v)):
        if not allowed[k]:
            continue
        x = -np.inf if np.isnan(v[k]) else v[k]
        if idx is None or x > best:
            best, idx = x, k
    second = -np.inf
    for k in range(len(v)):
        if allowed[k] and k != idx:
            x = -np.inf if np.isnan(v[k]) else v[k]
            second = max(second, x)
    return idx, np.float32(best), np.float32(second)


def student_check_ref(seg, cam, aux, cls, clsaux, losses, cls_label, counters=None):
    """every argument but the last two: an (a, b) pair of fp32 arrays -> the counters (a list of Python ints) advanced by one check"""
    f = lambda p: tuple(np.ascontiguousarray(np.asarray(x, dtype=np.float32)) for x in p)
    seg, cam, aux, cls, clsaux, losses = f(seg), f(cam), f(aux), f(cls), f(clsaux), f(losses)
    lab = np.asarray(cls_label, dtype=np.float32)
    B, K, h, w = seg[0].shape
    off, n = layout(K)
    c = [0] * n if counters is None else [int(v) for v in counters]
    assert len(c) == n
    c[off["checks"]] += 1
    present = lab != 0                                              # [B, K-1]
    allowed = np.concatenate([np.ones((B, 1), dtype=bool), present], axis=1)
    sel4 = lambda x, m: x[np.broadcast_to(m[:, :, None, None], x.shape)]
    _tensor_stats(c, off, 0, "seg", sel4(seg[0], allowed), sel4(seg[1], allowed))
    _tensor_stats(c, off, 1, "cam", sel4(cam[0], present), sel4(cam[1], present))
    _tensor_stats(c, off, 2, "cam_aux", sel4(aux[0], present), sel4(aux[1], present))
    _tensor_stats(c, off, 3, "cls", cls[0][present], cls[1][present])
    _tensor_stats(c, off, 4, "cls_aux", clsaux[0][present], clsaux[1][present])
    for b in range(B):
        for y in range(h):
            for x in range(w):
                ia, _, _ = _argmax(seg[0][b, :, y, x], allowed[b])
                ib, top, second = _argmax(seg[1][b, :, y, x], allowed[b])
                c[off["cells"]] += 1
                c[off["labelled"] + ib] += 1
                if ia == ib:
                    c[off["agree"] + ib] += 1
                    continue
                c[off["differ"]] += 1
                with np.errstate(invalid="ignore"):
                    m = np.float32(top - second)
                c[off["flip_hist"] + (0 if m < EDGES[0] else 1 if m < EDGES[1] else 2 if m < EDGES[2] else 3)] += 1
    sign = lambda v: int(v > 0) - int(v < 0)
    for name, (a, b_) in (("cls", cls), ("cls_aux", clsaux)):
        c[off[name + ".sign_flips"]] += sum(sign(x) != sign(y) for x, y in zip(a.reshape(-1), b_.reshape(-1)))
    c[off["cls_cols"]] += B * (K - 1)
    for j, name in enumerate(LOSSES):
        a, b_ = losses[0][j], losses[1][j]
        c[off[name + ".n"]] += 1
        d = np.float32(abs(np.float32(a - b_)))
        v1, v2 = _fixed(d, LOSS), _fixed(np.float32(abs(b_)), LOSS)
        if np.isfinite(a) and np.isfinite(b_) and v1 is not None and v2 is not None:
            c[off[name + ".sum_d"]] += v1
            c[off[name + ".sum_b"]] += v2
            c[off[name + ".max_abs"]] = max(c[off[name + ".max_abs"]], _bits(d))
        else:
            c[off["flags"]] |= 1 << (8 + j)
    return c


# ---- the cases of the kernel-level tests (CPU: torch restatement against this file; GPU: the kernel against this file) -----------------------
# (B, K, h = w): a single workgroup | 432 cells: no multiple of 64, several workgroups, VOC's class count | more classes than lanes (COCO's)
SHAPES = {"small": (2, 6, 4), "blocks": (3, 21, 12), "wide": (2, 81, 5)}


def make_case(name, seed=0):
    """-> dict of fp32 arrays: pairs seg / cam / cam_aux / cls / cls_aux / losses and cls_label.  Seeded normals; b = a + noise of magnitude
    1e-4, 1e-2 or 1 per cell; the last image has no present class; planted: NaN / inf in a only and in b only, an exact tie that both
    passes hold, an exact tie of the check pass where the training pass decides otherwise, and near-ties of margin 5e-4, 5e-3 and 5e-2
    and a real flip of margin 1,
    so that every bin of the flip histogram is populated whatever the noise does."""
    B, K, h = SHAPES[name]
    rng = np.random.RandomState(100 * len(name) + seed)
    f32 = np.float32
    lab = (rng.rand(B, K - 1) < (0.5 if K < 10 else 0.15)).astype(f32)
    lab[0, :2] = 1                                                   # image 0: channels 0, 1, 2 allowed at least
    lab[B - 1] = 0                                                   # the last image: background only

    def pair(C, spatial=True):
        shape = (B, C, h, h) if spatial else (B, C)
        a = rng.randn(*shape).astype(f32)
        mag = f32(10.0) ** rng.choice([-4, -2, 0], size=(B, 1, h, h) if spatial else (B, 1)).astype(f32)
        return a, (a + mag * rng.randn(*shape).astype(f32)).astype(f32)

    seg, cam, aux = pair(K), pair(K - 1), pair(K - 1)
    cls, clsaux = pair(K - 1, False), pair(K - 1, False)
    a, b = seg
    # image 0, row 0: the planted cells (channels 1 and 2 are allowed there)
    a[0, 1, 0, 0] = a[0, 2, 0, 0] = b[0, 1, 0, 0] = b[0, 2, 0, 0] = 20.0                 # a tie both passes hold: channel 1, agreeing
    a[0, 1, 0, 1], a[0, 2, 0, 1], b[0, 1, 0, 1], b[0, 2, 0, 1] = 20.0, 20.5, 20.0, 20.0  # the check pass ties (-> 1), the training pass says 2
    for x, m in ((2, 5e-4), (3, 5e-3)):
        a[0, 1, 1, x], a[0, 2, 1, x], b[0, 1, 1, x], b[0, 2, 1, x] = 10.0, 10.0 - m, 10.0, 10.0 + m
    a[0, 1, 2, 0], a[0, 2, 2, 0], b[0, 1, 2, 0], b[0, 2, 2, 0] = 10.0, 10.0 - 5e-2, 10.0, 10.0 + 5e-2
    a[0, 1, 2, 1], a[0, 2, 2, 1], b[0, 1, 2, 1], b[0, 2, 2, 1] = 10.0, 9.0, 10.0, 11.0                 # a real flip: margin 1
    a[0, 0, 3, 3] = np.nan                                            # allowed channels: counted; a only
    b[0, 1, 3, 2] = np.inf                                            # b only
    a[B - 1, 3, 0, 0] = np.nan                                        # not allowed (the last image has no class): never read
    cam[0][0, 0, 1, 1] = -np.inf
    aux[1][0, 1, 2, 2] = np.nan
    cls[1][0, 0] = np.inf
    clsaux[0][0, 1] = np.nan
    la = np.abs(rng.randn(4)).astype(f32) + f32(0.1)
    lb = (la * (1 + 1e-3 * rng.randn(4))).astype(f32)
    return dict(seg=seg, cam=cam, cam_aux=aux, cls=cls, cls_aux=clsaux, losses=(la, lb), cls_label=lab, K=K)


def ref_of_case(d, counters=None):
    return student_check_ref(d["seg"], d["cam"], d["cam_aux"], d["cls"], d["cls_aux"], d["losses"], d["cls_label"], counters)
