"""GPU suite of the reliability-weighted seg loss.

  1. cosa_label_reliability against the restatements of tests/seg_weight_ref.py: bytes and counters for beta in {0, 1}, the measured
     float32 bar for the powers, sentinels, run-to-run bytes, refusals.
  2. cosa_seg_loss_forward_rw / _backward_rw against the float64 restatement with the bars the project holds these kernels to (seg loss 1e-4
     relative, the gradient within 2e-3 of its maximum, energy 1e-3), and byte for byte against the _w entry points where the weights are
     all 1 or all 0; the sticky flag; refusals.
  3. trainer level (crop 64, b = 2, teacher graph on).
"""
import ctypes
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_weight_ref as R

pytestmark = pytest.mark.gpu

SENT = -7.25
ISENT = -0x5A5A5A5A5A5A5A5A
BETAS = (0.0, 1.0, 0.5, 2.0, 8.0)
FLOORS = (0.0, 0.25)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


# ---- 1. the weight kernel --------------------------------------------------------------------------------------------------------------------
W_SHAPES = [(2, 4, 64), (3, 20, 37), (2, 80, 48)]          # (B, C, S); 37 x 37 is odd: the scalar accesses


def _thresholds(shape_i, G):
    """(hi, lo) per set; the second set of the middle shape has lo == 0"""
    return [(0.7, 0.25), (0.6, 0.0) if shape_i == 1 else (0.65, 0.3)][:G]


@functools.lru_cache(maxsize=None)
def _wcase(shape_i, G):
    """image 0: no class present; image 1: every class present; further images: two classes.  Even images are labelled by the threshold rule,
    odd ones at random (standing in for PAR's moves), labels past C and 255 included.  Planted per set: a label whose class is absent from
    y, a pixel with v == 1 exactly, a NaN in a foreground pixel's own plane."""
    B, C, S = W_SHAPES[shape_i]
    rng = np.random.default_rng(1000 + 10 * shape_i + G)
    y = np.zeros((B, C), np.float32)
    y[1, :] = 1
    for b in range(2, B):
        y[b, rng.choice(C, size=2, replace=False)] = 1
    cams, masks = [], []
    for g, (hi, lo) in enumerate(_thresholds(shape_i, G)):
        cam = rng.uniform(0, 1, (B, C, S, S)).astype(np.float32)
        vc = cam * y[:, :, None, None]
        mx, am = vc.max(1), vc.argmax(1)
        mask = np.where(mx >= np.float32(hi), am + 1, np.where(mx < np.float32(lo), 0, 255)).astype(np.float32)
        rnd = rng.choice(np.array([0, 1, 2, C, C + 1, 255], np.float32), size=mask.shape, p=[0.3, 0.2, 0.15, 0.15, 0.05, 0.15])
        for b in range(1, B, 2):
            mask[b] = rnd[b]
        mask[0, 1, 1] = 2.0                                   # image 0 has no class: label 2's class is absent from y
        cam[1, C - 1, 2, 3], mask[1, 2, 3] = 1.0, float(C)    # v == 1 exactly
        cam[1, 0, 4, 5], mask[1, 4, 5] = np.nan, 1.0          # a NaN in a foreground pixel's own plane
        if B > 2:
            absent = int(np.flatnonzero(y[2] == 0)[0])
            mask[2, 0, 0] = float(absent + 1)
        cams.append(cam)
        masks.append(mask)
    return y, cams, masks


def _check_case(shape_i, G):
    """on the CPU restatement, before anything runs: the case holds what the test is about"""
    y, cams, masks = _wcase(shape_i, G)
    C = y.shape[1]
    for g, (hi, lo) in enumerate(_thresholds(shape_i, G)):
        r, lab = R.ratio_f64(cams[g], y, masks[g], hi, lo)
        assert ((r > 0) & (r < 1) & lab).sum() >= 0.05 * lab.sum(), (shape_i, g)
        assert ((r == 0) & lab).any() and ((r == 1) & lab).any()
        assert r[1, 2, 3] == 1.0 and r[1, 4, 5] == 0.0 and np.isnan(cams[g][1, 0, 4, 5]) and lab[0, 1, 1] and r[0, 1, 1] == 0.0
        assert (masks[g] == C + 1).any() and not lab[masks[g] == C + 1].any() and not lab[masks[g] == 255].any()
    assert y[0].sum() == 0 and y[1].sum() == C


def _raw_rel(y, cams, masks, thr, beta, floor, dev_thr=False, pads=(64, 61), stats=True, override=None):
    """cosa_label_reliability through the C ABI.  Every weight map lives inside a larger buffer of sentinels -- the second set's at an offset
    that is not 16-byte aligned --, the counters inside a larger int64 buffer.  override: {argument name: value} for the refusal tests."""
    from cosa_amd import _C
    L = _C.lib()
    dev = torch.device("cuda", 0)
    G, (B, C), S = len(cams), y.shape, cams[0].shape[-1]
    cam_t = [torch.from_numpy(c).to(dev).contiguous() for c in cams]
    mask_t = [torch.from_numpy(m).to(dev).contiguous() for m in masks]
    y_t = torch.from_numpy(y).to(dev).contiguous()
    n = B * S * S
    bufs = [torch.full((pads[g % 2] + n + 64,), SENT, device=dev) for g in range(G)]
    rel = [bufs[g][pads[g % 2]:pads[g % 2] + n] for g in range(G)]
    sbuf = torch.full((4 + 4 * G + 4,), ISENT, dtype=torch.int64, device=dev)
    sbuf[4:4 + 4 * G] = 0
    st = sbuf[4:4 + 4 * G]
    arr = lambda ts: (ctypes.c_void_p * max(len(ts), 1))(*[t.data_ptr() if t is not None else None for t in ts])
    tdev = torch.tensor(thr, dtype=torch.float32, device=dev).contiguous() if dev_thr else None
    hi = (ctypes.c_float * G)(*[0.0 if dev_thr else t[0] for t in thr])
    lo = (ctypes.c_float * G)(*[0.0 if dev_thr else t[1] for t in thr])
    a = dict(cams=arr(cam_t), labels=_C.ptr(y_t), masks=arr(mask_t), rel=arr(rel), hi=hi, lo=lo, tdev=_C.ptr(tdev), G=G, B=B, C=C, S=S,
             beta=float(beta), floor=float(floor), stats=_C.ptr(st if stats else None))
    a.update(override or {})
    rc = L.cosa_label_reliability(a["cams"], a["labels"], a["masks"], a["rel"], a["hi"], a["lo"], a["tdev"], a["G"], a["B"], a["C"], a["S"],
                                  a["beta"], a["floor"], a["stats"], _C.stream_ptr())
    torch.cuda.synchronize()
    keep = (cam_t, mask_t, y_t, tdev)                      # (alive until the synchronize above)
    del keep
    return dict(rc=rc, rel=[r.reshape(B, S, S) for r in rel], bufs=bufs, pads=[pads[g % 2] for g in range(G)], n=n, stats=st, sbuf=sbuf)


def _sentinels_ok(r):
    for buf, pad in zip(r["bufs"], r["pads"]):
        if not (bool((buf[:pad] == SENT).all()) and bool((buf[pad + r["n"]:] == SENT).all())):
            return False
    return bool((r["sbuf"][:4] == ISENT).all()) and bool((r["sbuf"][-4:] == ISENT).all())


@pytest.mark.parametrize("dev_thr", [False, True], ids=["host_thr", "device_thr"])
@pytest.mark.parametrize("G", [1, 2])
@pytest.mark.parametrize("shape_i", [0, 1, 2])
def test_weight_kernel_against_the_restatements(shape_i, G, dev_thr):
    _check_case(shape_i, G)
    y, cams, masks = _wcase(shape_i, G)
    C, thr = y.shape[1], _thresholds(shape_i, G)
    for beta in BETAS:
        for floor in FLOORS:
            r = _raw_rel(y, cams, masks, thr, beta, floor, dev_thr=dev_thr)
            assert r["rc"] == 0 and _sentinels_ok(r)
            for g, (hi, lo) in enumerate(thr):
                w = r["rel"][g].cpu().numpy()
                w32 = R.weight_f32(cams[g], y, masks[g], hi, lo, beta, floor)
                want_stats = R.weight_stats(w32, masks[g], C)
                got_stats = r["stats"][4 * g:4 * g + 4].tolist()
                if beta in (0.0, 1.0):
                    assert np.array_equal(w.view(np.uint32), w32.view(np.uint32)), (beta, floor, g)
                    assert got_stats == want_stats.tolist(), (beta, floor, g)
                else:
                    w64 = R.weight_f64(cams[g], y, masks[g], hi, lo, beta, floor)
                    e32, err = np.abs(w32.astype(np.float64) - w64).max(), np.abs(w.astype(np.float64) - w64).max()
                    print(f"shape {W_SHAPES[shape_i]} set {g} beta {beta} floor {floor}: e32 {e32:.3e} kernel {err:.3e}")
                    assert err <= 4 * e32 + 2.0 ** -24, (beta, floor, g, err, e32)
                    assert got_stats[1] == want_stats[1] and got_stats[3] == want_stats[3]
                    assert got_stats == R.weight_stats(w, masks[g], C).tolist()          # the counters are those of the map it wrote
                assert w.min() >= 0 and w.max() <= 1 and not np.isnan(w).any()
    # the counters accumulate, and a second run gives the same bytes
    a, b = _raw_rel(y, cams, masks, thr, 2.0, 0.25, dev_thr=dev_thr), _raw_rel(y, cams, masks, thr, 2.0, 0.25, dev_thr=dev_thr)
    for g in range(G):
        assert torch.equal(_bits(a["rel"][g]), _bits(b["rel"][g]))
    assert torch.equal(a["stats"], b["stats"])
    # no counters asked for: the same maps
    c = _raw_rel(y, cams, masks, thr, 2.0, 0.25, dev_thr=dev_thr, stats=False)
    assert c["rc"] == 0 and all(torch.equal(_bits(a["rel"][g]), _bits(c["rel"][g])) for g in range(G)) and bool((c["stats"] == 0).all())


def test_weight_wrapper_accumulates_and_takes_device_thresholds():
    from cosa_amd.utils import seg_helper as sh
    y, cams, masks = _wcase(1, 2)
    thr = _thresholds(1, 2)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a).to(dev)
    stats = sh.new_reliability_stats(2, dev)
    args = ([t(c) for c in cams], t(y), [t(m) for m in masks])
    a = sh.label_reliability(*args, [h for h, _ in thr], [l for _, l in thr], beta=1.0, floor=0.25, stats=stats)
    b = sh.label_reliability(*args, [torch.tensor(h, device=dev) for h, _ in thr], [torch.tensor(l, device=dev) for _, l in thr], beta=1.0,
                             floor=0.25, stats=stats)
    one = [R.weight_stats(R.weight_f32(cams[g], y, masks[g], *thr[g], 1.0, 0.25), masks[g], y.shape[1]) for g in range(2)]
    assert all(torch.equal(_bits(a[g]), _bits(b[g])) for g in range(2))
    assert stats.tolist() == [(2 * s).tolist() for s in one]
    host = sh._label_reliability_torch([torch.from_numpy(c) for c in cams], torch.from_numpy(y), [torch.from_numpy(m) for m in masks],
                                       [h for h, _ in thr], [l for _, l in thr], beta=1.0, floor=0.25)
    assert all(torch.equal(_bits(a[g].cpu()), _bits(host[g])) for g in range(2))
    s = sh.reliability_summary(stats)
    assert s[0]["n_bg"] == 2 * int(one[0][1]) and s[0]["bg"] == pytest.approx(one[0][0] / 2.0 ** 32 / one[0][1], abs=1e-12)


@pytest.mark.parametrize("S", [192, 183])
def test_weight_kernel_walks_more_chunks_than_workgroups(S):
    """a set and image take at most 32 workgroups, each walking chunks of 1024 pixels with the grid's stride: 192 x 192 (36 chunks, float4)
    and 183 x 183 (33 chunks, the last one partial, scalar) against the float32 restatement, bytes and counters"""
    rng = np.random.default_rng(S)
    B, C = 2, 3
    cam = rng.uniform(0, 1, (B, C, S, S)).astype(np.float32)
    y = np.array([[1, 0, 1], [1, 1, 1]], np.float32)
    mask = rng.choice(np.array([0, 1, 2, 3, 255], np.float32), size=(B, S, S)).astype(np.float32)
    r = _raw_rel(y, [cam], [mask], [(0.7, 0.25)], 1.0, 0.25)
    want = R.weight_f32(cam, y, mask, 0.7, 0.25, 1.0, 0.25)
    assert r["rc"] == 0 and _sentinels_ok(r)
    assert np.array_equal(r["rel"][0].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert r["stats"].tolist() == R.weight_stats(want, mask, C).tolist()


def test_weight_kernel_refusals_write_nothing():
    from cosa_amd import _C
    y, cams, masks = _wcase(0, 2)
    thr = _thresholds(0, 2)
    null = ctypes.c_void_p(0)
    one_null = (ctypes.c_void_p * 2)(None, None)
    bad = [dict(beta=-0.5), dict(beta=8.5), dict(beta=float("nan")), dict(floor=1.0), dict(floor=-0.1), dict(floor=float("nan")),
           dict(G=0), dict(G=5), dict(C=0), dict(C=256), dict(S=0), dict(B=0),
           dict(cams=None), dict(labels=null), dict(masks=None), dict(rel=None), dict(cams=one_null), dict(masks=one_null), dict(rel=one_null),
           dict(hi=None), dict(lo=None)]
    for over in bad:
        r = _raw_rel(y, cams, masks, thr, 1.0, 0.0, override=over)
        assert r["rc"] == 1, over                                                 # COSA_EINVAL
        assert _C.lib().cosa_last_error().startswith(b"cosa_label_reliability"), over
        assert all(bool((b == SENT).all()) for b in r["bufs"]) and bool((r["stats"] == 0).all()) and _sentinels_ok(r), over


# ---- 2. the weighted loss kernels -------------------------------------------------------------------------------------------------------------
L_SHAPES = [(6, 4, 64, None), (3, 8, 64, None), (21, 12, 192, None), (5, 5, 64, 7)]       # (K, hs, S, ws): tests/test_loss_flags_gpu.py's, + its 5 x 7 case
BLENDS = [(0.3, 0.5), (0.5, 0.25)]                                                       # (fg_alpha, aux_alpha)
W_SEG, W_REG = 0.1, 0.05


def _layer():
    from cosa_amd.utils import seg_helper
    return seg_helper.DenseEnergyLoss(weight=1e-7, sigma_rgb=15, sigma_xy=100, scale_factor=0.5)


@functools.lru_cache(maxsize=None)
def _linputs(K, hs, S, ws=None):
    torch.manual_seed(300 + K)
    rng = np.random.default_rng(300 + K)
    B = 2
    vals = [0, 1, K - 1, 255] if K < 8 else [0, 1, 5, K - 1, 255]
    mk = lambda: torch.from_numpy(rng.choice(vals, size=(B, S, S)).astype(np.float32))

    def wmap():
        w = rng.uniform(0, 1, (B, S, S)).astype(np.float32)
        plant = rng.uniform(0, 1, (B, S, S))
        w[plant < 0.05], w[plant > 0.95] = 0.0, 1.0
        return torch.from_numpy(w)
    return dict(B=B, K=K, hs=hs, ws=ws or hs, S=S, seg=torch.randn(B, K, hs, ws or hs) * 2, mA=mk(), mB=mk(), rA=wmap(), rB=wmap(),
                simg=torch.randn(B, 3, S, S), box=torch.tensor([[0, S, 0, S], [3, S - 4, 0, S - 14]], dtype=torch.int16),
                AS=torch.randn(B, K, S // 2, S // 2) * 1e4)


@functools.lru_cache(maxsize=None)
def _oracle_energy(K, hs, S, ws=None):
    """the regulariser sees no weight: value and gradient w.r.t. the low-resolution logits, once per shape"""
    from oracle import torch_oracle as to
    c = _linputs(K, hs, S, ws)
    lr = c["seg"].clone().requires_grad_(True)
    up = F.interpolate(lr, size=(S, S), mode="bilinear", align_corners=False)
    l_reg, g_up = to.energy_loss_and_grad(c["simg"], up.detach(), c["mA"].to(torch.uint8).unsqueeze(1), c["box"].numpy())
    (g_lr,) = torch.autograd.grad(up, lr, g_up)
    return float(l_reg), g_lr


@pytest.mark.parametrize("a,b", BLENDS)
@pytest.mark.parametrize("aux", [True, False])
@pytest.mark.parametrize("K,hs,S,ws", L_SHAPES)
def test_weighted_loss_kernels_against_the_float64_restatement(K, hs, S, ws, aux, a, b):
    from cosa_amd.utils import seg_helper
    c = _linputs(K, hs, S, ws)
    for r in (c["rA"], c["rB"]):
        lab = c["mA"] != 255
        assert int((r[lab] == 0).sum()) > 0 and int((r[lab] == 1).sum()) > 0
    mB, rB = (c["mB"], c["rB"]) if aux else (None, None)
    l_seg, g_seg = R.weighted_ce_f64(c["seg"], c["mA"], mB, c["rA"], rB, S, a, b if aux else 0.0)
    l_reg, g_reg = _oracle_energy(K, hs, S, ws)
    g_ref = W_SEG * g_seg + W_REG * g_reg.double()
    lr = c["seg"].cuda().requires_grad_(True)
    cu = lambda t: None if t is None else t.cuda()
    f_seg, f_reg = seg_helper.fused_seg_and_energy_loss(lr, cu(c["mA"]), cu(mB), cu(c["simg"]), c["box"], _layer(), fg_alpha=a, aux_alpha=b,
                                                        rel_main=cu(c["rA"]), rel_aux=cu(rB))
    (W_SEG * f_seg + W_REG * f_reg).sum().backward()
    g = lr.grad.cpu().double()
    f_seg, f_reg = f_seg.detach(), f_reg.detach()
    err, top = (g - g_ref).abs().max().item(), g_ref.abs().max().item()
    print(f"K {K} hs {hs}x{c['ws']} S {S} a {a} b {b} aux {aux}: seg {float(f_seg):.7f} / {l_seg:.7f}  energy {float(f_reg):.6e} / {l_reg:.6e}  "
          f"grad err {err:.3e} of max {top:.3e}")
    assert math.isfinite(float(f_seg)) and torch.isfinite(g).all()
    assert float(f_seg) == pytest.approx(l_seg, rel=1e-4)
    assert float(f_reg) == pytest.approx(l_reg, rel=1e-3, abs=1e-12)
    assert err <= 2e-3 * top, (err, top)
    # the forward-only form the checks use: the same value
    only = seg_helper.seg_loss_forward_only(lr.detach(), cu(c["mA"]), cu(mB), cu(c["simg"]), c["box"], fg_alpha=a, aux_alpha=b,
                                            rel_main=cu(c["rA"]), rel_aux=cu(rB))
    assert float(only) == float(f_seg)


def _raw_seg(c, weights, aux=True, rel=None, pad=64):
    """forward + backward through the C ABI: rel None -> the _w entry points, else (relA, relB) -> the _rw ones.  The gradient lives inside a
    larger buffer of sentinels and the workspace is followed by 256 sentinel bytes."""
    from cosa_amd import _C
    L = _C.lib()
    dev = torch.device("cuda", 0)
    B, K, hs, ws_, S = c["B"], c["K"], c["hs"], c["ws"], c["S"]
    Sq = S // 2
    seg, mA, simg, AS = (c[k].to(dev).contiguous() for k in ("seg", "mA", "simg", "AS"))
    mB = c["mB"].to(dev).contiguous() if aux else None
    box = c["box"].to(device=dev, dtype=torch.int32).contiguous()
    need = L.cosa_seg_loss_workspace_bytes(B, K, hs, ws_)
    wsp = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev)
    sums = torch.full((8,), SENT, device=dev)
    s_seg, s_img = torch.full((B, K, Sq, Sq), SENT, device=dev), torch.full((B, 3, Sq, Sq), SENT, device=dev)
    roi, unl = torch.full((B, Sq, Sq), SENT, device=dev), torch.full((B, Sq, Sq), 7, device=dev, dtype=torch.uint8)
    n = B * K * hs * ws_
    gbuf = torch.full((pad + n + pad,), SENT, device=dev)
    grad = gbuf[pad:pad + n]
    gs, gr = torch.tensor([W_SEG], device=dev), torch.tensor([W_REG * 1e-7], device=dev)
    fargs = (_C.ptr(seg), _C.ptr(mA), _C.ptr(mB), _C.ptr(simg), _C.ptr(box), _C.ptr(sums), _C.ptr(s_seg), _C.ptr(s_img), _C.ptr(roi), _C.ptr(unl),
             B, K, hs, ws_, S, _C.ptr(wsp), need, _C.stream_ptr())
    bargs = (_C.ptr(seg), _C.ptr(mA), _C.ptr(mB), _C.ptr(sums), _C.ptr(AS), _C.ptr(roi), _C.ptr(gs), _C.ptr(gr), _C.ptr(grad),
             *[float(w) for w in weights], B, K, hs, ws_, S, _C.ptr(wsp), need, _C.stream_ptr())
    if rel is None:
        rc_f, rc_b = L.cosa_seg_loss_forward_w(*fargs), L.cosa_seg_loss_backward_w(*bargs)
    else:
        rt = [None if r is None else r.to(dev).contiguous() for r in rel]
        tail = (_C.ptr(rt[0]), _C.ptr(rt[1]))
        rc_f, rc_b = L.cosa_seg_loss_forward_rw(*fargs, *tail), L.cosa_seg_loss_backward_rw(*bargs, *tail)
    torch.cuda.synchronize()
    return dict(rc_f=rc_f, rc_b=rc_b, sums=sums, s_seg=s_seg, s_img=s_img, roi=roi, unl=unl, gbuf=gbuf, grad=grad, ws=wsp, need=need, pad=pad, n=n)


@pytest.mark.parametrize("aux", [True, False])
@pytest.mark.parametrize("K,hs,S,ws", L_SHAPES)
def test_unit_weights_give_the_bytes_of_the_w_entry_points(K, hs, S, ws, aux):
    c = _linputs(K, hs, S, ws)
    weights = (0.35, 0.15, 0.35, 0.15) if aux else (0.7, 0.3, 0.0, 0.0)
    ones = torch.ones_like(c["rA"])
    old, new = _raw_seg(c, weights, aux=aux), _raw_seg(c, weights, aux=aux, rel=(ones, ones if aux else None))
    assert old["rc_f"] == old["rc_b"] == new["rc_f"] == new["rc_b"] == 0
    assert torch.isfinite(old["grad"]).all() and float(old["grad"].abs().max()) > 0 and float(old["sums"][3]) > 0
    for k in ("sums", "s_seg", "s_img", "roi", "unl", "grad"):
        assert torch.equal(_bits(old[k]), _bits(new[k])), k
    for r in (old, new):
        assert bool((r["gbuf"][:r["pad"]] == SENT).all()) and bool((r["gbuf"][r["pad"] + r["n"]:] == SENT).all())
        assert bool((r["ws"][r["need"]:] == 0xA5).all())
    # real weights through the same buffers: sentinels stay, and a second run gives the same bytes
    a, b = (_raw_seg(c, weights, aux=aux, rel=(c["rA"], c["rB"] if aux else None)) for _ in range(2))
    assert a["rc_f"] == a["rc_b"] == 0 and bool((a["gbuf"][:a["pad"]] == SENT).all()) and bool((a["gbuf"][a["pad"] + a["n"]:] == SENT).all())
    assert bool((a["ws"][a["need"]:] == 0xA5).all()) and not torch.equal(_bits(a["grad"]), _bits(old["grad"]))
    for k in ("sums", "grad", "s_seg"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    assert a["sums"][1::2].tolist() == old["sums"][1::2].tolist()                     # the denominators stay the plain counts


@pytest.mark.parametrize("K,hs,S,ws", L_SHAPES)
def test_zero_weights_on_the_second_map_give_the_gradient_of_zero_blend_weights(K, hs, S, ws):
    c = _linputs(K, hs, S, ws)
    ones = torch.ones_like(c["rA"])
    zeroed = _raw_seg(c, (0.35, 0.15, 0.35, 0.15), rel=(ones, torch.zeros_like(ones)))
    ref = _raw_seg(c, (0.35, 0.15, 0.0, 0.0))
    assert zeroed["rc_f"] == zeroed["rc_b"] == ref["rc_f"] == ref["rc_b"] == 0 and float(ref["grad"].abs().max()) > 0
    assert torch.equal(_bits(zeroed["grad"]), _bits(ref["grad"]))
    assert zeroed["sums"][[4, 6]].tolist() == [0.0, 0.0] and torch.equal(zeroed["sums"][[0, 1, 2, 3, 5, 7]], ref["sums"][[0, 1, 2, 3, 5, 7]])


@pytest.mark.parametrize("bad", [1.5, float("nan"), -0.25, float("inf")])
def test_a_weight_outside_the_unit_interval_gives_nan_through_the_sticky_flag(bad):
    c = _linputs(6, 4, 64)
    for which in (0, 1):
        rel = [c["rA"].clone(), c["rB"].clone()]
        at = torch.nonzero([c["mA"], c["mB"]][which] == 1)[0]
        rel[which][tuple(at)] = bad
        r = _raw_seg(c, (0.35, 0.15, 0.35, 0.15), rel=tuple(rel))
        assert r["rc_f"] == r["rc_b"] == 0
        assert bool(torch.isnan(r["sums"]).all()) and bool(torch.isnan(r["grad"]).all())
        assert bool((r["gbuf"][:r["pad"]] == SENT).all()) and bool(torch.isfinite(r["s_seg"]).all())


def test_rw_refusals_launch_nothing():
    from cosa_amd import _C
    c = _linputs(6, 4, 64)
    for aux, rel in ((True, (None, c["rB"])), (True, (None, None)), (False, (c["rA"], c["rB"])), (True, (c["rA"], None))):
        r = _raw_seg(c, (0.35, 0.15, 0.35, 0.15) if aux else (0.7, 0.3, 0.0, 0.0), aux=aux, rel=rel)
        assert r["rc_f"] == 1 and r["rc_b"] == 1, (aux, rel)
        assert b"weight map" in _C.lib().cosa_last_error()
        assert bool((r["sums"] == SENT).all()) and bool((r["gbuf"] == SENT).all()) and bool((r["ws"] == 0xA5).all())
        assert bool((r["s_seg"] == SENT).all()) and bool((r["roi"] == SENT).all()) and bool((r["unl"] == 7).all())


def test_without_weight_maps_no_rw_entry_point_is_called(monkeypatch):
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    L = _C.lib()
    calls = []

    def spy(name):
        real = getattr(L, name)

        def f(*a):
            calls.append(name)
            return real(*a)
        return f
    for name in ("cosa_seg_loss_forward_rw", "cosa_seg_loss_backward_rw"):
        monkeypatch.setattr(L, name, spy(name), raising=False)
    c = _linputs(6, 4, 64)
    cu = lambda t: t.cuda()

    def run(**kw):
        lr = c["seg"].cuda().requires_grad_(True)
        f_seg, f_reg = seg_helper.fused_seg_and_energy_loss(lr, cu(c["mA"]), cu(c["mB"]), cu(c["simg"]), c["box"], _layer(), fg_alpha=0.3, **kw)
        (W_SEG * f_seg + W_REG * f_reg).sum().backward()
        seg_helper.seg_loss_forward_only(lr.detach(), cu(c["mA"]), cu(c["mB"]), cu(c["simg"]), c["box"], fg_alpha=0.3, **kw)
        return float(f_seg)
    plain = run()
    assert calls == []
    weighted = run(rel_main=cu(c["rA"]), rel_aux=cu(c["rB"]))
    assert calls == ["cosa_seg_loss_forward_rw", "cosa_seg_loss_backward_rw", "cosa_seg_loss_forward_rw"] and weighted < plain
    with pytest.raises(ValueError):
        run(rel_main=cu(c["rA"]))                              # a second label map without its weight map
    with pytest.raises(ValueError):
        run(rel_aux=cu(c["rB"]))


# ---- 3. the trainer at S = 64, b = 2 -----------------------------------------------------------------------------------------------------------
LOSSES = ("overall_loss", "cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")
SEG = LOSSES.index("seg_loss")
REL_ARGS = ("seg_reliability", "seg_reliability_floor", "camweight_beta")


def _trainer(seed=3, drop=False, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, **over)
    if drop:                                                    # a trainer built without the arguments
        for k in REL_ARGS:
            delattr(args, k)
    return CoSATrainer(args, torch.device("cuda", 0), seed=seed)


def _steps(tr, first, last, after=None):
    from cosa_amd.train_step import synthetic_batch
    store = torch.zeros((last - first + 1, len(LOSSES)), dtype=torch.float32, device=tr.device)
    for k in range(first, last + 1):
        logs = tr.step(*synthetic_batch(2, 64, 20, tr.device, seed=900 + k), n_iter=tr.args.warmup_iters + k)      # past the warm-up
        for j, nm in enumerate(LOSSES):
            store[k - first, j] = logs[nm].float()
        if after is not None:
            after(k)
    torch.cuda.synchronize()
    return store


@functools.lru_cache(maxsize=None)
def _run_off():
    tr = _trainer(drop=True)
    assert tr.seg_rel_state is None and tr.seg_reliability() is None and tr.use_graph and tr.fused_losses
    losses = _steps(tr, 1, 2)
    return losses, tr.train_state().checksums(), tr.student.encoder.norm.weight.detach().clone()


@functools.lru_cache(maxsize=None)
def _run_on():
    """four uninterrupted steps with beta = 1 -> (losses, checksums after step 2, checksums after step 4, the final norm's weight after step 2)"""
    tr = _trainer(seg_reliability=True)
    mid = {}

    def after(k):
        if k == 2:
            mid["sums"], mid["norm"] = tr.train_state().checksums(), tr.student.encoder.norm.weight.detach().clone()
    losses = _steps(tr, 1, 4, after)
    return losses, mid["sums"], tr.train_state().checksums(), mid["norm"]


def test_switch_off_is_the_trainer_without_the_arguments():
    losses_a, sums_a, _ = _run_off()
    tr = _trainer(seg_reliability=False, camweight_beta=2.0, seg_reliability_floor=0.5)
    losses_b = _steps(tr, 1, 2)
    assert torch.equal(losses_a.view(torch.int32), losses_b.view(torch.int32)) and tr.train_state().checksums() == sums_a
    assert tr.seg_rel_state is None and not hasattr(tr, "extra_state")


def test_beta_zero_ends_on_the_bytes_of_the_switch_off_run():
    losses_a, sums_a, _ = _run_off()
    tr = _trainer(seg_reliability=True, camweight_beta=0.0, seg_reliability_floor=0.0)
    losses_b = _steps(tr, 1, 2)
    assert torch.equal(losses_a.view(torch.int32), losses_b.view(torch.int32)) and tr.train_state().checksums() == sums_a
    s = tr.seg_reliability()
    assert len(s) == 2 and all(d["bg"] in (None, 1.0) and d["fg"] in (None, 1.0) and d["n_bg"] + d["n_fg"] > 0 for d in s)
    assert tr.seg_reliability() == [dict(bg=None, n_bg=0, fg=None, n_fg=0)] * 2          # read and zeroed
    assert not hasattr(tr, "extra_state")                                                # no state-file entry


def test_beta_one_lowers_the_seg_loss_moves_the_weights_and_resumes(tmp_path):
    losses_off, _, norm_off = _run_off()
    losses_a, mid_a, end_a, norm_on = _run_on()
    assert bool(torch.isfinite(losses_a).all())
    assert float(losses_a[0, SEG]) < float(losses_off[0, SEG])               # weights in [0, 1] on the same pixels, the same counts: <=, and strictly
    for j, nm in enumerate(LOSSES):
        if nm not in ("seg_loss", "overall_loss"):
            assert float(losses_a[0, j]) == float(losses_off[0, j]), nm      # the first step's other terms do not see the switch
    assert not torch.equal(norm_on, norm_off)
    b = _trainer(seg_reliability=True)
    losses_b = _steps(b, 1, 2)
    assert torch.equal(losses_b.view(torch.int32), losses_a[:2].view(torch.int32)) and b.train_state().checksums() == mid_a
    path = str(tmp_path / "state_00000002.cosa")
    b.save_state(path, n_iter=1)
    b.wait_state()
    del b
    c = _trainer(seed=77, seg_reliability=True)
    try:
        assert c.load_state(path)["n_iter"] == 1
    finally:
        os.remove(path)
    losses_c = _steps(c, 3, 4)
    assert torch.equal(losses_c.view(torch.int32), losses_a[2:].view(torch.int32)) and c.train_state().checksums() == end_a
    s = c.seg_reliability()                                                   # only the two steps since the resume: the counters are not state
    assert sum(d["n_bg"] + d["n_fg"] for d in s) <= 2 * 2 * 2 * 64 * 64


def _first_step(tr, seed=901):
    """one step past warm-up -> (losses dict, d loss / d seg_pred)"""
    from cosa_amd.train_step import synthetic_batch
    grads = []

    def hook(_mod, _inp, out):
        if not grads:
            out[3].register_hook(lambda g: grads.append(g.detach().clone()))
    h = tr.student.register_forward_hook(hook)
    try:
        logs = tr.step(*synthetic_batch(2, 64, 20, tr.device, seed=seed), n_iter=tr.args.warmup_iters + 1)
    finally:
        h.remove()
    torch.cuda.synchronize()
    return {n: float(logs[n]) for n in LOSSES}, grads[0].float().cpu()


@pytest.mark.parametrize("over", [dict(), dict(aux_cam2seg=False, segfg_alpha=0.3, camweight_beta=2.0, seg_reliability_floor=0.25)],
                         ids=["defaults", "no_aux_beta2"])
def test_fused_against_torch_path(over):
    """identical weights and batch: the losses within 1e-4 relative, d loss / d seg_pred within 2e-3 of its maximum (the bars of
    tests/test_loss_flags_gpu.py::test_fused_against_torch_path)"""
    first, g = _first_step(_trainer(seg_reliability=True, **over))
    tr = _trainer(seg_reliability=True, fused_losses=False, **over)
    assert not tr.fused_losses
    ref, g_ref = _first_step(tr)
    print({k: (first[k], ref[k]) for k in LOSSES})
    for k in LOSSES:
        assert first[k] == pytest.approx(ref[k], rel=1e-4), (k, first[k], ref[k])
    err, top = (g - g_ref).abs().max().item(), g_ref.abs().max().item()
    print("seg_pred grad err", err, "of max", top)
    assert top > 0 and err <= 2e-3 * top, (err, top)


def test_usegmm_hands_the_kernel_device_thresholds(monkeypatch):
    from cosa_amd.utils import seg_helper
    real, seen = seg_helper.label_reliability, []

    def spy(cams, labels, masks, his, los, **kw):
        seen.append(all(torch.is_tensor(t) and t.is_cuda for t in list(his) + list(los)))
        return real(cams, labels, masks, his, los, **kw)
    monkeypatch.setattr(seg_helper, "label_reliability", spy)
    tr = _trainer(seg_reliability=True, usegmm=True, queue_update_ratio=4, gmmscale=4)
    losses = _steps(tr, 1, 2)
    assert seen == [True, True] and bool(torch.isfinite(losses).all())
    s = tr.seg_reliability()
    assert len(s) == 2 and s[0]["n_bg"] + s[0]["n_fg"] > 0


def test_counters_are_the_restatement_on_the_steps_own_cams_and_labels(monkeypatch):
    from cosa_amd.utils import seg_helper
    real, kept = seg_helper.label_reliability, []

    def spy(cams, labels, masks, his, los, **kw):
        kept.append(([c.detach().cpu().numpy().copy() for c in cams], labels.cpu().numpy().copy(), [m.cpu().numpy().copy() for m in masks],
                     [float(h) for h in his], [float(l) for l in los]))
        return real(cams, labels, masks, his, los, **kw)
    monkeypatch.setattr(seg_helper, "label_reliability", spy)
    tr = _trainer(seg_reliability=True, seg_reliability_floor=0.25)
    _steps(tr, 1, 2)
    assert len(kept) == 2 and len(kept[0][0]) == 2
    want = np.zeros((2, 4), np.int64)
    for cams, y, masks, his, los in kept:
        for g in range(2):
            want[g] += R.weight_stats(R.weight_f32(cams[g], y, masks[g], his[g], los[g], 1.0, 0.25), masks[g], y.shape[1])
    assert tr.seg_rel_state.cpu().numpy().tolist() == want.tolist()
    s = tr.seg_reliability()
    for g in range(2):
        for grp, (i_sum, i_n) in (("bg", (0, 1)), ("fg", (2, 3))):
            assert s[g]["n_" + grp] == want[g, i_n]
            if want[g, i_n]:
                assert s[g][grp] == pytest.approx(want[g, i_sum] / 2.0 ** 32 / want[g, i_n], abs=1e-12) and 0.25 <= s[g][grp] <= 1.0


def test_student_check_scores_the_weighted_term():
    """--student_check_iters 1: the seg term's `loss_rel` (the step's bf16 forward against the fp32 pass, both under the step's weight maps)
    stays at the level of the switch-off run.  A weighted mean of the same non-negative per-pixel terms moves by no more than its largest
    per-pixel share, so within an order of magnitude of the unweighted figure; a check that did not see the weights would instead show the
    gap between the weighted and the plain term (loss_rel = |a - b| / |b| with a weighted and b not), asserted here to be at least twice
    that bar."""
    figs = {}
    for tag, over in (("off", {}), ("on", dict(seg_reliability=True))):
        tr = _trainer(student_check_iters=1, **over)
        losses = _steps(tr, 1, 1)
        figs[tag] = (tr.student_check()["losses"]["seg_loss"]["loss_rel"], float(losses[0, SEG]))
    (rel_off, seg_off), (rel_on, seg_on) = figs["off"], figs["on"]
    bar = max(10 * rel_off, 1e-3)
    gap = abs(seg_off - seg_on) / seg_off
    print(f"student check seg loss_rel: off {rel_off:.3e} on {rel_on:.3e}; weighted against plain term: {gap:.3e}")
    assert rel_on <= bar and gap >= 2 * bar, (rel_on, bar, gap)


def test_grad_check_differences_the_weighted_objective():
    """--grad_check_iters 1 in fp64: r* with the switch on is no further from 1 than the same trainer's value with the switch off plus that
    run's own distance from 1"""
    r = {}
    for tag, over in (("off", {}), ("on", dict(seg_reliability=True))):
        tr = _trainer(grad_check_iters=1, **over)
        _steps(tr, 1, 1)
        s = tr.pop_grad_check()
        assert [d["dir"] for d in s] == ["all"] and s[0]["flags"] == 0
        r[tag] = s[0]["r_star"]
    print(f"grad check r*: off {r['off']:.6f} on {r['on']:.6f}")
    assert abs(r["on"] - 1.0) <= 2 * abs(r["off"] - 1.0), r
