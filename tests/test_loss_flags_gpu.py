"""GPU suite of the fused dense losses at every loss-flag setting (--segfg_alpha a, --aux_cam2seg_alpha b, --aux_cam2seg, --after_softmax).

  1. kernel level: cosa_seg_loss_forward_w / _backward_w and cosa_cam_loss_targets_m against oracle/torch_oracle.py on CPU copies of the
     inputs (the oracle is pinned to the reference at these settings by tests/test_loss_flags_cpu.py), with the bars
     tests/test_losses_gpu.py::test_hip_seg_and_energy_loss_vs_oracle holds the same kernels to: seg_loss 1e-4 relative, energy 1e-3,
     the gradient with respect to the low-resolution logits within 2e-3 of its maximum; the defaults byte for byte against the entry
     points that have them built in; sentinels, refusals, the fixed-point range.
  2. trainer level (crop 64, b = 2, teacher graph on): no flag setting reaches the torch path, fused against `fused_losses=False`,
     run-to-run bits, and the defaults' bits against the built-in entry points.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(6, 4, 64), (3, 8, 64), (21, 12, 192)]      # factor 16 (butterfly-grouped adds) / factor 8 (each quad's own sum) / several blocks, K = 21
# (fg_alpha, aux_alpha, auxiliary label map given)
SETTINGS = [(0.3, 0.5, True), (0.5, 0.25, True), (1.0, 0.5, True), (0.0, 1.0, True), (0.7, 0.0, True), (0.5, 0.5, False), (0.3, 0.5, False)]
W_SEG, W_REG = 0.1, 0.05
SENT = -7.25                                             # sentinel around the gradient (exact in fp32)


def _layer():
    from cosa_amd.utils import seg_helper
    return seg_helper.DenseEnergyLoss(weight=1e-7, sigma_rgb=15, sigma_xy=100, scale_factor=0.5)


@functools.lru_cache(maxsize=None)
def _inputs(K, hs, S, ws=None):
    """B = 2, one full and one partial box; label maps over {0, some classes, 255}; logits hs x hs, or hs x ws"""
    torch.manual_seed(100 + K)
    rng = np.random.default_rng(100 + K)
    B = 2
    vals = [0, 1, K - 1, 255] if K < 8 else [0, 1, 5, K - 1, 255]
    mk = lambda: torch.from_numpy(rng.choice(vals, size=(B, S, S)).astype(np.float32))
    return dict(B=B, K=K, hs=hs, S=S, seg=torch.randn(B, K, hs, ws or hs) * 2, mA=mk(), mB=mk(), simg=torch.randn(B, 3, S, S),
                box=torch.tensor([[0, S, 0, S], [3, S - 4, 0, S - 14]], dtype=torch.int16),
                AS=torch.randn(B, K, S // 2, S // 2) * 1e4)


@functools.lru_cache(maxsize=None)
def _oracle_energy(K, hs, S, ws=None):
    """the regulariser does not depend on the flags: value and gradient w.r.t. the low-resolution logits, once per shape"""
    from oracle import torch_oracle as to
    c = _inputs(K, hs, S, ws)
    lr = c["seg"].clone().requires_grad_(True)
    up = F.interpolate(lr, size=(S, S), mode="bilinear", align_corners=False)
    l_reg, g_up = to.energy_loss_and_grad(c["simg"], up.detach(), c["mA"].to(torch.uint8).unsqueeze(1), c["box"].numpy())
    (g_lr,) = torch.autograd.grad(up, lr, g_up)
    return float(l_reg), g_lr


def _oracle_seg(seg, mA, mB, S, a, b):
    """(1 - b) seg_loss(main, a) + b seg_loss(aux, a) of the up-sampled logits (main.py:200-203); mB None: seg_loss(main, a)"""
    from oracle import torch_oracle as to
    lr = seg.clone().requires_grad_(True)
    up = F.interpolate(lr, size=(S, S), mode="bilinear", align_corners=False)
    l = to.seg_loss(up, mA, fg_alpha=a)
    if mB is not None:
        l = (1 - b) * l + b * to.seg_loss(up, mB, fg_alpha=a)
    (g,) = torch.autograd.grad(l, lr)
    return float(l.detach()), g


def _fused(seg, mA, mB, simg, box, a, b, w_seg=W_SEG, w_reg=W_REG, **kw):
    from cosa_amd.utils import seg_helper
    lr = seg.cuda().requires_grad_(True)
    f_seg, f_reg = seg_helper.fused_seg_and_energy_loss(lr, mA.cuda(), None if mB is None else mB.cuda(), simg.cuda(), box, _layer(),
                                                        fg_alpha=a, aux_alpha=b, **kw)
    (w_seg * f_seg + w_reg * f_reg).sum().backward()
    return float(f_seg.detach()), float(f_reg.detach()), lr.grad.cpu()


def _check_against_oracle(c, mA, mB, a, b, energy):
    S = c["S"]
    l_seg, g_seg = _oracle_seg(c["seg"], mA, mB, S, a, b)
    l_reg, g_reg = energy
    g_ref = W_SEG * g_seg + W_REG * g_reg
    f_seg, f_reg, g = _fused(c["seg"], mA, mB, c["simg"], c["box"], a, b)
    err, top = (g - g_ref).abs().max().item(), g_ref.abs().max().item()
    print(f"K {c['K']} hs {c['hs']} S {S} a {a} b {b} aux {mB is not None}: seg {f_seg:.7f} / {l_seg:.7f}  energy {f_reg:.6e} / {l_reg:.6e}  "
          f"grad err {err:.3e} of max {top:.3e}")
    assert math.isfinite(f_seg) and torch.isfinite(g).all()
    assert f_seg == pytest.approx(l_seg, rel=1e-4)
    assert f_reg == pytest.approx(l_reg, rel=1e-3, abs=1e-12)
    assert err <= 2e-3 * top, (err, top)


@pytest.mark.parametrize("a,b,aux", SETTINGS)
@pytest.mark.parametrize("K,hs,S", SHAPES)
def test_weighted_seg_and_energy_loss_vs_oracle(K, hs, S, a, b, aux):
    c = _inputs(K, hs, S)
    _check_against_oracle(c, c["mA"], c["mB"] if aux else None, a, b, _oracle_energy(K, hs, S))


def test_per_pixel_scatter_shape_vs_oracle():
    """5 x 7 cells under 64 x 64 pixels: factors 12.8 and 9.14, so quads straddle cell borders and their gradient goes through the scatter's
    per-pixel adds (factor 16 takes the butterfly-grouped adds, factor 8 the quad's own sum).  The bars of the test above."""
    K, hs, ws, S = 5, 5, 7, 64
    c = _inputs(K, hs, S, ws)
    assert c["seg"].shape[-2:] == (hs, ws)
    _check_against_oracle(c, c["mA"], c["mB"], 0.3, 0.5, _oracle_energy(K, hs, S, ws))


def test_labels_outside_the_classes_are_ignored_like_255():
    """a label in [K, 255) is outside the contract; the kernels ignore it exactly as they ignore 255 (it used to index past the LDS tile):
    every 255 of both maps rewritten to 200 gives the same bytes in the sums, the energy-grid outputs and the gradient"""
    c = _inputs(6, 4, 64)
    assert int((c["mA"] == 255).sum()) > 0 and int((c["mB"] == 255).sum()) > 0
    other = dict(c, mA=torch.where(c["mA"] == 255, torch.full_like(c["mA"], 200.0), c["mA"]),
                 mB=torch.where(c["mB"] == 255, torch.full_like(c["mB"], 200.0), c["mB"]))
    assert int((other["mA"] == 255).sum()) == 0 and int((other["mB"] == 255).sum()) == 0 and int((other["mA"] == 200).sum()) > 0
    weights = (0.35, 0.15, 0.35, 0.15)
    ref, out = _raw_seg(c, weights), _raw_seg(other, weights)
    assert ref["rc_f"] == ref["rc_b"] == out["rc_f"] == out["rc_b"] == 0
    assert torch.isfinite(ref["grad"]).all() and float(ref["grad"].abs().max()) > 0 and float(ref["sums"][3]) > 0
    assert int(ref["unl"].sum()) > 0
    for k in ("sums", "s_seg", "s_img", "roi", "unl", "grad"):
        assert torch.equal(_bits(ref[k]), _bits(out[k])), k


@pytest.mark.parametrize("a,b", [(0.3, 0.5), (1.0, 0.25)])
def test_label_map_without_foreground_and_one_without_background(a, b):
    """a class group without a pixel has count 0: its term is 0 / 1e-6 = 0 and its coefficient w g / 1e-6 meets no pixel -- no NaN"""
    K, hs, S = 6, 4, 64
    c = _inputs(K, hs, S)
    mA = torch.where(c["mA"] == 255, c["mA"], torch.zeros_like(c["mA"]))                        # background and ignore only
    mB = torch.where(c["mB"] == 0, torch.full_like(c["mB"], 2.0), c["mB"])                      # foreground and ignore only
    assert int(((mA != 0) & (mA != 255)).sum()) == 0 and int((mB == 0).sum()) == 0
    _check_against_oracle(c, mA, mB, a, b, _energy_of(c, mA))
    _check_against_oracle(c, mB, None, a, b, _energy_of(c, mB))


def _energy_of(c, m):
    from oracle import torch_oracle as to
    lr = c["seg"].clone().requires_grad_(True)
    up = F.interpolate(lr, size=(c["S"], c["S"]), mode="bilinear", align_corners=False)
    l_reg, g_up = to.energy_loss_and_grad(c["simg"], up.detach(), m.to(torch.uint8).unsqueeze(1), c["box"].numpy())
    (g_lr,) = torch.autograd.grad(up, lr, g_up)
    return float(l_reg), g_lr


# ---- the raw entry points ------------------------------------------------------------------------------------------------------------------
def _raw_seg(c, weights, aux=True, bwd_weights=None, pad=64):
    """forward + backward through the C ABI: weights None -> the entry points with the defaults built in, else the _w ones.  The gradient
    lives inside a larger buffer of sentinels and the workspace is followed by 256 sentinel bytes."""
    from cosa_amd import _C
    L = _C.lib()
    dev = torch.device("cuda", 0)
    B, K, hs, S = c["B"], c["K"], c["hs"], c["S"]
    Sq = S // 2
    seg, mA, simg, AS = (c[k].to(dev).contiguous() for k in ("seg", "mA", "simg", "AS"))
    mB = c["mB"].to(dev).contiguous() if aux else None
    box = c["box"].to(device=dev, dtype=torch.int32).contiguous()
    need = L.cosa_seg_loss_workspace_bytes(B, K, hs, hs)
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=dev)
    sums = torch.full((8,), SENT, device=dev)
    s_seg, s_img = torch.empty((B, K, Sq, Sq), device=dev), torch.empty((B, 3, Sq, Sq), device=dev)
    roi, unl = torch.empty((B, Sq, Sq), device=dev), torch.empty((B, Sq, Sq), device=dev, dtype=torch.uint8)
    n = B * K * hs * hs
    gbuf = torch.full((pad + n + pad,), SENT, device=dev)
    grad = gbuf[pad:pad + n]
    gs, gr = torch.tensor([W_SEG], device=dev), torch.tensor([W_REG * 1e-7], device=dev)
    fwd = L.cosa_seg_loss_forward if weights is None else L.cosa_seg_loss_forward_w
    rc_f = fwd(_C.ptr(seg), _C.ptr(mA), _C.ptr(mB), _C.ptr(simg), _C.ptr(box), _C.ptr(sums), _C.ptr(s_seg), _C.ptr(s_img), _C.ptr(roi),
               _C.ptr(unl), B, K, hs, hs, S, _C.ptr(ws), need, _C.stream_ptr())
    bw = weights if bwd_weights is None else bwd_weights
    if bw is None:
        rc_b = L.cosa_seg_loss_backward(_C.ptr(seg), _C.ptr(mA), _C.ptr(mB), _C.ptr(sums), _C.ptr(AS), _C.ptr(roi), _C.ptr(gs), _C.ptr(gr),
                                        _C.ptr(grad), B, K, hs, hs, S, _C.ptr(ws), need, _C.stream_ptr())
    else:
        rc_b = L.cosa_seg_loss_backward_w(_C.ptr(seg), _C.ptr(mA), _C.ptr(mB), _C.ptr(sums), _C.ptr(AS), _C.ptr(roi), _C.ptr(gs), _C.ptr(gr),
                                          _C.ptr(grad), *[float(w) for w in bw], B, K, hs, hs, S, _C.ptr(ws), need, _C.stream_ptr())
    torch.cuda.synchronize()
    return dict(rc_f=rc_f, rc_b=rc_b, sums=sums, s_seg=s_seg, s_img=s_img, roi=roi, unl=unl, gbuf=gbuf, grad=grad, ws=ws, need=need, pad=pad, n=n)


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


@pytest.mark.parametrize("K,hs,S", SHAPES)
def test_default_weights_give_the_bits_of_the_builtin_entry_points(K, hs, S):
    """(0.25, 0.25, 0.25, 0.25) with both label maps through the weighted entry points = the entry points that have the defaults built in,
    byte for byte, on every output: default runs keep their bits"""
    c = _inputs(K, hs, S)
    old, new = _raw_seg(c, None), _raw_seg(c, (0.25, 0.25, 0.25, 0.25))
    assert old["rc_f"] == old["rc_b"] == new["rc_f"] == new["rc_b"] == 0
    assert torch.isfinite(old["grad"]).all() and float(old["grad"].abs().max()) > 0
    for k in ("sums", "grad", "s_seg", "s_img", "roi", "unl"):
        assert torch.equal(_bits(old[k]), _bits(new[k])), k
    # and through the autograd function: value and gradient
    a = _fused(c["seg"], c["mA"], c["mB"], c["simg"], c["box"], 0.5, 0.5)
    b = _fused(c["seg"], c["mA"], c["mB"], c["simg"], c["box"], 0.5, 0.5, _builtin_defaults=True)
    assert a[0] == b[0] and a[1] == b[1] and torch.equal(_bits(a[2]), _bits(b[2]))


@pytest.mark.parametrize("K,hs,S", SHAPES)
def test_sentinels_around_gradient_and_workspace_survive(K, hs, S):
    c = _inputs(K, hs, S)
    for weights, aux in (((0.35, 0.15, 0.35, 0.15), True), ((0.7, 0.3, 0.0, 0.0), False)):
        r = _raw_seg(c, weights, aux=aux)
        assert r["rc_f"] == r["rc_b"] == 0
        assert torch.isfinite(r["grad"]).all() and float(r["grad"].abs().max()) > 0
        assert bool((r["gbuf"][:r["pad"]] == SENT).all()) and bool((r["gbuf"][r["pad"] + r["n"]:] == SENT).all())
        assert bool((r["ws"][r["need"]:] == 0xA5).all())
        if not aux:     # nothing of a second label map: its four sums come back as zeros
            assert r["sums"][4:].tolist() == [0.0, 0.0, 0.0, 0.0] and float(r["sums"][1]) > 0


def test_zero_weight_and_missing_aux_map_contribute_nothing():
    """b = 0 with a second label map given = no second label map.  The sums of the main map are the same bits; in the gradient a zero
    coefficient adds an exact 0 to every pixel's term, but the compiler may contract the two- and the three-product forms into different
    fused multiply-adds, so single fp32 roundings per pixel may differ: 1e-6 of the largest gradient (~ 8 ulp), not bits"""
    c = _inputs(6, 4, 64)
    with_b, without = _raw_seg(c, (0.7, 0.3, 0.0, 0.0), aux=True), _raw_seg(c, (0.7, 0.3, 0.0, 0.0), aux=False)
    top = float(without["grad"].abs().max())
    assert top > 0 and float((with_b["grad"] - without["grad"]).abs().max()) <= 1e-6 * top
    assert torch.equal(with_b["sums"][:4], without["sums"][:4])


@pytest.mark.parametrize("bad", [(-0.1, 0.5, 0.3, 0.3), (0.25, 1.5, 0.25, 0.25), (0.25, 0.25, float("nan"), 0.25), (0.25, 0.25, 0.25, float("inf")),
                                 (0.25, 0.25, -1e-9, 0.25)])
def test_refused_weights_launch_nothing(bad):
    from cosa_amd import _C
    c = _inputs(6, 4, 64)
    r = _raw_seg(c, (0.25, 0.25, 0.25, 0.25), bwd_weights=bad)
    assert r["rc_f"] == 0 and r["rc_b"] == 1                                  # COSA_EINVAL
    assert b"[0, 1]" in _C.lib().cosa_last_error()
    assert bool((r["gbuf"] == SENT).all())                                   # no conversion kernel ran
    # the gradient cells of the workspace were not even cleared: only the forward's 64 x 8 sums and the flag word were written
    cells = r["ws"][64 * 8 * 8:64 * 8 * 8 + r["n"] * 8]
    assert bool((cells == 0xA5).all())


def test_refused_null_pointers_and_modes_launch_nothing():
    from cosa_amd import _C
    L = _C.lib()
    c = _inputs(6, 4, 64)
    r = _raw_seg(c, None, aux=False)                                           # the built-in entry points need both label maps
    assert r["rc_f"] == 1 and r["rc_b"] == 1
    assert bool((r["sums"] == SENT).all()) and bool((r["gbuf"] == SENT).all()) and bool((r["ws"] == 0xA5).all())
    seg = torch.randn(4, 6, 8, 8, device="cuda")
    lab = torch.ones(2, 5, device="cuda")
    out = torch.full((2, 5, 4, 4), SENT, device="cuda")
    for mode in (2, -1):
        assert _raw_cam([seg], lab, 64, out, 0.01, mode) == 1
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    # a null or an empty scale: refused as cosa_cam_label refuses it, with a message that names the scale
    two = [seg, torch.randn(4, 6, 4, 4, device="cuda")]
    n = len(two)
    hs, ws = _C.int_array([t.shape[2] for t in two]), _C.int_array([t.shape[3] for t in two])
    targets = lambda ptrs, hs: L.cosa_cam_loss_targets_m(ptrs, hs, ws, n, _C.ptr(lab), _C.ptr(out), 2, 6, 64, 4, 4, 0.01, 0, _C.stream_ptr())
    assert targets((ctypes.c_void_p * n)(two[0].data_ptr(), None), hs) == 1
    assert b"scale 1" in L.cosa_last_error()
    assert targets((ctypes.c_void_p * n)(*[t.data_ptr() for t in two]), _C.int_array([8, 0])) == 1
    assert b"scale 1" in L.cosa_last_error()
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert targets((ctypes.c_void_p * n)(*[t.data_ptr() for t in two]), hs) == 0
    assert _raw_cam([seg], lab, 64, out, 0.01, 1) == 0 and _raw_cam([seg], lab, 64, out, 0.0, 1) == 1


def test_weight_eight_on_one_foreground_pixel_is_finite_and_linear():
    """fg_alpha = 1, one foreground pixel per image, loss weight 8 (the shape of tests/test_losses_gpu.py's large-weight test): one add is
    0.5 * 8 / 2 = 2 per label map (the count runs over the batch) -- inside the fixed-point range (|v| < 16 holds for every g < 16 with this weight table) -- so the
    gradient is finite and 8 x the weight-1 gradient"""
    from cosa_amd.utils import seg_helper
    from cosa_amd.train_step import synthetic_batch
    dev = torch.device("cuda", 0)
    B, K, S = 2, 21, 224
    _, simg, _, box = synthetic_batch(B, S, 20, dev, seed=3)
    g = torch.Generator().manual_seed(1)
    few = torch.zeros(B, S, S, device=dev)
    few[:, 100, 120] = 3.0
    seg0 = torch.randn(B, K, S // 16, S // 16, generator=g).to(dev)
    grads = []
    for wgt in (1.0, 8.0):
        seg = seg0.clone().requires_grad_(True)
        l_seg, _ = seg_helper.fused_seg_and_energy_loss(seg, few, few.clone(), simg, box, _layer(), fg_alpha=1.0, aux_alpha=0.5)
        (l_seg * wgt).backward()
        assert math.isfinite(float(l_seg)) and torch.isfinite(seg.grad).all(), wgt
        grads.append(seg.grad.clone())
    assert float(grads[0].abs().max()) > 0.05                                    # the lone pixels' cells carry ~ 0.5 x bilinear weight x (1 - p)
    assert torch.allclose(grads[1], 8.0 * grads[0], rtol=1e-5, atol=1e-12)


# ---- cam_loss targets --------------------------------------------------------------------------------------------------------------------
def _raw_cam(scales, labels, S, out, temp, mode):
    """mode None: cosa_cam_loss_targets (the default branch built in), else cosa_cam_loss_targets_m(after_softmax=mode) -> status"""
    from cosa_amd import _C
    L = _C.lib()
    B, K = scales[0].shape[0] // 2, scales[0].shape[1]
    n = len(scales)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in scales])
    hs, ws = _C.int_array([t.shape[2] for t in scales]), _C.int_array([t.shape[3] for t in scales])
    lab = labels.contiguous().float()
    if mode is None:
        return L.cosa_cam_loss_targets(ptrs, hs, ws, n, _C.ptr(lab), _C.ptr(out), B, K, int(S), out.shape[2], out.shape[3], float(temp),
                                       _C.stream_ptr())
    return L.cosa_cam_loss_targets_m(ptrs, hs, ws, n, _C.ptr(lab), _C.ptr(out), B, K, int(S), out.shape[2], out.shape[3], float(temp), int(mode),
                                     _C.stream_ptr())


def test_cam_loss_targets_after_softmax_vs_reference_golden(golden):
    """cam_target_kernel's after_softmax branch, fed the golden seg as one full-size scale plus a zero flipped half, against the reference's
    seg_refine_by_label(after_softmax=True) output resized to the CAM grid (atol 2e-6, rtol 1e-5: the bars of the default branch's test);
    image 0 has no class present, image 1 two.  Chained with the loss kernel: the reference's cam_loss."""
    from cosa_amd.utils import seg_helper
    g = golden("loss_flags")
    dev = "cuda"
    seg, labels = torch.from_numpy(g["refine_seg"]).to(dev), torch.from_numpy(g["refine_labels"]).to(dev)
    cam = torch.from_numpy(g["camloss_cam"]).to(dev)
    ref = torch.from_numpy(g["refine_after"]).to(dev)
    assert labels.sum(1).tolist() == [0.0, 2.0]
    tgt = F.interpolate(ref[:, 1:], size=cam.shape[-2:], mode="bilinear", align_corners=False).contiguous()
    S = seg.shape[-1]
    scales = [torch.cat([seg, torch.zeros_like(seg)], 0).contiguous()]
    out = seg_helper.cam_loss_targets(scales, labels, S, tuple(cam.shape[-2:]), float(g["temp"]), after_softmax=True)
    print("after_softmax targets: max |diff|", (out - tgt).abs().max().item())
    assert torch.allclose(out, tgt, atol=2e-6, rtol=1e-5), (out - tgt).abs().max().item()
    assert float(out[0].abs().max()) == 0.0 and float(out[1, [0, 2, 4]].abs().max()) == 0.0 and float(out[1, [1, 3]].max()) > 0.05
    assert float(seg_helper.cam_loss_from_targets(cam, out)) == pytest.approx(float(g["camloss_after"]), rel=1e-5)
    # the default branch on the same input is another function (absent classes cannot take probability mass there)
    other = seg_helper.cam_loss_targets(scales, labels, S, tuple(cam.shape[-2:]), float(g["temp"]))
    assert not torch.allclose(other, out, atol=1e-3)


def test_cam_loss_targets_after_softmax_multi_scale_vs_oracle():
    """three low-resolution scales with live flipped halves (what the trainer feeds it) against the oracle on the summed full-resolution seg"""
    from cosa_amd.utils import seg_helper
    from oracle import torch_oracle as to
    torch.manual_seed(11)
    B, K, S, G = 2, 21, 64, 4
    scales = [torch.randn(2 * B, K, h, h) for h in (4, 2, 6)]
    labels = torch.zeros(B, K - 1)
    labels[0, [2, 7, 19]] = 1
    labels[1, [0]] = 1
    full = sum(F.interpolate(t[:B], size=(S, S), mode="bilinear", align_corners=False) +
               F.interpolate(t[B:], size=(S, S), mode="bilinear", align_corners=False).flip(-1) for t in scales)
    # T = 1: six bilinear blends of |z| <= ~4 are rounded differently by the kernel (fma) and by torch, <= ~1e-6 on a summed logit -- a
    # relative 2e-6 on a probability --, the fast exponential adds ~2e-6 at |x| <= 30: rtol 2e-5 leaves a factor 5, atol as in the golden test
    # (at the reference's T = 0.01 the softmax would amplify the blends' last bits 100 x; the golden test above covers that temperature)
    temp = 1.0
    ref = to.seg_refine_by_label(full, labels, temp, after_softmax=True)
    tgt = F.interpolate(ref[:, 1:], size=(G, G), mode="bilinear", align_corners=False)
    out = seg_helper.cam_loss_targets([t.cuda() for t in scales], labels.cuda(), S, (G, G), temp, after_softmax=True).cpu()
    assert torch.allclose(out, tgt, atol=2e-6, rtol=2e-5), (out - tgt).abs().max().item()
    assert float(out[0, [0, 1]].abs().max()) == 0.0 and float(out[0, 2].max()) > 0


def test_cam_loss_targets_mode_zero_is_the_builtin_entry_point_bit_for_bit():
    torch.manual_seed(12)
    B, K, S = 2, 21, 64
    scales = [torch.randn(2 * B, K, h, h, device="cuda") for h in (4, 2, 6)]
    labels = torch.zeros(B, K - 1, device="cuda")
    labels[0, [2, 7]] = 1
    old, new = torch.full((B, K - 1, 4, 4), SENT, device="cuda"), torch.full((B, K - 1, 4, 4), SENT, device="cuda")
    assert _raw_cam(scales, labels, S, old, 0.01, None) == 0 and _raw_cam(scales, labels, S, new, 0.01, 0) == 0
    torch.cuda.synchronize()
    assert bool((old != SENT).all()) and torch.equal(_bits(old), _bits(new))


# ---- the trainer -------------------------------------------------------------------------------------------------------------------------
CONFIGS = {"segfg_alpha": dict(segfg_alpha=0.3), "aux_alpha": dict(aux_cam2seg_alpha=0.25), "no_aux": dict(aux_cam2seg=False),
           "after_softmax": dict(after_softmax=True),
           "all_four": dict(segfg_alpha=0.3, aux_cam2seg_alpha=0.25, aux_cam2seg=False, after_softmax=True)}
LOSSES = ("cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")


def _trainer(seed=3, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, **over)
    return CoSATrainer(args, torch.device("cuda", 0), seed=seed)


def _batch(tr, k):
    from cosa_amd.train_step import synthetic_batch
    return synthetic_batch(2, 64, 20, tr.device, seed=700 + k)


def _state(tr):
    """clones of what a step writes: masters of both networks and the moments"""
    out = {}
    for tag, net in (("ON", tr.student), ("AN", tr.model_AN)):
        for n, p in net.named_parameters():
            out[f"{tag}.{n}"] = p.detach().clone()
    names = {id(p): n for n, p in tr.student.named_parameters()}
    for p, st in tr.optimizer.state.items():
        for k in ("exp_avg", "exp_avg_sq"):
            out[f"opt.{names[id(p)]}.{k}"] = st[k].clone()
    return out


def _assert_same_state(a, b):
    assert a.keys() == b.keys() and len(a) > 300
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


class _NoTorchLosses:
    """inside the block train_step's F.interpolate (the up-sampling of the student's logits -- train_step's own name `F` is replaced, the
    position-embedding set-up of models/vit.py keeps torch's) and the torch-path loss functions of seg_helper raise"""

    NAMES = ("seg_loss", "get_energy_loss", "seg_refine_by_label", "cam_loss")

    def __enter__(self):
        import types
        from cosa_amd import train_step
        from cosa_amd.utils import seg_helper

        def refuse(name):
            def f(*a, **k):
                raise AssertionError(f"the torch path was taken: {name} called")
            return f
        self.ts, self.sh, self.F = train_step, seg_helper, train_step.F
        proxy = types.SimpleNamespace(**{k: getattr(self.F, k) for k in dir(self.F) if not k.startswith("__")})
        proxy.interpolate = refuse("train_step.F.interpolate")
        train_step.F = proxy
        self.saved = {n: getattr(seg_helper, n) for n in self.NAMES}
        for n in self.NAMES:
            setattr(seg_helper, n, refuse("seg_helper." + n))
        return self

    def __exit__(self, *exc):
        self.ts.F = self.F
        for n, f in self.saved.items():
            setattr(self.sh, n, f)
        return False


def _run(tr, steps=2):
    """`steps` steps past warm-up -> (the five losses of the first step, d loss / d seg_pred of the first step)"""
    grads = []

    def hook(_mod, _inp, out):
        if not grads:
            out[3].register_hook(lambda g: grads.append(g.detach().clone()))
    h = tr.student.register_forward_hook(hook)
    try:
        first = None
        for k in range(steps):
            logs = tr.step(*_batch(tr, k), n_iter=tr.args.warmup_iters + 1 + k)
            if first is None:
                first = {n: float(logs[n]) for n in LOSSES}
    finally:
        h.remove()
    torch.cuda.synchronize()
    assert all(math.isfinite(v) for v in first.values()), first
    return first, grads[0].float().cpu()


@functools.lru_cache(maxsize=None)
def _fused_run(name):
    """a fused trainer of configuration `name`, two steps with the torch path barred -> (losses, seg_pred gradient, state)"""
    tr = _trainer(**CONFIGS[name])
    assert tr.fused_losses and tr.use_graph
    with _NoTorchLosses():
        first, g = _run(tr)
    return first, g, _state(tr)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_no_flag_setting_reaches_the_torch_path(name):
    first, g, _ = _fused_run(name)
    assert first["seg_loss"] > 0 and first["cam_loss"] > 0 and float(g.abs().max()) > 0


def test_the_bar_on_the_torch_path_bites():
    """the same bar makes a `fused_losses=False` trainer fail: the test above cannot pass by the bar not working"""
    tr = _trainer(fused_losses=False, segfg_alpha=0.3)
    with _NoTorchLosses():
        with pytest.raises(AssertionError, match="the torch path was taken"):
            tr.step(*_batch(tr, 0), n_iter=tr.args.warmup_iters + 1)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fused_against_torch_path(name):
    """identical weights and batch: the five losses within 1e-4 relative, d loss / d seg_pred within 2e-3 of its maximum"""
    first, g, _ = _fused_run(name)
    tr = _trainer(fused_losses=False, **CONFIGS[name])
    assert not tr.fused_losses
    ref, g_ref = _run(tr, steps=1)
    print(name, {k: (first[k], ref[k]) for k in LOSSES})
    for k in LOSSES:
        assert first[k] == pytest.approx(ref[k], rel=1e-4), (k, first[k], ref[k])
    err, top = (g - g_ref).abs().max().item(), g_ref.abs().max().item()
    print(name, "seg_pred grad err", err, "of max", top)
    assert top > 0 and err <= 2e-3 * top, (err, top)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fused_trainers_of_one_seed_end_in_the_same_bits(name):
    _, g, state = _fused_run(name)
    tr = _trainer(**CONFIGS[name])
    _, g2 = _run(tr)
    assert torch.equal(_bits(g), _bits(g2))
    _assert_same_state(state, _state(tr))


def test_default_flags_keep_the_bits_of_the_builtin_entry_points(monkeypatch):
    """two steps at default flags: the weighted entry points (what the trainer calls now) against a trainer whose losses go through the
    entry points with the defaults built in"""
    from cosa_amd.utils import seg_helper
    a = _trainer()
    la, ga = _run(a)
    sa = _state(a)
    fused, calls = seg_helper.fused_seg_and_energy_loss, []

    def builtin_fused(*args, fg_alpha=0.5, aux_alpha=0.5, **kw):
        calls.append("seg")
        return fused(*args, fg_alpha=fg_alpha, aux_alpha=aux_alpha, _builtin_defaults=True, **kw)

    def builtin_targets(seg_scales, cls_label, S, out_hw, softmaxtemp, after_softmax=False):
        assert not after_softmax
        calls.append("cam")
        out = torch.empty((seg_scales[0].shape[0] // 2, seg_scales[0].shape[1] - 1) + tuple(out_hw), device=seg_scales[0].device)
        assert _raw_cam(seg_scales, cls_label, S, out, softmaxtemp, None) == 0
        return out
    monkeypatch.setattr(seg_helper, "fused_seg_and_energy_loss", builtin_fused)
    monkeypatch.setattr(seg_helper, "cam_loss_targets", builtin_targets)
    b = _trainer()
    lb, gb = _run(b)
    assert calls == ["seg", "cam"] * 2
    assert la == lb and torch.equal(_bits(ga), _bits(gb))
    _assert_same_state(sa, _state(b))
