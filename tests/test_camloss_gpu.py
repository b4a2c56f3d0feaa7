"""GPU suite of --camloss_version v2 | v3.

  1. kernel level: cosa_cam_lossv2, cosa_cam_lossv3 and cosa_cam_label against the float64 restatement (tests/camloss_ref.py, pinned to the
     reference by tests/test_camloss_cpu.py) on CPU copies of the inputs, with the bars tests/test_loss_flags_gpu.py holds the fused losses
     to: value 1e-4 relative, gradient within 2e-3 of its maximum; sentinels, refusals, run-to-run bytes; the public functions through autograd.
  2. trainer level (crop 64, b = 2, teacher graph on): the fused path is taken, fused against `fused_losses=False`, run-to-run bits, v1
     untouched, the student check under v3.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import camloss_ref as R
from test_loss_flags_gpu import _NoTorchLosses as _FlagBar, _assert_same_state, _batch, _bits, _state, _trainer

pytestmark = pytest.mark.gpu

SENT = -7.25                                             # sentinel around the outputs (exact in fp32)
PAD = 64
V2_PLANES = [(4, 4), (5, 7), (40, 40)]                   # one element per thread at most / an odd plane / 6.25 elements per thread, not a multiple of 64
V3_SHAPES = [(5, 4, 64), (2, 8, 64), (20, 12, 192)]      # (C, h, S): factor 16 (grouped adds) / factor 8 (per-quad adds) / several blocks, K = 21
t64 = lambda a: torch.from_numpy(np.asarray(a)).double()


def _guarded(n, dtype=torch.float32, fill=SENT):
    """a buffer of n elements with PAD sentinels on either side -> (whole, view)"""
    whole = torch.full((n + 2 * PAD,), fill, device="cuda", dtype=dtype)
    return whole, whole[PAD:PAD + n]


def _intact(whole, n, fill=SENT):
    return bool((whole[:PAD] == fill).all()) and bool((whole[PAD + n:] == fill).all())


def _raw_v2(cam, y, null=None, ws_short=False):
    from cosa_amd import _C
    L = _C.lib()
    B, C, h, w = cam.shape
    x, yy = cam.cuda().contiguous(), y.cuda().float().contiguous()
    gw, g = _guarded(x.numel())
    lw, l = _guarded(1)
    need = int(L.cosa_cam_lossv2_workspace_bytes(B, C)) or 256
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = lambda t, name: _C.ptr(None if null == name else t)
    rc = L.cosa_cam_lossv2(ptr(x, "cam"), ptr(yy, "targets"), ptr(g, "grad"), ptr(l, "loss"), B, C, h, w, ptr(ws, "ws"),
                           need - 8 if ws_short else need, _C.stream_ptr())
    torch.cuda.synchronize()
    return dict(rc=rc, loss=l.clone(), grad=g.clone().view(B, C, h, w), gw=gw, lw=lw, ws=ws, need=need, n=x.numel())


def _raw_v3(cam, label, S=None, null=None, ws_short=False):
    from cosa_amd import _C
    L = _C.lib()
    B, C, h, w = cam.shape
    x, lab = cam.cuda().contiguous(), label.cuda().to(torch.uint8).contiguous()
    gw, g = _guarded(x.numel())
    lw, l = _guarded(1)
    need = int(L.cosa_cam_lossv3_workspace_bytes(*cam.shape)) or 256
    ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    ptr = lambda t, name: _C.ptr(None if null == name else t)
    rc = L.cosa_cam_lossv3(ptr(x, "cam"), ptr(lab, "label"), ptr(g, "grad"), ptr(l, "loss"), B, C, h, w, S or label.shape[-1], ptr(ws, "ws"),
                           need - 8 if ws_short else need, _C.stream_ptr())
    torch.cuda.synchronize()
    return dict(rc=rc, loss=l.clone(), grad=g.clone().view(cam.shape), gw=gw, lw=lw, ws=ws, need=need, n=x.numel())


def _raw_label(scales, cls, S, T, thre, after, out=None, K=None):
    from cosa_amd import _C
    dev = [s.cuda().contiguous() for s in scales]
    B = dev[0].shape[0] // 2
    ow, o = (None, out) if out is not None else _guarded(B * S * S, torch.uint8, 0x5A)
    n = len(dev)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in dev])
    hs, ws = _C.int_array([t.shape[2] for t in dev]), _C.int_array([t.shape[3] for t in dev])
    lab = cls.cuda().float().contiguous()
    rc = _C.lib().cosa_cam_label(ptrs, hs, ws, n, _C.ptr(lab), _C.ptr(o), B, K or dev[0].shape[1], S, T, thre, after, _C.stream_ptr())
    torch.cuda.synchronize()
    return rc, o.clone().view(B, S, S), ow


def _check(what, r, loss64, grad64):
    """the project's bars for a fused loss: value 1e-4 relative, gradient within 2e-3 of its maximum (measured: printed)"""
    assert r["rc"] == 0
    le = abs(float(r["loss"]) - float(loss64)) / abs(float(loss64))
    top = float(grad64.abs().max())
    ge = float((r["grad"].cpu().double() - grad64).abs().max()) / top
    print(f"{what}: loss {float(r['loss']):.7f} rel err {le:.2e}, grad err {ge:.2e} of max {top:.3e}")
    assert le <= 1e-4 and top > 0 and ge <= 2e-3, (what, le, ge)
    assert _intact(r["gw"], r["n"]) and _intact(r["lw"], 1) and bool((r["ws"][r["need"]:] == 0xA5).all())


# ---- v2 ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _v2_case(h, w):
    rng = np.random.default_rng(10 * h + w)
    cam = torch.from_numpy(R.special_cam(rng, 2, 5, h, w))
    y = torch.from_numpy(rng.uniform(0, 1, (2, 5, h, w)).astype(np.float32))
    return cam, y, R.v2_loss(cam.double(), y.double()), R.v2_grad(cam.double(), y.double())


@pytest.mark.parametrize("h,w", V2_PLANES)
def test_v2_kernel_vs_float64(h, w):
    cam, y, loss64, grad64 = _v2_case(h, w)
    r = _raw_v2(cam, y)
    _check(f"v2 {h}x{w}", r, loss64, grad64)
    assert not r["grad"][0, 1].any() and float(r["grad"][0, 0].abs().max()) > 0          # the all-non-positive plane; the all-positive one
    r2 = _raw_v2(cam, y)
    assert torch.equal(_bits(r["loss"]), _bits(r2["loss"])) and torch.equal(_bits(r["grad"]), _bits(r2["grad"]))


# ---- v3 ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _v3_case(C, h, S):
    rng = np.random.default_rng(100 * C + h)
    cam = torch.from_numpy(R.special_cam(rng, 2, C, h, h))
    vals = [0, 1, C, 255] if C < 8 else [0, 1, 5, C, 255]
    lab = torch.from_numpy(rng.choice(vals, size=(2, S, S)).astype(np.uint8))
    return cam, lab, R.v3_loss(cam.double(), lab), R.v3_grad(cam.double(), lab)


@pytest.mark.parametrize("C,h,S", V3_SHAPES)
def test_v3_kernel_vs_float64(C, h, S):
    cam, lab, loss64, grad64 = _v3_case(C, h, S)
    r = _raw_v3(cam, lab)
    _check(f"v3 C={C} h={h} S={S}", r, loss64, grad64)
    assert not r["grad"][0, 1].any() and not r["grad"][1, :, 0, 0].any()                # the all-non-positive plane, the dead cell
    r2 = _raw_v3(cam, lab)
    assert torch.equal(_bits(r["loss"]), _bits(r2["loss"])) and torch.equal(_bits(r["grad"]), _bits(r2["grad"]))


@pytest.mark.parametrize("C,h,S", V3_SHAPES[:2])
def test_v3_label_map_without_foreground_and_one_without_background(C, h, S):
    cam = _v3_case(C, h, S)[0]
    rng = np.random.default_rng(5)
    for name, vals in (("no foreground", [0, 255]), ("no background", [1, C, 255]), ("all ignored", [255])):
        lab = torch.from_numpy(rng.choice(vals, size=(2, S, S)).astype(np.uint8))
        r = _raw_v3(cam, lab)
        assert r["rc"] == 0 and torch.isfinite(r["loss"]).all() and torch.isfinite(r["grad"]).all(), name
        want = R.v3_loss(cam.double(), lab)
        assert float(r["loss"]) == pytest.approx(float(want), rel=1e-4, abs=1e-12), name
        g64 = R.v3_grad(cam.double(), lab)
        assert float((r["grad"].cpu().double() - g64).abs().max()) <= 2e-3 * float(g64.abs().max()), name


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def _untouched(r):
    return bool((r["gw"] == SENT).all()) and bool((r["lw"] == SENT).all()) and bool((r["ws"] == 0xA5).all())


def test_refusals_launch_nothing():
    from cosa_amd import _C
    cam, y = _v2_case(4, 4)[:2]
    lab = _v3_case(5, 4, 64)[1]
    for name in ("cam", "targets", "grad", "loss", "ws"):
        r = _raw_v2(cam, y, null=name)
        assert r["rc"] == 1 and _untouched(r), name
    for name in ("cam", "label", "grad", "loss", "ws"):
        r = _raw_v3(cam, lab, null=name)
        assert r["rc"] == 1 and _untouched(r), name
    for r in (_raw_v2(cam, y, ws_short=True), _raw_v3(cam, lab, ws_short=True)):
        assert r["rc"] == 1 and _untouched(r)
    # a plane outside the envelope (81 x 80), more than 128 classes, an up-sampling factor below 8, an odd label map
    big = torch.zeros(1, 1, 81, 80)
    r = _raw_v2(big, big)
    assert r["rc"] == 1 and _untouched(r) and b"envelope" in _C.lib().cosa_last_error()
    r = _raw_v3(big, torch.zeros(1, 648, 648, dtype=torch.uint8))
    assert r["rc"] == 1 and _untouched(r) and b"envelope" in _C.lib().cosa_last_error()
    wide = torch.zeros(1, 128, 2, 2)
    r = _raw_v2(wide, wide)
    assert r["rc"] == 1 and _untouched(r) and b"128" in _C.lib().cosa_last_error()
    r = _raw_v3(wide, torch.zeros(1, 16, 16, dtype=torch.uint8))
    assert r["rc"] == 1 and _untouched(r)
    r = _raw_v3(cam, lab[:, :28, :28])                       # 4 -> 28: factor 7
    assert r["rc"] == 1 and _untouched(r) and b"factor" in _C.lib().cosa_last_error()
    r = _raw_v3(cam, lab[:, :33, :33])
    assert r["rc"] == 1 and _untouched(r)
    # the label kernel: a non-finite threshold or temperature, a zero temperature, more than 128 classes, a bad mode, a null scale
    scales, cls = R.label_case()
    scales, cls = [torch.from_numpy(s) for s in scales], torch.from_numpy(cls)
    ow, o = _guarded(2 * 64 * 64, torch.uint8, 0x5A)
    for T, thre, after, K in ((0.01, float("nan"), 0, None), (0.01, float("inf"), 0, None), (float("inf"), 0.25, 0, None), (float("nan"), 0.25, 1, None),
                              (0.0, 0.25, 0, None), (0.01, 0.25, 2, None), (0.01, 0.25, 0, 129)):
        rc, _, _ = _raw_label(scales, cls, 64, T, thre, after, out=o, K=K)
        assert rc == 1 and bool((ow == 0x5A).all()), (T, thre, after, K)
    L = _C.lib()
    assert L.cosa_cam_label(None, None, None, 3, _C.ptr(cls.cuda()), _C.ptr(o), 2, 6, 64, 0.01, 0.25, 0, _C.stream_ptr()) == 1
    torch.cuda.synchronize()
    assert bool((ow == 0x5A).all())


# ---- the label kernel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,thre", R.LABEL_SETTINGS)
@pytest.mark.parametrize("after", [0, 1])
def test_label_kernel_vs_float64(T, thre, after):
    scales, cls = R.label_case()
    lab64, excus = R.label_from_scales([t64(s) for s in scales], t64(cls), R.LABEL_S, T, thre, bool(after))
    ts, tc = [torch.from_numpy(s) for s in scales], torch.from_numpy(cls)
    rc, got, ow = _raw_label(ts, tc, R.LABEL_S, T, thre, after)
    assert rc == 0 and _intact(ow, got.numel(), 0x5A)
    diff = got.cpu().long() != lab64
    print(f"label T={T} thre={thre} after={after}: {int(diff.sum())} of {diff.numel()} pixels differ, {int(excus.sum())} excusable, "
          f"ignore share {float((got == 255).float().mean()):.3f}")
    assert not bool((diff & ~excus).any())
    assert float(excus.float().mean()) <= R.LABEL_EXCUSED_MAX
    rc2, got2, _ = _raw_label(ts, tc, R.LABEL_S, T, thre, after)
    assert rc2 == 0 and torch.equal(got, got2)
    # the host-side form the trainer calls
    from cosa_amd.utils import seg_helper as sh
    assert torch.equal(sh.cam_label_from_scales([t.cuda() for t in ts], tc.cuda(), R.LABEL_S, T, thre, bool(after)), got)


# ---- the public functions through autograd -----------------------------------------------------------------------------------
def test_public_functions_take_the_kernels_and_match_the_golden(golden, monkeypatch):
    from cosa_amd.utils import seg_helper as sh
    g = golden("camloss")
    seg = torch.from_numpy(g["seg_ps"]).cuda()
    for name in ("_cam_lossv2_torch", "_cam_lossv3_torch", "_cam_minmax_norm"):
        monkeypatch.setattr(sh, name, lambda *a, **k: (_ for _ in ()).throw(AssertionError("the torch composition was taken")))
    for tag, fn in (("v2", lambda x: sh.cam_lossv2(x, seg)), ("v3_25", lambda x: sh.cam_lossv3_wrap(x, seg, 0.25)),
                    ("v3_50", lambda x: sh.cam_lossv3_wrap(x, seg, seg_confident_thre=0.5))):
        head, _, thre = tag.partition("_")
        lw, gw = g[head + "_loss" + ("_" + thre if thre else "")], g[head + "_grad" + ("_" + thre if thre else "")]
        x = torch.from_numpy(g["cam"]).cuda().requires_grad_(True)
        loss = fn(x)
        (3.0 * loss).backward()                                                     # the upstream gradient scales the stored one
        le, ge = abs(loss.item() - lw) / abs(lw), np.abs(x.grad.cpu().numpy() / 3.0 - gw).max() / np.abs(gw).max()
        print(f"{tag} against the reference's float64: loss rel err {le:.2e}, grad err {ge:.2e} of max")
        assert le <= 1e-4 and ge <= 2e-3, tag
    with pytest.raises(AssertionError, match="torch composition"):                  # detach=True is the composition's
        sh.cam_lossv2(torch.from_numpy(g["cam"]).cuda(), seg, detach=True)


# ---- trainer level -----------------------------------------------------------------------------------------------------------
CONFIGS = {"v2": dict(camloss_version="v2"),
           "v3": dict(camloss_version="v3"),
           "v2_aux": dict(camloss_version="v2", aux_seg2cam=True),
           "v3_aux_all": dict(camloss_version="v3", aux_seg2cam=True, segconf_thre=0.5, seg_softmaxtemp=1.0, after_softmax=True)}
LOSSES = ("cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")
# An untrained teacher's seg logits are ~0.03: at T = 1 the softmax over all 21 classes is flat, nothing passes segconf_thre = 0.5, every
# pixel is ignored and the fourth configuration would compare zeros.  Its trainers (fused and torch alike) therefore get the teacher's last
# decoder layer multiplied by 256 before the first step: measured on the committed batch, 1 % of the pixels then carry a foreground label
# (with --after_softmax the present classes win only where they beat all 21).  The configuration itself is the issue's.
TEACHER_SEG_GAIN = {"v3_aux_all": 256.0}


def _trainer_of(name, **over):
    tr = _trainer(**over, **CONFIGS[name])
    gain = TEACHER_SEG_GAIN.get(name)
    if gain:
        with torch.no_grad():
            tr.model_AN.decoder.conv8.weight.mul_(gain)
        if tr._teacher_shadows is not None:
            tr._teacher_shadows.refresh(force=True)
    return tr


class _NoTorchLosses(_FlagBar):
    """tests/test_loss_flags_gpu.py's bar plus the torch compositions of cam_lossv2 / cam_lossv3 and the torch label map"""
    NAMES = _FlagBar.NAMES + ("_cam_lossv2_torch", "_cam_lossv3_torch", "_cam_label_torch", "_cam_minmax_norm")


def _run(tr, steps=2):
    """`steps` steps past warm-up -> (the five losses of the first step, d loss / d cam_pred and d loss / d cam_aux_pred of the first step
    (None without the blend), the first step's v3 label map or None)"""
    grads = {}

    def hook(_mod, _inp, out):
        if not grads:
            grads["pending"] = True
            for key, i in (("cam", 4), ("aux", 5)):
                if out[i].requires_grad:
                    out[i].register_hook(lambda g_, key=key: grads.__setitem__(key, g_.detach().float().cpu()))
    h = tr.student.register_forward_hook(hook)
    try:
        first = label = None
        for k in range(steps):
            logs = tr.step(*_batch(tr, k), n_iter=tr.args.warmup_iters + 1 + k)
            if first is None:
                first = {n: float(logs[n]) for n in LOSSES}
                label = getattr(tr, "cam_label_last", None)
                label = None if label is None else label.clone().cpu().long()
    finally:
        h.remove()
    torch.cuda.synchronize()
    assert all(math.isfinite(v) for v in first.values()), first
    return first, grads, label


@functools.lru_cache(maxsize=None)
def _fused_run(name):
    """a fused trainer of configuration `name`, two steps with the torch path barred and the fused calls counted"""
    from cosa_amd.utils import seg_helper as sh
    tr = _trainer_of(name)
    assert tr.fused_losses and tr.use_graph and tr.camloss_version == CONFIGS[name]["camloss_version"]
    calls = []
    saved = {n: getattr(sh, n) for n in ("cam_lossv2_from_targets", "cam_lossv3", "cam_loss_from_targets")}

    def counted(n):
        def f(*a, **k):
            calls.append(n)
            return saved[n](*a, **k)
        return f
    try:
        for n in ("cam_lossv2_from_targets", "cam_lossv3", "cam_loss_from_targets"):
            setattr(sh, n, counted(n))
        with _NoTorchLosses():
            first, grads, label = _run(tr)
    finally:
        for n, f in saved.items():
            setattr(sh, n, f)
    return first, grads, label, _state(tr), calls


@pytest.mark.parametrize("name", list(CONFIGS))
def test_selected_version_runs_on_the_fused_path(name):
    first, grads, label, _, calls = _fused_run(name)
    cfg = CONFIGS[name]
    per_step = 2 if cfg.get("aux_seg2cam") else 1
    assert calls == [{"v2": "cam_lossv2_from_targets", "v3": "cam_lossv3"}[cfg["camloss_version"]]] * (2 * per_step), calls
    assert first["cam_loss"] > 0 and float(grads["cam"].abs().max()) > 0
    assert ("aux" in grads and float(grads["aux"].abs().max()) > 0) == bool(cfg.get("aux_seg2cam"))
    assert (label is not None) == (cfg["camloss_version"] == "v3")


@pytest.mark.parametrize("version", ["v2", "v3"])
def test_the_bar_on_the_torch_path_bites(version):
    tr = _trainer(fused_losses=False, camloss_version=version)
    with _NoTorchLosses():
        with pytest.raises(AssertionError, match="the torch path was taken"):
            tr.step(*_batch(tr, 0), n_iter=tr.args.warmup_iters + 1)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fused_against_torch_path(name):
    """identical weights and batch: the same v3 label map first, then the five losses within 1e-4 relative and d loss / d cam_pred (and
    d cam_aux_pred with the blend) within 2e-3 of their maxima"""
    first, grads, label, _, _ = _fused_run(name)
    tr = _trainer_of(name, fused_losses=False)
    assert not tr.fused_losses
    ref, g_ref, label_ref = _run(tr, steps=1)
    if label is not None:
        n_diff = int((label != label_ref).sum())
        print(name, "label maps differ at", n_diff, "of", label.numel(), "pixels; ignore share", float((label == 255).float().mean()))
        assert n_diff == 0
    print(name, {k: (first[k], ref[k]) for k in LOSSES})
    for k in LOSSES:
        assert first[k] == pytest.approx(ref[k], rel=1e-4), (k, first[k], ref[k])
    assert grads.keys() == g_ref.keys()
    for key in ("cam", "aux"):
        if key in g_ref:
            err, top = (grads[key] - g_ref[key]).abs().max().item(), g_ref[key].abs().max().item()
            print(name, key, "grad err", err, "of max", top)
            assert top > 0 and err <= 2e-3 * top, (key, err, top)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fused_trainers_of_one_seed_end_in_the_same_bits(name):
    _, grads, label, state, _ = _fused_run(name)
    tr = _trainer_of(name)
    _, g2, label2 = _run(tr)
    assert torch.equal(_bits(grads["cam"]), _bits(g2["cam"]))
    assert label is None or torch.equal(label, label2)
    _assert_same_state(state, _state(tr))


def test_v1_is_the_trainer_without_the_field():
    from cosa_amd.train_step import CoSATrainer, default_args
    a = _trainer(camloss_version="v1")
    la, ga, _ = _run(a)
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3)
    del args.camloss_version, args.segconf_thre
    b = CoSATrainer(args, torch.device("cuda", 0), seed=3)
    lb, gb, _ = _run(b)
    assert la == lb and torch.equal(_bits(ga["cam"]), _bits(gb["cam"]))
    _assert_same_state(_state(a), _state(b))
    assert not hasattr(a, "cam_label_last")


def test_student_check_under_v3_reports_a_finite_cam_loss():
    tr = _trainer(camloss_version="v3", student_check_iters=1)
    tr.step(*_batch(tr, 0), n_iter=tr.args.warmup_iters + 1)
    torch.cuda.synchronize()
    last = tr.student_check_last
    assert last is not None and torch.isfinite(last["loss_b"]).all() and float(last["loss_b"][3]) > 0
    print("student check under v3: cam loss", float(last["loss_a"][3]), "(training forward)", float(last["loss_b"][3]), "(fp32 pass)")
    assert tr.student_check() is not None
