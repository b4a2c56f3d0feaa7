"""GPU suite of the supervised-contrastive token loss: the kernels of csrc/tokcon_kernels.hip against the float64
restatement (tests/token_contrast_ref.py) evaluated on the same bf16-rounded inputs, the four-way junction, and the trainer with the term
off and on.

Tolerances.  Nothing is fixed in advance: per shape, e32 is the largest error of the fp32 torch composition (seg_helper._token_contrast_torch
on the host, fp32 copies of the same bf16 tokens) against float64 over this file's seeds of that shape -- once for the loss, once for the
gradient elements.  The kernels follow the same fp32 arithmetic in another summation order, so the bars are
    loss:      |L - ref| <= 4 e32(loss)
    gradient:  |d - ref| <= 2^-8 |ref| + 4 e32(gradient)          (the first term: the one bf16 rounding)
The planted all-zero token row has a gradient of the order 1 / 1e-12; its e32 is taken over that row alone and the other rows' e32 without
it, so neither bar is widened by the other (both are at most the e32 over all rows)."""
import functools
import os

import numpy as np
import pytest
import torch

import token_contrast_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(16, 64, 2), (16, 80, 3), (8, 72, 2), (16, 224, 2)]          # (p, S, B): n = 16, 25, 81, 196
SEEDS = (0, 1, 2)
TAU = 0.5
D = 768
SINGLE = 9          # the class planted with a single token


def _case(p, S, B, seed):
    """-> (tokens bf16 [B,n,768] on the host, label map int64 [B,S,S], token labels as planted uint8 [B,n], the zero row's index).
    Image 0: >= half of the tokens labelled over 3 or 4 classes, one more class with a single token, one all-zero token row.  The last image:
    all 255 (seed 0), a single class (seed 1), drawn like image 0 (seed 2); images in between are drawn."""
    rng = np.random.default_rng(1000 * S + 10 * p + seed)
    g = S // p
    n = g * g
    classes = [0, 1, 2, 5][:3 + seed % 2]
    y = np.full((B, n), R.IGNORE, dtype=np.int64)
    for b in range(B):
        lab = rng.permutation(n)[:max((n + 1) // 2 + 1, int(0.6 * n))]
        y[b, lab] = rng.choice(classes, size=lab.size)
        for c in classes[:2]:                                   # (two tokens of a class at least: anchors exist at n = 16 too)
            y[b, lab[2 * c:2 * c + 2]] = c
        y[b, lab[-1]] = SINGLE
    if seed == 0:
        y[B - 1] = R.IGNORE
    elif seed == 1:
        y[B - 1] = 2
    mask = np.empty((B, S, S), dtype=np.int64)
    for b in range(B):
        for t in range(n):
            r, c = divmod(t, g)
            cell = mask[b, r * p:(r + 1) * p, c * p:(c + 1) * p]
            if y[b, t] != R.IGNORE:
                cell[:] = y[b, t]
            elif rng.random() < 0.5:
                cell[:] = R.IGNORE
            else:                                               # one pixel of another class: short of the unanimous cell purity 1 asks for
                cell[:] = 1
                cell[rng.integers(p), rng.integers(p)] = 3
    x = torch.from_numpy(rng.standard_normal((B, n, D)).astype(np.float32)).to(torch.bfloat16)
    zero_row = int(np.flatnonzero(y[0] == 0)[0])
    x[0, zero_row] = 0
    return x, mask, y.astype(np.uint8), zero_row


@functools.lru_cache(maxsize=None)
def _reference(p, S, B, seed):
    """the case, its float64 loss / M / gradient, and the fp32 composition's errors against them (loss, gradient rows but the zero row,
    the zero row) -- computed once and shared"""
    from cosa_amd.utils import seg_helper
    x, mask, y, zr = _case(p, S, B, seed)
    assert np.array_equal(R.token_labels(mask, p), y)
    L, M, g = R.loss_and_grad(x.float().numpy(), y, TAU)
    x32 = x.float().requires_grad_(True)
    l32 = seg_helper._token_contrast_torch(x32, torch.from_numpy(y), TAU)
    l32.backward()
    err = np.abs(x32.grad.double().numpy() - g)
    rest = np.ones(err.shape[:2], dtype=bool)
    rest[0, zr] = False
    return dict(x=x, mask=mask, y=y, zero_row=zr, L=L, M=M, g=g, e_loss=abs(float(l32.detach()) - L), e_rest=float(err[rest].max()),
                e_zero=float(err[0, zr].max()))


@functools.lru_cache(maxsize=None)
def _e32(p, S, B):
    refs = [_reference(p, S, B, s) for s in SEEDS]
    return max(r["e_loss"] for r in refs), max(r["e_rest"] for r in refs), max(r["e_zero"] for r in refs)


def _run(x, labels):
    from cosa_amd.utils import seg_helper
    xd = x.cuda().requires_grad_(True)
    loss, m = seg_helper.token_contrast_loss(xd, labels, TAU, return_count=True)
    loss.backward()
    return loss.detach(), m, xd.grad


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p,S,B", SHAPES)
def test_kernels_against_the_float64_restatement(p, S, B, seed):
    from cosa_amd.utils import seg_helper
    ref = _reference(p, S, B, seed)
    e_loss, e_rest, e_zero = _e32(p, S, B)
    labels = seg_helper.token_labels(torch.from_numpy(ref["mask"]).cuda(), p)
    assert labels.dtype == torch.uint8 and np.array_equal(labels.cpu().numpy(), ref["y"])
    assert torch.equal(seg_helper.token_labels(torch.from_numpy(ref["mask"]).to(torch.uint8).cuda(), p), labels)
    loss, m, grad = _run(ref["x"], labels)
    assert grad.dtype == torch.bfloat16 and loss.dtype == torch.float32
    d = grad.double().cpu().numpy()
    err = np.abs(d - ref["g"])
    zr = ref["zero_row"]
    rest = np.ones(err.shape[:2], dtype=bool)
    rest[0, zr] = False
    print(f"n={(S // p) ** 2} B={B} seed={seed}: M={int(m)} loss err {abs(float(loss) - ref['L']):.3e} (e32 {e_loss:.3e}), "
          f"grad err {err[rest].max():.3e} (e32 {e_rest:.3e}, max |ref| {np.abs(ref['g'][rest]).max():.3e}), "
          f"zero row err {err[0, zr].max():.3e} (e32 {e_zero:.3e}, max |ref| {np.abs(ref['g'][0, zr]).max():.3e})")
    assert int(m) == ref["M"] and ref["M"] > 0
    assert np.isfinite(d).all() and abs(float(loss) - ref["L"]) <= 4 * e_loss
    bar = 2.0 ** -8 * np.abs(ref["g"]) + 4 * e_rest
    bar[0, zr] = 2.0 ** -8 * np.abs(ref["g"][0, zr]) + 4 * e_zero
    assert (err <= bar).all(), float((err - bar).max())
    assert np.abs(ref["g"][0, zr]).max() > 1e6                  # the zero row's gradient is the one over the clamped norm
    if seed == 0:
        assert not d[B - 1].any()                               # the all-255 image: an exact zero
    single = np.argwhere(ref["y"] == SINGLE)
    assert len(single) and all(np.abs(d[b, t]).max() > 0 for b, t in single)          # not an anchor, still a negative
    # the same bytes on every run
    loss2, m2, grad2 = _run(ref["x"], labels)
    assert torch.equal(loss.view(torch.int32), loss2.view(torch.int32)) and torch.equal(grad.view(torch.int16), grad2.view(torch.int16)) and int(m2) == int(m)


@pytest.mark.parametrize("p,S,B", SHAPES[:2] + SHAPES[3:])
def test_a_batch_without_anchors_gives_exact_zeros(p, S, B):
    ref = _reference(p, S, B, 2)
    n = ref["y"].shape[1]
    for y in (np.full((B, n), R.IGNORE, dtype=np.uint8), np.tile((np.arange(n) % 255).astype(np.uint8), (B, 1))):      # none labelled; every class once
        if n > 255:
            y[:, 255:] = R.IGNORE
        assert R.loss_and_grad(ref["x"].float().numpy(), y, TAU, want_grad=False)[1] == 0
        loss, m, grad = _run(ref["x"], torch.from_numpy(y).cuda())
        assert int(m) == 0 and float(loss) == 0.0 and not bool(grad.float().abs().sum() != 0) and bool(torch.isfinite(grad.float()).all())


def test_upstream_scalar_and_purity_reach_the_kernels():
    from cosa_amd.utils import seg_helper
    p, S, B = SHAPES[0]
    ref = _reference(p, S, B, 2)
    labels = torch.from_numpy(ref["y"]).cuda()
    _, _, g1 = _run(ref["x"], labels)
    xd = ref["x"].cuda().requires_grad_(True)
    (seg_helper.token_contrast_loss(xd, labels, TAU) * 0.25).backward()          # a power of two: the same bits, scaled
    assert torch.equal(xd.grad.float(), g1.float() * 0.25)
    mask = torch.from_numpy(ref["mask"]).cuda()
    for purity in (0.75, 0.999):
        assert np.array_equal(seg_helper.token_labels(mask, p, purity).cpu().numpy(), R.token_labels(ref["mask"], p, purity)), purity
    assert (R.token_labels(ref["mask"], p, 0.75) != ref["y"]).any()              # (the cells one pixel short are labelled at 0.75)


def test_four_way_junction_against_the_fp32_sum_in_consumer_order():
    from cosa_amd import _C
    B, N = 3, 26
    gen = torch.Generator().manual_seed(5)
    gs = [(torch.randn(B, N - 1, D, generator=gen) * 10.0 ** k).to(torch.bfloat16).cuda() for k in (0, -2, 1, -1)]
    for live in ((0, 1, 2, 3), (0, 2, 3), (3,)):
        ptrs = [_C.ptr(gs[k]) if k in live else _C.ptr(None) for k in range(4)]
        dx = torch.full((B, N, D), float("nan"), device="cuda")
        _C.check(_C.lib().cosa_token_junction_bwd4(*ptrs, _C.ptr(dx), B, N, D, _C.stream_ptr()), "cosa_token_junction_bwd4")
        want = gs[live[0]].float()
        for k in live[1:]:
            want = want + gs[k].float()
        assert not dx[:, 0].any() and torch.equal(dx[:, 1:], want), live


def test_fanout_of_four_keeps_the_three_way_bytes_and_adds_the_fourth():
    from cosa_amd import nn_ops
    B, N = 2, 17
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(B, N, D, generator=gen).cuda()
    ws = [torch.randn(B, N - 1, D, generator=gen).to(torch.bfloat16).cuda() for _ in range(4)]

    def grad(n_views, n_live):
        xr = x.clone().requires_grad_(True)
        views = nn_ops.patch_fanout_bf16(xr, n_views)
        sum((v * w).sum() for v, w in zip(views[:n_live], ws)).backward()
        return xr.grad

    assert torch.equal(grad(4, 3), grad(3, 3))
    want = torch.zeros_like(x)
    want[:, 1:] = ((ws[0].float() + ws[1].float()) + ws[2].float()) + ws[3].float()
    assert torch.equal(grad(4, 4), want)


# ---- the trainer at S = 64, b = 2 ------------------------------------------------------------------------------------------------------------
LOSSES = ("overall_loss", "cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")


PURITY = 0.51       # the trainer tests: at 64 x 64 a crop has 16 tokens, and unanimous cells alone leave some steps without an anchor


def _trainer(seed=3, drop=False, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    if over.get("tokcon_weight", 0.0) > 0:
        over.setdefault("tokcon_purity", PURITY)
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, **over)
    if drop:                                                    # a trainer built without the arguments
        for k in ("tokcon_weight", "tokcon_temp", "tokcon_purity"):
            delattr(args, k)
    return CoSATrainer(args, torch.device("cuda", 0), seed=seed)


def _steps(tr, first, last, names=LOSSES, after=None):
    from cosa_amd.train_step import synthetic_batch
    store = torch.zeros((last - first + 1, len(names)), dtype=torch.float32, device=tr.device)
    for k in range(first, last + 1):
        logs = tr.step(*synthetic_batch(2, 64, 20, tr.device, seed=900 + k), n_iter=tr.args.warmup_iters + k)      # past the warm-up
        assert ("tok_loss" in logs) == ("tok_loss" in names)
        for j, nm in enumerate(names):
            store[k - first, j] = logs[nm].float()
        if after is not None:
            after(k)
    torch.cuda.synchronize()
    return store


@functools.lru_cache(maxsize=None)
def _run_off():
    tr = _trainer(drop=True)
    losses = _steps(tr, 1, 2)
    return losses, tr.train_state().checksums(), tr.student.encoder.norm.weight.detach().clone()


@functools.lru_cache(maxsize=None)
def _run_on():
    """four uninterrupted steps with the term on -> (losses, checksums after step 2, checksums after step 4, the final norm's weight after step 2)"""
    tr = _trainer(tokcon_weight=0.1)
    mid = {}

    def after(k):
        if k == 2:
            mid["sums"], mid["norm"] = tr.train_state().checksums(), tr.student.encoder.norm.weight.detach().clone()
    losses = _steps(tr, 1, 4, LOSSES + ("tok_loss",), after)
    return losses, mid["sums"], tr.train_state().checksums(), mid["norm"]


def test_trainer_with_weight_zero_is_the_trainer_without_the_argument():
    losses_a, sums_a, _ = _run_off()
    tr = _trainer(tokcon_weight=0.0)
    losses_b = _steps(tr, 1, 2)
    assert torch.equal(losses_a.view(torch.int32), losses_b.view(torch.int32)) and tr.train_state().checksums() == sums_a
    assert len(tr._loss_weights[False]) == 5


def test_trainer_with_the_term_on_and_its_resume(tmp_path):
    _, _, norm_off = _run_off()
    losses_a, mid_a, end_a, norm_on = _run_on()
    tok = losses_a[:, -1]
    assert bool(torch.isfinite(losses_a).all()) and bool((tok > 0).all())
    assert not torch.equal(norm_on, norm_off)                   # the encoder's gradients differ from the off run's: so do its weights
    # a second run: the same bytes; saved at step 2 of 4 and resumed in a third: the bytes of the uninterrupted run
    b = _trainer(tokcon_weight=0.1)
    assert len(b._loss_weights) == 0
    losses_b = _steps(b, 1, 2, LOSSES + ("tok_loss",))
    assert torch.equal(losses_b.view(torch.int32), losses_a[:2].view(torch.int32)) and b.train_state().checksums() == mid_a
    assert b._loss_weights[False].tolist()[5] == pytest.approx(0.1) and len(b._loss_weights[False]) == 6
    path = str(tmp_path / "state_00000002.cosa")
    b.save_state(path, n_iter=1)
    b.wait_state()
    del b
    c = _trainer(seed=77, tokcon_weight=0.1)
    try:
        assert c.load_state(path)["n_iter"] == 1
    finally:
        os.remove(path)
    losses_c = _steps(c, 3, 4, LOSSES + ("tok_loss",))
    assert torch.equal(losses_c.view(torch.int32), losses_a[2:].view(torch.int32)) and c.train_state().checksums() == end_a


def test_warm_up_weighs_the_term_zero():
    from cosa_amd.train_step import synthetic_batch
    tr = _trainer(tokcon_weight=0.1)
    logs = tr.step(*synthetic_batch(2, 64, 20, tr.device, seed=901), n_iter=1)
    assert tr._loss_weights[True].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0, 0.0] and bool(torch.isfinite(logs["tok_loss"]))
    assert float(logs["overall_loss"]) == pytest.approx(float(logs["cls_loss"]) + float(logs["cls_aux_loss"]), rel=1e-6)
