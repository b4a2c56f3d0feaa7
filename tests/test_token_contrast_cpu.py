"""CPU suite of the supervised-contrastive token loss: the float64 restatement against central differences, the label
rule, the torch composition against the restatement, the flag table and every refusal."""
import types

import numpy as np
import pytest
import torch

import token_contrast_ref as R


def _draw(seed, B=2, n=7, D=5, classes=3, labelled=0.7):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, n, D))
    y = rng.integers(0, classes, (B, n))
    y[rng.random((B, n)) > labelled] = R.IGNORE
    return x, y


def test_restated_gradient_equals_central_differences():
    for seed, tau in ((0, 0.5), (1, 0.07), (2, 2.0)):
        x, y = _draw(seed)
        y[0, :3] = 1                                   # at least one class with several tokens
        L, M, g = R.loss_and_grad(x, y, tau)
        assert M >= 3 and L > 0
        h = 1e-6
        num = np.zeros_like(x)
        for idx in np.ndindex(*x.shape):
            xp, xm = x.copy(), x.copy()
            xp[idx] += h
            xm[idx] -= h
            num[idx] = (R.loss_only(xp, y, tau) - R.loss_only(xm, y, tau)) / (2 * h)
        assert np.abs(num - g).max() <= 1e-8 * max(1.0, np.abs(g).max()), (seed, np.abs(num - g).max())


def test_restatement_special_cases():
    x, _ = _draw(3, B=2, n=6)
    none = np.full((2, 6), R.IGNORE)
    L, M, g = R.loss_and_grad(x, none, 0.5)
    assert L == 0.0 and M == 0 and not g.any()
    singles = np.array([[0, 1, 2, 255, 255, 255]] * 2)          # every class once: no anchor
    assert R.loss_and_grad(x, singles, 0.5)[:2] == (0.0, 0)
    y = np.array([[0, 0, 1, 255, 255, 255], [255] * 6])         # class 1 single: no anchor, still a negative of the two anchors
    L, M, g = R.loss_and_grad(x, y, 0.5)
    assert M == 2 and np.abs(g[0, 2]).max() > 0 and not g[1].any() and not g[0, 3:].any()


def test_label_rule():
    from cosa_amd.utils import seg_helper
    p, g = 4, 3
    mask = np.full((2, p * g, p * g), 7, dtype=np.int64)
    cell = lambda b, r, c: mask[b, r * p:(r + 1) * p, c * p:(c + 1) * p]
    cell(0, 0, 0)[:] = 3                                        # unanimous
    cell(0, 0, 1)[:] = 3
    cell(0, 0, 1)[0, 0] = 0                                     # one pixel short of need at purity 1
    cell(0, 0, 2)[:] = 255                                      # 255 only
    cell(0, 1, 0)[:] = 0                                        # background is a class like any other
    cell(0, 1, 1)[:] = 2
    cell(0, 1, 1)[0, :] = 255                                   # 12 of 16: purity 0.75 takes it ...
    cell(0, 1, 2)[:] = 2
    cell(0, 1, 2)[0, :] = 5
    cell(0, 1, 2)[1, 0] = 255                                   # ... 11 of 16: one short of it
    cell(0, 2, 0)[:3, :] = 255                                  # 255 holds 12 of 16: never a label
    want1 = np.full((2, 9), 7, dtype=np.uint8)
    want1[0, :6] = [3, 255, 255, 0, 255, 255]
    want1[0, 6] = 255
    want75 = want1.copy()
    want75[0, 1], want75[0, 4] = 3, 2
    assert R.need_of(p, 1.0) == 16 and R.need_of(p, 0.75) == 12 and seg_helper.token_need(p, 0.75) == 12 and seg_helper.token_need(16, 1.0) == 256
    for purity, want in ((1.0, want1), (0.75, want75)):
        assert np.array_equal(R.token_labels(mask, p, purity), want), purity
        got = seg_helper.token_labels(torch.from_numpy(mask), p, purity)
        assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), purity
    for bad in (0.5, 1.01, 0.0):
        with pytest.raises(ValueError):
            seg_helper.token_labels(torch.from_numpy(mask), p, bad)
    with pytest.raises(ValueError):
        seg_helper.token_labels(torch.from_numpy(mask), 5)


@pytest.mark.parametrize("seed,tau", [(10, 0.5), (11, 0.1), (12, 3.0)])
def test_torch_composition_equals_the_restatement_in_float64(seed, tau):
    from cosa_amd.utils import seg_helper
    x, y = _draw(seed, B=3, n=11, D=8, classes=4)
    y[1] = R.IGNORE                                             # an image that is all 255
    y[2] = 2                                                    # an image of a single class
    x[0, 4] = 0.0                                               # an all-zero token row
    L, M, g = R.loss_and_grad(x, y, tau)
    xt = torch.from_numpy(x).requires_grad_(True)
    loss, m = seg_helper.token_contrast_loss(xt, torch.from_numpy(y), tau, return_count=True)
    assert loss.dtype == torch.float64 and int(m) == M
    loss.backward()
    assert abs(float(loss.detach()) - L) <= 1e-12 * max(1.0, abs(L))
    assert np.abs(xt.grad.numpy() - g).max() <= 1e-12 * max(1.0, np.abs(g).max())
    # M = 0: an exact zero, a zero gradient, no NaN
    xt = torch.from_numpy(x).requires_grad_(True)
    loss = seg_helper._token_contrast_torch(xt, torch.full((3, 11), 255), tau)
    loss.backward()
    assert float(loss) == 0.0 and not xt.grad.numpy().any()


def test_flag_table_and_launcher_refusals():
    from cosa_amd import args as cosa_args, main as launcher
    a, changed = cosa_args.parse(["exp"])
    assert (a.tokcon_weight, a.tokcon_temp, a.tokcon_purity) == (0.0, 0.5, 1.0) and not changed
    assert all(f in [n for n, _t, _d in cosa_args.EXTRA] and f not in [n for n, _t, _d in cosa_args.FLAGS]
               for f in ("tokcon_weight", "tokcon_temp", "tokcon_purity"))
    launcher.check_supported(a)
    b, changed = cosa_args.parse(["exp", "--tokcon_weight", "0.1", "--tokcon_temp", "0.2", "--tokcon_purity", "0.75"])
    assert (b.tokcon_weight, b.tokcon_temp, b.tokcon_purity) == (0.1, 0.2, 0.75) and set(changed) == {"tokcon_weight", "tokcon_temp", "tokcon_purity"}
    launcher.check_supported(b)
    t = launcher._trainer_args(b)
    assert (t.tokcon_weight, t.tokcon_temp, t.tokcon_purity) == (0.1, 0.2, 0.75)
    for extra, word in ((["--tokcon_weight", "-0.1"], "--tokcon_weight"), (["--tokcon_weight", "0.1", "--tokcon_temp", "0.001"], "--tokcon_temp"),
                        (["--tokcon_temp", "11"], "--tokcon_temp"), (["--tokcon_purity", "0.5"], "--tokcon_purity"),
                        (["--tokcon_purity", "1.5"], "--tokcon_purity"), (["--tokcon_weight", "0.1", "--grad_check_iters", "5"], "--grad_check_iters")):
        bad, _ = cosa_args.parse(["exp"] + extra)
        with pytest.raises(ValueError, match=word):
            launcher.check_supported(bad)
    ok, _ = cosa_args.parse(["exp", "--grad_check_iters", "5"])           # the check alone stays allowed
    launcher.check_supported(ok)


def test_trainer_refusals():
    from cosa_amd.train_step import CoSATrainer, default_args
    d = default_args("VOC12")
    assert (d.tokcon_weight, d.tokcon_temp, d.tokcon_purity) == (0.0, 0.5, 1.0)
    dev = torch.device("cpu")
    for over, word in ((dict(tokcon_weight=-1.0), "tokcon_weight"), (dict(tokcon_weight=0.1, tokcon_temp=20.0), "tokcon_temp"),
                       (dict(tokcon_weight=0.1, tokcon_purity=0.4), "tokcon_purity"), (dict(tokcon_weight=float("nan")), "tokcon_weight"),
                       (dict(tokcon_weight=0.1, grad_check_iters=3), "grad_check_iters")):
        with pytest.raises(ValueError, match=word):          # (before anything is built)
            CoSATrainer(default_args("VOC12", crop_size=64, **over), dev)
    stub = types.SimpleNamespace(_tokcon=(0.1, 0.5, 1.0), fused_losses=False,
                                 student=types.SimpleNamespace(encoder=types.SimpleNamespace(residual_stream="bf16")))
    with pytest.raises(ValueError, match="residual_stream"):
        CoSATrainer._token_contrast(stub, torch.zeros(1, 8, 2, 2), torch.zeros(1, 8, 8, dtype=torch.long))
    stub.student.encoder.residual_stream = "fp32"              # the same call on the torch path: a labelled 2 x 2 map of one class
    feat = torch.randn(1, 8, 2, 2, dtype=torch.float64)
    got = CoSATrainer._token_contrast(stub, feat, torch.ones(1, 8, 8, dtype=torch.long))
    want = R.loss_only(feat.permute(0, 2, 3, 1).reshape(1, 4, 8).numpy(), np.ones((1, 4)), 0.5)
    assert abs(float(got) - want) <= 1e-12


def test_launcher_interval_keys_line_and_resume_refusal(tmp_path, monkeypatch):
    from cosa_amd import main as launcher
    from test_label_stats_cpu import _host_trainer
    assert launcher.interval_keys(False) == ('overall_loss', 'cls_loss', 'cls_acc', 'cls_aux_loss', 'cls_aux_acc', 'seg_loss', 'cam_loss', 'reg_loss')
    assert launcher.interval_keys(True) == launcher.interval_keys(False) + ('tok_loss',)
    vals = [1.0, 2.0, 0.5, 3.0, 0.25, 4.0, 5.0, 6.0, 7.0]
    off = launcher.interval_line("H\n", vals[:8], False)
    assert off == ("H\n overall_loss: 1.0000, cls_loss: 2.0000, cls_acc: 0.500,  cls_aux_loss: 3.0000, cls_aux_acc: 0.250, seg_loss: 4.0000, "
                   "cam_loss: 5.0000, reg_loss: 6.0000 ...")
    assert launcher.interval_line("H\n", vals, True) == off[:-4] + ", tok_loss: 7.0000 ..."
    logs = {k: torch.tensor(float(i)) for i, k in enumerate(("overall_loss", "cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss", "tok_loss"))}
    t8, t9 = (launcher.interval_terms(logs, torch.tensor(0.5), torch.tensor(0.25), on) for on in (False, True))
    assert t8.dtype == torch.float64 and t8.tolist() == [0.0, 1.0, 0.5, 2.0, 0.25, 3.0, 4.0, 5.0] and t9.tolist() == t8.tolist() + [6.0]
    # a state file written under the other setting: the refusal names the flag
    for on_file in (False, True):
        a = _host_trainer(monkeypatch, seed=1)
        a._add_extra_state("launcher.acc", torch.zeros(9 if on_file else 8, dtype=torch.float64))
        path = str(tmp_path / f"state_0000000{int(on_file)}.cosa")
        a.save_state(path, n_iter=0)
        a.wait_state()
        same = _host_trainer(monkeypatch, seed=2)
        same._add_extra_state("launcher.acc", torch.zeros(9 if on_file else 8, dtype=torch.float64))
        assert launcher.load_state_checked(same, path, on_file)["n_iter"] == 0
        other = _host_trainer(monkeypatch, seed=2)
        other._add_extra_state("launcher.acc", torch.zeros(8 if on_file else 9, dtype=torch.float64))
        with pytest.raises(ValueError, match="--tokcon_weight"):
            launcher.load_state_checked(other, path, not on_file)
