"""The soft-label seg loss on the host: seg_helper.seg_softloss / seg_softlossv2 in float64 against the golden vectors
the reference's own functions wrote (tests/golden/seg_soft.npz) and, where the reference tree is present, against the live functions; the
torch composition's sets, gate, ties and absent classes against the float64 restatement (tests/seg_soft_ref.py); flags, refusals, the
launcher's keys, line and state-file marker."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_soft_ref as R
from cosa_amd.utils import seg_helper as sh

ALPHAS = (("a05", 0.5), ("a03", 0.3))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("seg_soft")


def test_golden_inputs_populate_both_sets(gold):
    assert gold["pred"].shape == (2, 5, 32, 32) and gold["pred"].dtype == np.float64 and gold["probs"].dtype == np.float64
    lab = gold["probs"].argmax(1)
    assert int((lab == 0).sum()) == int(gold["n_bg"]) >= 900 and int((lab != 0).sum()) == int(gold["n_fg"]) >= 900
    assert np.allclose(gold["probs"].sum(1), 1.0, atol=1e-12)


@pytest.mark.parametrize("tag,alpha", ALPHAS)
def test_softloss_against_golden(gold, tag, alpha):
    """float64 on both sides; the (count + 1e-6) denominators move a mean over >= 900 pixels by 1e-6 / 900 ~ 1e-9 of itself, nothing else
    differs: rtol 1e-7 on the value and, per element relative to the largest, on the gradient"""
    want_l, want_g = float(gold["loss_" + tag]), gold["grad_" + tag]
    top = np.abs(want_g).max()
    p = torch.from_numpy(gold["pred"]).clone().requires_grad_(True)
    loss = sh.seg_softloss(p, torch.from_numpy(gold["probs"]), fg_alpha=alpha)
    loss.backward()
    l64, g64 = R.full_f64(gold["pred"], gold["probs"], alpha)
    for what, l, g in (("restatement", l64, g64), ("seg_softloss", float(loss.detach()), p.grad.numpy())):
        err_l, err_g = abs(l - want_l) / abs(want_l), np.abs(g - want_g).max() / top
        print(f"{what} fg_alpha {alpha}: loss {err_l:.3e} grad {err_g:.3e}")
        assert err_l <= 1e-7 and err_g <= 1e-7, (what, err_l, err_g)
    assert loss.dtype == torch.float64 and top > 0


def test_softlossv2_against_golden(gold):
    p = torch.from_numpy(gold["pred"]).clone().requires_grad_(True)
    loss = sh.seg_softlossv2(p, torch.from_numpy(gold["probs"]))
    loss.backward()
    err_l = abs(float(loss.detach()) - float(gold["loss_v2"])) / float(gold["loss_v2"])
    err_g = np.abs(p.grad.numpy() - gold["grad_v2"]).max() / np.abs(gold["grad_v2"]).max()
    print(f"seg_softlossv2: loss {err_l:.3e} grad {err_g:.3e}")
    assert err_l <= 1e-7 and err_g <= 1e-7
    # rows [N,K], as seg_softloss hands them over in the reference, and no row at all: 0 and a zero gradient where the reference gives NaN
    rows, qrows = (torch.from_numpy(gold[k]).permute(0, 2, 3, 1).reshape(-1, 5) for k in ("pred", "probs"))
    assert float(sh.seg_softlossv2(rows, qrows)) == pytest.approx(float(loss.detach()), rel=1e-12)
    e = rows[:0].clone().requires_grad_(True)
    z = sh.seg_softlossv2(e, qrows[:0])
    z.backward()
    assert float(z.detach()) == 0.0 and e.grad.shape == (0, 5)


def test_against_live_reference(gold):
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip("reference tree not present")
    ref = ref_loader.seg_helper()
    pred, probs = torch.from_numpy(gold["pred"]), torch.from_numpy(gold["probs"])
    for _tag, alpha in ALPHAS:
        pa, pb = (pred.clone().requires_grad_(True) for _ in range(2))
        la, lb = ref.seg_softloss(pa, probs, fg_alpha=alpha), sh.seg_softloss(pb, probs, fg_alpha=alpha)
        la.backward()
        lb.backward()
        assert float(lb.detach()) == pytest.approx(float(la.detach()), rel=1e-7)
        assert float((pa.grad - pb.grad).abs().max()) <= 1e-7 * float(pa.grad.abs().max())
    pa, pb = (pred.clone().requires_grad_(True) for _ in range(2))
    assert float(sh.seg_softlossv2(pb, probs).detach()) == pytest.approx(float(ref.seg_softlossv2(pa, probs).detach()), rel=1e-7)


def test_dropin_exposes_the_functions():
    import dropin.utils.seg_helper as d
    for name in ("seg_softloss", "seg_softlossv2", "seg_soft_loss", "seg_soft_targets_torch", "check_seg_soft_settings"):
        assert getattr(d, name) is getattr(sh, name)


# ---- sets, gate, ties, absent classes -----------------------------------------------------------------------------------------------------
def _case(seed=11, B=2, K=5, S=32, hs=(4, 2, 6)):
    g = torch.Generator().manual_seed(seed)
    scales = [torch.randn(2 * B, K, h, h, generator=g, dtype=torch.float64) * 2 for h in hs]
    for s in scales:
        s[:B, 0, :, : s.shape[-1] // 2] += 3.0                   # the background wins on the left half (and, un-flipped, of the flipped half)
        s[B:, 0, :, (s.shape[-1] + 1) // 2:] += 3.0
    y = torch.zeros(B, K - 1)
    y[0, [0, 2]] = 1
    y[1, :] = 1
    lr = torch.randn(B, K, 4, 4, generator=g, dtype=torch.float64)
    boxes = torch.tensor([[0, S, 0, S], [3, S - 5, 2, S - 9]])
    return lr, scales, y, boxes, S


def test_targets_absent_classes_and_temperature():
    lr, scales, y, boxes, S = _case()
    for temp in (0.05, 1.0, 20.0):
        q = sh.seg_soft_targets_torch(scales, y, S, temp)
        want = R.targets_f64(scales, y, S, temp)
        assert q.dtype == torch.float64 and float((q - want).abs().max()) <= 1e-12
        assert not q[0, [2, 4]].any() and bool((q[0, [0, 1, 3]] > 0).all())          # an absent class: 0 exactly
        assert float((q.sum(1) - 1).abs().max()) <= 1e-12
    # the temperature acts on the mean of the passes: the summed seg_ps with n_scales gives the same target
    up = [F.interpolate(s, size=(S, S), mode="bilinear", align_corners=False) for s in scales]
    seg_ps = sum(u[:2] + u[2:].flip(-1) for u in up)
    assert float((sh.seg_soft_targets_torch(seg_ps, y, S, 0.7, n_scales=3) - R.targets_f64(scales, y, S, 0.7)).abs().max()) <= 1e-12
    with pytest.raises(ValueError, match="n_scales"):
        sh.seg_soft_targets_torch(seg_ps, y, S, 0.7)


@pytest.mark.parametrize("conf", [0.0, 0.6])
def test_composition_against_the_restatement_sets_and_gate(conf):
    lr, scales, y, boxes, S = _case()
    want_l, want_g, n_bg, n_fg, q = R.loss_and_grad_f64(lr, scales, y, boxes, S, 0.3, conf, 0.3)
    x = lr.clone().requires_grad_(True)
    loss = sh.seg_soft_loss(x, scales, y, boxes, S, temp=0.3, conf=conf, fg_alpha=0.3)        # host tensors: the torch composition
    loss.backward()
    assert float(loss.detach()) == pytest.approx(want_l, rel=1e-12) and float((x.grad - want_g).abs().max()) <= 1e-12 * float(want_g.abs().max())
    inside = int((boxes[:, 1] - boxes[:, 0]).mul(boxes[:, 3] - boxes[:, 2]).sum())
    gated = int((q.max(1).values <= conf).sum())
    assert n_bg > 100 and n_fg > 100 and (n_bg + n_fg == inside if conf == 0 else (n_bg + n_fg < inside and gated > 50))
    # a negative bound counts from the end, as cam2mask reads a box
    neg = torch.tensor([[0, S, 0, S], [3, -5, 2, -9]])
    assert float(sh.seg_soft_loss(lr, scales, y, neg, S, temp=0.3, conf=conf, fg_alpha=0.3)) == float(loss.detach())


def test_a_tie_takes_the_lower_index_and_an_empty_set_gives_zero():
    S = 8
    q = torch.zeros(1, 3, S, S, dtype=torch.float64)
    q[:, 0], q[:, 1] = 0.5, 0.5                                  # every pixel tied between the background and class 1: background
    pred = torch.randn(1, 3, S, S, dtype=torch.float64, generator=torch.Generator().manual_seed(2)).requires_grad_(True)
    only_bg = sh.seg_softloss(pred, q, fg_alpha=0.0).detach()
    both = sh.seg_softloss(pred, q, fg_alpha=0.5).detach()
    assert float(both) == pytest.approx(0.5 * float(only_bg), rel=1e-12) and bool(torch.isfinite(both))    # the foreground set is empty: 0, not NaN
    (g,) = torch.autograd.grad(sh.seg_softloss(pred, q, fg_alpha=1.0), pred)
    assert not g.any()                                           # ... and a zero gradient from it
    q2 = q.clone()
    q2[:, 1] += 1e-9
    assert float(sh.seg_softloss(pred, q2, fg_alpha=0.0).detach()) == 0.0  # the tie broken: every pixel is foreground now


# ---- settings, flags, refusals --------------------------------------------------------------------------------------------------------------
def test_settings_ranges():
    for w, t, c in ((0.0, 1.0, 0.0), (0.5, 0.05, 0.0), (2.0, 20.0, 0.999)):
        sh.check_seg_soft_settings(w, t, c)
    for w, t, c, word in ((-0.1, 1.0, 0.0, "seg_soft_weight"), (float("nan"), 1.0, 0.0, "seg_soft_weight"), (0.1, 0.04, 0.0, "seg_soft_temp"),
                          (0.1, 20.5, 0.0, "seg_soft_temp"), (0.1, float("nan"), 0.0, "seg_soft_temp"), (0.1, 1.0, -0.1, "seg_soft_conf"),
                          (0.1, 1.0, 1.0, "seg_soft_conf"), (0.1, 1.0, float("nan"), "seg_soft_conf")):
        with pytest.raises(ValueError, match="--" + word):
            sh.check_seg_soft_settings(w, t, c, flag="--")
    lr, scales, y, boxes, S = _case()
    with pytest.raises(ValueError, match="seg_soft_temp"):
        sh.seg_soft_loss(lr, scales, y, boxes, S, temp=0.01)


def test_flag_table_defaults_and_launcher_refusals():
    from cosa_amd import args as cosa_args, main as launcher
    names = ("seg_soft_weight", "seg_soft_temp", "seg_soft_conf")
    a, changed = cosa_args.parse(["exp"])
    assert (a.seg_soft_weight, a.seg_soft_temp, a.seg_soft_conf) == (0.0, 1.0, 0.0) and not changed
    assert all(f in [n for n, _t, _d in cosa_args.EXTRA] and f not in [n for n, _t, _d in cosa_args.FLAGS] for f in names)
    launcher.check_supported(a)
    b, changed = cosa_args.parse(["exp", "--seg_soft_weight", "0.1", "--seg_soft_temp", "2", "--seg_soft_conf", "0.6"])
    assert (b.seg_soft_weight, b.seg_soft_temp, b.seg_soft_conf) == (0.1, 2.0, 0.6) and set(changed) == set(names)
    launcher.check_supported(b)
    t = launcher._trainer_args(b)
    assert (t.seg_soft_weight, t.seg_soft_temp, t.seg_soft_conf) == (0.1, 2.0, 0.6)
    for extra, word in ((["--seg_soft_weight", "-0.1"], "--seg_soft_weight"), (["--seg_soft_temp", "0.01"], "--seg_soft_temp"),
                        (["--seg_soft_temp", "21"], "--seg_soft_temp"), (["--seg_soft_conf", "1"], "--seg_soft_conf"),
                        (["--seg_soft_weight", "0.1", "--grad_check_iters", "5"], "--grad_check_iters")):
        bad, _ = cosa_args.parse(["exp"] + extra)
        with pytest.raises(ValueError, match=word):
            launcher.check_supported(bad)
    launcher.check_supported(cosa_args.parse(["exp", "--grad_check_iters", "5"])[0])          # the check alone stays allowed
    launcher.check_supported(cosa_args.parse(["exp", "--seg_soft_weight", "0.1", "--student_check_iters", "5"])[0])


def test_default_args_and_trainer_refusals():
    from cosa_amd.train_step import CoSATrainer, default_args, seg_soft_settings
    d = default_args("VOC12")
    assert (d.seg_soft_weight, d.seg_soft_temp, d.seg_soft_conf) == (0.0, 1.0, 0.0) and seg_soft_settings(d) == (0.0, 1.0, 0.0)
    assert seg_soft_settings(default_args(seg_soft_weight=0.2, seg_soft_temp=0.5, seg_soft_conf=0.3)) == (0.2, 0.5, 0.3)
    import types
    assert seg_soft_settings(types.SimpleNamespace()) == (0.0, 1.0, 0.0)                       # args without the fields: off
    for over, word in ((dict(seg_soft_weight=-1.0), "seg_soft_weight"), (dict(seg_soft_weight=0.1, seg_soft_temp=30.0), "seg_soft_temp"),
                       (dict(seg_soft_conf=1.5), "seg_soft_conf"), (dict(seg_soft_weight=0.1, grad_check_iters=3), "grad_check_iters")):
        with pytest.raises(ValueError, match=word):          # (before anything is built)
            CoSATrainer(default_args("VOC12", crop_size=64, **over), torch.device("cpu"))


def test_launcher_interval_keys_line_and_terms():
    from cosa_amd import main as launcher
    base = launcher.BASE_KEYS
    assert launcher.interval_keys(False) == launcher.interval_keys(False, False) == base
    assert launcher.interval_keys(True, False) == base + ("tok_loss",) and launcher.interval_keys(False, True) == base + ("soft_loss",)
    assert launcher.interval_keys(True, True) == base + ("tok_loss", "soft_loss")
    vals = [1.0, 2.0, 0.5, 3.0, 0.25, 4.0, 5.0, 6.0, 7.0, 8.0]
    off = launcher.interval_line("H\n", vals[:8], False)
    assert launcher.interval_line("H\n", vals[:8], False, False) == off and off.endswith("reg_loss: 6.0000 ...")
    assert launcher.interval_line("H\n", vals[:9], True, False) == off[:-4] + ", tok_loss: 7.0000 ..."
    assert launcher.interval_line("H\n", vals[:9], False, True) == off[:-4] + ", soft_loss: 7.0000 ..."
    assert launcher.interval_line("H\n", vals, True, True) == off[:-4] + ", tok_loss: 7.0000, soft_loss: 8.0000 ..."
    logs = {k: torch.tensor(float(i)) for i, k in enumerate(("overall_loss", "cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss",
                                                            "tok_loss", "soft_loss"))}
    t = {(a, b): launcher.interval_terms(logs, torch.tensor(0.5), torch.tensor(0.25), a, b).tolist() for a in (False, True) for b in (False, True)}
    assert t[False, False] == [0.0, 1.0, 0.5, 2.0, 0.25, 3.0, 4.0, 5.0]
    assert t[True, False] == t[False, False] + [6.0] and t[False, True] == t[False, False] + [7.0] and t[True, True] == t[False, False] + [6.0, 7.0]


def test_state_files_of_the_other_setting_are_refused_by_the_flags_name(tmp_path, monkeypatch):
    from cosa_amd import main as launcher
    from test_label_stats_cpu import _host_trainer

    def trainer(seed, tok, soft):
        tr = _host_trainer(monkeypatch, seed=seed)
        tr._add_extra_state("launcher.acc", torch.zeros(len(launcher.interval_keys(tok, soft)), dtype=torch.float64))
        if soft:
            tr._add_extra_state(launcher.EXTRA_KEYS_STATE, launcher.extra_keys_word(tok, soft, "cpu"))
        return tr

    paths = {}
    for tok, soft in ((False, False), (True, False), (False, True), (True, True)):
        a = trainer(1, tok, soft)
        (tmp_path / f"t{int(tok)}s{int(soft)}").mkdir()           # (a folder each: a save prunes the older state files next to it)
        paths[tok, soft] = str(tmp_path / f"t{int(tok)}s{int(soft)}" / "state_00000000.cosa")
        a.save_state(paths[tok, soft], n_iter=0)
        a.wait_state()
        assert launcher.load_state_checked(trainer(2, tok, soft), paths[tok, soft], tok, soft)["n_iter"] == 0
    # a file written with the term off holds the tensors it always held
    off = trainer(1, False, False)
    assert sorted(off.extra_state) == ["launcher.acc"] and sorted(trainer(1, False, True).extra_state) == ["launcher.acc", "launcher.extra_keys"]
    for (tok_f, soft_f), (tok_r, soft_r), word in (((False, False), (False, True), "--seg_soft_weight"), ((False, True), (False, False), "--seg_soft_weight"),
                                                   ((True, False), (False, True), "--seg_soft_weight"),      # nine sums both: the marker tells
                                                   ((False, True), (True, False), "--seg_soft_weight"),
                                                   ((True, True), (True, False), "--seg_soft_weight"),
                                                   ((False, True), (True, True), "--tokcon_weight"), ((False, False), (True, False), "--tokcon_weight")):
        with pytest.raises(ValueError, match=word):
            launcher.load_state_checked(trainer(2, tok_r, soft_r), paths[tok_f, soft_f], tok_r, soft_r)
