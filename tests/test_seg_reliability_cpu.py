"""--seg_reliability on the host: the float64 restatement (tests/seg_weight_ref.py) and the torch path's
seg_weightloss against the golden vectors the reference wrote (tests/golden/seg_weight.npz) and, where the reference tree is present,
against the live reference; the torch composition of the weight against the numpy restatements; flags, refusals and the trainer's fields."""
import numpy as np
import pytest
import torch

import seg_weight_ref as R
from cosa_amd.utils import seg_helper as sh

ALPHAS = (("a0", 0.0), ("a03", 0.3), ("a1", 1.0))


@pytest.fixture(scope="module")
def gold(golden):
    return golden("seg_weight")


def _inputs(gold):
    return (torch.from_numpy(gold["pred"]), torch.from_numpy(gold["mask"].astype(np.float32)), torch.from_numpy(gold["weights"]))


def test_golden_inputs_hold_the_planted_weights(gold):
    w, lab = gold["weights"], gold["mask"] != 255
    assert gold["pred"].shape == (2, 6, 64, 64) and sorted(np.unique(gold["mask"]).tolist()) == [0, 1, 3, 5, 255]
    assert (w[lab] == 0).sum() > 50 and (w[lab] == 1).sum() > 50 and ((w > 0) & (w < 1)).mean() > 0.8 and w.min() >= 0 and w.max() <= 1


@pytest.mark.parametrize("tag,alpha", ALPHAS)
def test_restatement_and_product_against_golden(gold, tag, alpha):
    """the bar tests/test_loss_flags_cpu.py holds seg_loss to against the same kind of vector: 1e-6 relative on the value (fp32 sums over
    2 x 64 x 64 pixels in another order than the reference's).  The gradient: every element is w (p - [k == l]) / count, a handful of fp32
    roundings of its own magnitude in the golden file and in the product -- 1e-6 of the largest element"""
    pred, mask, w = _inputs(gold)
    want_l, want_g = float(gold["loss_" + tag]), gold["grad_" + tag].astype(np.float64)
    top = np.abs(want_g).max()
    l64, g64 = R.weighted_ce_full_f64(pred, mask, w, alpha)
    p = pred.clone().requires_grad_(True)
    lp = sh.seg_weightloss(p, mask, w, fg_alpha=alpha)
    lp.backward()
    for what, l, g in (("restatement", l64, g64.numpy()), ("seg_weightloss", float(lp.detach()), p.grad.double().numpy())):
        err_l, err_g = abs(l - want_l) / abs(want_l), np.abs(g - want_g).max() / top
        print(f"{what} fg_alpha {alpha}: loss {err_l:.3e} grad {err_g:.3e}")
        assert err_l <= 1e-6, (what, err_l)
        assert err_g <= 1e-6, (what, err_g)
    assert top > 0 and np.isfinite(want_g).all()


def test_against_live_reference(gold):
    from oracle import ref_loader
    if not ref_loader.available():
        pytest.skip("reference tree not present")
    ref = ref_loader.seg_helper()
    pred, mask, w = _inputs(gold)
    for _tag, alpha in ALPHAS:
        pa, pb = (pred.clone().requires_grad_(True) for _ in range(2))
        la, lb = ref.seg_weightloss(pa, mask, w, fg_alpha=alpha), sh.seg_weightloss(pb, mask, w, fg_alpha=alpha)
        la.backward()
        lb.backward()
        assert float(lb.detach()) == pytest.approx(float(la.detach()), rel=1e-6)
        assert float((pa.grad - pb.grad).abs().max()) <= 1e-6 * float(pa.grad.abs().max())
        l64, _ = R.weighted_ce_full_f64(pred, mask, w, alpha)
        assert l64 == pytest.approx(float(la.detach()), rel=1e-6)


@pytest.mark.parametrize("alpha", [0.0, 0.3, 0.5, 1.0])
def test_unit_weights_give_seg_loss(gold, alpha):
    pred, mask, w = _inputs(gold)
    pa, pb = (pred.clone().requires_grad_(True) for _ in range(2))
    la, lb = sh.seg_loss(pa, mask, fg_alpha=alpha), sh.seg_weightloss(pb, mask, torch.ones_like(w), fg_alpha=alpha)
    la.backward()
    lb.backward()
    assert float(lb) == pytest.approx(float(la), rel=1e-6)
    assert float((pa.grad - pb.grad).abs().max()) <= 1e-6 * float(pa.grad.abs().max())
    # and weights of zero give an exact zero with a zero gradient
    pc = pred.clone().requires_grad_(True)
    lc = sh.seg_weightloss(pc, mask, torch.zeros_like(w), fg_alpha=alpha)
    lc.backward()
    assert float(lc) == 0.0 and float(pc.grad.abs().max()) == 0.0


# ---- the weight -----------------------------------------------------------------------------------------------------------------------------
def _weight_case(seed=5, B=3, C=5, S=24):
    rng = np.random.default_rng(seed)
    cam = rng.uniform(0, 1, (B, C, S, S)).astype(np.float32)
    y = np.zeros((B, C), np.float32)
    y[0, [1, 3]] = 1
    y[1, :] = 1                                            # every class present: the maximum has no absent 0 to start from
    hi, lo = 0.7, 0.25                                     # image 2: no class present
    vc = cam * y[:, :, None, None]
    mx, am = vc.max(1), vc.argmax(1)
    mask = np.where(mx >= np.float32(hi), am + 1, np.where(mx < np.float32(lo), 0, 255)).astype(np.float32)
    moved = rng.uniform(0, 1, mask.shape) < 0.3           # labels the CAM does not support (PAR's moves, absent classes, labels past C)
    mask = np.where(moved, rng.choice([0, 1, 2, 4, 5, 7, 255], size=mask.shape), mask).astype(np.float32)
    cam[1, 2, 3, 4], mask[1, 3, 4] = 1.0, 3.0             # v == 1 exactly
    cam[1, 0, 5, 6], mask[1, 5, 6] = np.nan, 1.0          # a NaN in a foreground pixel's own plane
    return cam, y, mask, hi, lo


def test_the_weight_case_holds_what_it_should():
    cam, y, mask, hi, lo = _weight_case()
    r, lab = R.ratio_f64(cam, y, mask, hi, lo)
    assert ((r > 0) & (r < 1) & lab).sum() >= 0.05 * lab.sum() and ((r == 0) & lab).any() and ((r == 1) & lab).any()
    assert r[1, 3, 4] == 1.0 and r[1, 5, 6] == 0.0 and (mask == 7).any() and not lab[mask == 7].any()


@pytest.mark.parametrize("floor", [0.0, 0.25])
@pytest.mark.parametrize("beta", [0.0, 1.0])
def test_torch_weight_is_the_float32_restatement_bit_for_bit(beta, floor):
    cam, y, mask, hi, lo = _weight_case()
    t = torch.from_numpy
    stats = sh.new_reliability_stats(2, "cpu")
    w_main, w_aux = sh._label_reliability_torch([t(cam), t(cam)], t(y), [t(mask), t(mask)], [hi, lo], [lo, lo], beta=beta, floor=floor,
                                                stats=stats)
    for w, (h, l_), row in ((w_main, (hi, lo), 0), (w_aux, (lo, lo), 1)):          # (the second set: hi == lo, one threshold)
        want = R.weight_f32(cam, y, mask, h, l_, beta, floor)
        assert w.dtype == torch.float32 and np.array_equal(w.numpy().view(np.uint32), want.view(np.uint32))
        assert stats[row].tolist() == R.weight_stats(want, mask, cam.shape[1]).tolist()
    lab = (mask <= cam.shape[1])
    assert float(w_main.numpy()[~lab].max()) == 0.0
    if beta == 0.0:
        assert bool((w_main.numpy()[lab] == 1.0).all())                          # beta 0: every labelled pixel weighs 1
    else:
        assert float(w_main.numpy()[lab].min()) == np.float32(floor)             # an unsupported label weighs the floor
    # the public function takes host tensors down the same path, and accumulates into the counters
    again = sh.label_reliability([t(cam)], t(y), [t(mask)], [hi], [lo], beta=beta, floor=floor, stats=stats[:1])
    assert torch.equal(again[0], w_main) and stats[0].tolist() == (2 * R.weight_stats(R.weight_f32(cam, y, mask, hi, lo, beta, floor), mask, 5)).tolist()


@pytest.mark.parametrize("floor", [0.0, 0.25])
@pytest.mark.parametrize("beta", [0.5, 2.0, 8.0])
def test_torch_weight_with_a_power_against_float64(beta, floor):
    """|w - w64| <= 4 e32 + 2^-24 with e32 the largest error of the numpy-float32 formula against float64 on the same inputs (the bar the
    kernel is held to on the device)"""
    cam, y, mask, hi, lo = _weight_case()
    t = torch.from_numpy
    w = sh._label_reliability_torch([t(cam)], t(y), [t(mask)], [hi], [lo], beta=beta, floor=floor)[0].double().numpy()
    w64 = R.weight_f64(cam, y, mask, hi, lo, beta, floor)
    e32 = np.abs(R.weight_f32(cam, y, mask, hi, lo, beta, floor).astype(np.float64) - w64).max()
    err = np.abs(w - w64).max()
    print(f"beta {beta} floor {floor}: e32 {e32:.3e} torch {err:.3e}")
    assert 0 < e32 < 1e-5 and err <= 4 * e32 + 2.0 ** -24


def test_raw_and_validated_cams_give_the_same_map_and_summary():
    cam, y, mask, hi, lo = _weight_case()
    t = torch.from_numpy
    stats = sh.new_reliability_stats(1, "cpu")
    a = sh.label_reliability([t(cam)], t(y), [t(mask)], [hi], [lo], stats=stats)[0]
    b = sh.label_reliability([sh.cam_validation(t(cam), t(y))], t(y), [t(mask)], [torch.tensor(hi)], [torch.tensor(lo)])[0]
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    (s,) = sh.reliability_summary(stats)
    l = mask.astype(np.int64)
    assert s["n_bg"] == int((l == 0).sum()) and s["n_fg"] == int(((l >= 1) & (l <= 5)).sum())
    assert s["bg"] == pytest.approx(float(a.numpy()[l == 0].astype(np.float64).mean()), abs=2.0 ** -32)
    assert s["fg"] == pytest.approx(float(a.numpy()[(l >= 1) & (l <= 5)].astype(np.float64).mean()), abs=2.0 ** -32)
    assert sh.reliability_summary(sh.new_reliability_stats(1, "cpu")) == [dict(bg=None, n_bg=0, fg=None, n_fg=0)]


def test_dropin_exposes_the_functions():
    import dropin.utils.seg_helper as d
    for name in ("seg_weightloss", "label_reliability", "reliability_summary", "check_reliability_settings"):
        assert getattr(d, name) is getattr(sh, name)


# ---- flags and refusals ----------------------------------------------------------------------------------------------------------------------
BAD = [dict(camweight_beta=-0.5), dict(camweight_beta=8.5), dict(camweight_beta=float("nan")), dict(seg_reliability_floor=-0.1),
       dict(seg_reliability_floor=1.0), dict(seg_reliability_floor=float("nan"))]


def test_settings_ranges():
    for beta, floor in ((0.0, 0.0), (8.0, 0.999), (1.0, 0.25)):
        sh.check_reliability_settings(beta, floor)
    for beta, floor, word in ((-1e-3, 0.0, "camweight_beta"), (8.01, 0.0, "camweight_beta"), (float("nan"), 0.0, "camweight_beta"),
                              (1.0, -1e-3, "seg_reliability_floor"), (1.0, 1.0, "seg_reliability_floor"), (1.0, float("inf"), "seg_reliability_floor")):
        with pytest.raises(ValueError, match="--" + word):
            sh.check_reliability_settings(beta, floor, flag="--")
    cam, y, mask, hi, lo = _weight_case()
    t = torch.from_numpy
    with pytest.raises(ValueError):
        sh.label_reliability([t(cam)], t(y), [t(mask)], [hi], [lo], beta=9.0)
    with pytest.raises(ValueError):
        sh.label_reliability([t(cam)] * 5, t(y), [t(mask)] * 5, [hi] * 5, [lo] * 5)
    with pytest.raises(ValueError):
        sh.label_reliability([t(cam)], t(y), [t(mask)], [hi], [lo], stats=torch.zeros(4, dtype=torch.int64))


def test_flags_parse_and_belong_to_extra(capsys):
    from cosa_amd import args as cosa_args, main as launcher
    extra = {f: (typ, d) for f, typ, d in cosa_args.EXTRA}
    assert extra["seg_reliability"][1] is False and extra["seg_reliability_floor"][1] == 0.0
    assert "camweight_beta" not in extra and ("camweight_beta", float, 1.0) in cosa_args.FLAGS            # the reference's flag stays one
    a, changed = cosa_args.parse(["EXP"])
    assert a.seg_reliability is False and a.seg_reliability_floor == 0.0 and a.camweight_beta == 1.0 and not changed
    launcher.check_supported(a)
    assert "camweight_beta" not in capsys.readouterr().out
    a, changed = cosa_args.parse(["EXP", "--seg_reliability", "true", "--seg_reliability_floor", "0.25", "--camweight_beta", "2"])
    assert a.seg_reliability is True and changed == dict(seg_reliability=True, seg_reliability_floor=0.25, camweight_beta=2.0)
    launcher.check_supported(a)
    assert "camweight_beta" not in capsys.readouterr().out
    t = launcher._trainer_args(a)
    assert t.seg_reliability is True and t.seg_reliability_floor == 0.25 and t.camweight_beta == 2.0
    # the reference's flag with the switch off: accepted, with a note that says what reads it
    launcher.check_supported(cosa_args.parse(["EXP", "--camweight_beta", "2"])[0])
    out = capsys.readouterr().out
    assert "note: --camweight_beta: only read with --seg_reliability true" in out
    for argv in (["--camweight_beta", "9"], ["--camweight_beta", "-1"], ["--seg_reliability_floor", "1"], ["--seg_reliability_floor", "-0.5"],
                 ["--seg_reliability", "true", "--camweight_beta", "nan"]):
        with pytest.raises(ValueError, match="--camweight_beta|--seg_reliability_floor"):
            launcher.check_supported(cosa_args.parse(["EXP"] + argv)[0])


def test_launcher_line_and_record(tmp_path):
    import json
    from cosa_amd import main as launcher
    from cosa_amd import train_step as ts
    summary = [dict(bg=0.6124, n_bg=10, fg=0.3706, n_fg=4), dict(bg=None, n_bg=0, fg=0.5, n_fg=2)]
    assert launcher.seg_rel_line(summary) == " seg_rel: main bg 0.612 fg 0.371, aux bg - fg 0.500"
    assert launcher.seg_rel_line(summary[:1]) == " seg_rel: main bg 0.612 fg 0.371"
    targs = ts.default_args(seg_reliability=True, camweight_beta=2.0, seg_reliability_floor=0.25)
    launcher.append_seg_reliability(tmp_path, summary, 2000, targs)
    launcher.append_seg_reliability(tmp_path, summary[:1], 4000, targs)
    rows = [json.loads(x) for x in (tmp_path / "seg_reliability.jsonl").read_text().splitlines()]
    assert rows[0] == dict(iters=2000, beta=2.0, floor=0.25, main=summary[0], aux=summary[1]) and rows[1]["iters"] == 4000 and "aux" not in rows[1]


def test_default_args_and_a_trainer_that_refuses_bad_values():
    from cosa_amd import train_step as ts
    a = ts.default_args()
    assert a.seg_reliability is False and a.seg_reliability_floor == 0.0 and a.camweight_beta == 1.0
    assert ts.reliability_settings(a) == (False, 1.0, 0.0)
    assert ts.reliability_settings(ts.default_args(seg_reliability=True, camweight_beta=2, seg_reliability_floor=0.5)) == (True, 2.0, 0.5)
    for bad in BAD:
        with pytest.raises(ValueError, match="camweight_beta|seg_reliability_floor"):
            ts.CoSATrainer(ts.default_args(seg_reliability=True, crop_size=64, compute_dtype=torch.float32, **bad), torch.device("cpu"))


def test_monitor_table_and_interval_keys_are_untouched():
    """the term has no monitor row, no interval key and no state-file entry (its counters since the last evaluation are lost on resume)"""
    from cosa_amd import main as launcher, monitors
    assert not any("rel" in m.name for m in monitors.MONITORS)
    assert launcher.interval_keys(False) == launcher.BASE_KEYS and "seg_rel" not in "".join(launcher.interval_keys(True))
