"""The gradient guard without a GPU: the two flags, and the plain torch restatement of the guard's semantics that
the non-fused path and host trainers run (and that the GPU tests compare the kernels with)."""
import math

import pytest
import torch


def test_flags_parse_default_off_and_reach_default_args():
    from cosa_amd import args as cosa_args
    from cosa_amd.train_step import default_args
    a, changed = cosa_args.parse(["EXP"])
    assert a.clip_grad_norm == 0.0 and a.skip_nonfinite is False
    assert "clip_grad_norm" not in changed and "skip_nonfinite" not in changed
    a, changed = cosa_args.parse(["EXP", "--clip_grad_norm", "1.5", "--skip_nonfinite", "true"])
    assert a.clip_grad_norm == 1.5 and a.skip_nonfinite is True
    assert changed["clip_grad_norm"] == 1.5 and changed["skip_nonfinite"] is True
    d = default_args("VOC12")
    assert d.clip_grad_norm == 0.0 and d.skip_nonfinite is False
    d = default_args("VOC12", **{k: v for k, v in vars(a).items() if k != "dataset"})          # main._trainer_args
    assert d.clip_grad_norm == 1.5 and d.skip_nonfinite is True


def _toy(seed=0):
    """three small student tensors (one without a gradient), a teacher, and PolyWarmupAdamW over the student"""
    from cosa_amd.utils import torch_helper
    g = torch.Generator().manual_seed(seed)
    student = [torch.nn.Parameter(torch.randn(n, generator=g)) for n in (5, 7, 3)]
    teacher = [torch.randn(p.shape, generator=g) for p in student]
    opt = torch_helper.PolyWarmupAdamW([{"params": student[:2], "lr": 1e-2, "weight_decay": 1e-2}, {"params": student[2:], "lr": 1e-1, "weight_decay": 0.0}],
                                       lr=1e-2, weight_decay=1e-2, betas=(0.9, 0.999), warmup_iter=2, max_iter=50, warmup_ratio=1e-6, power=0.9,
                                       fused=False)
    return student, teacher, opt


def _grads(student, seed, scale=1.0):
    g = torch.Generator().manual_seed(100 + seed)
    for p in student[:2]:
        p.grad = torch.randn(p.shape, generator=g) * scale
    student[2].grad = None


def _snapshot(student, teacher, opt):
    out = [p.detach().clone() for p in student] + [t.clone() for t in teacher]
    for p in student:
        st = opt.state.get(p, {})
        out += [st[k].clone() for k in ("exp_avg", "exp_avg_sq") if k in st]
    return out


def test_torch_restatement_clips_like_clip_grad_norm():
    from cosa_amd.utils import torch_helper
    sa, ta, oa = _toy()
    sb, tb, ob = _toy()
    state = torch_helper.new_guard_state("cpu")
    for it in range(3):
        _grads(sa, it, scale=3.0)
        _grads(sb, it, scale=3.0)
        norm = torch.linalg.vector_norm(torch.cat([p.grad.double() for p in sa[:2]])).item()
        torch_helper.guarded_torch_step(oa, ta, sa, 0.9, 1.0, True, state)
        assert torch_helper.guard_norm(state).item() == pytest.approx(norm, rel=1e-6)
        assert torch_helper.guard_coef(state).item() == pytest.approx(1.0 / (norm + 1e-6), rel=1e-6) and norm > 1
        torch.nn.utils.clip_grad_norm_([p for p in sb], 1.0)
        ob.step()
        torch_helper.ema_update(tb, sb, 0.9)
    for a, b in zip(_snapshot(sa, ta, oa), _snapshot(sb, tb, ob)):
        assert torch.allclose(a, b, rtol=2e-6, atol=1e-8), (a - b).abs().max().item()
    assert torch_helper.guard_counters(state) == {"applied": 3, "skipped": 0, "clipped": 3}
    assert oa.global_step == ob.global_step == 3


def test_torch_restatement_inactive_guard_is_the_plain_step():
    from cosa_amd.utils import torch_helper
    sa, ta, oa = _toy()
    sb, tb, ob = _toy()
    state = torch_helper.new_guard_state("cpu")
    for it in range(3):
        _grads(sa, it)
        _grads(sb, it)
        torch_helper.guarded_torch_step(oa, ta, sa, 0.9, 1e9, True, state)
        ob.step()
        torch_helper.ema_update(tb, sb, 0.9)
    for a, b in zip(_snapshot(sa, ta, oa), _snapshot(sb, tb, ob)):
        assert torch.equal(a, b)
    assert torch_helper.guard_counters(state) == {"applied": 3, "skipped": 0, "clipped": 0}
    assert torch_helper.guard_coef(state).item() == 1.0 and torch_helper.guard_skip(state).item() == 0


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_torch_restatement_skips_and_the_schedule_goes_on(bad):
    """a refused step changes nothing, but global_step (the LR schedule) and the bias-correction count advance: the run then equals one
    whose optimizer took its steps 1 and 3 with the step counts 1 and 3"""
    from cosa_amd.utils import torch_helper
    sa, ta, oa = _toy()
    sb, tb, ob = _toy()
    state = torch_helper.new_guard_state("cpu")
    _grads(sa, 0)
    torch_helper.guarded_torch_step(oa, ta, sa, 0.9, 0.0, True, state)
    before = _snapshot(sa, ta, oa)
    _grads(sa, 1)
    sa[1].grad[3] = bad
    torch_helper.guarded_torch_step(oa, ta, sa, 0.9, 0.0, True, state)
    assert torch_helper.guard_skip(state).item() == 1 and not math.isfinite(torch_helper.guard_norm(state).item())
    for a, b in zip(_snapshot(sa, ta, oa), before):
        assert torch.equal(a, b)
    assert oa.global_step == 2 and all(float(oa.state[p]["step"]) == 2.0 for p in sa[:2])
    _grads(sa, 2)
    torch_helper.guarded_torch_step(oa, ta, sa, 0.9, 0.0, True, state)
    assert torch_helper.guard_counters(state) == {"applied": 2, "skipped": 1, "clipped": 0}
    assert oa.global_step == 3 and all(bool(torch.isfinite(t).all()) for t in _snapshot(sa, ta, oa))
    # the same run by hand: step 2 advances the counts only
    _grads(sb, 0)
    ob.step()
    torch_helper.ema_update(tb, sb, 0.9)
    ob.global_step += 1
    for p in sb[:2]:
        ob.state[p]["step"] += 1
    _grads(sb, 2)
    ob.step()
    torch_helper.ema_update(tb, sb, 0.9)
    for a, b in zip(_snapshot(sa, ta, oa), _snapshot(sb, tb, ob)):
        assert torch.equal(a, b)
    assert [g["lr"] for g in oa.param_groups] == [g["lr"] for g in ob.param_groups]
    # the switch is what protects: without it the same gradient is applied
    sc, tc, oc = _toy()
    state_c = torch_helper.new_guard_state("cpu")
    _grads(sc, 1)
    sc[1].grad[3] = bad
    torch_helper.guarded_torch_step(oc, tc, sc, 0.9, 0.0, False, state_c)
    assert not bool(torch.isfinite(tc[1]).all())
    assert torch_helper.guard_counters(state_c) == {"applied": 1, "skipped": 0, "clipped": 0}


def test_skip_on_the_very_first_step_creates_the_moments():
    from cosa_amd.utils import torch_helper
    s, t, o = _toy()
    state = torch_helper.new_guard_state("cpu")
    _grads(s, 0)
    s[0].grad[0] = float("nan")
    torch_helper.guarded_torch_step(o, t, s, 0.9, 1.0, True, state)
    assert o.global_step == 1 and float(o.state[s[0]]["step"]) == 1.0 and int(o.state[s[0]]["exp_avg"].abs().sum()) == 0
    _grads(s, 1)
    torch_helper.guarded_torch_step(o, t, s, 0.9, 1.0, True, state)
    assert float(o.state[s[0]]["step"]) == 2.0 and torch_helper.guard_counters(state)["skipped"] == 1
