"""Gradient accumulation without a GPU: the flag, the torch restatement of cosa_grad_accumulate against the explicit
fp32 expression, and host trainers (the real CoSATrainer set-up of tests/test_resume_cpu.py around a toy network and a toy loss): weight
parity with a step on pre-averaged gradients, mixed None gradients, the guard, resumption through the launcher's batch counter, N = 1."""
import numpy as np
import pytest
import torch

import test_resume_cpu as RC
from cosa_amd import checkpoint as ck

INF, NAN = float("inf"), float("nan")


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---- the flag ------------------------------------------------------------------------------------------------------------------------------
def test_flag_parses_default_one_and_zero_is_refused():
    from cosa_amd import args as cosa_args
    from cosa_amd import main as launcher
    from cosa_amd.train_step import default_args
    a, changed = cosa_args.parse(["EXP"])
    assert a.accum_steps == 1 and "accum_steps" not in changed
    launcher.check_supported(a)
    b, changed = cosa_args.parse(["EXP", "--accum_steps", "4"])
    assert b.accum_steps == 4 and changed["accum_steps"] == 4
    launcher.check_supported(b)
    assert {k: v for k, v in vars(b).items() if k != "accum_steps"} == {k: v for k, v in vars(a).items() if k != "accum_steps"}
    assert default_args("VOC12").accum_steps == 1
    assert default_args("VOC12", **{k: v for k, v in vars(b).items() if k != "dataset"}).accum_steps == 4
    for bad in ("0", "-2"):
        c, _ = cosa_args.parse(["EXP", "--accum_steps", bad])
        with pytest.raises(ValueError, match="accum_steps"):
            launcher.check_supported(c)


# ---- the torch restatement, element-wise -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 7])
def test_restatement_is_the_explicit_fp32_expression_bit_for_bit(n):
    from cosa_amd.utils import torch_helper
    g = torch.Generator().manual_seed(n)
    shapes = [(1,), (3,), (4, 5), (1031,)]
    micro = [[torch.randn(s, generator=g) * 10.0 ** float(torch.randint(-3, 4, (1,), generator=g)) for s in shapes] + [None] for _ in range(n)]
    micro[0][3][5], micro[n - 1][3][6], micro[0][3][7], micro[n - 1][3][7] = INF, NAN, INF, -INF        # inf, NaN, inf + -inf
    micro[1][3][8] = 3.0e38
    micro[0][3][8] = 3.0e38                                                                            # overflows to inf in the sum
    kept = [[None if t is None else t.clone() for t in m] for m in micro]
    acc = None
    for k in range(n):
        acc = torch_helper.accumulate_grads_torch(acc, micro[k], k, n)
    scale = torch.tensor(np.float32(1.0) / np.float32(n))
    assert torch_helper.accum_scale(n) == float(scale) and scale.dtype == torch.float32
    assert acc[-1] is None and len(acc) == len(shapes) + 1
    for i in range(len(shapes)):
        want = kept[0][i].clone()
        for k in range(1, n):
            want = want + kept[k][i]                     # fl(acc + g), in micro-step order
        want = want * scale                              # one more rounding
        assert acc[i].dtype == torch.float32 and torch.equal(torch.isnan(acc[i]), torch.isnan(want))
        ok = ~torch.isnan(want)
        assert torch.equal(_bits(acc[i])[ok], _bits(want)[ok]), i
    assert torch.isinf(acc[3][5]) and torch.isnan(acc[3][6]) and torch.isnan(acc[3][7]) and torch.isinf(acc[3][8])
    for m, k_ in zip(micro, kept):                       # the gradients are only read
        for a, b in zip(m, k_):
            assert (a is None and b is None) or torch.equal(_bits(a), _bits(b))
    assert [torch_helper.accum_mode(k, 4) for k in range(4)] == [0, 1, 1, 2] and [torch_helper.accum_mode(k, 2) for k in range(2)] == [0, 2]
    for k, m in ((0, 1), (2, 2), (-1, 3)):
        with pytest.raises(ValueError):
            torch_helper.accum_mode(k, m)


def test_restatement_refuses_mixed_none_gradients_by_name():
    from cosa_amd.utils import torch_helper
    acc = torch_helper.accumulate_grads_torch(None, [torch.ones(3), None], 0, 3, ["w", "b"])
    with pytest.raises(RuntimeError, match="^b: .grad is set"):
        torch_helper.accumulate_grads_torch(acc, [torch.ones(3), torch.ones(2)], 1, 3, ["w", "b"])
    with pytest.raises(RuntimeError, match="^w: .grad is None"):
        torch_helper.accumulate_grads_torch(acc, [None, None], 2, 3, ["w", "b"])


# ---- host trainers -----------------------------------------------------------------------------------------------------------------------------
def _toy_losses(tr, without=()):
    """a differentiable stand-in for CoSATrainer.forward_losses on the toy network (the real one needs the HIP kernels); `without`: micro-steps
    (by call count) whose loss does not reach the decoder"""
    calls = [0]

    def forward_losses(wimg, simg, cls_label, img_box, n_iter):
        m = tr.student
        h = m.norm(torch.tanh(m.encoder.proj(simg)))
        loss = m.classifier(h[:, :, None, None]).square().mean() + 0.1 * wimg.mean() * h.sum()
        if calls[0] not in without:
            loss = loss + (m.decoder(h) - cls_label).square().mean()
        calls[0] += 1
        return loss, dict(overall_loss=loss.detach())

    return forward_losses


def _batch(k, b=2):
    g = torch.Generator().manual_seed(900 + k)
    return torch.randn(b, 5, generator=g), torch.randn(b, 5, generator=g), torch.randn(b, 3, generator=g), None


def _trainer(monkeypatch, seed=3, without=(), **over):
    tr = RC._host_trainer(monkeypatch, seed, **over)
    monkeypatch.setattr(tr, "forward_losses", _toy_losses(tr, without))
    return tr


def _weights(tr):
    out = [p.detach().clone() for p in tr.student.parameters()] + [p.detach().clone() for p in tr.model_AN.parameters()]
    for grp in tr.optimizer.param_groups:
        for p in grp["params"]:
            st = tr.optimizer.state.get(p, {})
            out += [st[k].clone() for k in ("exp_avg", "exp_avg_sq") if k in st]
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("n", [2, 3])
def test_host_trainer_equals_one_step_on_the_pre_averaged_gradients(monkeypatch, n):
    from cosa_amd.utils import torch_helper
    a = _trainer(monkeypatch, accum_steps=n)
    b = _trainer(monkeypatch, accum_steps=1)
    _same(_weights(a), _weights(b))
    scale = torch.tensor(np.float32(1.0) / np.float32(n))
    for rnd in range(2):
        batches = [_batch(10 * rnd + k) for k in range(n)]
        for k, x in enumerate(batches):
            before = _weights(a)
            logs = a.step(*x, n_iter=rnd)
            assert "overall_loss" in logs
            if k < n - 1:                                # only the closing micro-step moves anything
                _same(_weights(a), before)
                assert a.optimizer.global_step == rnd
        grads = []
        for x in batches:
            loss, _ = b.forward_losses(*x, rnd)
            b.optimizer.zero_grad(set_to_none=True)
            loss.backward()
            grads.append([None if p.grad is None else p.grad.clone() for p in b.student.parameters()])
        for i, p in enumerate(b.student.parameters()):
            if grads[0][i] is None:
                continue
            s = grads[0][i]
            for k in range(1, n):
                s = s + grads[k][i]
            p.grad = s * scale                           # n = 2: ((g1 + g2) * 0.5)
        b.optimizer.step()
        torch_helper.ema_update(b._ema_pairs[0], b._ema_pairs[1], b.args.momentum)
        _same(_weights(a), _weights(b))
        assert a.optimizer.global_step == b.optimizer.global_step == rnd + 1 and a._micro_k == 0 and a._accum is None
    assert any(not torch.equal(x, y) for x, y in zip(_weights(a), _weights(_trainer(monkeypatch))))      # (steps were taken)


def test_host_trainer_refuses_a_parameter_that_loses_its_gradient_between_micro_steps(monkeypatch):
    tr = _trainer(monkeypatch, accum_steps=2, without=(1,))
    tr.step(*_batch(0), n_iter=0)
    with pytest.raises(RuntimeError, match=r"decoder\.weight: \.grad is None"):
        tr.step(*_batch(1), n_iter=0)


def test_host_guard_refuses_the_whole_step_for_one_poisoned_micro_batch(monkeypatch):
    tr = _trainer(monkeypatch, accum_steps=2, skip_nonfinite=True)
    for k in range(2):
        tr.step(*_batch(k), n_iter=0)
    assert tr.guard_counters() == {"applied": 1, "skipped": 0, "clipped": 0}
    before = _weights(tr)
    tr.step(*_batch(2), n_iter=1)
    hook = tr.student.classifier.weight.register_hook(lambda g: torch.where(torch.arange(g.numel()).reshape(g.shape) == 3, torch.full_like(g, NAN), g))
    try:
        logs = tr.step(*_batch(3), n_iter=1)             # micro-batch 1 of the step: one NaN in one gradient
    finally:
        hook.remove()
    assert not bool(torch.isfinite(logs["grad_norm"]))
    _same(_weights(tr), before)
    assert tr.guard_counters() == {"applied": 1, "skipped": 1, "clipped": 0} and tr.optimizer.global_step == 2
    for k in range(2):                                   # the next step is taken: nothing of the poisoned accumulator is left
        tr.step(*_batch(4 + k), n_iter=2)
    assert tr.guard_counters() == {"applied": 2, "skipped": 1, "clipped": 0}
    assert all(bool(torch.isfinite(t).all()) for t in _weights(tr))
    # poisoned in micro-batch 0 instead: mode "acc = g" carries it too
    hook = tr.student.norm.bias.register_hook(lambda g: torch.full_like(g, INF))
    try:
        tr.step(*_batch(6), n_iter=3)
    finally:
        hook.remove()
    tr.step(*_batch(7), n_iter=3)
    assert tr.guard_counters() == {"applied": 2, "skipped": 2, "clipped": 0}


def test_accum_steps_1_is_inert(monkeypatch):
    from cosa_amd import train_step
    a = _trainer(monkeypatch, accum_steps=1)
    monkeypatch.setattr(train_step, "build_model", lambda args: RC._TinyNet())
    args = train_step.default_args("VOC12", crop_size=64, batch_size=2, usegmm=True, max_iters=100)
    delattr(args, "accum_steps")                         # a namespace from before the flag
    b = train_step.CoSATrainer(args, torch.device("cpu"), seed=3)
    monkeypatch.setattr(b, "forward_losses", _toy_losses(b))
    for k in range(2):
        a.step(*_batch(k), n_iter=k)
        b.step(*_batch(k), n_iter=k)
    _same(_weights(a), _weights(b))
    for tr in (a, b):
        assert tr._accum_steps == 1 and tr._accum is None and tr._micro_k == 0 and tr._fused_step is None
        assert tr.optimizer.global_step == 2


# ---- resumption: the launcher's counter counts batches ----------------------------------------------------------------------------------------
EPOCH = 5            # batches per pass over the "dataset": odd, so that with N = 2 an optimizer step straddles two passes


def _launch(monkeypatch, tmp_path, steps, n, save_iters, resume=None, seed=3):
    """the launcher's loop (cosa_amd/main.py) around a host trainer: shuffled passes drawn from the global generators, next_batch, a state
    file every save_iters optimizer steps -> (trainer, {iteration: path}, pos)"""
    from cosa_amd import main as launcher
    tr = _trainer(monkeypatch, seed=seed, accum_steps=n)
    pos = {"rng": None, "epoch": None, "consumed": 0}

    def new_iter(skip=0):
        pos["rng"] = ck.pack_rng(None)
        pos["epoch"], pos["consumed"] = int(np.random.randint(1000)), skip
        order = torch.randperm(EPOCH).tolist()                         # (what a sampler draws)
        return iter([_batch(100 * pos["epoch"] + i) for i in order][skip:])

    first = 0
    if resume is not None:
        got = tr.load_state(resume)
        ck.unpack_rng(got["loader"]["rng"])
        it = new_iter(skip=int(got["loader"]["consumed"]))
        assert pos["epoch"] == got["loader"]["epoch"]
        ck.unpack_rng(got["rng_at_save"])
        first = int(got["n_iter"]) + 1
    else:
        it = new_iter()
    files = {}
    for n_iter in range(first, steps):
        for _ in range(n):
            it, batch = launcher.next_batch(it, new_iter, pos)
            tr.step(*batch, n_iter=n_iter)
        if (n_iter + 1) % save_iters == 0:
            files[n_iter + 1] = str(tmp_path / f"state_{n_iter + 1:08d}.cosa")
            tr.save_state(files[n_iter + 1], n_iter=n_iter, loader=dict(pos))
            tr.wait_state()
    return tr, files, pos


def test_an_interrupted_run_resumes_bit_for_bit_and_consumed_counts_batches(monkeypatch, tmp_path):
    from cosa_amd.utils import torch_helper
    torch_helper.setup_seed(21)
    straight, files, pos_a = _launch(monkeypatch, tmp_path / "a", 6, 2, 100)
    assert not files and pos_a["consumed"] == 12 - 2 * EPOCH
    (tmp_path / "b").mkdir()
    torch_helper.setup_seed(21)
    cut, files, pos_b = _launch(monkeypatch, tmp_path / "b", 4, 2, 2)
    assert sorted(files) == [2, 4]
    h2 = ck.load_trainer(_trainer(monkeypatch, seed=8, accum_steps=2), files[2])
    h4 = ck.load_trainer(_trainer(monkeypatch, seed=8, accum_steps=2), files[4])
    assert h2["loader"]["consumed"] == 4 and h4["loader"]["consumed"] == 8 - EPOCH            # batches, not optimizer steps
    torch_helper.setup_seed(999)                                                            # a new process: other generator states
    resumed, _, pos_c = _launch(monkeypatch, tmp_path / "b", 6, 2, 100, resume=files[4], seed=77)
    assert resumed.train_state().checksums() == straight.train_state().checksums()
    assert resumed.optimizer.global_step == straight.optimizer.global_step == 6 and pos_c["consumed"] == pos_a["consumed"]
    assert cut.train_state().checksums() != straight.train_state().checksums()
    # a state file is written between optimizer steps only
    mid = _trainer(monkeypatch, accum_steps=2)
    mid.step(*_batch(0), n_iter=0)
    with pytest.raises(AssertionError, match="inside an optimizer step"):
        mid.save_state(str(tmp_path / "state_00000001.cosa"), n_iter=0)
