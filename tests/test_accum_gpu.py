"""Gradient accumulation on the GPU: cosa_grad_accumulate through the C ABI on a synthetic record table against the
explicit fp32 torch expression, FusedAdamWEMAStep with an accumulator against a second instance stepped on pre-averaged gradients, and the
trainer: N micro-batches equal one step on the mean of their gradients bit for bit, and one poisoned micro-batch refuses the whole step."""
import functools

import numpy as np
import pytest
import torch

import test_grad_guard_gpu as GG

pytestmark = pytest.mark.gpu

CHUNK = 65536
# the scalar path below one vector (1, 3), one vector (4), scalar with a tail (7), exactly one chunk and one element into the next, a scalar
# multi-chunk tensor, a vector tensor spanning three chunks; NULL_AT: a record without a gradient in the middle
SIZES = (1, 3, 4, 7, CHUNK, 1000, CHUNK + 1, 3 * CHUNK + 5, 2 * CHUNK + 1024)
NULL_AT = 5
PAD = 8                     # floats of poison between the accumulators: a write past a tensor's end lands there
POISON = -1.2345678e-20
INF, NAN = float("inf"), float("nan")
REC = np.dtype([("p", "u8"), ("g", "u8"), ("m", "u8"), ("v", "u8"), ("tp", "u8"), ("p16", "u8"), ("t16", "u8"),
                ("lr", "f4"), ("wd", "f4"), ("n", "i8"), ("t16_f16", "i4"), ("p16_f16", "i4")])


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same_bits(a, b, what=""):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


@functools.lru_cache(maxsize=None)
def _micro_grads():
    """four micro-steps of host gradients for SIZES, with inf, -inf and NaN planted where the sums meet them in different ways"""
    g = torch.Generator().manual_seed(13)
    out = [[torch.randn(n, generator=g) * 0.01 for n in SIZES] for _ in range(4)]
    out[0][4][CHUNK - 1] = INF                           # last element of a full chunk, first micro-step
    out[1][6][CHUNK] = -INF                              # the one scalar element of a second chunk, second micro-step
    out[1][7][3 * CHUNK + 4] = NAN                       # last element of the scalar multi-chunk tensor
    out[0][8][CHUNK + 7], out[1][8][CHUNK + 7] = INF, -INF       # inf + -inf = NaN
    out[0][8][5], out[1][8][5] = 3.0e38, 3.0e38          # finite + finite = inf
    out[1][0][0] = NAN
    return out


class _Table:
    """gradient buffers, a poisoned accumulator arena and the record table / chunk list / pointer array the kernel reads"""

    def __init__(self):
        from cosa_amd import _C
        L = _C.lib()
        assert REC.itemsize == L.cosa_optim_record_bytes() and L.cosa_optim_chunk_elems() == CHUNK
        self.dev = dev = torch.device("cuda", 0)
        self.g = [torch.empty(n, device=dev) for n in SIZES]
        offs, total = [], PAD
        for n in SIZES:
            offs.append(total)
            total += (n + 3) // 4 * 4 + PAD
        self.arena = torch.full((total,), POISON, device=dev)
        self.acc = [self.arena[o:o + n] for o, n in zip(offs, SIZES)]
        self.mask = torch.zeros(total, dtype=torch.bool, device=dev)            # what the kernel may write
        for i, (o, n) in enumerate(zip(offs, SIZES)):
            if i != NULL_AT:
                self.mask[o:o + n] = True
        rec = np.zeros(len(SIZES), REC)
        chunks = []
        for i, n in enumerate(SIZES):
            rec[i]["g"] = 0 if i == NULL_AT else self.g[i].data_ptr()
            rec[i]["n"] = n
            chunks += [(i, c) for c in range((n + CHUNK - 1) // CHUNK)]
        self.n_chunks = len(chunks)
        self.d_rec = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        self.d_chunks = torch.tensor(chunks, dtype=torch.int32, device=dev).contiguous()
        self.d_ptrs = torch.tensor([a.data_ptr() for a in self.acc], dtype=torch.int64, device=dev)
        assert all(a.data_ptr() % 16 == 0 for a in self.acc)

    def call(self, mode, scale, records=True, chunks=True, ptrs=True, n_chunks=None):
        from cosa_amd import _C
        return _C.lib().cosa_grad_accumulate(_C.ptr(self.d_rec) if records else None, _C.ptr(self.d_chunks) if chunks else None,
                                             self.n_chunks if n_chunks is None else n_chunks, _C.ptr(self.d_ptrs) if ptrs else None,
                                             mode, scale, _C.stream_ptr())


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4])
def test_kernel_equals_the_fp32_torch_expression_bit_for_bit(n):
    from cosa_amd import _C
    from cosa_amd.utils import torch_helper
    host = _micro_grads()
    t = _Table()
    scale = torch_helper.accum_scale(n)
    assert scale == float(np.float32(1.0) / np.float32(n))
    for k in range(n):
        for i, g in enumerate(t.g):
            g.copy_(host[k][i])
        t.g[NULL_AT].fill_(NAN)                          # whatever lies in "its" buffer: the record has g == NULL
        _C.check(t.call(torch_helper.accum_mode(k, n), scale), "cosa_grad_accumulate")
        for i, g in enumerate(t.g):
            if i != NULL_AT:
                _same_bits(g.cpu(), host[k][i], ("gradient buffer written", k, i))
    s32 = torch.tensor(np.float32(1.0) / np.float32(n), device=t.dev)
    for i in range(len(SIZES)):
        if i == NULL_AT:
            continue
        want = host[0][i].to(t.dev)
        for k in range(1, n):
            want = want + host[k][i].to(t.dev)
        want = want * s32
        got = t.acc[i]
        assert torch.equal(torch.isnan(got), torch.isnan(want)), i
        ok = ~torch.isnan(want)
        assert torch.equal(_bits(got)[ok], _bits(want)[ok]), (n, i, SIZES[i])
    # IEEE: inf stays inf, inf + -inf and anything + NaN are NaN, an overflowing sum is inf
    assert float(t.acc[4][CHUNK - 1]) == INF and float(t.acc[6][CHUNK]) == -INF and float(t.acc[8][5]) == INF
    assert all(bool(torch.isnan(x)) for x in (t.acc[7][3 * CHUNK + 4], t.acc[8][CHUNK + 7], t.acc[0][0]))
    assert bool(torch.isfinite(t.acc[8][:5]).all()) and bool(torch.isfinite(t.acc[7][:3 * CHUNK + 4]).all())
    # the record without a gradient, and every byte between the accumulators, stay as poisoned
    untouched = t.arena[~t.mask]
    assert untouched.numel() >= 1000 + PAD * (len(SIZES) + 1)
    _same_bits(untouched, torch.full_like(untouched, POISON), "a byte outside the accumulators was written")


def test_kernel_bad_arguments_return_a_status_and_write_nothing():
    from cosa_amd import _C
    L = _C.lib()
    t = _Table()
    for g in t.g:
        g.fill_(1.0)
    for kw, word in ((dict(mode=0, scale=0.5, records=False), b"null"), (dict(mode=0, scale=0.5, chunks=False), b"null"),
                     (dict(mode=0, scale=0.5, ptrs=False), b"null"), (dict(mode=0, scale=0.5, n_chunks=0), b"chunks"),
                     (dict(mode=0, scale=0.5, n_chunks=-3), b"chunks"), (dict(mode=3, scale=0.5), b"mode 3"), (dict(mode=-1, scale=0.5), b"mode -1"),
                     (dict(mode=2, scale=NAN), b"scale"), (dict(mode=2, scale=INF), b"scale"), (dict(mode=0, scale=-INF), b"scale")):
        rc = t.call(**kw)
        assert rc != 0 and word in L.cosa_last_error(), (kw, L.cosa_last_error())
    with pytest.raises(_C.CosaError, match="scale"):
        _C.check(rc, "cosa_grad_accumulate")
    torch.cuda.synchronize()
    _same_bits(t.arena, torch.full_like(t.arena, POISON), "a refused call wrote")
    _C.check(t.call(0, 0.5), "cosa_grad_accumulate")      # ... and the same table is accepted
    assert float(t.acc[8].sum()) == SIZES[8]


# ---- 2. FusedAdamWEMAStep ------------------------------------------------------------------------------------------------------------------------
P_SIZES = (1, 3, 4, 7, CHUNK, CHUNK + 1, 3 * CHUNK + 5, 2 * CHUNK + 1024)
FROZEN = 1000


def _fused(accum_steps, **kw):
    """a small parameter set (two groups, one frozen tensor in no group), its teacher, PolyWarmupAdamW and the fused step over them"""
    from cosa_amd.utils import torch_helper
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7)
    student = [torch.nn.Parameter(torch.randn(n, generator=g).to(dev)) for n in P_SIZES + (FROZEN,)]
    student[-1].requires_grad = False
    teacher = [torch.randn(p.shape, generator=g).to(dev) for p in student]
    opt = torch_helper.PolyWarmupAdamW([{"params": student[:4], "lr": 1e-2, "weight_decay": 1e-2}, {"params": student[4:-1], "lr": 1e-1, "weight_decay": 0.0}],
                                       lr=1e-2, weight_decay=1e-2, betas=(0.9, 0.999), warmup_iter=2, max_iter=50, warmup_ratio=1e-6, power=0.9)
    if accum_steps is not None:
        kw["accum_steps"] = accum_steps
    return student, teacher, opt, torch_helper.FusedAdamWEMAStep(opt, student, teacher, 0.9, **kw)


def _round_grads(rnd, k):
    g = torch.Generator().manual_seed(1000 + 10 * rnd + k)
    return [torch.randn(n, generator=g) * 0.01 for n in P_SIZES]


def _snapshot(student, teacher, opt):
    out = [p.detach().clone() for p in student] + [t.clone() for t in teacher]
    for p in student[:-1]:
        out += [opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()]
    return out


@pytest.mark.parametrize("config", ["plain", "guard", "tensor_stats"])
def test_fused_step_with_an_accumulator_equals_a_step_on_pre_averaged_gradients(config):
    from cosa_amd.utils import torch_helper
    kw = {"plain": {}, "guard": dict(max_norm=0.05, skip_nonfinite=True),
          "tensor_stats": dict(tensor_stats=True, max_norm=0.05, skip_nonfinite=True)}[config]
    sa, ta, oa, fa = _fused(2, **kw)
    sb, tb, ob, fb = _fused(1, **kw)
    sc, tc, oc, fc = _fused(None, **kw)                 # built without the argument
    dev = sa[0].device
    assert fb.acc is None and fb.acc_slices is None and fb.d_acc_ptrs is None and fc.acc is None and fc.accum_steps == 1
    assert fa.acc.dtype == torch.float32 and fa.acc_slices[-1] is None and all(a.data_ptr() % 16 == 0 for a in fa.acc_slices[:-1])
    assert [a.numel() for a in fa.acc_slices[:-1]] == list(P_SIZES) and fa.acc.numel() == sum((n + 3) // 4 * 4 for n in P_SIZES)
    assert fa.d_acc_ptrs.tolist() == [a.data_ptr() for a in fa.acc_slices[:-1]] + [0]
    with pytest.raises(RuntimeError, match="accum_steps=1"):
        fb.accumulate(0)
    half = torch.tensor(0.5, device=dev)
    for rnd in range(2):
        g1, g2 = ([g.to(dev) for g in _round_grads(rnd, k)] for k in range(2))
        before = _snapshot(sa, ta, oa)
        for k, gs in enumerate((g1, g2)):
            for p, g in zip(sa, gs):
                p.grad = g.clone()
            fa.accumulate(k)
            for p, g in zip(sa, gs):
                _same_bits(p.grad, g, "accumulate wrote a gradient")
            if k == 0:
                with pytest.raises(RuntimeError, match="1 of 2 micro-steps"):
                    fa.step()
        for x, y in zip(_snapshot(sa, ta, oa), before):
            _same_bits(x, y, "accumulate moved a weight")
        for p in sa:
            p.grad = None                                # step() reads the accumulator, not p.grad
        for s_, gs_ in ((sb, (g1, g2)), (sc, (g1, g2))):
            for p, x, y in zip(s_, *gs_):
                p.grad = (x + y) * half
        if config == "tensor_stats" and rnd == 1:
            fa.arm(), fb.arm(), fc.arm()
        fa.step(), fb.step(), fc.step()
        for other, name in (((sb, tb, ob), "accum_steps=1"), ((sc, tc, oc), "default")):
            for x, y in zip(_snapshot(sa, ta, oa), _snapshot(*other)):
                _same_bits(x, y, (name, rnd))
        if config != "plain":
            _same_bits(torch_helper.guard_norm(fa.guard).reshape(1), torch_helper.guard_norm(fb.guard).reshape(1), "guard_norm")
            assert torch.equal(fa.guard, fb.guard)
            assert torch_helper.guard_counters(fa.guard) == {"applied": rnd + 1, "skipped": 0, "clipped": rnd + 1}
    assert not torch.equal(sa[6], _fused(1)[0][6])                               # (steps were taken)
    if config == "tensor_stats":
        g_sq = fa.stats_table[:, 0].contiguous().view(torch.float64)                # the sampled gradient is the accumulator's mean
        assert torch.equal(fa.stats_table, fb.stats_table) and bool((g_sq[:-1] > 0).all()) and float(g_sq[-1]) == 0.0
        assert torch.equal(fa.blame, fb.blame)


def test_fused_step_refuses_mixed_none_gradients_and_out_of_order_micro_steps():
    sa, _, _, fa = _fused(3, names=[f"t{i}" for i in range(len(P_SIZES) + 1)])
    gs = [g.to(sa[0].device) for g in _round_grads(0, 0)]
    for p, g in zip(sa, gs):
        p.grad = g
    with pytest.raises(RuntimeError, match="micro-step 0 of 3 is next"):
        fa.accumulate(1)
    fa.accumulate(0)
    sa[2].grad = None
    with pytest.raises(RuntimeError, match=r"^t2: \.grad is None"):
        fa.accumulate(1)
    sa[2].grad = gs[2]
    fa.accumulate(1)
    fa.accumulate(2)
    with pytest.raises(RuntimeError, match="after step"):
        fa.accumulate(0)
    fa.step()
    torch.cuda.synchronize()


# ---- 3. the trainer ------------------------------------------------------------------------------------------------------------------------------
def _trainer(seed=3, **over):
    """tests/test_grad_guard_gpu.py's trainer with the teacher's graph on: the third teacher pass is captured, the following ones replayed"""
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, **over)
    return CoSATrainer(args, torch.device("cuda", 0), seed=seed)


def _batch(tr, k):
    from cosa_amd.train_step import synthetic_batch
    return synthetic_batch(2, 64, 20, tr.device, seed=500 + k)


def test_trainer_two_micro_batches_equal_one_step_on_their_mean_gradient():
    """rests on the step's run-to-run bit reproducibility: A and B run the same forward and backward passes on the same weights"""
    from cosa_amd import nn_ops
    a = _trainer(accum_steps=2)
    b = _trainer(accum_steps=1)
    assert a._fused_step.acc is not None and b._fused_step.acc is None and a.use_graph and b.use_graph
    half = torch.tensor(0.5, device=a.device)
    for rnd in range(2):
        n_iter = a.args.warmup_iters + 1 + rnd
        batches = [_batch(a, 2 * rnd + k) for k in range(2)]
        for k, x in enumerate(batches):
            before = a.optimizer.global_step
            logs = a.step(*x, n_iter=n_iter)
            assert a.optimizer.global_step == before + k and "overall_loss" in logs
        grads = []
        for x in batches:
            loss, _ = b.forward_losses(*x, n_iter)
            b.optimizer.zero_grad(set_to_none=True)
            nn_ops.wgrad_arena_begin(b.device)
            loss.backward()
            grads.append([None if p.grad is None else p.grad.clone() for p in b.student.parameters()])
        for p, g1, g2 in zip(b.student.parameters(), *grads):
            assert (g1 is None) == (g2 is None)
            p.grad = None if g1 is None else (g1 + g2) * half
        b._fused_step.step()
        b._student_shadows.refresh()
        GG._assert_same_state(GG._state(a), GG._state(b))
    assert a._graph is not None and b._graph is not None and a.optimizer.global_step == b.optimizer.global_step == 2
    fresh = _trainer()
    assert any(not torch.equal(p, q) for p, q in zip(a.model_AN.parameters(), fresh.model_AN.parameters()))        # (steps were taken)


def test_trainer_one_poisoned_micro_batch_refuses_the_whole_step():
    tr = _trainer(accum_steps=2, skip_nonfinite=True)
    n_iter = tr.args.warmup_iters + 1
    for k in range(2):
        tr.step(*_batch(tr, k), n_iter=n_iter)
    s1 = GG._state(tr)
    hook = tr.student.classifier.weight.register_hook(lambda g: torch.full_like(g, INF))
    try:
        tr.step(*_batch(tr, 2), n_iter=n_iter + 1)       # micro-batch 0 of the second step arrives with an inf gradient
    finally:
        hook.remove()
    logs = tr.step(*_batch(tr, 3), n_iter=n_iter + 1)
    assert not bool(torch.isfinite(logs["grad_norm"]))
    GG._assert_same_state(GG._state(tr), s1)
    assert tr.guard_counters() == {"applied": 1, "skipped": 1, "clipped": 0} and tr.optimizer.global_step == 2
    for k in range(2):
        tr.step(*_batch(tr, 4 + k), n_iter=n_iter + 2)
    s3 = GG._state(tr)
    assert tr.guard_counters() == {"applied": 2, "skipped": 1, "clipped": 0}
    assert all(bool(torch.isfinite(v.float()).all()) for v in s3.values())
    assert any(not torch.equal(s3[k], s1[k]) for k in s1 if k.startswith("AN.") and ".shadow." not in k)
