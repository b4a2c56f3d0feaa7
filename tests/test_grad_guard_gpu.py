"""The gradient guard on the GPU: the global-norm reduction and the guarded optimizer kernel through the C ABI on a
synthetic parameter set, then the trainer: a guard that never fires changes no bit, a non-finite step is refused as a whole, the fused path
agrees with the torch restatement, and a guarded run resumes bit for bit."""
import functools
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the smallest sizes that reach the vector (n % 4 == 0) and the scalar path, a chunk boundary (65536) from either side, a multi-chunk tensor,
# and -- last -- a frozen tensor (no gradient: EMA only)
SIZES = (1, 3, 4, 65535, 65536, 65537, 200003)
FROZEN = 1000
B1, B2, EPS, EMA, STEP, LR, WD = 0.9, 0.999, 1e-8, 0.9, 3, 1e-3, 1e-2
KEYS = ("p", "m", "v", "tp", "p16", "t16")


def _params(seed=0):
    """host tensors of the synthetic set: masters, gradients, moments (as after two steps), teacher"""
    g = torch.Generator().manual_seed(seed)
    out = {k: [] for k in ("p", "g", "m", "v", "tp")}
    for n in SIZES + (FROZEN,):
        out["p"].append(torch.randn(n, generator=g))
        out["g"].append(torch.randn(n, generator=g) * 0.01)
        out["m"].append(torch.randn(n, generator=g) * 0.002)
        out["v"].append(torch.rand(n, generator=g) * 1e-5 + 1e-8)
        out["tp"].append(torch.randn(n, generator=g))
    return out


class _Set:
    """the set on the device + the record table and chunk list the optimizer kernels read (the layout of include/cosa_hip.h)"""

    def __init__(self, host, frozen_grad_fill=None):
        from cosa_amd import _C
        L = _C.lib()
        dev = torch.device("cuda", 0)
        self.t = {k: [x.to(dev) for x in v] for k, v in host.items()}
        n = len(self.t["p"])
        self.t["p16"] = [p.to(torch.bfloat16) for p in self.t["p"]]
        # the teacher's shadows: fp16 for every other tensor, bf16 for the rest (both store paths of the kernel)
        self.t["t16"] = [tp.to(torch.float16 if i % 2 else torch.bfloat16) for i, tp in enumerate(self.t["tp"])]
        if frozen_grad_fill is not None:
            self.t["g"][-1].fill_(frozen_grad_fill)
        dt = np.dtype([("p", "u8"), ("g", "u8"), ("m", "u8"), ("v", "u8"), ("tp", "u8"), ("p16", "u8"), ("t16", "u8"),
                       ("lr", "f4"), ("wd", "f4"), ("n", "i8"), ("t16_f16", "i4"), ("p16_f16", "i4")])
        assert dt.itemsize == L.cosa_optim_record_bytes()
        rec = np.zeros(n, dt)
        chunk = L.cosa_optim_chunk_elems()
        chunks = []
        for i in range(n):
            frozen = i == n - 1
            rec[i] = (self.t["p"][i].data_ptr(), 0 if frozen else self.t["g"][i].data_ptr(), 0 if frozen else self.t["m"][i].data_ptr(),
                      0 if frozen else self.t["v"][i].data_ptr(), self.t["tp"][i].data_ptr(), self.t["p16"][i].data_ptr(),
                      self.t["t16"][i].data_ptr(), LR * (1 + i), WD, self.t["p"][i].numel(), int(self.t["t16"][i].dtype == torch.float16), 0)
            chunks += [(i, c) for c in range((self.t["p"][i].numel() + chunk - 1) // chunk)]
        self.n_chunks = len(chunks)
        self.d_rec = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        self.d_chunks = torch.tensor(chunks, dtype=torch.int32, device=dev).contiguous()
        self.guard = torch.zeros(5, dtype=torch.int64, device=dev)
        assert L.cosa_grad_guard_bytes() == 40
        self.ws = torch.empty(L.cosa_grad_norm_workspace_bytes(self.n_chunks), dtype=torch.uint8, device=dev)
        assert self.ws.numel() == 8 * self.n_chunks

    def norm(self, max_norm, skip_nonfinite):
        from cosa_amd import _C
        _C.check(_C.lib().cosa_grad_norm(_C.ptr(self.d_rec), _C.ptr(self.d_chunks), self.n_chunks, max_norm, int(skip_nonfinite), _C.ptr(self.ws),
                                         self.ws.numel(), _C.ptr(self.guard), _C.stream_ptr()), "cosa_grad_norm")

    def guarded(self):
        from cosa_amd import _C
        _C.check(_C.lib().cosa_fused_adamw_ema_guarded(_C.ptr(self.d_rec), _C.ptr(self.d_chunks), self.n_chunks, B1, B2, EPS, STEP, EMA,
                                                       _C.ptr(self.guard), _C.stream_ptr()), "cosa_fused_adamw_ema_guarded")

    def unguarded(self):
        from cosa_amd import _C
        _C.check(_C.lib().cosa_fused_adamw_ema(_C.ptr(self.d_rec), _C.ptr(self.d_chunks), self.n_chunks, B1, B2, EPS, STEP, EMA, _C.stream_ptr()),
                 "cosa_fused_adamw_ema")

    def record(self):
        """the guard record on the host: norm, coef, skip, applied, skipped, clipped"""
        g = self.guard.cpu()
        f, i = g.view(torch.float32), g.view(torch.int32)
        return {"norm": float(f[0]), "coef": float(f[1]), "skip": int(i[2]), "applied": int(g[2]), "skipped": int(g[3]), "clipped": int(g[4]),
                "norm_bits": int(i[0])}

    def outputs(self):
        """every buffer the optimizer kernel writes, as bytes on the host"""
        return {k: [x.reshape(-1).view(torch.uint8).cpu() for x in self.t[k]] for k in KEYS}


def _same_bytes(a, b):
    for k in KEYS:
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert torch.equal(x, y), (k, i)


@functools.lru_cache(maxsize=None)
def _host():
    return _params()


@functools.lru_cache(maxsize=None)
def _reference_norm():
    """float64 on the CPU, over the concatenated gradients of the tensors that have one"""
    return float(torch.linalg.vector_norm(torch.cat([g.double() for g in _host()["g"][:-1]])))


# ---- 1. the norm --------------------------------------------------------------------------------------------------------------------------
def test_norm_against_float64_and_run_to_run():
    want = _reference_norm()
    s = _Set(_host())
    s.norm(0.0, False)
    r1 = s.record()
    print("norm", r1["norm"], "float64 reference", want, "relative error", abs(r1["norm"] - want) / want)
    assert r1["norm"] == pytest.approx(want, rel=1e-6)
    assert r1["coef"] == 1.0 and r1["skip"] == 0 and (r1["applied"], r1["skipped"], r1["clipped"]) == (1, 0, 0)
    s.norm(0.0, False)
    r2 = s.record()
    assert r2["norm_bits"] == r1["norm_bits"] and r2["applied"] == 2
    # the frozen tensor's record has g = NULL: whatever lies in "its" gradient buffer, a NaN included, does not move the result
    for fill in (1e30, float("nan")):
        f = _Set(_host(), frozen_grad_fill=fill)
        f.norm(0.0, True)
        rf = f.record()
        assert rf["norm_bits"] == r1["norm_bits"] and rf["skip"] == 0


# ---- 2. a guard that neither clips nor skips is the old kernel ------------------------------------------------------------------------------
def test_inactive_guard_equals_the_unguarded_kernel_bit_for_bit():
    a, b = _Set(_host()), _Set(_host())
    before = a.outputs()
    a.unguarded()
    b.norm(1e9, True)
    b.guarded()
    r = b.record()
    assert r["coef"] == 1.0 and r["skip"] == 0 and (r["applied"], r["skipped"], r["clipped"]) == (1, 0, 0)
    out_a, out_b = a.outputs(), b.outputs()
    _same_bytes(out_a, out_b)
    assert not torch.equal(out_a["p"][6], before["p"][6]) and not torch.equal(out_a["t16"][7], before["t16"][7])      # (a step was taken)
    assert torch.equal(out_a["p16"][7], before["p16"][7])                                                        # frozen: its bf16 copy stays


# ---- 3. clipping ------------------------------------------------------------------------------------------------------------------------------
def test_clipping_against_the_torch_restatement():
    """g * coef, then torch's AdamW and ema_update -- what tests/test_network_gpu.py::test_fused_adamw_ema_step_vs_torch compares the
    unguarded kernel with, at its tolerance (rtol 2e-5, atol 1e-7)"""
    from cosa_amd.utils import torch_helper
    host = _host()
    max_norm = 0.5 * _reference_norm()
    s = _Set(host)
    g_before = [g.clone() for g in s.t["g"]]
    s.norm(max_norm, True)
    s.guarded()
    r = s.record()
    coef = np.float32(max_norm) / (np.float32(r["norm"]) + np.float32(1e-6))
    print("coef", r["coef"], "restated", float(coef))
    assert r["coef"] == pytest.approx(float(coef), rel=2e-7) and 0.49 < r["coef"] < 0.51
    assert r["skip"] == 0 and (r["applied"], r["skipped"], r["clipped"]) == (1, 0, 1)
    for a, b in zip(s.t["g"], g_before):
        assert torch.equal(a, b)                                                  # the gradients are only read
    n = len(SIZES)
    ps = [torch.nn.Parameter(p.clone()) for p in host["p"]]
    tps = [t.clone() for t in host["tp"]]
    opt = torch.optim.AdamW([{"params": [ps[i]], "lr": float(np.float32(LR * (1 + i))), "weight_decay": WD} for i in range(n)], betas=(B1, B2), eps=EPS,
                            foreach=False)
    for i in range(n):
        ps[i].grad = host["g"][i] * float(r["coef"])
        opt.state[ps[i]] = {"step": torch.tensor(float(STEP - 1)), "exp_avg": host["m"][i].clone(), "exp_avg_sq": host["v"][i].clone()}
    opt.step()
    torch_helper.ema_update(tps, ps, EMA)
    worst = {}
    for i in range(n + 1):
        pairs = [("p", ps[i].detach()), ("tp", tps[i])]
        if i < n:
            pairs += [("m", opt.state[ps[i]]["exp_avg"]), ("v", opt.state[ps[i]]["exp_avg_sq"])]
        for k, ref in pairs:
            got = s.t[k][i].cpu()
            worst[k] = max(worst.get(k, 0.0), float(((got - ref).abs() / (1e-7 / 2e-5 + ref.abs())).max()))
            assert torch.allclose(got, ref, rtol=2e-5, atol=1e-7), (k, i, (got - ref).abs().max().item())
    print("largest |got - ref| / (atol/rtol + |ref|) per buffer (bar 2e-5):", worst)
    for i in range(n + 1):                                                        # the shadows are casts of the masters just written
        if i < n:
            assert torch.equal(s.t["p16"][i], s.t["p"][i].to(torch.bfloat16))
        assert torch.equal(s.t["t16"][i], s.t["tp"][i].to(s.t["t16"][i].dtype))


# ---- 4. skipping ------------------------------------------------------------------------------------------------------------------------------
PLACEMENTS = {"inf_last_of_last_chunk": (6, 200003 - 1, float("inf")),       # the 200 003 tensor's last element: the end of its fourth chunk
              "nan_in_scalar_tail": (5, 65536, float("nan")),                # the 65 537 tensor's second chunk is one scalar-path element
              "neg_inf_single_element": (0, 0, float("-inf"))}


@pytest.mark.parametrize("case", list(PLACEMENTS))
def test_one_nonfinite_element_refuses_the_whole_step(case):
    tensor, index, value = PLACEMENTS[case]
    s = _Set(_host())
    s.t["g"][tensor][index] = value
    before = s.outputs()
    s.norm(0.0, True)
    s.guarded()
    r = s.record()
    assert r["skip"] == 1 and (r["applied"], r["skipped"], r["clipped"]) == (0, 1, 0) and not math.isfinite(r["norm"])
    _same_bytes(s.outputs(), before)
    # the switch is what protects: the same inputs with skip_nonfinite off are applied, and poison the tensor
    u = _Set(_host())
    u.t["g"][tensor][index] = value
    u.norm(0.0, False)
    u.guarded()
    ru = u.record()
    assert ru["skip"] == 0 and (ru["applied"], ru["skipped"]) == (1, 0)
    assert not bool(torch.isfinite(u.t["p"][tensor]).all()) and not bool(torch.isfinite(u.t["tp"][tensor]).all())
    assert not torch.equal(u.outputs()["p"][4], before["p"][4])                   # ... and every other tensor took its step


# ---- 5. bad arguments -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_an_error_with_a_message():
    from cosa_amd import _C
    L = _C.lib()
    s = _Set(_host())
    before = s.outputs()
    rc = L.cosa_grad_norm(_C.ptr(s.d_rec), _C.ptr(s.d_chunks), s.n_chunks, 1.0, 1, _C.ptr(s.ws), s.ws.numel(), None, _C.stream_ptr())
    assert rc != 0 and b"null guard" in L.cosa_last_error()
    rc = L.cosa_grad_norm(_C.ptr(s.d_rec), _C.ptr(s.d_chunks), s.n_chunks, 1.0, 1, _C.ptr(s.ws), s.ws.numel() - 1, _C.ptr(s.guard), _C.stream_ptr())
    assert rc != 0 and b"workspace" in L.cosa_last_error() and str(s.ws.numel()).encode() in L.cosa_last_error()
    rc = L.cosa_grad_norm(_C.ptr(s.d_rec), _C.ptr(s.d_chunks), s.n_chunks, -1.0, 1, _C.ptr(s.ws), s.ws.numel(), _C.ptr(s.guard), _C.stream_ptr())
    assert rc != 0 and b"max_norm" in L.cosa_last_error()
    rc = L.cosa_fused_adamw_ema_guarded(_C.ptr(s.d_rec), _C.ptr(s.d_chunks), s.n_chunks, B1, B2, EPS, STEP, EMA, None, _C.stream_ptr())
    assert rc != 0 and b"null guard" in L.cosa_last_error()
    with pytest.raises(_C.CosaError, match="null guard"):
        _C.check(rc, "cosa_fused_adamw_ema_guarded")
    _same_bytes(s.outputs(), before)                                              # nothing was launched
    assert int(s.guard.abs().sum()) == 0


# ---- the trainer ------------------------------------------------------------------------------------------------------------------------------
def _trainer(seed=3, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, teacher_graph=False, teacher_async=False, **over)
    return CoSATrainer(args, torch.device("cuda", 0), seed=seed)


def _step(tr, k, poison=False):
    """step k of the fixed batch sequence; poison: classifier.weight's gradient arrives as inf (arithmetic, through a tensor hook)"""
    from cosa_amd.train_step import synthetic_batch
    batch = synthetic_batch(2, 64, 20, tr.device, seed=500 + k)
    hook = tr.student.classifier.weight.register_hook(lambda g: torch.full_like(g, float("inf"))) if poison else None
    try:
        return tr.step(*batch, n_iter=tr.args.warmup_iters + k)
    finally:
        if hook is not None:
            hook.remove()


def _state(tr):
    """clones of everything a step writes: masters of both networks, moments, 16-bit shadows, W^T copies"""
    out = {}
    for tag, net in (("ON", tr.student), ("AN", tr.model_AN)):
        for n, p in net.named_parameters():
            out[f"{tag}.{n}"] = p.detach().clone()
    names = {id(p): n for n, p in tr.student.named_parameters()}
    for p, st in tr.optimizer.state.items():
        for k in ("exp_avg", "exp_avg_sq"):
            out[f"opt.{names[id(p)]}.{k}"] = st[k].clone()
    for tag, sh in (("ON", tr._student_shadows), ("AN", tr._teacher_shadows)):
        for i, s16 in enumerate(sh.shadows):
            out[f"{tag}.shadow.{i}"] = s16.clone()
        for i, t in enumerate(sh.t16):
            out[f"{tag}.wT.{i}"] = t.clone()
    return out


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k


@functools.lru_cache(maxsize=None)
def _never_firing_run():
    """two steps behind a guard that never fires -> (state, first step's norm, counters)"""
    tr = _trainer(clip_grad_norm=1e9, skip_nonfinite=True)
    norm1 = _step(tr, 1)["grad_norm"]
    logs = _step(tr, 2)
    assert logs["grad_norm"].is_cuda and logs["grad_norm"].dim() == 0
    return _state(tr), float(norm1), tr.guard_counters()


@functools.lru_cache(maxsize=None)
def _refused_run():
    """three steps, the second poisoned, behind the guard -> (state after 1, after 2, after 3, counters, checksums of the full state)"""
    tr = _trainer(skip_nonfinite=True)
    _step(tr, 1)
    s1 = _state(tr)
    logs = _step(tr, 2, poison=True)
    s2 = _state(tr)
    norm2 = float(logs["grad_norm"])
    _step(tr, 3)
    return s1, s2, _state(tr), tr.guard_counters(), tr.train_state().checksums(), norm2


# ---- 6. ----
def test_a_guard_that_never_fires_changes_no_bit():
    guarded, norm1, counters = _never_firing_run()
    tr = _trainer()
    assert tr.guard_state is None and tr.guard_counters() is None
    logs = _step(tr, 1)
    assert "grad_norm" not in logs
    _step(tr, 2)
    _assert_same_state(_state(tr), guarded)
    assert counters == {"applied": 2, "skipped": 0, "clipped": 0} and math.isfinite(norm1) and norm1 > 0


# ---- 7. ----
def test_a_nonfinite_step_is_refused_as_a_whole():
    s1, s2, s3, counters, _, norm2 = _refused_run()
    assert not math.isfinite(norm2)
    _assert_same_state(s2, s1)
    assert any(not torch.equal(s3[k], s1[k]) for k in s1 if k.startswith("AN.") and ".shadow." not in k)
    assert all(bool(torch.isfinite(v.float()).all()) for v in s3.values())
    assert counters == {"applied": 2, "skipped": 1, "clipped": 0}
    # the same scenario with the guard off: the teacher is gone
    tr = _trainer()
    _step(tr, 1)
    _step(tr, 2, poison=True)
    assert not all(bool(torch.isfinite(p).all()) for p in tr.model_AN.parameters())


# ---- 8. ----
def test_fused_equals_non_fused_under_clipping():
    """One step of both paths from the same weights and batch, clipped to half the norm that step reports.  The bar is the one of
    tests/test_network_gpu.py::test_fused_adamw_ema_step_vs_torch (rtol 2e-5, atol 1e-7), which also compares the two optimizers on the same
    gradients: a second step would compare two forward passes on weights that differ in their last bits instead."""
    _, norm1, _ = _never_firing_run()
    runs = []
    for fused in (True, False):
        tr = _trainer(clip_grad_norm=0.5 * norm1, skip_nonfinite=True, fused_optimizer=fused)
        assert (tr._fused_step is not None) == fused
        logs = _step(tr, 1)
        assert float(logs["grad_norm"]) == pytest.approx(norm1, rel=1e-6)
        assert tr.guard_counters() == {"applied": 1, "skipped": 0, "clipped": 1}
        coef = float(tr.guard_state.view(torch.float32)[1])
        assert coef == pytest.approx(0.5 * norm1 / (norm1 + 1e-6), rel=1e-5) and coef < 0.51
        runs.append({k: v for k, v in _state(tr).items() if ".shadow." not in k and ".wT." not in k})
    a, b = runs
    assert a.keys() == b.keys() and any(k.startswith("opt.") for k in a)
    for k in a:
        assert torch.allclose(a[k], b[k], rtol=2e-5, atol=1e-7), (k, (a[k] - b[k]).abs().max().item())


# ---- 9. ----
def test_a_guarded_run_resumes_bit_for_bit(tmp_path, capsys):
    _, _, s3, counters_a, sums_a, _ = _refused_run()
    path, plain = str(tmp_path / "state_00000002.cosa"), str(tmp_path / "state_00000000.cosa")
    b = _trainer(skip_nonfinite=True)
    _step(b, 1)
    _step(b, 2, poison=True)
    b.save_state(path, n_iter=1)
    b.wait_state()
    del b
    d = _trainer(seed=5)                                                         # no guard: its file has no guard entry
    d.save_state(plain, n_iter=-1)
    d.wait_state()
    try:
        c = _trainer(seed=77, skip_nonfinite=True)                                # another seed: nothing of C's own survives the load
        extra = c.load_state(path)
        assert extra["n_iter"] == 1 and c.optimizer.global_step == 2
        assert c.guard_counters() == {"applied": 1, "skipped": 1, "clipped": 0}
        _step(c, 3)
        assert c.train_state().checksums() == sums_a
        assert c.guard_counters() == counters_a
        _assert_same_state(_state(c), s3)
        # a file written without a guard loads into a guarded trainer: the counters start at zero
        capsys.readouterr()
        c.load_state(plain)
        assert "counters start at zero" in capsys.readouterr().out
        assert c.guard_counters() == {"applied": 0, "skipped": 0, "clipped": 0} and int(c.guard_state.abs().sum()) == 0
        for (n, p), (_, q) in zip(c.student.named_parameters(), d.student.named_parameters()):
            assert torch.equal(p, q), n
        # ... and a file written with a guard into a trainer without one: the entry is ignored with a note
        d.load_state(path)
        assert "ignored" in capsys.readouterr().out
        assert d.guard_state is None and d.optimizer.global_step == 2
    finally:
        for p in (path, plain):
            if os.path.exists(p):
                os.remove(p)
