"""Per-tensor training diagnostics on the GPU: cosa_tensor_stats and cosa_grad_blame through the C ABI on a
hand-made record table against the numpy float64 yardstick (tests/tensor_stats_ref.py), then the trainer: the flag changes no bit of a
step, a sample equals the torch restatement, a planted inf is blamed on its tensor, and the blame counters resume with the run."""
import functools
import os

import numpy as np
import pytest
import torch

import tensor_stats_ref as R

pytestmark = pytest.mark.gpu

# the scalar path (1, 3), the float4 path (4), the chunk boundary of 65536 from either side, a one-element tail chunk (65537), three chunks
# on the float4 path (131076) and on the scalar path (2 * 65536 + 1)
SIZES = (1, 3, 4, 65535, 65536, 65537, 131076, 2 * 65536 + 1)
FROZEN = 3                                   # the index of the tensor without a gradient (65535 elements)
CHUNK = 65536
SENTINEL = 0x5A
PAD = 256                                    # sentinel bytes on either side of out, the workspace and blame
REC = np.dtype([("p", "u8"), ("g", "u8"), ("m", "u8"), ("v", "u8"), ("tp", "u8"), ("p16", "u8"), ("t16", "u8"),
                ("lr", "f4"), ("wd", "f4"), ("n", "i8"), ("t16_f16", "i4"), ("p16_f16", "i4")])
# what gets planted: (buffer, tensor index, element, value)
PLANTS = (("g", 1, 2, float("inf")),         # the last element of the size-3 tensor's gradient
          ("g", 5, 65536, float("nan")),     # the first element of the size-65537 tensor's second chunk
          ("tp", 6, 70001, float("-inf")))   # one teacher element of the 131076 tensor
KEYS = ("p", "g", "tp", "m", "v")


@functools.lru_cache(maxsize=None)
def _host():
    """seeded normal values, scaled per tensor from 1e-6 to 1e3"""
    g = torch.Generator().manual_seed(12)
    scales = np.logspace(-6, 3, len(SIZES))
    out = {k: [] for k in KEYS}
    for n, s in zip(SIZES, scales):
        out["p"].append(torch.randn(n, generator=g) * float(s))
        out["g"].append(torch.randn(n, generator=g) * float(s))
        out["tp"].append(out["p"][-1] + torch.randn(n, generator=g) * float(s) * 0.01)
        out["m"].append(torch.randn(n, generator=g))
        out["v"].append(torch.rand(n, generator=g))
    return out


def _padded(nbytes, dev):
    """(whole buffer filled with the sentinel, the 8-byte aligned view of nbytes in its middle)"""
    whole = torch.full((nbytes + 2 * PAD,), SENTINEL, dtype=torch.uint8, device=dev)
    return whole, whole[PAD:PAD + nbytes]


def _pads_intact(whole):
    return bool((whole[:PAD] == SENTINEL).all()) and bool((whole[-PAD:] == SENTINEL).all())


class _Set:
    """the tensors on the device, the record table and chunk list of the optimizer kernels (include/cosa_hip.h), first_chunk, and the
    outputs of both calls between sentinels"""

    def __init__(self, plants=()):
        from cosa_amd import _C
        L = _C.lib()
        dev = torch.device("cuda", 0)
        self.t = {k: [x.clone().to(dev) for x in v] for k, v in _host().items()}
        for key, i, e, val in plants:
            self.t[key][i][e] = val
        T = len(SIZES)
        assert REC.itemsize == L.cosa_optim_record_bytes() and L.cosa_optim_chunk_elems() == CHUNK
        rec = np.zeros(T, REC)
        chunks, first = [], []
        for i in range(T):
            frozen = i == FROZEN
            rec[i] = (self.t["p"][i].data_ptr(), 0 if frozen else self.t["g"][i].data_ptr(), 0 if frozen else self.t["m"][i].data_ptr(),
                      0 if frozen else self.t["v"][i].data_ptr(), self.t["tp"][i].data_ptr(), 0, 0, 1e-3, 1e-2, SIZES[i], 0, 0)
            first.append(len(chunks))
            chunks += [(i, c) for c in range((SIZES[i] + CHUNK - 1) // CHUNK)]
        self.T, self.n_chunks, self.first = T, len(chunks), first + [len(chunks)]
        assert self.n_chunks == 13
        self.d_rec = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        self.d_chunks = torch.tensor(chunks, dtype=torch.int32, device=dev).contiguous()
        self.d_first = torch.tensor(self.first, dtype=torch.int32, device=dev)
        assert L.cosa_tensor_stats_workspace_bytes(self.n_chunks) == 48 * self.n_chunks
        self.out_whole, self.out = _padded(48 * T, dev)
        self.ws_whole, self.ws = _padded(48 * self.n_chunks, dev)
        self.blame_whole, self.blame = _padded(8 * T, dev)
        self.blame.zero_()
        self.guard = torch.zeros(5, dtype=torch.int64, device=dev)
        self.norm_ws = torch.zeros(L.cosa_grad_norm_workspace_bytes(self.n_chunks), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()

    def call(self, **over):
        """the raw C call -> status; `over` replaces arguments by name"""
        from cosa_amd import _C
        a = dict(records=_C.ptr(self.d_rec), chunks=_C.ptr(self.d_chunks), first_chunk=_C.ptr(self.d_first), n_tensors=self.T,
                 n_chunks=self.n_chunks, workspace=_C.ptr(self.ws), workspace_bytes=self.ws.numel(), out=_C.ptr(self.out))
        a.update(over)
        return _C.lib().cosa_tensor_stats(a["records"], a["chunks"], a["first_chunk"], a["n_tensors"], a["n_chunks"], a["workspace"],
                                          a["workspace_bytes"], a["out"], _C.stream_ptr())

    def stats(self):
        """-> the table as raw int64 [T, 6] on the host"""
        from cosa_amd import _C
        _C.check(self.call(), "cosa_tensor_stats")
        return self.out.cpu().numpy().view(np.int64).reshape(self.T, 6).copy()

    def norm_partials(self):
        """cosa_grad_norm on the same table -> its per-chunk partials as float64 on the host"""
        from cosa_amd import _C
        _C.check(_C.lib().cosa_grad_norm(_C.ptr(self.d_rec), _C.ptr(self.d_chunks), self.n_chunks, 0.0, 1, _C.ptr(self.norm_ws),
                                         self.norm_ws.numel(), _C.ptr(self.guard), _C.stream_ptr()), "cosa_grad_norm")
        return self.norm_ws.cpu().numpy().view(np.float64).copy()

    def blame_once(self):
        from cosa_amd import _C
        _C.check(_C.lib().cosa_grad_blame(_C.ptr(self.norm_ws), _C.ptr(self.d_first), self.T, self.n_chunks, _C.ptr(self.blame),
                                          _C.stream_ptr()), "cosa_grad_blame")
        return self.blame.cpu().numpy().view(np.int64).copy()

    def inputs(self):
        return {k: [x.view(torch.uint8).cpu() for x in self.t[k]] for k in KEYS}

    def reference(self):
        """the numpy float64 rows of what the buffers hold"""
        h = {k: [x.cpu().numpy() for x in self.t[k]] for k in ("p", "g", "tp")}
        return R.table(h["p"], h["tp"], [None if i == FROZEN else g for i, g in enumerate(h["g"])])


@functools.lru_cache(maxsize=None)
def _plain():
    """the unplanted set, run once -> (set, raw table, reference rows)"""
    s = _Set()
    before = s.inputs()
    raw = s.stats()
    return s, raw, s.reference(), before


def _assert_rows(raw, want, only=None):
    got = R.decode(raw)
    for i in range(len(SIZES)) if only is None else only:
        for k in range(3):
            err = abs(got[i, k] - want[i][k]) / want[i][k] if want[i][k] else abs(got[i, k])
            print(f"tensor {i} (n = {SIZES[i]}) {R.SLOTS[k]}: relative error {err:.3e}, bound {R.sum_bound(SIZES[i]):.3e}")
            assert err <= R.sum_bound(SIZES[i]), (i, R.SLOTS[k], got[i, k], want[i][k])
        assert got[i, 3] == want[i][3] and raw[i, 4] == want[i][4] and raw[i, 5] == want[i][5], (i, got[i], want[i])


# ---- 1. ----
def test_sums_maxima_and_counts_against_float64():
    s, raw, want, _ = _plain()
    _assert_rows(raw, want)
    got = R.decode(raw)
    assert tuple(got[FROZEN, [0, 3, 4]]) == (0.0, 0.0, 0.0) and got[FROZEN, 1] > 0 and got[FROZEN, 2] > 0      # frozen: weights only
    assert all(got[i, 0] > 0 and got[i, 3] > 0 for i in range(len(SIZES)) if i != FROZEN) and not raw[:, 4:].any()
    assert got[0, 3] == abs(float(_host()["g"][0][0]))                                                       # the one-element tensor


# ---- 2. ----
def test_g_sq_is_the_index_order_sum_of_the_guards_partials_bit_for_bit():
    s, raw, _, _ = _plain()
    partials = s.norm_partials()
    assert partials.shape == (s.n_chunks,) and np.isfinite(partials).all()
    for i in range(s.T):
        acc = np.float64(0.0)
        for c in range(s.first[i], s.first[i + 1]):
            acc = acc + partials[c]
        assert np.float64(acc).view(np.int64) == raw[i, 0], (i, acc, raw[i, :1].view(np.float64))
    assert s.first[7 + 1] - s.first[7] == 3 and s.first[5 + 1] - s.first[5] == 2


# ---- 3. ----
def test_planted_nonfinite_values_are_counted_left_out_and_blamed():
    _, plain_raw, _, _ = _plain()
    s = _Set(PLANTS)
    raw = s.stats()
    want = s.reference()
    assert [want[1][4], want[5][4], want[6][5]] == [1, 1, 1] and sum(r[4] + r[5] for r in want) == 3
    _assert_rows(raw, want)                                           # counts exact; the sums over the finite elements keep the bound
    assert np.isfinite(R.decode(raw)).all()
    touched = {i for _, i, _, _ in PLANTS}
    for i in range(s.T):
        if i not in touched:
            assert np.array_equal(raw[i], plain_raw[i]), i              # every other tensor's row: the bits of the unplanted run
    assert raw[6, 0] == plain_raw[6, 0] and raw[6, 1] == plain_raw[6, 1]      # a planted teacher element leaves g_sq and w_sq alone
    partials = s.norm_partials()
    bad = [c for c in range(s.n_chunks) if not np.isfinite(partials[c])]
    assert bad == [s.first[1], s.first[5] + 1]
    assert s.blame_once().tolist() == [0, 1, 0, 0, 0, 1, 0, 0]
    assert s.blame_once().tolist() == [0, 2, 0, 0, 0, 2, 0, 0]
    assert _pads_intact(s.blame_whole) and _pads_intact(s.out_whole) and _pads_intact(s.ws_whole)
    # finite gradients: nothing is blamed
    p, _, _, _ = _plain()
    p.norm_partials()
    assert not p.blame_once().any()


# ---- 4. ----
def test_same_bytes_from_run_to_run_sentinels_and_inputs_untouched():
    s, raw, _, before = _plain()
    again = s.stats()
    assert np.array_equal(raw, again)
    other = _Set()                                                    # other allocations, the same values
    assert np.array_equal(other.stats(), raw)
    for whole in (s.out_whole, s.ws_whole, s.blame_whole, other.out_whole, other.ws_whole):
        assert _pads_intact(whole)
    after = s.inputs()
    for k in KEYS:
        for i, (x, y) in enumerate(zip(before[k], after[k])):
            assert torch.equal(x, y), (k, i)


def test_refused_arguments_return_a_status_and_leave_out_untouched():
    from cosa_amd import _C
    L = _C.lib()
    s = _Set()
    dev = s.d_rec.device
    s.out.fill_(0x33)
    bad_first = {"not monotone": [0, 1, 2, 3, 5, 4, 6, 9, 13], "ends at": [0, 1, 2, 3, 4, 5, 7, 10, 12], "must be 0": [1, 1, 2, 3, 4, 5, 7, 10, 13]}
    cases = [(dict(records=None), b"null"), (dict(chunks=None), b"null"), (dict(first_chunk=None), b"null"), (dict(out=None), b"null"),
             (dict(workspace=None), b"workspace"), (dict(workspace_bytes=s.ws.numel() - 1), b"workspace"),
             (dict(n_tensors=0), b"positive"), (dict(n_tensors=-1), b"positive"), (dict(n_chunks=0), b"positive"),
             (dict(n_tensors=s.T - 1), b"ends at"), (dict(n_chunks=s.n_chunks - 1, workspace_bytes=s.ws.numel()), b"ends at")]
    keep = []
    for word, fc in bad_first.items():
        assert len(fc) == s.T + 1
        keep.append(torch.tensor(fc, dtype=torch.int32, device=dev))
        cases.append((dict(first_chunk=_C.ptr(keep[-1])), word.encode()))
    torch.cuda.synchronize()
    for over, word in cases:
        rc = s.call(**over)
        assert rc != 0 and word in L.cosa_last_error(), (over, L.cosa_last_error())
    torch.cuda.synchronize()
    assert bool((s.out == 0x33).all()) and _pads_intact(s.out_whole) and _pads_intact(s.ws_whole)
    assert bool((s.ws == SENTINEL).all())                             # nothing was launched: the workspace was never written
    for args, word in (((None, _C.ptr(s.d_first), s.T, s.n_chunks, _C.ptr(s.blame)), b"null"),
                       ((_C.ptr(s.norm_ws), None, s.T, s.n_chunks, _C.ptr(s.blame)), b"null"),
                       ((_C.ptr(s.norm_ws), _C.ptr(s.d_first), s.T, s.n_chunks, None), b"null"),
                       ((_C.ptr(s.norm_ws), _C.ptr(s.d_first), 0, s.n_chunks, _C.ptr(s.blame)), b"positive"),
                       ((_C.ptr(s.norm_ws), _C.ptr(s.d_first), s.T, 0, _C.ptr(s.blame)), b"positive")):
        rc = L.cosa_grad_blame(*args, _C.stream_ptr())
        assert rc != 0 and word in L.cosa_last_error(), L.cosa_last_error()
    torch.cuda.synchronize()
    assert not s.blame.any() and _pads_intact(s.blame_whole)
    with pytest.raises(_C.CosaError, match="positive"):
        _C.check(rc, "cosa_grad_blame")
    assert s.call() == 0                                              # ... and the same set is taken once the arguments are right


# ---- the trainer --------------------------------------------------------------------------------------------------------------------------
BLOCK_WEIGHT = "encoder.blocks.3.mlp.fc1.weight"
PLANT_AT = 12345


def _trainer(seed=3, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, teacher_graph=False, teacher_async=False, **over)
    return CoSATrainer(args, torch.device("cuda", 0), seed=seed)


def _planted(g):
    g = g.clone()
    g.view(-1)[PLANT_AT] = float("inf")
    return g


def _step(tr, k, poison=False):
    """step k of the fixed batch sequence; poison: one element of BLOCK_WEIGHT's gradient arrives as inf (a value, through a tensor hook)"""
    from cosa_amd.train_step import synthetic_batch
    batch = synthetic_batch(2, 64, 20, tr.device, seed=500 + k)
    hook = dict(tr.student.named_parameters())[BLOCK_WEIGHT].register_hook(_planted) if poison else None
    try:
        return tr.step(*batch, n_iter=tr.args.warmup_iters + k)
    finally:
        if hook is not None:
            hook.remove()


def _state(tr):
    """clones of what a step writes: masters of both networks (the EMA teacher among them) and the moments"""
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
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k


@functools.lru_cache(maxsize=None)
def _sampled_run():
    """three steps with the flag on and no guard, the sample armed on step 2 -> (state after 3, the table after 3, the restatement of
    step 2 from the weights cloned before it and the gradients read after it, sizes, names, the summary)"""
    from cosa_amd.utils import torch_helper
    tr = _trainer(tensor_stats=True)
    assert tr.tensor_stats_state is None and tr._fused_step.blame is None and tr._fused_step.tensor_stats
    _step(tr, 1)
    assert int(tr.tensor_stats_table.abs().sum()) == 0                # not armed: step 1 launched nothing that writes the table
    student, teacher = [p.detach().clone() for p in tr.student.parameters()], [p.detach().clone() for p in tr.model_AN.parameters()]
    tr.request_tensor_stats()
    _step(tr, 2)
    grads = [p.grad if gi >= 0 else None for p, gi in zip(tr.student.parameters(), tr._fused_step.group_idx)]
    want = torch_helper.tensor_stats_torch(student, teacher, grads).cpu().numpy()
    table2 = tr.tensor_stats_table.cpu().numpy().copy()
    _step(tr, 3)
    return _state(tr), table2, tr.tensor_stats_table.cpu().numpy().copy(), want, list(tr._fused_step.sizes), list(tr._fused_step.names), tr.tensor_stats()


# ---- 5. ----
def test_the_flag_and_an_armed_sample_change_no_bit_of_three_steps():
    on_state, table2, table3, _, _, _, _ = _sampled_run()
    tr = _trainer()
    assert tr.tensor_stats() is None and tr.tensor_stats_state is None and tr._fused_step.d_first_chunk is None
    for k in (1, 2, 3):
        _step(tr, k)
    _assert_same_state(_state(tr), on_state)
    assert np.array_equal(table2, table3) and table2.any()            # the table is step 2's sample: step 3, unarmed, left it alone


# ---- 6. ----
def test_the_sample_equals_the_torch_restatement_of_that_step():
    _, table2, _, want, sizes, names, summary = _sampled_run()
    got, ref = R.decode(table2), R.decode(want)
    worst = 0.0
    for i, n in enumerate(names):
        for k in range(3):
            err = abs(got[i, k] - ref[i, k]) / ref[i, k] if ref[i, k] else abs(got[i, k])
            worst = max(worst, err / R.sum_bound(sizes[i]))
            assert err <= R.sum_bound(sizes[i]), (n, R.SLOTS[k], got[i, k], ref[i, k])
        assert got[i, 3] == ref[i, 3] and table2[i, 4] == want[i, 4] == 0 and table2[i, 5] == want[i, 5] == 0, n
    print("largest error / bound over all tensors and sums:", worst)
    assert len(names) == len(set(names)) and BLOCK_WEIGHT in names and sum(sizes) > 80e6
    assert summary["worst"] is None and summary["global"]["grad_norm"] > 0 and summary["global"]["n"] == sum(sizes)
    assert 0 < summary["global"]["ema_gap_rel"] < 1 and summary["tensors"]["encoder.head.weight"]["grad_norm"] == 0.0
    assert set(summary["groups"]) == {"-1", "0", "1", "2", "3"}


STATE_FILE = "state_00000003.cosa"


@functools.lru_cache(maxsize=None)
def _blamed_run(directory):
    """three steps behind --skip_nonfinite with the flag on, step 2 poisoned -> (guard counters, blame, names, summary, the state file)"""
    tr = _trainer(skip_nonfinite=True, tensor_stats=True)
    assert tr.tensor_stats_state is tr._fused_step.blame
    _step(tr, 1)
    tr.request_tensor_stats()
    _step(tr, 2, poison=True)
    _step(tr, 3)
    path = os.path.join(directory, STATE_FILE)
    tr.save_state(path, n_iter=2)
    tr.wait_state()
    return tr.guard_counters(), tr.tensor_stats_state.cpu().tolist(), list(tr._fused_step.names), tr.tensor_stats(), path


@pytest.fixture(scope="module")
def blamed_run(tmp_path_factory):
    return _blamed_run(str(tmp_path_factory.mktemp("tensor_stats")))


# ---- 7. ----
def test_a_planted_inf_is_blamed_on_its_tensor(blamed_run):
    counters, blame, names, summary, _ = blamed_run
    assert counters == {"applied": 2, "skipped": 1, "clipped": 0}
    at = names.index(BLOCK_WEIGHT)
    assert blame[at] == 1 and sum(blame) == 1
    assert summary["worst"] == BLOCK_WEIGHT
    t = summary["tensors"][BLOCK_WEIGHT]                              # the sample was armed on the poisoned step: it saw the element too
    assert t["blamed"] == 1 and t["g_nonfinite"] == 1 and t["grad_norm"] > 0 and summary["global"]["g_nonfinite"] == 1


# ---- 8. ----
def test_the_blame_counters_resume_with_the_run(blamed_run, tmp_path, capsys):
    _, blame, names, _, path = blamed_run
    tr = _trainer(seed=77, skip_nonfinite=True, tensor_stats=True)    # another seed: nothing of its own survives the load
    capsys.readouterr()
    assert tr.load_state(path)["n_iter"] == 2
    assert "note:" not in capsys.readouterr().out
    assert tr.tensor_stats_state.cpu().tolist() == blame and tr.guard_counters() == {"applied": 2, "skipped": 1, "clipped": 0}
    assert tr.tensor_stats_state is tr._fused_step.blame              # restored in place: the step's kernels go on counting in it
    plain = _trainer(seed=5, skip_nonfinite=True)                     # a state written without the flag: zeros and the note
    without = str(tmp_path / "state_00000000.cosa")
    plain.save_state(without, n_iter=-1)
    plain.wait_state()
    tr.load_state(without)
    assert "blame counters start at zero" in capsys.readouterr().out
    assert not tr.tensor_stats_state.any()
    for (n, p), (_, q) in zip(tr.student.named_parameters(), plain.student.named_parameters()):
        assert torch.equal(p, q), n
    plain.load_state(path)                                            # ... and the file that has them into a run without the flag
    out = capsys.readouterr().out
    assert "per-tensor blame counters" in out and "ignored" in out and plain.tensor_stats_state is None
