"""Per-tensor training diagnostics without a GPU: the row layout, the torch restatement host trainers run and the
summary against the numpy yardstick (tests/tensor_stats_ref.py), the flag, a host trainer's blame counters through a state file in both
directions, and the launcher's interval read, log line and .jsonl record."""
import json
import math

import numpy as np
import pytest
import torch

import tensor_stats_ref as R

INF, NAN = float("inf"), float("nan")


def _toy():
    """(names, student, teacher, grads, group_idx): a frozen tensor, a one-element tensor, planted inf / NaN / -inf in g, p and tp, an
    all-zero weight whose teacher is zero too, and a zero weight under a non-zero teacher"""
    g = torch.Generator().manual_seed(5)
    rn = lambda *s: torch.randn(*s, generator=g)
    names = ["a.weight", "a.bias", "one", "frozen", "zero", "zero_student", "planted_g", "planted_w"]
    student = [rn(7, 5), rn(7), rn(1), rn(11), torch.zeros(6), torch.zeros(4), rn(9) * 1e-3, rn(3, 4) * 1e2]
    teacher = [p + 0.01 * rn(*p.shape) for p in student]
    teacher[4] = torch.zeros(6)
    grads = [rn(*p.shape) * 0.1 for p in student]
    grads[3] = None                                                   # frozen: no gradient
    grads[6][2], grads[6][5], grads[6][8] = INF, NAN, -INF
    student[7][0, 1] = NAN                                            # p alone
    teacher[7][1, 0] = -INF                                           # tp alone
    student[7][2, 3], teacher[7][2, 3] = INF, NAN                     # both: one element, counted once
    return names, student, teacher, grads, [0, 1, 0, -1, 2, 2, 3, 3]


def _close(got, want, n):
    return got == want if want == 0 else abs(got - want) <= R.sum_bound(n) * abs(want)


def test_layout_is_six_eight_byte_slots_in_the_documented_order():
    from cosa_amd.utils import torch_helper
    off, nbytes = torch_helper.tensor_stats_layout()
    assert nbytes == R.ROW_BYTES == 48 and list(off) == list(R.SLOTS) == list(torch_helper.TENSOR_STATS_SLOTS)
    assert [off[k] for k in R.SLOTS] == [0, 8, 16, 24, 32, 40]
    t = torch_helper.new_tensor_stats(3, "cpu")
    assert t.shape == (3, 6) and t.dtype == torch.int64 and t.element_size() * t.shape[1] == nbytes


def test_torch_restatement_equals_the_numpy_reference():
    from cosa_amd.utils import torch_helper
    names, student, teacher, grads, _ = _toy()
    want = R.table([p.numpy() for p in student], [t.numpy() for t in teacher], [None if g is None else g.numpy() for g in grads])
    raw = torch_helper.tensor_stats_torch(student, teacher, grads)
    assert raw.dtype == torch.int64 and raw.shape == (len(names), 6)
    got = R.decode(raw.numpy())
    assert np.array_equal(got, torch_helper.tensor_stats_values(raw).numpy())
    for i, n in enumerate(names):
        size = student[i].numel()
        for k in range(3):                                            # float64 sums in another order: the worst-case bound of such a sum
            assert _close(got[i, k], want[i][k], size), (n, R.SLOTS[k], got[i, k], want[i][k])
        assert got[i, 3] == want[i][3] and got[i, 4] == want[i][4] and got[i, 5] == want[i][5], (n, got[i], want[i])
        assert all(math.isfinite(v) for v in got[i])
    by = dict(zip(names, got))
    assert tuple(by["frozen"][[0, 3, 4]]) == (0.0, 0.0, 0.0) and by["frozen"][1] > 0 and by["frozen"][2] > 0
    assert by["planted_g"][4] == 3 and by["planted_g"][0] > 0 and by["planted_g"][5] == 0
    assert by["planted_w"][5] == 3 and by["planted_w"][4] == 0
    assert tuple(by["zero"][[1, 2, 5]]) == (0.0, 0.0, 0.0) and by["zero_student"][1] == 0.0 and by["zero_student"][2] > 0
    assert by["one"][3] == abs(float(grads[2][0]))
    # a gradient that is non-finite throughout: no finite maximum, a zero sum
    allbad = R.decode(torch_helper.tensor_stats_torch([torch.ones(2)], [torch.ones(2)], [torch.tensor([INF, NAN])]).numpy())[0]
    assert tuple(allbad) == (0.0, 2.0, 0.0, 0.0, 2.0, 0.0)


def test_summary_pools_per_group_and_names_the_worst_tensor():
    from cosa_amd.utils import torch_helper
    names, student, teacher, grads, groups = _toy()
    sizes = [p.numel() for p in student]
    raw = torch_helper.tensor_stats_torch(student, teacher, grads)
    rows = R.decode(raw.numpy()).tolist()
    blame = [0, 2, 0, 0, 0, 0, 2, 0]
    want = R.summary(rows, blame, names, groups, sizes)
    for table, bl in ((raw, torch.tensor(blame)), (raw.numpy(), blame), (rows, blame), (torch_helper.tensor_stats_values(raw), blame)):
        got = torch_helper.tensor_stats_summary(table, bl, names, groups, sizes)
        assert got.keys() == want.keys() == {"tensors", "groups", "global", "worst"}
        assert list(got["tensors"]) == names and set(got["groups"]) == {"-1", "0", "1", "2", "3"}
        for part in ("tensors", "groups"):
            for k, w in want[part].items():
                assert got[part][k] == pytest.approx(w, rel=1e-12, abs=0), (part, k)
        assert got["global"] == pytest.approx(want["global"], rel=1e-12, abs=0)
        # two tensors were blamed twice: the one that also holds non-finite elements in this sample comes first
        assert got["worst"] == want["worst"] == "planted_g"
        json.dumps(got)
    g0 = want["groups"]["0"]                                          # a.weight and one, pooled: square roots of the pooled sums
    assert g0["n"] == 36 and g0["grad_norm"] == pytest.approx(math.sqrt(rows[0][0] + rows[2][0]), rel=1e-15)
    assert got["groups"]["3"]["g_nonfinite"] == 3 and got["groups"]["3"]["w_nonfinite"] == 3 and got["groups"]["1"]["blamed"] == 2
    assert got["global"]["blamed"] == 4 and got["global"]["n"] == sum(sizes)
    # a zero weight norm gives zeros, not NaN or 1e12, whatever the teacher holds
    for n in ("zero", "zero_student"):
        assert got["tensors"][n]["weight_norm"] == 0.0 and got["tensors"][n]["ema_gap_rel"] == 0.0
    assert got["tensors"]["zero_student"]["ema_gap"] > 0
    t = got["tensors"]["a.weight"]
    assert t["ema_gap_rel"] == pytest.approx(t["ema_gap"] / (t["weight_norm"] + 1e-12), rel=1e-15) and 0 < t["ema_gap_rel"] < 0.1
    # the worst rule: blame first, then g_nonfinite, None when all are zero; no blame vector (no guard) counts as zeros
    assert torch_helper.tensor_stats_summary(raw, None, names, groups, sizes)["worst"] == "planted_g"
    assert torch_helper.tensor_stats_summary(raw, [0, 1, 0, 0, 0, 0, 0, 0], names, groups, sizes)["worst"] == "a.bias"
    clean = torch_helper.tensor_stats_torch(student[:3], teacher[:3], grads[:3])
    s = torch_helper.tensor_stats_summary(clean, None, names[:3], groups[:3])
    assert s["worst"] is None and s["global"]["n"] is None and s["global"]["blamed"] == 0
    z = torch_helper.tensor_stats_summary(torch_helper.new_tensor_stats(2, "cpu"), None, ["x", "y"], [0, 0], [3, 4])
    assert z["global"] == {"n": 7, "grad_norm": 0.0, "grad_absmax": 0.0, "weight_norm": 0.0, "ema_gap": 0.0, "ema_gap_rel": 0.0,
                           "g_nonfinite": 0, "w_nonfinite": 0, "blamed": 0} and z["worst"] is None
    with pytest.raises(ValueError):
        torch_helper.tensor_stats_summary(raw, None, names[:-1], groups, sizes)


def test_blame_restatement_advances_the_tensors_with_a_nonfinite_gradient():
    from cosa_amd.utils import torch_helper
    _, _, _, grads, _ = _toy()
    blame = torch.zeros(len(grads), dtype=torch.int64)
    for k in (1, 2):
        torch_helper.grad_blame_torch(grads, blame)
        assert blame.tolist() == [0, 0, 0, 0, 0, 0, k, 0]


def test_flag_parses_default_off_and_reaches_default_args():
    from cosa_amd import args as cosa_args
    from cosa_amd.train_step import default_args
    a, changed = cosa_args.parse(["EXP"])
    assert a.tensor_stats is False and "tensor_stats" not in changed
    a, changed = cosa_args.parse(["EXP", "--tensor_stats", "true"])
    assert a.tensor_stats is True and changed["tensor_stats"] is True
    assert default_args("VOC12").tensor_stats is False
    assert default_args("VOC12", **{k: v for k, v in vars(a).items() if k != "dataset"}).tensor_stats is True


class _TinyNet(torch.nn.Module):
    """the toy network of tests/test_resume_cpu.py: the real CoSATrainer set-up around it"""

    def __init__(self):
        super().__init__()
        self.encoder = torch.nn.Module()
        self.encoder.proj = torch.nn.Linear(5, 7)
        self.encoder.head = torch.nn.Linear(7, 3)
        self.norm = torch.nn.LayerNorm(7)
        self.decoder = torch.nn.Linear(7, 3)
        self.classifier = torch.nn.Conv2d(7, 2, 1, bias=False)

    def get_param_groups(self):
        return [list(self.encoder.proj.parameters()), list(self.norm.parameters()), list(self.decoder.parameters()),
                list(self.classifier.parameters())]

    def check_nograd_precision(self, mode):
        pass


def _host_trainer(monkeypatch, seed, **over):
    from cosa_amd import train_step
    monkeypatch.setattr(train_step, "build_model", lambda args: _TinyNet())
    args = train_step.default_args("VOC12", crop_size=48, batch_size=3, num_classes=5, max_iters=100, **over)
    return train_step.CoSATrainer(args, torch.device("cpu"), seed=seed)


def _give_gradients(tr, seed, poison=None):
    g = torch.Generator().manual_seed(seed)
    for n, p in tr.student.named_parameters():
        p.grad = torch.randn(p.shape, generator=g) if p.requires_grad else None
        if n == poison:
            p.grad.view(-1)[-1] = INF


def test_host_trainer_samples_on_request_and_blames_behind_a_guard(monkeypatch):
    off = _host_trainer(monkeypatch, seed=1)
    assert off.tensor_stats() is None and off.tensor_stats_state is None and off.tensor_stats_table is None and not hasattr(off, "extra_state")
    with pytest.raises(RuntimeError):
        off.request_tensor_stats()
    unguarded = _host_trainer(monkeypatch, seed=1, tensor_stats=True)
    assert unguarded.tensor_stats_state is None and unguarded.tensor_stats_table.shape == (9, 6)        # no guard: no blame, no per-step work
    tr = _host_trainer(monkeypatch, seed=1, tensor_stats=True, skip_nonfinite=True)
    names = [n for n, _ in tr.student.named_parameters()]
    assert tr.tensor_stats_state.tolist() == [0] * len(names) and "encoder.head.weight" in names
    with torch.no_grad():                                             # a teacher that has moved away from the student
        for p in tr.model_AN.parameters():
            p.mul_(1.01)
    _give_gradients(tr, 3)
    tr._tensor_stats_torch_step()                                     # not armed: the table stays as it is
    assert int(tr.tensor_stats_table.abs().sum()) == 0 and int(tr.tensor_stats_state.sum()) == 0
    tr.request_tensor_stats()
    _give_gradients(tr, 4, poison="norm.weight")
    tr._tensor_stats_torch_step()
    params, tparams = list(tr.student.parameters()), list(tr.model_AN.parameters())
    want = R.table([p.detach().numpy() for p in params], [p.detach().numpy() for p in tparams],
                   [None if p.grad is None else p.grad.numpy() for p in params])
    got = R.decode(tr.tensor_stats_table.numpy())
    for i, n in enumerate(names):
        for k in range(6):
            assert _close(got[i, k], want[i][k], params[i].numel()), (n, R.SLOTS[k])
    s = tr.tensor_stats()
    assert s["worst"] == "norm.weight" and s["tensors"]["norm.weight"]["blamed"] == 1 and s["tensors"]["norm.weight"]["g_nonfinite"] == 1
    assert s["global"]["blamed"] == 1 and s["tensors"]["encoder.head.weight"]["grad_norm"] == 0.0          # the frozen head
    assert s["tensors"]["encoder.head.weight"]["ema_gap_rel"] == pytest.approx(0.01, rel=1e-4)
    assert set(s["groups"]) == {"-1", "0", "1", "2", "3"} and s["groups"]["1"]["blamed"] == 1
    _give_gradients(tr, 5)
    tr._tensor_stats_torch_step()                                     # the sample is one step's: it stays; the blame is the run's
    assert np.array_equal(R.decode(tr.tensor_stats_table.numpy()), got) and tr.tensor_stats()["tensors"]["norm.weight"]["blamed"] == 1


def test_blame_counters_reconcile_with_state_files_in_both_directions(tmp_path, monkeypatch, capsys):
    a = _host_trainer(monkeypatch, seed=1, tensor_stats=True, skip_nonfinite=True)
    a.tensor_stats_state += torch.arange(a.tensor_stats_state.numel())
    a.guard_state[3] = 4
    plain = _host_trainer(monkeypatch, seed=2, skip_nonfinite=True)
    with_blame, without = str(tmp_path / "state_00000003.cosa"), str(tmp_path / "state_00000000.cosa")
    a.save_state(with_blame, n_iter=2)
    a.wait_state()
    plain.save_state(without, n_iter=-1)
    plain.wait_state()
    assert "aux.tensor_stats.blame" in a.train_state().names and a.train_state().names[-1] == "guard.state"
    assert "aux.tensor_stats.blame" not in plain.train_state().names
    # the counters survive the file, in place and without a note
    b = _host_trainer(monkeypatch, seed=9, tensor_stats=True, skip_nonfinite=True)
    held = b.tensor_stats_state
    capsys.readouterr()
    assert b.load_state(with_blame)["n_iter"] == 2
    assert "note:" not in capsys.readouterr().out
    assert b.tensor_stats_state is held and held.tolist() == list(range(held.numel())) and int(b.guard_state[3]) == 4
    for p, q in zip(a.student.parameters(), b.student.parameters()):
        assert torch.equal(p, q)
    # a file without them into a run that keeps them: zero counters and a note
    b.load_state(without)
    assert "blame counters start at zero" in capsys.readouterr().out
    assert int(b.tensor_stats_state.abs().sum()) == 0
    for p, q in zip(plain.student.parameters(), b.student.parameters()):
        assert torch.equal(p, q)
    # ... and a file that has them into a run without the flag: ignored, with a note
    plain.load_state(with_blame)
    out = capsys.readouterr().out
    assert "per-tensor blame counters" in out and "ignored" in out and plain.tensor_stats_state is None and int(plain.guard_state[3]) == 4
    for p, q in zip(a.student.parameters(), plain.student.parameters()):
        assert torch.equal(p, q)
    # without a guard the flag keeps no counters: such a run reads and writes the files of a run without the flag
    c = _host_trainer(monkeypatch, seed=4, tensor_stats=True)
    assert c.tensor_stats_state is None and c.train_state().names == _host_trainer(monkeypatch, seed=4).train_state().names


@pytest.mark.parametrize("with_blame", [False, True])
def test_launcher_reads_table_and_blame_in_the_intervals_one_transfer(with_blame, tmp_path):
    from cosa_amd import main as launcher
    from cosa_amd import monitors
    from cosa_amd.utils import torch_helper
    M = monitors.BY_NAME
    names, student, teacher, grads, groups = _toy()
    sizes = [p.numel() for p in student]
    table = torch_helper.tensor_stats_torch(student, teacher, grads)
    kept = table.clone()
    blame = torch.tensor([0, 0, 0, 0, 0, 0, 3, 0]) if with_blame else None
    acc = torch.arange(8, dtype=torch.float64) * 20
    guard = torch_helper.new_guard_state("cpu")
    guard[2:5] = torch.tensor([17, 3, 0])
    stats = torch.arange(27, dtype=torch.int64)
    vals, host = launcher.read_interval(acc, 20, [(M["guard"], guard), (M["label_stats"], stats), (M["tensor_stats"], (table, blame))])
    assert set(host) == {"guard", "label_stats", "tensor_stats"}
    gvals, svals, (tvals, bvals) = host["guard"], host["label_stats"], host["tensor_stats"]
    assert vals == [float(i) for i in range(8)] and acc.numel() == 8 and int(acc.abs().sum()) == 0
    assert gvals[1:] == [3.0, 0.0] and svals == list(range(27)) and int(stats.abs().sum()) == 0
    assert torch.equal(table, kept)                                   # a sample, not an accumulator: nothing is zeroed
    assert np.array_equal(np.array(tvals), R.decode(kept.numpy())) and len(tvals) == len(names) and len(tvals[0]) == 6
    assert bvals == ([0, 0, 0, 0, 0, 0, 3, 0] if with_blame else None)
    if with_blame:
        assert blame.tolist() == bvals                                # the run's: never zeroed
    # without the monitor its values are absent, and alone it reads the same
    assert set(launcher.read_interval(acc, 20, [(M["guard"], guard)])[1]) == {"guard"}
    v2, h2 = launcher.read_interval(acc, 20, [(M["tensor_stats"], (table, blame))])
    assert set(h2) == {"tensor_stats"}
    t2, b2 = h2["tensor_stats"]
    assert t2 == tvals and b2 == bvals and len(v2) == 8
    summary = torch_helper.tensor_stats_summary(tvals, bvals, names, groups, sizes)
    want = R.summary(R.decode(kept.numpy()).tolist(), bvals, names, groups, sizes)
    assert summary["global"] == pytest.approx(want["global"], rel=1e-12, abs=0) and summary["worst"] == "planted_g"
    line = M["tensor_stats"].line(summary, None)
    assert line == " ema_gap: %.3e, worst: planted_g" % want["global"]["ema_gap_rel"]
    quiet = torch_helper.tensor_stats_summary(torch_helper.tensor_stats_torch(student[:2], teacher[:2], grads[:2]), None, names[:2], groups[:2])
    assert M["tensor_stats"].line(quiet, None).endswith(", worst: -")
    for it in (20, 40):
        monitors.append_monitor(tmp_path, M["tensor_stats"], summary, it, None)
    lines = (tmp_path / "tensor_stats.jsonl").read_text().splitlines()
    recs = [json.loads(x) for x in lines]
    assert [r["iters"] for r in recs] == [20, 40] and recs[0]["worst"] == "planted_g" and list(recs[0]["tensors"]) == names
    assert recs[0]["tensors"]["planted_g"]["blamed"] == (3 if with_blame else 0)
