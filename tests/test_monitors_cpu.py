"""The monitor table (cosa_amd/monitors.py) without a GPU: read_interval over every subset of the five monitors, the
table's state-file entries against a host trainer's TrainState, and state files between a trainer with all five on and one with none."""
import itertools

import pytest
import torch

import test_student_check_cpu as SC

K = 3
# what turns each monitor on in a host trainer (the blame counters of --tensor_stats exist only behind a gradient guard)
FLAGS = {"guard": dict(clip_grad_norm=1.0), "label_stats": dict(label_stats=True), "tensor_stats": dict(tensor_stats=True, clip_grad_norm=1.0),
         "teacher_check": dict(teacher_check_iters=2), "student_check": dict(student_check_iters=2)}
ALL_ON = {k: v for f in FLAGS.values() for k, v in f.items()}
# the table's seven rows in its order: the five a host trainer can turn on (FLAGS), then --gt_stats and --act_stats_iters
NAMES = list(FLAGS) + ["gt_stats", "act_stats"]
# the notes of the parent commit's TrainState._optional_notes, entry by entry: (the file has it and the run does not, only the run has it)
NOTES = {
    "guard.state": ("the file holds a gradient guard's counters and this run has no guard (--clip_grad_norm 0, --skip_nonfinite "
                    "false): the entry is ignored",
                    "written without a gradient guard: this run's guard counters start at zero"),
    "aux.label_stats.counters": ("the file holds pseudo-label statistics and this run does not collect them (--label_stats false): the entry "
                                 "is ignored",
                                 "written without pseudo-label statistics: this run's label counters start at zero"),
    "aux.tensor_stats.blame": ("the file holds per-tensor blame counters and this run does not keep them (--tensor_stats false, or no "
                               "gradient guard): the entry is ignored",
                               "written without per-tensor blame counters: this run's blame counters start at zero"),
    "aux.teacher_check.counters": ("the file holds a teacher check's counters and this run makes no checks (--teacher_check_iters 0): the entry "
                                   "is ignored",
                                   "written without a teacher check: this run's check counters start at zero"),
    "aux.student_check.counters": ("the file holds a student check's counters and this run makes no checks (--student_check_iters 0): the entry "
                                   "is ignored",
                                   "written without a student check: this run's check counters start at zero"),
    "aux.gt_stats.counters": ("the file holds ground-truth statistics and this run does not collect them (--gt_stats false): the entry is "
                              "ignored",
                              "written without ground-truth statistics: this run's ground-truth counters start at zero"),
    "aux.act_stats.counters": ("the file holds activation statistics and this run collects none (--act_stats_iters 0): the entry is ignored",
                               "written without activation statistics: this run's activation counters start at zero"),
}


def _five():
    """the rows of FLAGS, in the table's order"""
    from cosa_amd import monitors
    return monitors.MONITORS[:len(FLAGS)]


def _tensors():
    """{monitor name: its tensors} as the monitors' own CPU tests build them (K = 3), and the 8 running sums"""
    from cosa_amd.utils import seg_helper, torch_helper
    guard = torch_helper.new_guard_state("cpu")
    guard.view(torch.float32)[0] = 2.5
    guard[2:5] = torch.tensor([17, 2, 1])
    student = torch.arange(seg_helper.student_check_layout(K)[1], dtype=torch.int64) + 1000
    student[7] = (1 << 62) + 12345
    return torch.arange(8, dtype=torch.float64) * 20, {
        "guard": guard, "label_stats": torch.arange(4 * K + 7, dtype=torch.int64) + 100,
        "tensor_stats": (torch.arange(12, dtype=torch.float64).reshape(2, 6), torch.tensor([5, 0])),
        "teacher_check": torch.arange(seg_helper.teacher_check_layout(K)[1], dtype=torch.int64) + 5, "student_check": student}


def test_every_subset_reads_what_the_full_set_reads_in_one_transfer(monkeypatch):
    from cosa_amd import main as launcher
    from cosa_amd import monitors
    assert [m.name for m in monitors.MONITORS] == NAMES
    calls, tolist = [], torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda t: calls.append(t.numel()) or tolist(t))

    def read(names):
        acc, tensors = _tensors()
        before = len(calls)
        out = launcher.read_interval(acc, 20, [(m, tensors[m.name]) for m in monitors.MONITORS if m.name in names])
        assert len(calls) == before + 1 and acc.numel() == 8 and not acc.any()
        return out, tensors

    (vals, full), _ = read(set(FLAGS))
    assert vals == [float(i) for i in range(8)] and set(full) == set(FLAGS) and full["guard"] == [2.5, 2.0, 1.0]
    assert full["label_stats"] == list(range(100, 119)) and full["tensor_stats"][1] == [5, 0] and len(full["tensor_stats"][0]) == 2
    assert full["student_check"][7] == (1 << 62) + 12345
    for r in range(6):
        for names in itertools.combinations(FLAGS, r):
            (v, host), tensors = read(set(names))
            assert v == vals and host == {k: full[k] for k in names} and list(host) == list(names)
            for k in ("label_stats", "teacher_check", "student_check"):          # an interval's: zeroed when read, untouched when not
                assert bool(tensors[k].any()) == (k not in names)
            assert tensors["guard"][2:5].tolist() == [17, 2, 1] and tensors["tensor_stats"][1].tolist() == [5, 0]      # the run's: kept
            assert torch.equal(tensors["tensor_stats"][0], torch.arange(12, dtype=torch.float64).reshape(2, 6))


@pytest.mark.parametrize("on", [None] + list(FLAGS) + ["all"])
def test_state_names_are_the_trainers_optional_entries(monkeypatch, on):
    from cosa_amd import monitors
    tr = SC._host_trainer(monkeypatch, seed=1, **({} if on is None else ALL_ON if on == "all" else FLAGS[on]))
    state = tr.train_state()
    want = set(FLAGS) if on == "all" else {on, "guard"} if on == "tensor_stats" else {on}
    for m in monitors.MONITORS:
        assert (m.tensors(tr) is not None) == (m.name in want)
        assert (m.state_name in state.names) == (m.name in want), m.name
    assert state._optional_notes() == NOTES and list(state._optional_notes()) == [m.state_name for m in monitors.MONITORS]


def test_state_files_between_all_monitors_on_and_none(tmp_path, monkeypatch, capsys):
    full, none = SC._host_trainer(monkeypatch, seed=1, **ALL_ON), SC._host_trainer(monkeypatch, seed=2)
    for m in _five():                                                        # counters that a load must carry or leave alone
        t = m.tensors(full)
        (t[1] if isinstance(t, tuple) else t).fill_(3)
    with_all, without = str(tmp_path / "state_00000003.cosa"), str(tmp_path / "state_00000000.cosa")
    full.save_state(with_all, n_iter=2)
    none.save_state(without, n_iter=-1)
    full.wait_state()
    none.wait_state()
    want, want_none = ([p.detach().clone() for p in tr.student.parameters()] for tr in (full, none))
    capsys.readouterr()
    assert none.load_state(with_all)["n_iter"] == 2
    assert capsys.readouterr().out.splitlines() == [f"note: {with_all}: {NOTES[m.state_name][0]}" for m in _five()]
    assert all(torch.equal(p, q) for p, q in zip(none.student.parameters(), want)) and not hasattr(none, "extra_state")
    assert full.load_state(without)["n_iter"] == -1
    assert capsys.readouterr().out.splitlines() == [f"note: {without}: {NOTES[m.state_name][1]}" for m in _five()]
    assert all(torch.equal(p, q) for p, q in zip(full.student.parameters(), want_none))
    for m in _five():
        t = m.tensors(full)
        assert not (t[1] if isinstance(t, tuple) else t).any(), m.name
