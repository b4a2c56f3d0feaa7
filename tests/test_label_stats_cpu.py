"""Per-step pseudo-label statistics without a GPU: the counter layout, the summary, the torch restatement host
trainers run against the numpy yardstick (tests/label_stats_ref.py), the flag, a host trainer's counters through a state file, and the
launcher's log line."""
import json

import numpy as np
import pytest
import torch

import label_stats_ref as R


def _t(d, dev="cpu"):
    return {k: (torch.from_numpy(v).to(dev) if v is not None else None) for k, v in d.items()}


def test_layout_offsets_match_the_documented_order():
    from cosa_amd.utils import seg_helper
    for K in (2, 21, 81):
        off, n = seg_helper.label_stats_layout(K)
        want, want_n = R.layout(K)
        assert off == want and n == want_n == 4 * K + 7
        assert list(off) == list(seg_helper.LABEL_STATS_SLOTS)
        assert off["steps"] == 0 and off["pix"] == 1 and off["main"] == 2 and off["aux"] == K + 3 and off["agree"] == 2 * K + 4
        assert off["inter"] == 2 * K + 5 and off["pred"] == 3 * K + 5 and off["bad_cam"] == 4 * K + 5 and off["bad_cam_aux"] == 4 * K + 6
    for bad in (1, 129, 0, -3):
        with pytest.raises(ValueError):
            seg_helper.label_stats_layout(bad)


def test_summary_on_hand_made_counters():
    from cosa_amd.utils import seg_helper
    K = 3
    off, n = R.layout(K)
    c = np.zeros(n, np.int64)
    c[off["steps"]], c[off["pix"]] = 5, 100
    c[off["main"]:off["main"] + K + 1] = [50, 30, 0, 20]          # bg, class 1, class 2 (never labelled), ignore
    c[off["aux"]:off["aux"] + K + 1] = [40, 20, 30, 10]
    c[off["agree"]] = 75
    c[off["pred"]:off["pred"] + K] = [60, 20, 0]                  # class 2: neither predicted nor labelled -> empty union
    c[off["inter"]:off["inter"] + K] = [45, 15, 0]
    c[off["bad_cam"]], c[off["bad_cam_aux"]] = 2, 1
    for counters in (c, c.tolist(), torch.from_numpy(c)):
        s = seg_helper.label_stats_summary(counters, K)
        assert (s["steps"], s["pix"], s["teacher_nonfinite"]) == (5, 100, 3)
        assert (s["ignore_frac"], s["bg_frac"], s["fg_frac"]) == (0.2, 0.5, 0.3)
        assert (s["aux_ignore_frac"], s["aux_bg_frac"], s["aux_fg_frac"]) == (0.1, 0.4, 0.5)
        assert s["aux_agree"] == 0.75
        assert s["student_iou"] == [45 / 65, 15 / 35, None]
        assert s["student_miou"] == (45 / 65 + 15 / 35) / 2       # the class with the empty union is left out of the mean
    z = seg_helper.label_stats_summary(np.zeros(n, np.int64), K)
    assert z["ignore_frac"] == z["bg_frac"] == z["fg_frac"] == z["aux_agree"] == z["student_miou"] == 0.0 and z["steps"] == 0
    assert z["student_iou"] == [None] * K
    json.dumps(z)
    with pytest.raises(ValueError):
        seg_helper.label_stats_summary(np.zeros(n + 1, np.int64), K)


CASES = {"K5": dict(B=3, K=5, S=48, h=3, seed=11, box_kinds=("full", "interior", "row"), label_kinds=("some", "all", "none")),
         "K21": dict(B=2, K=21, S=64, h=4, seed=12, box_kinds=("empty", "interior"), label_kinds=("some", "some"))}


@pytest.mark.parametrize("case", list(CASES))
def test_torch_restatement_equals_the_numpy_reference(case, oracle_c):
    """on inputs whose top-two resized logits differ by more than 1e-4 everywhere (asserted by the helper): an ulp between F.interpolate
    and spec R cannot flip a label, so the counters are equal as integers"""
    from cosa_amd.utils import seg_helper
    d = R.draw(oracle_c, margin=1e-4, **CASES[case])
    K = CASES[case]["K"]
    off, n = R.layout(K)
    want = R.reference(oracle_c, d["mask_main"], d["mask_aux"], d["seg"], d["cls"], d["boxes"], d["cam"], d["cam_aux"])
    t = _t(d)
    counters = seg_helper.new_label_stats(K, "cpu")
    scale = seg_helper.label_stats_torch(t["mask_main"], t["mask_aux"], t["seg"], t["cls"], t["boxes"], t["cam"], t["cam_aux"], counters)
    assert np.array_equal(counters.numpy(), want) and want[off["pix"]] > 0 and want[off["pred"]:off["pred"] + K].sum() > 0
    assert scale.view(torch.int32).item() == 0x3f800000
    # a second call accumulates; NULL inputs leave their slots alone; an inf in a present plane inside the box is counted, a NaN in an absent one is not
    b, cl = (1, int(np.nonzero(d["cls"][1])[0][0])) if case == "K21" else (0, int(np.nonzero(d["cls"][0])[0][0]))
    y, x = int(d["boxes"][b][0]), int(d["boxes"][b][2])
    cam = d["cam"].copy()
    cam[b, cl, y, x] = np.inf
    absent = np.nonzero(d["cls"][b] == 0)[0]
    if len(absent):
        cam[b, absent[0], y, x] = np.nan
    want2 = R.reference(oracle_c, d["mask_main"], None, d["seg"], d["cls"], d["boxes"], cam, None)
    assert want2[off["bad_cam"]] == 1 and want2[off["aux"]:off["aux"] + K + 1].sum() == 0 and want2[off["agree"]] == 0
    scale = seg_helper.label_stats_torch(t["mask_main"], None, t["seg"], t["cls"], t["boxes"], torch.from_numpy(cam), None, counters)
    assert np.array_equal(counters.numpy(), want + want2) and counters[off["steps"]] == 2
    assert bool(torch.isnan(scale).all())


def test_flag_parses_default_off_and_reaches_default_args():
    from cosa_amd import args as cosa_args
    from cosa_amd.train_step import default_args
    a, changed = cosa_args.parse(["EXP"])
    assert a.label_stats is False and "label_stats" not in changed
    a, changed = cosa_args.parse(["EXP", "--label_stats", "true"])
    assert a.label_stats is True and changed["label_stats"] is True
    assert default_args("VOC12").label_stats is False
    assert default_args("VOC12", **{k: v for k, v in vars(a).items() if k != "dataset"}).label_stats is True


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


def test_host_trainer_counts_and_carries_its_counters_through_a_state_file(tmp_path, monkeypatch, capsys, oracle_c):
    off, n = R.layout(5)
    inputs = [R.draw(oracle_c, margin=1e-4, **dict(CASES["K5"], seed=20 + k)) for k in range(3)]
    want = sum(R.reference(oracle_c, d["mask_main"], d["mask_aux"], d["seg"], d["cls"], d["boxes"], d["cam"], d["cam_aux"]) for d in inputs)
    off_tr = _host_trainer(monkeypatch, seed=1)
    assert off_tr.label_stats_state is None and off_tr.label_stats() is None and not hasattr(off_tr, "extra_state")
    a = _host_trainer(monkeypatch, seed=1, label_stats=True)
    assert a.extra_state["label_stats.counters"] is a.label_stats_state and int(a.label_stats_state.abs().sum()) == 0
    for d in inputs:
        t = _t(d)
        scale = a.update_label_stats(t["mask_main"], t["mask_aux"], t["seg"], t["cls"], t["boxes"], t["cam"], t["cam_aux"])
        assert scale is a._step_scale and float(scale) == 1.0
    s = a.label_stats()
    assert s["steps"] == 3 and np.array_equal(a.label_stats_state.numpy(), want)
    assert s["pix"] == int(want[off["pix"]]) and 0 < s["ignore_frac"] < 1 and s["teacher_nonfinite"] == 0
    with_stats, without = str(tmp_path / "state_00000003.cosa"), str(tmp_path / "state_00000000.cosa")
    a.save_state(with_stats, n_iter=2)
    a.wait_state()
    off_tr.save_state(without, n_iter=-1)
    off_tr.wait_state()
    # the counters survive the file, in place
    b = _host_trainer(monkeypatch, seed=9, label_stats=True)
    held = b.label_stats_state
    capsys.readouterr()
    assert b.load_state(with_stats)["n_iter"] == 2
    assert "note:" not in capsys.readouterr().out
    assert b.label_stats_state is held and np.array_equal(held.numpy(), want)
    for p, q in zip(a.student.parameters(), b.student.parameters()):
        assert torch.equal(p, q)
    # a file without the counters into a run that collects them: zero counters and a note
    b.load_state(without)
    assert "label counters start at zero" in capsys.readouterr().out
    assert int(b.label_stats_state.abs().sum()) == 0
    for p, q in zip(off_tr.student.parameters(), b.student.parameters()):
        assert torch.equal(p, q)
    # ... and a file that has them into a run that does not: ignored, with a note
    c = _host_trainer(monkeypatch, seed=5)
    c.load_state(with_stats)
    out = capsys.readouterr().out
    assert "pseudo-label statistics" in out and "ignored" in out and c.label_stats_state is None
    for p, q in zip(a.student.parameters(), c.student.parameters()):
        assert torch.equal(p, q)
    # the launcher's own tensor next to the counters (main.py keeps both in extra_state): both orders of presence reconcile
    d = _host_trainer(monkeypatch, seed=6, label_stats=True)
    d.extra_state = dict(d.extra_state, **{"launcher.acc": torch.arange(8, dtype=torch.float64)})
    both = str(tmp_path / "state_00000004.cosa")
    d.label_stats_state += 3
    d.save_state(both, n_iter=3)
    d.wait_state()
    e = _host_trainer(monkeypatch, seed=7)
    e.extra_state = {"launcher.acc": torch.zeros(8, dtype=torch.float64)}
    e.load_state(both)
    assert torch.equal(e.extra_state["launcher.acc"], torch.arange(8, dtype=torch.float64))
    for p, q in zip(d.student.parameters(), e.student.parameters()):
        assert torch.equal(p, q)


def test_launcher_line_and_jsonl_record_from_a_counter_vector():
    from cosa_amd import monitors
    from cosa_amd.utils import seg_helper
    m = monitors.BY_NAME["label_stats"]
    K = 3
    off, n = R.layout(K)
    c = np.zeros(n, np.int64)
    c[off["steps"]], c[off["pix"]] = 20, 1000
    c[off["main"]:off["main"] + K + 1] = [500, 250, 125, 125]
    c[off["aux"]:off["aux"] + K + 1] = [500, 250, 125, 125]
    c[off["agree"]] = 875
    c[off["pred"]:off["pred"] + K] = [475, 300, 100]
    c[off["inter"]:off["inter"] + K] = [400, 200, 100]
    c[off["bad_cam_aux"]] = 4
    s = seg_helper.label_stats_summary(c.astype(np.float64).tolist(), K)          # as the launcher reads them: doubles out of the interval's one sync
    line = m.line(s, None)
    miou = (400 / 575 + 200 / 350 + 100 / 125) / 3
    assert line == " ignore: 0.125, fg: 0.375, aux_agree: 0.875, student_miou: %.3f, teacher_nonfinite: 4" % miou
    rec = json.loads(monitors.monitor_record(m, s, 40, None))
    assert rec["iters"] == 40 and rec["steps"] == 20 and rec["student_iou"] == [400 / 575, 200 / 350, 100 / 125]
    assert rec["class_pixels"] == [500, 250, 125, 125] and rec["aux_class_pixels"] == [500, 250, 125, 125]
    assert rec["teacher_nonfinite_aux"] == 4 and "\n" not in monitors.monitor_record(m, s, 40, None)


@pytest.mark.parametrize("with_guard", [False, True])
@pytest.mark.parametrize("with_stats", [False, True])
def test_launcher_reads_an_interval_in_one_transfer_and_zeroes_what_is_the_intervals(with_guard, with_stats, tmp_path):
    from cosa_amd import main as launcher
    from cosa_amd import monitors
    from cosa_amd.utils import seg_helper, torch_helper
    K = 3
    off, n = R.layout(K)
    acc = torch.arange(8, dtype=torch.float64) * 20
    guard = None
    if with_guard:
        guard = torch_helper.new_guard_state("cpu")
        guard.view(torch.float32)[0] = 2.5
        guard[2:5] = torch.tensor([17, 2, 1])
    stats = None
    if with_stats:
        stats = torch.arange(n, dtype=torch.int64) + 100
    on = [(monitors.BY_NAME[k], t) for k, t in (("guard", guard), ("label_stats", stats)) if t is not None]
    vals, host = launcher.read_interval(acc, 20, on)
    assert vals == [float(i) for i in range(8)] and int(acc.abs().sum()) == 0 and acc.numel() == 8
    assert set(host) == {m.name for m, _ in on}
    gvals, svals = host.get("guard"), host.get("label_stats")
    assert gvals == ([2.5, 2.0, 1.0] if with_guard else None)
    if with_guard:
        assert guard[2:5].tolist() == [17, 2, 1]                      # the guard's counters are the run's
    if with_stats:
        assert svals == list(range(100, 100 + n)) and all(isinstance(v, int) for v in svals) and int(stats.abs().sum()) == 0
        summary = seg_helper.label_stats_summary(svals, K)
        for it in (20, 40):
            monitors.append_monitor(tmp_path, monitors.BY_NAME["label_stats"], summary, it, None)
        lines = (tmp_path / "label_stats.jsonl").read_text().splitlines()
        assert [json.loads(x)["iters"] for x in lines] == [20, 40] and json.loads(lines[0])["steps"] == 100
    else:
        assert svals is None


def test_a_mask_value_that_is_no_label_is_counted_in_pix_only(oracle_c):
    from cosa_amd.utils import seg_helper
    d = R.draw(oracle_c, margin=1e-4, **CASES["K5"])
    d["mask_main"][0, 5, 6] = 1.5                                     # image 0's box is the whole crop
    off, n = R.layout(5)
    want = R.reference(oracle_c, d["mask_main"], d["mask_aux"], d["seg"], d["cls"], d["boxes"], d["cam"], d["cam_aux"])
    assert want[off["main"]:off["main"] + 6].sum() == want[off["pix"]] - 1
    t = _t(d)
    counters = seg_helper.new_label_stats(5, "cpu")
    seg_helper.label_stats_torch(t["mask_main"], t["mask_aux"], t["seg"], t["cls"], t["boxes"], t["cam"], t["cam_aux"], counters)
    assert np.array_equal(counters.numpy(), want)
