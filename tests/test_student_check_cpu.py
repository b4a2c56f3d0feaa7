"""The --student_check monitor without a GPU: the NumPy restatement of the counter rules (tests/student_check_ref.py)
on hand-written cases, seg_helper.student_check_torch against it with exact equality on the shapes of the GPU test, the summary on
constructed counters, and the flags, formatters, read_interval and host-trainer plumbing."""
import functools
import json
import math

import numpy as np
import pytest
import torch

import student_check_ref as ref


def _bits(v):
    return int(np.float32(v).view(np.uint32))


def _hand(B=1, K=3, h=2, present=((1, 1),)):
    """small tensors of distinct values, a == b"""
    lab = np.array(present, dtype=np.float32)
    mk = lambda *s: (np.arange(int(np.prod(s)), dtype=np.float32).reshape(s) * 0.25 + 1.0)
    pair = lambda x: (x.copy(), x.copy())
    return dict(seg=pair(mk(B, K, h, h)), cam=pair(mk(B, K - 1, h, h)), cam_aux=pair(mk(B, K - 1, h, h) + 7), cls=pair(mk(B, K - 1) - 1.5),
                cls_aux=pair(mk(B, K - 1)), losses=pair(np.array([0.5, 0.25, 1.0, 2.0], dtype=np.float32)), cls_label=lab, K=K)


def test_identical_tensors_give_zero_differences_and_full_agreement():
    d = _hand()
    off, n = ref.layout(3)
    c = ref.ref_of_case(d)
    assert len(c) == n == 62 + 6 and c[off["checks"]] == 1 and c[off["flags"]] == 0
    for t in ref.TENSORS:
        assert c[off[t + ".max_abs"]] == 0 and c[off[t + ".sum_d2"]] == 0 and c[off[t + ".nonfinite_a"]] == c[off[t + ".nonfinite_b"]] == 0
        assert c[off[t + ".sum_b2"]] > 0 and c[off[t + ".range"]] > 0
    assert c[off["seg.n"]] == 12 and c[off["cam.n"]] == 8 and c[off["cls.n"]] == 2
    assert c[off["cells"]] == 4 and c[off["differ"]] == 0 and c[off["flip_hist"]:off["flip_hist"] + 4] == [0, 0, 0, 0]
    assert c[off["labelled"]:off["labelled"] + 3] == c[off["agree"]:off["agree"] + 3] == [0, 0, 4]          # the values grow with the channel
    assert c[off["cls.sign_flips"]] == c[off["cls_aux.sign_flips"]] == 0 and c[off["cls_cols"]] == 2
    for l in ref.LOSSES:
        assert c[off[l + ".sum_d"]] == 0 and c[off[l + ".max_abs"]] == 0 and c[off[l + ".n"]] == 1
    assert c[off["seg_loss.sum_b"]] == 1 << 32 and c[off["cls_loss_aux.sum_b"]] == 1 << 30
    # the fixed-point sums are what the rule says: sum b^2 of the cam tensor, 2^-20 units
    want = sum(int(np.rint(np.float64(np.float32(v * v)) * 2.0 ** 20)) for v in d["cam"][1].reshape(-1))
    assert c[off["cam.sum_b2"]] == want
    # a second check accumulates
    c2 = ref.ref_of_case(d, c)
    assert c2[off["checks"]] == 2 and c2[off["cells"]] == 8 and c2[off["cam.sum_b2"]] == 2 * want and c2[off["cam.range"]] == c[off["cam.range"]]


def test_one_moved_element_shows_in_exactly_one_tensor():
    d = _hand()
    base = ref.ref_of_case(d)
    off, _ = ref.layout(3)
    d["cam_aux"][0][0, 1, 1, 0] += np.float32(0.5)                                         # the training pass's value: b's sums stay
    c = ref.ref_of_case(d)
    changed = {k for k, v in off.items() if c[v] != base[v]}
    assert changed == {"cam_aux.max_abs", "cam_aux.sum_d2"}
    assert c[off["cam_aux.max_abs"]] == _bits(0.5) and c[off["cam_aux.sum_d2"]] == 1 << 30                # 0.25 x 2^32


def test_a_tie_takes_the_lowest_index_and_bins_by_the_check_margin():
    d = _hand(K=4, present=((1, 1, 1),))
    off, _ = ref.layout(4)
    a, b = d["seg"]
    a[0, :, 0, 0] = [5, 9, 9, 1]                                                            # tie 1 / 2 -> 1
    b[0, :, 0, 0] = [5, 9, 9, 9]                                                            # tie 1 / 2 / 3 -> 1: agree
    a[0, :, 0, 1] = [5, 1, 9, 9.5]                                                          # -> 3
    b[0, :, 0, 1] = [5, 1, 9, 9]                                                            # tie -> 2: differ, margin 0
    a[0, :, 1, 0] = [5, 1, 2, 3]                                                            # -> 0
    b[0, :, 1, 0] = [5, 5.05, 2, 3]                                                         # -> 1, margin 0.05: bin 2
    a[0, :, 1, 1] = [np.nan, 1, 2, 3]                                                       # NaN reads as -inf -> 3
    b[0, :, 1, 1] = [7, 1, 2, 3]                                                            # -> 0, margin 4: bin 3
    c = ref.ref_of_case(d)
    assert c[off["cells"]] == 4 and c[off["differ"]] == 3 and c[off["flip_hist"]:off["flip_hist"] + 4] == [1, 0, 1, 1]
    assert c[off["labelled"]:off["labelled"] + 4] == [1, 2, 1, 0] and c[off["agree"]:off["agree"] + 4] == [0, 1, 0, 0]
    assert c[off["seg.nonfinite_a"]] == 1 and c[off["seg.nonfinite_b"]] == 0 and c[off["flags"]] == 1


def test_an_image_without_a_class_allows_background_only():
    d = _hand(present=((0, 0),))
    off, _ = ref.layout(3)
    d["seg"][0][0, 1:] = 100.0                                                             # a's absent channels would win: not allowed
    d["seg"][1][0, 2, 0, 0] = np.nan                                                       # never read
    d["cam"][1][:] = np.inf
    c = ref.ref_of_case(d)
    assert c[off["seg.n"]] == 4 and c[off["cam.n"]] == c[off["cam_aux.n"]] == c[off["cls.n"]] == 0 and c[off["flags"]] == 0
    assert c[off["cells"]] == 4 and c[off["differ"]] == 0 and c[off["labelled"]] == c[off["agree"]] == 4
    assert c[off["seg.max_abs"]] == 0 and c[off["cls_cols"]] == 2


def test_terms_outside_the_range_set_the_flag_and_add_nothing():
    d = _hand()
    off, _ = ref.layout(3)
    base = ref.ref_of_case(d)
    d["cls"][0][0, 0] += np.float32(40.0)                                                  # |a - b|^2 = 1600 >= 2^10
    d["losses"][1][3] = np.float32(np.inf)
    c = ref.ref_of_case(d)
    assert c[off["flags"]] == (1 << 3) | (1 << 11) and c[off["cls.sum_d2"]] == 0 and c[off["cls.max_abs"]] == _bits(40.0)
    assert c[off["cls.sum_b2"]] == base[off["cls.sum_b2"]]
    assert c[off["cam_loss.sum_d"]] == c[off["cam_loss.sum_b"]] == c[off["cam_loss.max_abs"]] == 0 and c[off["cam_loss.n"]] == 1


@functools.lru_cache(maxsize=None)
def _case_and_ref(name):
    d = ref.make_case(name)
    return d, ref.ref_of_case(d)


def _torch_call(fn, d, counters, dev=None):
    t = lambda p: tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev or "cpu") for x in p)
    return fn(t(d["seg"]), t(d["cam"]), t(d["cam_aux"]), t(d["cls"]), t(d["cls_aux"]), t(d["losses"]),
              torch.from_numpy(d["cls_label"]).to(dev or "cpu"), counters)


@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_torch_restatement_equals_the_numpy_one(name):
    from cosa_amd.utils import seg_helper
    d, want = _case_and_ref(name)
    K = d["K"]
    off, n = seg_helper.student_check_layout(K)
    assert (off, n) == ref.layout(K)
    # the case hits what it was built to hit
    assert all(v > 0 for v in want[off["flip_hist"]:off["flip_hist"] + 4]) and want[off["differ"]] < want[off["cells"]]
    assert want[off["seg.nonfinite_a"]] == 1 and want[off["seg.nonfinite_b"]] == 1 and want[off["cam.nonfinite_a"]] == 1
    assert want[off["cam_aux.nonfinite_b"]] == 1 and want[off["cls.nonfinite_b"]] == 1 and want[off["cls_aux.nonfinite_a"]] == 1
    assert want[off["flags"]] == 0b11111 and want[off["labelled"]] >= ref.SHAPES[name][2] ** 2      # the image without a class: all background
    c = seg_helper.new_student_check(K, "cpu")
    assert _torch_call(seg_helper.student_check_torch, d, c) is c
    got = c.tolist()
    assert got == want, [(k, got[v], want[v]) for k, v in off.items() if got[v] != want[v]]
    _torch_call(seg_helper.student_check_torch, d, c)                                       # accumulates: sums double, maxima stay
    want2 = ref.ref_of_case(d, want)
    assert c.tolist() == want2 and want2[off["checks"]] == 2 and want2[off["seg.max_abs"]] == want[off["seg.max_abs"]]


def test_shape_checks_raise_value_error():
    from cosa_amd.utils import seg_helper
    d, _ = _case_and_ref("small")
    c = seg_helper.new_student_check(d["K"], "cpu")
    with pytest.raises(ValueError):
        _torch_call(seg_helper.student_check_torch, d, c[:-1].clone())
    bad = dict(d, cam=(d["cam"][0][:, :-1], d["cam"][1][:, :-1]))
    with pytest.raises(ValueError):
        _torch_call(seg_helper.student_check_torch, bad, c)
    with pytest.raises(ValueError):
        seg_helper.student_check_layout(257)
    with pytest.raises(ValueError):
        seg_helper.student_check_layout(1)
    assert seg_helper.student_check_layout(256)[1] == 62 + 512


def test_summary_on_constructed_counters():
    from cosa_amd.utils import seg_helper
    K = 4
    off, n = seg_helper.student_check_layout(K)
    c = [0] * n
    c[off["checks"]], c[off["flags"]] = 3, 1 << 9
    c[off["seg.n"]], c[off["seg.sum_d2"]], c[off["seg.sum_b2"]] = 100, 4 << 32, 400 << 20                    # sqrt(4 / 400) = 0.1
    c[off["seg.max_abs"]], c[off["seg.range"]], c[off["seg.nonfinite_b"]] = _bits(0.75), _bits(12.5), 2
    c[off["cam.sum_d2"]], c[off["cam.sum_b2"]] = 1 << 32, 0                                                  # an empty denominator: 0.0
    c[off["cells"]], c[off["differ"]] = 1000, 10
    c[off["flip_hist"]:off["flip_hist"] + 4] = [6, 2, 1, 1]
    c[off["labelled"]:off["labelled"] + K] = [500, 0, 300, 200]
    c[off["agree"]:off["agree"] + K] = [500, 0, 294, 196]
    c[off["cls.sign_flips"]], c[off["cls_aux.sign_flips"]], c[off["cls_cols"]] = 1, 2, 60
    c[off["seg_loss.sum_d"]], c[off["seg_loss.sum_b"]], c[off["seg_loss.max_abs"]], c[off["seg_loss.n"]] = 3 << 22, 3 << 32, _bits(0.002), 3
    c[off["cls_loss.sum_d"]], c[off["cls_loss.sum_b"]], c[off["cls_loss.n"]] = 1 << 20, 1 << 32, 3
    s = seg_helper.student_check_summary(c, K)
    assert s["checks"] == 3 and s["flags"] == 512 and s["seg"]["rel_l2"] == pytest.approx(0.1, rel=1e-12) and s["seg"]["max_abs"] == 0.75
    assert s["seg"]["range"] == 12.5 and s["seg"]["nonfinite_b"] == 2 and s["seg"]["nonfinite_a"] == 0 and s["cam"]["rel_l2"] == 0.0
    assert s["seg_agree"] == 0.99 and s["flip_hist"] == [6, 2, 1, 1] and s["class_agree"] == [1.0, None, 0.98, 0.98]
    assert s["cls_sign_flips"] == 1 and s["cls_aux_sign_flips"] == 2
    assert s["losses"]["seg_loss"]["loss_rel"] == 2.0 ** -10 and s["losses"]["cls_loss"]["loss_rel"] == 2.0 ** -12
    assert s["losses"]["cam_loss"]["loss_rel"] == 0.0 and s["loss_rel"] == 2.0 ** -10 and s["losses"]["seg_loss"]["n"] == 3
    assert s["losses"]["seg_loss"]["max_abs"] == float(np.float32(0.002))
    json.dumps(s)
    with pytest.raises(ValueError):
        seg_helper.student_check_summary(c[:-1], K)
    empty = seg_helper.student_check_summary(torch.zeros(n, dtype=torch.int64), K)
    assert empty["checks"] == 0 and empty["seg_agree"] == 1.0 and empty["seg"]["rel_l2"] == 0.0 and not math.isnan(empty["loss_rel"])


def test_flags_parse_and_a_negative_interval_is_refused():
    from cosa_amd import args as cosa_args
    from cosa_amd import main as launcher
    from cosa_amd.train_step import default_args
    a, _ = cosa_args.parse(["EXP"])
    assert a.student_check_iters == 0 and a.student_check_mode == "fp32"
    d = default_args()
    assert d.student_check_iters == 0 and d.student_check_mode == "fp32"
    a, _ = cosa_args.parse(["EXP", "--student_check_iters", "50", "--student_check_mode", "bf16"])
    assert a.student_check_iters == 50 and a.student_check_mode == "bf16"
    launcher.check_supported(a)
    a, _ = cosa_args.parse(["EXP", "--student_check_iters", "-1"])
    with pytest.raises(ValueError):
        launcher.check_supported(a)


def test_log_line_and_jsonl_record(tmp_path):
    from types import SimpleNamespace
    from cosa_amd import monitors
    m, targs = monitors.BY_NAME["student_check"], SimpleNamespace(student_check_mode="fp32")
    summary = {"seg": {"rel_l2": 1.2e-3}, "seg_agree": 0.99987, "flip_hist": [4, 2, 1, 0], "loss_rel": 3.1e-4, "checks": 2}
    assert m.line(summary, targs) == " scheck[fp32]: seg rel 1.2e-03, agree 0.99987, flips>=1e-1 0, loss rel 3.1e-04"
    rec = json.loads(monitors.monitor_record(m, summary, 40, targs))
    assert rec["iters"] == 40 and rec["mode"] == "bf16" and rec["check_mode"] == "fp32" and rec["flip_hist"] == [4, 2, 1, 0]
    monitors.append_monitor(tmp_path, m, summary, 20, targs)
    monitors.append_monitor(tmp_path, m, summary, 40, targs)
    assert [json.loads(x)["iters"] for x in (tmp_path / "student_check.jsonl").read_text().splitlines()] == [20, 40]


@pytest.mark.parametrize("with_teacher_check", [False, True])
def test_read_interval_carries_and_zeroes_the_counters(with_teacher_check):
    from cosa_amd import main as launcher
    from cosa_amd import monitors
    from cosa_amd.utils import seg_helper, torch_helper
    K = 3
    _, n = seg_helper.student_check_layout(K)
    acc = torch.arange(8, dtype=torch.float64) * 20
    guard = torch_helper.new_guard_state("cpu")
    guard.view(torch.float32)[0] = 2.5
    guard[2:5] = torch.tensor([17, 2, 1])
    stats = torch.arange(4 * 3 + 7, dtype=torch.int64) + 100
    check = torch.arange(n, dtype=torch.int64) + 1000
    check[7] = (1 << 62) + 12345                                                           # a fixed-point sum past 2^53: exact all the same
    check[5] = 0x7f7fffff
    want = check.tolist()
    tc = None
    if with_teacher_check:
        tc = torch.arange(seg_helper.teacher_check_layout(K)[1], dtype=torch.int64) + 5
        tc_want = tc.tolist()
    on = dict(guard=guard, label_stats=stats, teacher_check=tc, student_check=check)
    vals, host = launcher.read_interval(acc, 20, [(m, on[m.name]) for m in monitors.MONITORS if on.get(m.name) is not None])
    assert set(host) == {"guard", "label_stats", "student_check"} | ({"teacher_check"} if with_teacher_check else set()) and acc.numel() == 8
    gvals, svals, tvals, cvals, scvals = (host.get(k) for k in ("guard", "label_stats", "tensor_stats", "teacher_check", "student_check"))
    assert vals == [float(i) for i in range(8)] and gvals == [2.5, 2.0, 1.0] and svals == list(range(100, 119)) and tvals is None
    assert scvals == want and all(isinstance(v, int) for v in scvals) and int(check.abs().sum()) == 0 and int(acc.abs().sum()) == 0
    assert cvals == (tc_want if with_teacher_check else None)
    # without the argument: what it was
    acc = torch.arange(8, dtype=torch.float64) * 20
    assert launcher.read_interval(acc, 20, []) == ([float(i) for i in range(8)], {})


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
        if mode == "fp16c8":
            raise NotImplementedError(mode)


def _host_trainer(monkeypatch, seed, **over):
    from cosa_amd import train_step
    monkeypatch.setattr(train_step, "build_model", lambda args: _TinyNet())
    args = train_step.default_args("VOC12", **dict(dict(crop_size=48, batch_size=3, num_classes=6, max_iters=100), **over))
    return train_step.CoSATrainer(args, torch.device("cpu"), seed=seed)


def test_host_trainer_state_and_its_trip_through_a_state_file(tmp_path, monkeypatch, capsys):
    from cosa_amd.utils import seg_helper
    off_tr = _host_trainer(monkeypatch, seed=1)
    assert off_tr.student_check_state is None and off_tr.student_check() is None and off_tr.model_SK is None
    a = _host_trainer(monkeypatch, seed=1, student_check_iters=2)
    assert a.args.student_check_mode == "fp32" and a.extra_state["student_check.counters"] is a.student_check_state
    assert a.student_check_state.shape == (62 + 12,) and int(a.student_check_state.abs().sum()) == 0
    with pytest.raises(ValueError):
        _host_trainer(monkeypatch, seed=1, student_check_iters=-2)
    with pytest.raises(ValueError):                                                     # no set_nograd_precision name
        _host_trainer(monkeypatch, seed=1, student_check_iters=2, student_check_mode="auto")
    with pytest.raises(NotImplementedError):                                            # at set-up, not in a step
        _host_trainer(monkeypatch, seed=1, student_check_iters=2, student_check_mode="fp16c8")
    both = _host_trainer(monkeypatch, seed=1, student_check_iters=2, teacher_check_iters=3)
    assert set(both.extra_state) == {"student_check.counters", "teacher_check.counters"}
    # the counters are state of the run
    d = ref.make_case("small")
    _torch_call(seg_helper.student_check_torch, d, a.student_check_state)
    want = a.student_check_state.clone()
    assert a.student_check()["checks"] == 1 and want.tolist() == ref.ref_of_case(d)
    path, without = str(tmp_path / "state_00000003.cosa"), str(tmp_path / "state_00000000.cosa")
    a.save_state(path, n_iter=2)
    a.wait_state()
    off_tr.save_state(without, n_iter=-1)
    off_tr.wait_state()
    c = _host_trainer(monkeypatch, seed=9, student_check_iters=2)
    held = c.student_check_state
    capsys.readouterr()
    assert c.load_state(path)["n_iter"] == 2 and "note:" not in capsys.readouterr().out
    assert c.student_check_state is held and torch.equal(held, want)
    c.load_state(without)
    assert "student check" in capsys.readouterr().out and int(c.student_check_state.abs().sum()) == 0
    e = _host_trainer(monkeypatch, seed=5)
    e.load_state(path)
    out = capsys.readouterr().out
    assert "student check" in out and "ignored" in out and e.student_check_state is None
