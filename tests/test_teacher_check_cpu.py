"""The --teacher_check monitor without a GPU: the flags, the counter layout, seg_helper.teacher_check_torch against a
brute-force numpy count written here, the summary on hand-made counters, the launcher's interval read and its log / jsonl lines, and a host
trainer's counters through a state file."""
import json
import struct

import numpy as np
import pytest
import torch

EDGES = [np.float32(e) for e in (1e-6, 1e-5, 1e-4, 3e-4, 1e-3, 3e-3, 1e-2)] + [np.float32(np.inf)]
BAR = np.float32(1e-3)


def _bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def brute_force(cams, auxs, tgts, labels, aux_labels, cls, boxes, K, ignore=255, bar=BAR):
    """the rules of cosa_teacher_check, one element at a time: -> {slot name: int or list of ints}"""
    out = {"checks": 1}
    for name, ab in (("cam", cams), ("aux", auxs), ("tgt", tgts)):
        planes = over = worst = bad_a = bad_b = 0
        hist = [0] * 8
        if ab is not None:
            a, b = ab
            for i in range(a.shape[0]):
                for c in range(a.shape[1]):
                    if cls is not None and cls[i, c] == 0:
                        continue
                    fig, nonfinite = np.float32(0), False
                    for x, y in zip(a[i, c].ravel(), b[i, c].ravel()):
                        fx, fy = bool(np.isfinite(x)), bool(np.isfinite(y))
                        bad_a, bad_b = bad_a + (not fx), bad_b + (not fy)
                        if fx and fy:
                            with np.errstate(over="ignore"):
                                fig = max(fig, np.abs(np.float32(x) - np.float32(y)))
                        else:
                            nonfinite = True
                    if nonfinite:
                        fig = np.float32(np.inf)
                    planes += 1
                    over += bool(fig > bar)
                    hist[next(k for k, e in enumerate(EDGES) if fig <= e)] += 1
                    worst = max(worst, _bits(fig))
        out.update({f"{name}.planes": planes, f"{name}.over": over, f"{name}.worst": worst, f"{name}.hist": hist,
                    f"{name}.nonfinite_a": bad_a, f"{name}.nonfinite_b": bad_b})
    for name, ab in (("main", labels), ("aux_label", aux_labels)):
        pix = agree = ign_a = ign_b = 0
        cnt_a, cnt_b, inter = [0] * K, [0] * K, [0] * K
        if ab is not None:
            a, b = ab
            S = a.shape[-1]
            is_cls = lambda v: v >= 0 and v < K and v == np.floor(v)
            for i, (y0, y1, x0, x1) in enumerate(boxes):
                for y in range(max(y0, 0), min(y1, S)):
                    for x in range(max(x0, 0), min(x1, S)):
                        va, vb = a[i, y, x], b[i, y, x]
                        pix += 1
                        agree += bool(va == vb)
                        ign_a, ign_b = ign_a + bool(va == ignore), ign_b + bool(vb == ignore)
                        if is_cls(va):
                            cnt_a[int(va)] += 1
                        if is_cls(vb):
                            cnt_b[int(vb)] += 1
                        if is_cls(va) and va == vb:
                            inter[int(va)] += 1
        out.update({f"{name}.pix": pix, f"{name}.agree": agree, f"{name}.ign_a": ign_a, f"{name}.ign_b": ign_b,
                    f"{name}.cnt_a": cnt_a, f"{name}.cnt_b": cnt_b, f"{name}.inter": inter})
    return out


def as_vector(d, K):
    from cosa_amd.utils import seg_helper
    off, n = seg_helper.teacher_check_layout(K)
    v = np.zeros(n, np.int64)
    for name, val in d.items():
        val = np.atleast_1d(np.asarray(val, np.int64))
        v[off[name]:off[name] + len(val)] = val
    return v


def edge_case_inputs():
    """B = 2, C = 5 (K = 6), S = 6, targets 3 x 3.  Planes of image 0: class 0 a figure exactly equal to the bar, class 1 one ulp above it,
    class 2 a NaN in pass A only, class 3 INACTIVE and full of garbage, class 4 identical.  Image 1: class 0 an inf in pass B, class 2
    a small figure; the rest inactive.  Image 1's box is partial; the label maps hold values that are no label."""
    rng = np.random.default_rng(3)
    B, C, S, h = 2, 5, 6, 3
    a = rng.random((B, C, S, S)).astype(np.float32)
    b = a.copy()
    bar, above = BAR, np.nextafter(BAR, np.float32(1))
    a[0, 0, 2, 3], b[0, 0, 2, 3] = np.float32(0), bar                                   # |a - b| == bar exactly: not over, bin 4
    a[0, 1, 1, 1], b[0, 1, 1, 1] = above, np.float32(0)                                 # one ulp above: over, bin 5
    a[0, 2, 4, 4] = np.nan                                                              # figure inf, last bin, nonfinite_a
    a[0, 3], b[0, 3] = np.float32(np.nan), np.float32(-np.inf)                          # inactive: never counted
    b[1, 0, 0, 5] = np.inf
    b[1, 2, 5, 0] = a[1, 2, 5, 0] + np.float32(2e-5)
    cls = np.array([[1, 1, 1, 0, 1], [1, 0, 2, 0, 0]], np.float32)                      # (any non-zero value is "present")
    aux_a = rng.random((B, C, S, S)).astype(np.float32)
    aux_b = (aux_a + np.float32(5e-3) * rng.random((B, C, S, S)).astype(np.float32)).astype(np.float32)
    tgt_a = rng.random((B, C, h, h)).astype(np.float32)
    tgt_b = tgt_a.copy()
    tgt_b[1, 2, 1, 1] += np.float32(4e-4)
    K = C + 1
    la = rng.integers(0, K, (B, S, S)).astype(np.float32)
    lb = la.copy()
    lb[0, 0, :4] = 255
    la[0, 1, 0] = 255
    lb[1, 3, 3] = (la[1, 3, 3] + 1) % K
    la[1, 2, 2], lb[1, 2, 2] = 2.5, 2.5                                                 # no label, the same in both: agree only
    la[0, 5, 5] = -1                                                                    # no label
    lb[1, 4, 4] = np.nan
    la[1, 3, 2] = K                                                                     # no label (one past the last class)
    aux_la = rng.integers(0, K, (B, S, S)).astype(np.float32)
    aux_lb = np.where(rng.random((B, S, S)) < 0.2, 255, aux_la).astype(np.float32)
    boxes = [[0, S, 0, S], [1, 5, 2, 6]]
    return dict(cams=(a, b), auxs=(aux_a, aux_b), tgts=(tgt_a, tgt_b), labels=(la, lb), aux_labels=(aux_la, aux_lb), cls=cls, boxes=boxes, K=K)


def _torch_call(d, counters, fn=None, **over):
    from cosa_amd.utils import seg_helper
    d = dict(d, **over)
    t = lambda p: tuple(torch.from_numpy(np.ascontiguousarray(x)) for x in p) if p is not None else None
    fn = fn or seg_helper.teacher_check_torch
    return fn(t(d["cams"]), t(d["auxs"]), t(d["tgts"]), t(d["labels"]), t(d["aux_labels"]),
              torch.from_numpy(d["cls"]) if d["cls"] is not None else None, d["boxes"], counters)


def test_flags_parse_and_auto_resolves():
    from cosa_amd import args as cosa_args
    from cosa_amd.train_step import default_args, resolve_teacher_check_mode
    a, changed = cosa_args.parse(["EXP"])
    assert a.teacher_check_iters == 0 and a.teacher_check_mode == "auto" and "teacher_check_iters" not in changed
    a, changed = cosa_args.parse(["EXP", "--teacher_check_iters", "100", "--teacher_check_mode", "fp16c8-x2"])
    assert a.teacher_check_iters == 100 and a.teacher_check_mode == "fp16c8-x2" and changed["teacher_check_iters"] == 100
    d = default_args("VOC12")
    assert d.teacher_check_iters == 0 and d.teacher_check_mode == "auto"
    assert default_args("VOC12", **{k: v for k, v in vars(a).items() if k != "dataset"}).teacher_check_iters == 100
    assert resolve_teacher_check_mode("auto", "fp16x3") == "bf16x3"
    for other in ("bf16", "fp16", "bf16x3", "fp16c8-x2", "fp16c4"):
        assert resolve_teacher_check_mode("auto", other) == "fp16x3"
    assert resolve_teacher_check_mode("bf16", "fp16x3") == "bf16"


def test_check_supported_refuses_a_negative_interval():
    from cosa_amd import args as cosa_args
    from cosa_amd import main as launcher
    a, _ = cosa_args.parse(["EXP", "--teacher_check_iters", "-1"])
    with pytest.raises(ValueError, match="teacher_check_iters"):
        launcher.check_supported(a)
    a, _ = cosa_args.parse(["EXP", "--teacher_check_iters", "3"])
    launcher.check_supported(a)


def test_layout_needs_no_device():
    from cosa_amd.utils import seg_helper
    for K in (2, 21, 81, 256):
        off, n = seg_helper.teacher_check_layout(K)
        assert n == 48 + 6 * K and list(off) == list(seg_helper.TEACHER_CHECK_SLOTS) and off["checks"] == 0
        order = sorted(off.values())
        assert order == [off[s] for s in seg_helper.TEACHER_CHECK_SLOTS] and len(set(order)) == len(order)
        assert off["cam.hist"] - off["cam.worst"] == 1 and off["cam.nonfinite_a"] - off["cam.hist"] == 8
        assert off["main.cnt_b"] - off["main.cnt_a"] == K and n - off["aux_label.inter"] == K
        assert seg_helper.new_teacher_check(K, "cpu").shape == (n,)
    for bad in (1, 257):
        with pytest.raises(ValueError):
            seg_helper.teacher_check_layout(bad)


def test_torch_restatement_against_a_brute_force_count():
    from cosa_amd.utils import seg_helper
    d = edge_case_inputs()
    K = d["K"]
    want = brute_force(d["cams"], d["auxs"], d["tgts"], d["labels"], d["aux_labels"], d["cls"], d["boxes"], K)
    # the inputs hit what they were built to hit
    assert want["cam.planes"] == 6 and want["cam.over"] == 3 and want["cam.hist"] == [1, 0, 1, 0, 1, 1, 0, 2]
    assert want["cam.nonfinite_a"] == 1 and want["cam.nonfinite_b"] == 1 and want["cam.worst"] == 0x7f800000
    assert want["tgt.hist"][3] == 0 and want["tgt.over"] == 0 and 0 < want["tgt.worst"] < _bits(1e-3)
    assert want["main.pix"] == 36 + 16 and want["main.ign_b"] == 4 and want["main.ign_a"] == 1
    assert sum(want["main.cnt_a"]) + want["main.ign_a"] == want["main.pix"] - 3            # 2.5, -1 and K are counted nowhere
    counters = seg_helper.new_teacher_check(K, "cpu")
    assert _torch_call(d, counters) is counters
    assert np.array_equal(counters.numpy(), as_vector(want, K))
    # a second call accumulates: sums add, worst is a maximum
    _torch_call(d, counters, cams=(d["cams"][0], d["cams"][0]))
    second = brute_force((d["cams"][0], d["cams"][0]), d["auxs"], d["tgts"], d["labels"], d["aux_labels"], d["cls"], d["boxes"], K)
    both = as_vector(want, K) + as_vector(second, K)
    off, _ = seg_helper.teacher_check_layout(K)
    for s in seg_helper.TEACHER_CHECK_SETS:
        both[off[s + ".worst"]] = max(want[s + ".worst"], second[s + ".worst"])
    assert np.array_equal(counters.numpy(), both)


def test_torch_restatement_with_absent_pairs_and_every_plane_active():
    from cosa_amd.utils import seg_helper
    d = edge_case_inputs()
    K = d["K"]
    want = brute_force(d["cams"], d["auxs"], None, d["labels"], None, None, d["boxes"], K)
    assert want["cam.planes"] == 10 and want["tgt.planes"] == 0 and want["aux_label.pix"] == 0
    counters = seg_helper.new_teacher_check(K, "cpu")
    _torch_call(d, counters, tgts=None, aux_labels=None, cls=None)
    assert np.array_equal(counters.numpy(), as_vector(want, K))
    with pytest.raises(ValueError):
        _torch_call(d, seg_helper.new_teacher_check(K + 1, "cpu"))
    with pytest.raises(ValueError):
        _torch_call(d, counters, labels=(d["labels"][0][:, :-1], d["labels"][1][:, :-1]))


def test_summary_on_hand_made_counters():
    from cosa_amd.utils import seg_helper
    K = 4
    off, n = seg_helper.teacher_check_layout(K)
    c = np.zeros(n, np.int64)
    c[off["checks"]] = 3
    c[off["cam.planes"]], c[off["cam.over"]], c[off["cam.worst"]] = 12, 0, _bits(np.float32(3.1e-4))
    c[off["cam.hist"]:off["cam.hist"] + 8] = [0, 2, 6, 3, 1, 0, 0, 0]
    c[off["aux.planes"]], c[off["aux.over"]], c[off["aux.worst"]] = 12, 2, 0x7f800000
    c[off["aux.hist"]:off["aux.hist"] + 8] = [0, 0, 10, 0, 0, 1, 0, 1]
    c[off["aux.nonfinite_b"]] = 7
    c[off["main.pix"]], c[off["main.agree"]], c[off["main.ign_a"]], c[off["main.ign_b"]] = 10000, 9995, 100, 102
    c[off["main.cnt_a"]:off["main.cnt_a"] + K] = [5000, 4900, 0, 0]                      # classes 2 and 3 absent from both maps
    c[off["main.cnt_b"]:off["main.cnt_b"] + K] = [5001, 4897, 0, 0]
    c[off["main.inter"]:off["main.inter"] + K] = [4999, 4896, 0, 0]
    s = seg_helper.teacher_check_summary(c.astype(np.float64).tolist(), K)               # as the launcher reads them: doubles
    assert s["checks"] == 3 and s["exemption_evaluated"] is False and "NOT evaluated" in s["criterion"] and s["bar"] == 1e-3
    assert s["cam"] == {"planes": 12, "over": 0, "worst": float(np.float32(3.1e-4)), "worst_bits": _bits(np.float32(3.1e-4)),
                        "hist": [0, 2, 6, 3, 1, 0, 0, 0], "nonfinite_a": 0, "nonfinite_b": 0}
    assert s["aux"]["worst"] == "inf" and s["aux"]["over"] == 2 and s["aux"]["nonfinite_b"] == 7 and s["tgt"]["planes"] == 0
    assert s["main"]["agree"] == 0.9995 and s["main"]["iou"] == [4999 / 5002, 4896 / 4901, None, None]
    assert s["main"]["miou"] == (4999 / 5002 + 4896 / 4901) / 2 and s["main"]["ign_b"] == 102
    assert s["aux_label"] == {"pix": 0, "agree": 1.0, "miou": 1.0, "iou": [None] * K, "ign_a": 0, "ign_b": 0}       # pix = 0: no NaN
    assert s["conforms"] is False and s["conforms_without_tgt"] is False
    json.dumps(s)                                                                        # (inf is spelled out: the record is strict JSON)
    w = seg_helper.teacher_check_worst(s)
    assert w == {"worst": float("inf"), "over": 2, "planes": 24, "agree": 0.9995, "miou": s["main"]["miou"]}
    # the same without the failing set: conforms -- and one pixel of agreement less than the bar does not
    c[off["aux.over"]], c[off["aux.worst"]] = 0, _bits(np.float32(1e-3))
    assert seg_helper.teacher_check_summary(c, K)["conforms"] is True
    c[off["tgt.planes"]], c[off["tgt.over"]] = 12, 5                                     # the targets alone over the bar
    t = seg_helper.teacher_check_summary(c, K)
    assert t["conforms"] is False and t["conforms_without_tgt"] is True
    c[off["tgt.over"]] = 0
    c[off["main.agree"]] = 9989
    assert seg_helper.teacher_check_summary(c, K)["conforms"] is False
    z = seg_helper.teacher_check_summary(np.zeros(n, np.int64), K)
    assert z["checks"] == 0 and z["conforms"] is None and z["conforms_without_tgt"] is None and z["cam"]["worst"] == 0.0
    with pytest.raises(ValueError):
        seg_helper.teacher_check_summary(np.zeros(n + 1, np.int64), K)


def test_log_line_and_jsonl_record(tmp_path):
    from types import SimpleNamespace
    from cosa_amd import monitors
    from cosa_amd.utils import seg_helper
    m, targs = monitors.BY_NAME["teacher_check"], SimpleNamespace(teacher_precision="fp16x3", teacher_check_mode="bf16x3")
    K = 3
    off, n = seg_helper.teacher_check_layout(K)
    c = np.zeros(n, np.int64)
    c[off["checks"]] = 1
    for s_, w_ in (("cam", 3.1e-4), ("aux", 2e-4), ("tgt", 1e-5)):
        c[off[s_ + ".planes"]], c[off[s_ + ".worst"]] = 28, _bits(np.float32(w_))
    for p in ("main", "aux_label"):
        c[off[p + ".pix"]], c[off[p + ".agree"]] = 100000, 99987 if p == "main" else 99999
        c[off[p + ".cnt_a"]:off[p + ".cnt_a"] + K] = [50000, 50000, 0]
        c[off[p + ".cnt_b"]:off[p + ".cnt_b"] + K] = [50000, 50000, 0]
        c[off[p + ".inter"]:off[p + ".inter"] + K] = [49995, 49996, 0]
    s = seg_helper.teacher_check_summary(c, K)
    miou = (49995 / 50005 + 49996 / 50004) / 2
    assert m.line(s, targs) == " tcheck[bf16x3]: worst 3.1e-04, over 0/84, agree 0.99987, miou %.5f" % miou
    rec = monitors.monitor_record(m, s, 40, targs)
    assert "\n" not in rec
    rec = json.loads(rec)
    assert rec["iters"] == 40 and rec["mode"] == "fp16x3" and rec["check_mode"] == "bf16x3" and rec["checks"] == 1
    assert rec["cam"]["planes"] == 28 and rec["exemption_evaluated"] is False and rec["conforms"] is True
    for it in (20, 40):
        monitors.append_monitor(tmp_path, m, s, it, targs)
    assert [json.loads(x)["iters"] for x in (tmp_path / "teacher_check.jsonl").read_text().splitlines()] == [20, 40]


def _interval_inputs():
    from cosa_amd.utils import torch_helper
    acc = torch.arange(8, dtype=torch.float64) * 20
    guard = torch_helper.new_guard_state("cpu")
    guard.view(torch.float32)[0] = 2.5
    guard[2:5] = torch.tensor([17, 2, 1])
    stats = torch.arange(4 * 3 + 7, dtype=torch.int64) + 100
    return acc, guard, stats


def _on(**tensors):
    """read_interval's monitor list of what is given (not None), in the table's order"""
    from cosa_amd import monitors
    return [(m, tensors[m.name]) for m in monitors.MONITORS if tensors.get(m.name) is not None]


def test_read_interval_without_the_argument_is_what_it_was():
    from cosa_amd import main as launcher
    acc, guard, stats = _interval_inputs()
    vals, host = launcher.read_interval(acc, 20, _on(guard=guard, label_stats=stats))
    assert set(host) == {"guard", "label_stats"} and vals == [float(i) for i in range(8)] and host["guard"] == [2.5, 2.0, 1.0]
    assert host["label_stats"] == list(range(100, 119))
    acc, _, _ = _interval_inputs()
    out = launcher.read_interval(acc, 20, [])
    assert out == ([float(i) for i in range(8)], {})
    acc, guard, stats = _interval_inputs()
    table, blame = torch.arange(12, dtype=torch.float64).reshape(2, 6), torch.tensor([5, 0])
    _, host = launcher.read_interval(acc, 20, _on(guard=guard, label_stats=stats, tensor_stats=(table, blame)))
    assert set(host) == {"guard", "label_stats", "tensor_stats"} and host["tensor_stats"][1] == [5, 0] and len(host["tensor_stats"][0]) == 2


@pytest.mark.parametrize("with_tensor_stats", [False, True])
def test_read_interval_carries_and_zeroes_the_check_counters(with_tensor_stats):
    from cosa_amd import main as launcher
    from cosa_amd.utils import seg_helper
    K = 3
    _, n = seg_helper.teacher_check_layout(K)
    acc, guard, stats = _interval_inputs()
    check = torch.arange(n, dtype=torch.int64) + 1000
    check[3] = 0x7f800000                                                               # a bit pattern: exact through the double
    ts = (torch.arange(12, dtype=torch.float64).reshape(2, 6), torch.tensor([5, 0])) if with_tensor_stats else None
    vals, host = launcher.read_interval(acc, 20, _on(guard=guard, label_stats=stats, tensor_stats=ts, teacher_check=check))
    assert set(host) == {"guard", "label_stats", "teacher_check"} | ({"tensor_stats"} if with_tensor_stats else set())
    gvals, svals, tvals, cvals = host["guard"], host["label_stats"], host.get("tensor_stats"), host["teacher_check"]
    assert vals == [float(i) for i in range(8)] and gvals == [2.5, 2.0, 1.0] and svals == list(range(100, 119))
    want = list(range(1000, 1000 + n))
    want[3] = 0x7f800000
    assert cvals == want and all(isinstance(v, int) for v in cvals) and int(check.abs().sum()) == 0
    if with_tensor_stats:
        assert tvals[1] == [5, 0] and len(tvals[0]) == 2 and len(tvals[0][0]) == 6
    else:
        assert tvals is None


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
        self.refused = None

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
    assert off_tr.teacher_check_state is None and off_tr.teacher_check() is None and not hasattr(off_tr, "extra_state")
    a = _host_trainer(monkeypatch, seed=1, teacher_check_iters=2)
    assert a.args.teacher_check_mode == "bf16x3" and a.args.teacher_precision == "fp16x3"
    assert a.extra_state["teacher_check.counters"] is a.teacher_check_state and int(a.teacher_check_state.abs().sum()) == 0
    assert _host_trainer(monkeypatch, seed=1, teacher_check_iters=2, teacher_precision="bf16").args.teacher_check_mode == "fp16x3"
    with pytest.raises(NotImplementedError):                                            # at set-up, not in a step
        _host_trainer(monkeypatch, seed=1, teacher_check_iters=2, teacher_check_mode="fp16c8")
    with pytest.raises(ValueError):
        _host_trainer(monkeypatch, seed=1, teacher_check_iters=-2)
    # which steps check: the one closing every N-th optimizer iteration; with --accum_steps its last micro-batch
    assert [a._is_check_step(i) for i in range(4)] == [False, True, False, True]
    b = _host_trainer(monkeypatch, seed=1, teacher_check_iters=2, accum_steps=3)
    seen = []
    for k in range(3):
        b._micro_k = k
        seen.append(b._is_check_step(1))
    assert seen == [False, False, True] and not b._is_check_step(0)
    b._micro_k = 0
    # the counters are state of the run
    d = edge_case_inputs()
    _torch_call(d, a.teacher_check_state)
    want = a.teacher_check_state.clone()
    assert a.teacher_check()["checks"] == 1
    path, without = str(tmp_path / "state_00000003.cosa"), str(tmp_path / "state_00000000.cosa")
    a.save_state(path, n_iter=2)
    a.wait_state()
    off_tr.save_state(without, n_iter=-1)
    off_tr.wait_state()
    c = _host_trainer(monkeypatch, seed=9, teacher_check_iters=2)
    held = c.teacher_check_state
    capsys.readouterr()
    assert c.load_state(path)["n_iter"] == 2 and "note:" not in capsys.readouterr().out
    assert c.teacher_check_state is held and torch.equal(held, want)
    c.load_state(without)
    assert "check counters start at zero" in capsys.readouterr().out and int(c.teacher_check_state.abs().sum()) == 0
    e = _host_trainer(monkeypatch, seed=5)
    e.load_state(path)
    out = capsys.readouterr().out
    assert "teacher check" in out and "ignored" in out and e.teacher_check_state is None
    for p, q in zip(a.student.parameters(), e.student.parameters()):
        assert torch.equal(p, q)
