"""Per-step pseudo-label statistics on the GPU: cosa_label_stats against the numpy yardstick
(tests/label_stats_ref.py) -- every comparison of counters is exact integer equality --, then the trainer: the flag changes no bit of a
step, a non-finite teacher CAM is refused through the gradient guard, and the counters resume with the run."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import label_stats_ref as R

pytestmark = pytest.mark.gpu

# B, K, S, h = w: every tap clamps | - | a class index beyond one wavefront's lanes | the envelope's edge | S no multiple of 4: the scalar
# loads and the row tail (X + k < S), and 650 items per image: wavefronts that span two images
SHAPES = {"K5": (3, 5, 48, 3), "K21": (2, 21, 64, 4), "K81": (2, 81, 80, 5), "K128": (1, 128, 32, 2), "S50": (2, 5, 50, 3)}
INTEGER_LOGITS = "K21"                       # small-integer logits: ties between classes, the first maximum decides


def _oracle():
    from oracle import c_oracle
    c_oracle.build()
    return c_oracle


@functools.lru_cache(maxsize=None)
def _case(name):
    """the calls of one shape: the four box kinds and the three label kinds dealt over its images, as many calls as it takes to use each
    once -> [(inputs, reference counters)], computed once and shared"""
    B, K, S, h = SHAPES[name]
    oc = _oracle()
    calls = []
    for i in range(math.ceil(4 / B)):
        boxes = tuple(R.BOX_KINDS[(i * B + b) % 4] for b in range(B))
        labels = tuple(R.LABEL_KINDS[(i + b) % 3] for b in range(B))
        d = R.draw(oc, B, K, S, h, seed=100 * len(name) + i, box_kinds=boxes, label_kinds=labels, integer_logits=name == INTEGER_LOGITS)
        d = {k: np.ascontiguousarray(v) for k, v in d.items()}
        calls.append((d, R.reference(oc, d["mask_main"], d["mask_aux"], d["seg"], d["cls"], d["boxes"], d["cam"], d["cam_aux"])))
    return calls


def _dev(d):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(v).to(dev) for k, v in d.items()}


def _run(t, counters, aux=True, cams=True, scale=None):
    from cosa_amd.utils import seg_helper
    return seg_helper.label_stats(t["mask_main"], t["mask_aux"] if aux else None, t["seg"], t["cls"], t["boxes"], t["cam"] if cams else None,
                                  t["cam_aux"] if cams else None, counters, step_scale=scale)


@pytest.mark.parametrize("name", list(SHAPES))
def test_counters_equal_the_numpy_reference(name):
    from cosa_amd.utils import seg_helper
    K = SHAPES[name][1]
    off, n = R.layout(K)
    calls = _case(name)
    assert {tuple(b) == (0, SHAPES[name][2], 0, SHAPES[name][2]) for d, _ in calls for b in d["boxes"]} == {True, False}
    assert any((d["boxes"][:, 1] - d["boxes"][:, 0] == 1).any() for d, _ in calls) and any((d["boxes"][:, 1] == d["boxes"][:, 0]).any() for d, _ in calls)
    assert any((d["cls"].sum(1) == 0).any() for d, _ in calls) and any((d["cls"].sum(1) == K - 1).any() for d, _ in calls)
    counters = seg_helper.new_label_stats(K, torch.device("cuda", 0))
    total = np.zeros(n, np.int64)
    for i, (d, want) in enumerate(calls):          # the calls accumulate: after each, the counters are exactly the sum of the references so far
        scale = _run(_dev(d), counters)
        total += want
        got = counters.cpu().numpy()
        assert np.array_equal(got, total), np.nonzero(got != total)[0]
        assert scale.view(torch.int32).item() == 0x3f800000          # the bits of 1.0f
    assert total[off["steps"]] == len(calls) and total[off["main"] + K] > 0 and total[off["agree"]] > 0
    assert 0 < total[off["inter"]:off["inter"] + K].sum() < total[off["pred"]:off["pred"] + K].sum()
    if name == INTEGER_LOGITS:                       # the ties are there: some pixel's two largest resized logits are equal
        d = calls[0][0]
        assert R.top_two_margin(R.resized_logits(_oracle(), d["seg"], d["cls"], SHAPES[name][2])) == 0.0


@pytest.mark.parametrize("name", ["K5", "K21"])
def test_null_inputs_leave_their_slots_untouched(name):
    from cosa_amd.utils import seg_helper
    K = SHAPES[name][1]
    off, n = R.layout(K)
    d, _ = _case(name)[0]
    oc = _oracle()
    t = _dev(d)
    sentinel = 7
    for aux, cams in ((False, True), (True, False), (False, False)):
        want = R.reference(oc, d["mask_main"], d["mask_aux"] if aux else None, d["seg"], d["cls"], d["boxes"], d["cam"] if cams else None,
                           d["cam_aux"] if cams else None)
        counters = torch.full((n,), sentinel, dtype=torch.int64, device=t["seg"].device)
        scale = _run(t, counters, aux=aux, cams=cams)
        got = counters.cpu().numpy() - sentinel
        assert np.array_equal(got, want), (aux, cams, np.nonzero(got != want)[0])
        if not aux:
            assert not got[off["aux"]:off["aux"] + K + 1].any() and got[off["agree"]] == 0
        assert scale.view(torch.int32).item() == 0x3f800000


def test_unaligned_views_take_the_scalar_loads_and_a_value_that_is_no_label_is_not_counted():
    """S % 4 == 0 but every full-resolution tensor is a view one float off 16-byte alignment; one mask pixel holds 1.5"""
    from cosa_amd.utils import seg_helper
    B, K, S, _ = SHAPES["K5"]
    off, n = R.layout(K)
    d = dict(_case("K5")[0][0])
    d["mask_main"] = d["mask_main"].copy()
    assert tuple(d["boxes"][0]) == (0, S, 0, S)
    d["mask_main"][0, 5, 6] = 1.5
    want = R.reference(_oracle(), d["mask_main"], d["mask_aux"], d["seg"], d["cls"], d["boxes"], d["cam"], d["cam_aux"])
    assert want[off["main"]:off["main"] + K + 1].sum() == want[off["pix"]] - 1
    t = _dev(d)
    for k in ("mask_main", "mask_aux", "cam", "cam_aux"):
        flat = torch.empty(t[k].numel() + 1, device=t[k].device)
        flat[1:] = t[k].reshape(-1)
        t[k] = flat[1:].view(t[k].shape)
        assert t[k].is_contiguous() and t[k].data_ptr() % 16 == 4
    counters = seg_helper.new_label_stats(K, t["seg"].device)
    _run(t, counters)
    got = counters.cpu().numpy()
    assert np.array_equal(got, want), np.nonzero(got != want)[0]


def test_two_runs_give_identical_counters_and_two_calls_add_up():
    from cosa_amd.utils import seg_helper
    K = SHAPES["K81"][1]
    (d0, w0), (d1, w1) = _case("K81")[:2]
    runs = []
    for _ in range(2):
        counters = seg_helper.new_label_stats(K, torch.device("cuda", 0))
        _run(_dev(d0), counters)
        _run(_dev(d1), counters)
        runs.append(counters.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], w0 + w1)


def test_nonfinite_cam_elements_of_present_planes_only():
    """an inf in a present plane (inside the box) and a NaN in an absent one: bad_cam == 1, step_scale NaN, every other slot as without
    them; the step-local flag does not outlive the call"""
    from cosa_amd.utils import seg_helper
    K = SHAPES["K5"][1]
    off, n = R.layout(K)
    # an image with present AND absent classes and a box more than one row high
    d, want, b = next((d, w, b) for d, w in _case("K5") for b in range(SHAPES["K5"][0])
                      if 0 < d["cls"][b].sum() < K - 1 and d["boxes"][b][1] - d["boxes"][b][0] > 1)
    y, x = int(d["boxes"][b][0]) + 1, int(d["boxes"][b][3]) - 1
    present, absent = int(np.nonzero(d["cls"][b])[0][-1]), int(np.nonzero(d["cls"][b] == 0)[0][0])
    t = _dev(d)
    t["cam"][b, present, y, x] = float("inf")
    t["cam"][b, absent, y, x] = float("nan")
    t["cam_aux"][b, absent] = float("nan")                          # a whole absent plane: never read
    counters = seg_helper.new_label_stats(K, t["seg"].device)
    scale = torch.ones(1, device=t["seg"].device)
    assert _run(t, counters, scale=scale) is scale
    got = counters.cpu().numpy()
    expect = want.copy()
    expect[off["bad_cam"]] = 1
    assert np.array_equal(got, expect), np.nonzero(got != expect)[0]
    assert got[off["bad_cam"]] == 1 and got[off["bad_cam_aux"]] == 0 and bool(torch.isnan(scale).all())
    _run(_dev(d), counters, scale=scale)                            # the clean inputs again, same scale tensor
    assert scale.view(torch.int32).item() == 0x3f800000
    assert np.array_equal(counters.cpu().numpy(), expect + want)
    t["cam_aux"][b, present, y, x] = float("-inf")                  # ... and the auxiliary set has its own slot
    _run(t, counters, scale=scale)
    got = counters.cpu().numpy()
    assert got[off["bad_cam"]] == 2 and got[off["bad_cam_aux"]] == 1 and bool(torch.isnan(scale).all())


def test_outside_the_envelope_returns_a_status_and_touches_nothing():
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    L = _C.lib()
    ws = torch.zeros(8, dtype=torch.uint8, device=dev)

    def call(B, K, S, h, counters, scale):
        z = lambda *s: torch.zeros(*s, device=dev)
        return L.cosa_label_stats(_C.ptr(z(B, S, S)), None, _C.ptr(z(B, K, h, h)), _C.ptr(z(B, K - 1)), _C.ptr(torch.zeros(B, 4, dtype=torch.int32, device=dev)),
                                  None, None, B, K, S, h, h, 255, _C.ptr(counters), _C.ptr(scale), _C.ptr(ws), _C.stream_ptr())

    for K, S, h, word in ((129, 16, 2, b"K must be"), (5, 16, 17, b"envelope")):
        counters = torch.full((4 * K + 7,), 3, dtype=torch.int64, device=dev)
        scale = torch.full((1,), 5.0, device=dev)
        rc = call(1, K, S, h, counters, scale)
        assert rc != 0 and word in L.cosa_last_error()
        torch.cuda.synchronize()
        assert bool((counters == 3).all()) and float(scale) == 5.0
    with pytest.raises(ValueError):
        seg_helper.new_label_stats(129, dev)
    with pytest.raises(_C.CosaError):                               # host tensors raise as everywhere
        seg_helper.label_stats(torch.zeros(1, 8, 8), None, torch.zeros(1, 3, 2, 2), torch.zeros(1, 2), [[0, 8, 0, 8]], None, None,
                               torch.zeros(19, dtype=torch.int64))


# ---- the trainer --------------------------------------------------------------------------------------------------------------------------
def _trainer(seed=3, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, teacher_graph=False, teacher_async=False, **over)
    return CoSATrainer(args, torch.device("cuda", 0), seed=seed)


def _step(tr, k, poison=False):
    """step k of the fixed batch sequence; poison: the teacher's main CAM arrives with one inf in a plane of a present class of image 0
    (whose box is the whole crop) -- a value in a tensor, nothing else"""
    from cosa_amd.train_step import synthetic_batch
    batch = synthetic_batch(2, 64, 20, tr.device, seed=500 + k)
    if poison:
        plain = tr._teacher

        def teacher(wimg, cls_label):
            cam, cam_aux, seg = plain(wimg, cls_label)
            cam = cam.clone()
            cam[0, int(torch.nonzero(cls_label[0])[0]), 10, 21] = float("inf")
            return cam, cam_aux, seg

        tr._teacher = teacher
    try:
        return tr.step(*batch, n_iter=tr.args.warmup_iters + k)
    finally:
        if poison:
            del tr._teacher


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


STATE_FILE = "state_00000002.cosa"


@functools.lru_cache(maxsize=None)
def _counting_run(directory):
    """four steps with the flag and the guard on, a state file after the second -> (state after 2, counters after 2, counters after 4,
    guard counters after 2, state after 4, the file)"""
    tr = _trainer(skip_nonfinite=True, label_stats=True)
    _step(tr, 1)
    _step(tr, 2)
    s2, c2 = _state(tr), tr.label_stats_state.cpu().numpy().copy()
    guard2 = tr.guard_counters()
    path = os.path.join(directory, STATE_FILE)
    tr.save_state(path, n_iter=1)
    tr.wait_state()
    _step(tr, 3)
    _step(tr, 4)
    return s2, c2, tr.label_stats_state.cpu().numpy().copy(), guard2, _state(tr), path


@pytest.fixture(scope="module")
def counting_run(tmp_path_factory):
    return _counting_run(str(tmp_path_factory.mktemp("label_stats")))


def test_the_flag_changes_no_bit_of_a_step(counting_run):
    s2, c2, _, guard2, _, _ = counting_run
    tr = _trainer(skip_nonfinite=True)
    assert tr.label_stats_state is None and tr.label_stats() is None
    _step(tr, 1)
    _step(tr, 2)
    _assert_same_state(_state(tr), s2)
    off, _ = R.layout(21)
    assert c2[off["steps"]] == 2 and c2[off["pix"]] > 0 and c2[off["bad_cam"]] == c2[off["bad_cam_aux"]] == 0
    assert c2[off["main"]:off["main"] + 22].sum() == c2[off["pix"]] == c2[off["aux"]:off["aux"] + 22].sum()
    assert guard2 == tr.guard_counters() == {"applied": 2, "skipped": 0, "clipped": 0}


def test_a_nonfinite_teacher_cam_is_refused_through_the_guard():
    tr = _trainer(skip_nonfinite=True, label_stats=True)
    _step(tr, 1)
    before = _state(tr)
    logs = _step(tr, 2, poison=True)
    assert tr.guard_counters() == {"applied": 1, "skipped": 1, "clipped": 0}
    _assert_same_state(_state(tr), before)                          # masters, moments and the EMA teacher keep their bytes
    s = tr.label_stats()
    assert s["teacher_nonfinite"] == 1 and s["teacher_nonfinite_aux"] == 0 and s["steps"] == 2
    assert math.isfinite(float(logs["overall_loss"])) and not math.isfinite(float(logs["grad_norm"]))
    _step(tr, 3)                                                    # the next step is taken again
    assert tr.guard_counters() == {"applied": 2, "skipped": 1, "clipped": 0} and tr.label_stats()["teacher_nonfinite"] == 1
    assert all(bool(torch.isfinite(v).all()) for v in _state(tr).values())


def test_without_skip_nonfinite_the_monitor_only_counts():
    tr = _trainer(label_stats=True)
    assert tr.guard_state is None
    _step(tr, 1)
    before = _state(tr)
    _step(tr, 2, poison=True)
    after = _state(tr)
    assert any(not torch.equal(after[k], before[k]) for k in before if k.startswith("AN."))          # the step was applied
    assert tr.label_stats()["teacher_nonfinite"] == 1 and tr.label_stats()["steps"] == 2


def test_the_counters_resume_with_the_run(counting_run):
    """saved at iteration 2 of an interval of 4 (the counters are zeroed only at a log interval's end), resumed in a fresh trainer"""
    _, c2, c4, _, s4, path = counting_run
    tr = _trainer(seed=77, skip_nonfinite=True, label_stats=True)   # another seed: nothing of its own survives the load
    assert tr.load_state(path)["n_iter"] == 1
    assert np.array_equal(tr.label_stats_state.cpu().numpy(), c2)
    _step(tr, 3)
    _step(tr, 4)
    assert np.array_equal(tr.label_stats_state.cpu().numpy(), c4) and c4[0] == 4
    _assert_same_state(_state(tr), s4)
