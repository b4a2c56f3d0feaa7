"""The --teacher_check monitor on the GPU: cosa_teacher_check against seg_helper.teacher_check_torch on CPU copies
-- every counter an integer, every comparison exact equality --, then the trainer at crop 64: the flag changes no bit of the run, a check
against the teacher's own mode finds nothing, a check against bf16 equals the two passes run by hand, the counters are reproducible, resume
with the run and count once per optimizer step under --accum_steps, and --usegmm's queues and trackers are not touched; then the tool."""
import copy
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, C, S, h): the float4 path, one plane = 16 wavefronts | S % 64 != 0: tails inside a wavefront | S % 4 != 0: the scalar path, at COCO's
# class count | every plane active, no auxiliary label pair, no targets
SHAPES = {"vec": (2, 4, 64, 4), "tails": (3, 20, 40, 5), "scalar": (1, 80, 34, 17), "bare": (2, 20, 64, 4)}
BARE = "bare"


@functools.lru_cache(maxsize=None)
def _case(name, seed=0):
    """inputs of one call on the host (torch, fp32) -> dict; figures spread over every histogram bin, planes that are equal, one non-finite
    element in an active plane of each pass, inactive planes full of NaN, a full, a partial and (B > 2) an empty box, label maps with
    ignore and with values that are no label"""
    B, C, S, h = SHAPES[name]
    g = torch.Generator().manual_seed(1000 * len(name) + seed)
    r = lambda *s: torch.rand(*s, generator=g)
    K = C + 1
    cls = (r(B, C) < (0.9 if C < 8 else 0.4)).float()
    cls[0, 0], cls[0, 1] = 1, 0                                        # at least one active and one inactive plane
    act = torch.ones(B, C, dtype=torch.bool) if name == BARE else cls != 0

    def pair(hh):
        a = r(B, C, hh, hh)
        mag = 10.0 ** (-1 - 6 * r(B, C, 1, 1))                         # 1e-7 .. 1e-1 per plane: every bin
        b = a + mag * (r(B, C, hh, hh) - 0.5)
        same = r(B, C) < 0.2
        b[same] = a[same]
        if name != BARE:
            a[~act], b[~act] = float("nan"), float("inf")              # never read
        return a.contiguous(), b.contiguous()

    cams, auxs, tgts = pair(S), pair(S), pair(h)
    bi, ci = (int(v) for v in torch.nonzero(act)[0])
    cams[0][bi, ci, S // 2, S - 1] = float("nan")
    bi, ci = (int(v) for v in torch.nonzero(act)[-1])
    auxs[1][bi, ci, 0, 0] = float("-inf")

    def labels():
        a = torch.randint(0, K, (B, S, S), generator=g).float()
        a[r(B, S, S) < 0.1] = 255
        b = torch.where(r(B, S, S) < 0.05, torch.randint(0, K, (B, S, S), generator=g).float(), a)
        b[r(B, S, S) < 0.02] = 255
        a[0, 1, 1], b[0, 1, 1] = 0.5, 0.5
        a[0, 2, S - 1], b[0, S - 1, 2] = float(K), -1.0
        return a.contiguous(), b.contiguous()

    boxes = [[0, S, 0, S], [3, S - 5, 2, S - 1], [7, 7, 0, S]][:B]
    return dict(cams=cams, auxs=auxs, tgts=None if name == BARE else tgts, labels=labels(), aux_labels=None if name == BARE else labels(),
                cls=None if name == BARE else cls, boxes=boxes, K=K)


def _call(fn, d, counters, dev=None):
    t = lambda p: tuple(x.to(dev) if dev is not None else x for x in p) if p is not None else None
    cls = d["cls"].to(dev) if dev is not None and d["cls"] is not None else d["cls"]
    return fn(t(d["cams"]), t(d["auxs"]), t(d["tgts"]), t(d["labels"]), t(d["aux_labels"]), cls, d["boxes"], counters)


@functools.lru_cache(maxsize=None)
def _want(name, seed=0):
    from cosa_amd.utils import seg_helper
    d = _case(name, seed)
    c = seg_helper.new_teacher_check(d["K"], "cpu")
    _call(seg_helper.teacher_check_torch, d, c)
    return c.numpy().copy()


@pytest.mark.parametrize("name", list(SHAPES))
def test_kernel_counters_equal_the_torch_restatement(name):
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    d, want = _case(name), _want(name)
    off, n = seg_helper.teacher_check_layout(d["K"])
    # the case hits what it was built to hit
    assert want[off["checks"]] == 1 and want[off["cam.nonfinite_a"]] == 1 and want[off["aux.nonfinite_b"]] == 1
    assert want[off["cam.worst"]] == 0x7f800000 and want[off["cam.hist"] + 7] >= 1 and want[off["cam.over"]] >= 1
    for s_ in seg_helper.TEACHER_CHECK_SETS:
        assert want[off[s_ + ".hist"]:off[s_ + ".hist"] + 8].sum() == want[off[s_ + ".planes"]]
    if SHAPES[name][1] >= 20:
        assert (want[off["cam.hist"]:off["cam.hist"] + 8] > 0).sum() >= 4 and want[off["cam.over"]] < want[off["cam.planes"]]
    assert want[off["main.pix"]] > want[off["main.agree"]] > 0
    if name == BARE:
        assert want[off["cam.planes"]] == SHAPES[name][0] * SHAPES[name][1] and want[off["tgt.planes"]] == 0 and want[off["aux_label.pix"]] == 0
    else:
        assert 0 < want[off["cam.planes"]] < SHAPES[name][0] * SHAPES[name][1] and want[off["tgt.planes"]] == want[off["cam.planes"]]
    counters = seg_helper.new_teacher_check(d["K"], dev)
    assert _call(seg_helper.teacher_check, d, counters, dev) is counters
    got = counters.cpu().numpy()
    assert np.array_equal(got, want), [(k, got[v], want[v]) for k, v in off.items() if not np.array_equal(got[v:v + 1], want[v:v + 1])]


def test_two_calls_accumulate_and_two_runs_give_identical_bytes():
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    d0, d1 = _case("tails"), _case("tails", 1)
    want = seg_helper.new_teacher_check(d0["K"], "cpu")
    _call(seg_helper.teacher_check_torch, d0, want)
    _call(seg_helper.teacher_check_torch, d1, want)
    runs = []
    for _ in range(2):
        counters = seg_helper.new_teacher_check(d0["K"], dev)
        _call(seg_helper.teacher_check, d0, counters, dev)
        _call(seg_helper.teacher_check, d1, counters, dev)
        runs.append(counters.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes() and np.array_equal(runs[0], want.numpy()) and runs[0][0] == 2


def _raw_call(d, counters, ws, ws_bytes, dev, K=None, h=None, ignore=255, bar=1e-3, S=None):
    from cosa_amd import _C
    f = lambda t: t.to(dev).contiguous() if t is not None else None
    none = (None, None)
    ts = [f(t) for t in d["cams"] + d["auxs"] + (d["tgts"] or none) + d["labels"] + (d["aux_labels"] or none)]
    cls = f(d["cls"])
    boxes = torch.tensor(d["boxes"], dtype=torch.int32, device=dev)
    B, C, S0 = d["cams"][0].shape[:3]
    h0 = d["tgts"][0].shape[-1] if d["tgts"] is not None else 0
    rc = _C.lib().cosa_teacher_check(*[_C.ptr(t) for t in ts], _C.ptr(cls), _C.ptr(boxes), B, C, K if K is not None else C + 1,
                                     S if S is not None else S0, h if h is not None else h0, h if h is not None else h0, ignore, bar,
                                     _C.ptr(counters), _C.ptr(ws), ws_bytes, _C.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_sentinels_around_counters_and_workspace_survive():
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    for name in ("vec", "scalar"):
        d, want = _case(name), _want(name)
        B, C = SHAPES[name][:2]
        n = want.size
        need = _C.lib().cosa_teacher_check_workspace_bytes(B, C)
        assert need == 3 * B * C * 4
        cbuf = torch.full((n + 16,), -0x0123456789abcdef, dtype=torch.int64, device=dev)
        cbuf[8:8 + n] = 0
        wbuf = torch.full((need + 128,), 0xa5, dtype=torch.uint8, device=dev)
        assert _raw_call(d, cbuf[8:8 + n], wbuf[64:64 + need], need, dev) == 0
        c, w = cbuf.cpu().numpy(), wbuf.cpu().numpy()
        assert np.array_equal(c[8:8 + n], want)
        assert (c[:8] == -0x0123456789abcdef).all() and (c[8 + n:] == -0x0123456789abcdef).all()
        assert (w[:64] == 0xa5).all() and (w[64 + need:] == 0xa5).all()


def test_outside_the_envelope_returns_a_status_and_touches_nothing():
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    L = _C.lib()
    d = _case("vec")
    n = _want("vec").size
    ws = torch.zeros(1024, dtype=torch.uint8, device=dev)
    for kw, word in ((dict(K=4), b"K == C + 1"), (dict(h=65), b"envelope"), (dict(ignore=3), b"class index"), (dict(bar=-1.0), b"bar"),
                     (dict(S=0), b"envelope")):
        counters = torch.full((n,), 3, dtype=torch.int64, device=dev)
        assert _raw_call(d, counters, ws, ws.numel(), dev, **kw) != 0 and word in L.cosa_last_error(), kw
        assert bool((counters == 3).all()) and int(ws.sum()) == 0
    counters = torch.full((n,), 3, dtype=torch.int64, device=dev)
    assert _raw_call(d, counters, ws, 8, dev) != 0 and b"workspace" in L.cosa_last_error() and bool((counters == 3).all())
    assert L.cosa_teacher_check_workspace_bytes(1, 256) == 0
    big = torch.zeros(1, 256, 4, 4)                                                     # C = 256: K would be 257
    with pytest.raises(ValueError):
        seg_helper.teacher_check((big.to(dev), big.to(dev)), (big.to(dev), big.to(dev)), None, (torch.zeros(1, 4, 4, device=dev),) * 2, None, None,
                                 [[0, 4, 0, 4]], torch.zeros(48 + 6 * 257, dtype=torch.int64, device=dev))
    with pytest.raises(_C.CosaError):                                                   # host tensors raise as everywhere
        _call(seg_helper.teacher_check, d, seg_helper.new_teacher_check(d["K"], "cpu"))


# ---- the trainer --------------------------------------------------------------------------------------------------------------------------
LOSSES = ("cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")
STEPS = 6


def _trainer(seed=3, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, **over)              # (teacher graph and side stream on: the defaults)
    return CoSATrainer(args, torch.device("cuda", 0), seed=seed)


def _batch(tr, k):
    from cosa_amd.train_step import synthetic_batch
    return synthetic_batch(2, 64, 20, tr.device, seed=500 + k)


def _step(tr, k, n_iter=None):
    """step k = 1.. of the fixed batch sequence; with --teacher_check_iters 2 the odd ones are check steps"""
    logs = tr.step(*_batch(tr, k), n_iter=tr.args.warmup_iters + k if n_iter is None else n_iter)
    return torch.stack([logs[n].reshape(()).float() for n in LOSSES]).clone()


def _state(tr):
    """clones of what a step writes: masters of both networks (the EMA teacher among them), the moments, and the 16-bit shadows"""
    out = {}
    for tag, net in (("ON", tr.student), ("AN", tr.model_AN)):
        for n, p in net.named_parameters():
            out[f"{tag}.{n}"] = p.detach().clone()
    names = {id(p): n for n, p in tr.student.named_parameters()}
    for p, st in tr.optimizer.state.items():
        for k in ("exp_avg", "exp_avg_sq"):
            out[f"opt.{names[id(p)]}.{k}"] = st[k].clone()
    for tag, sh in (("ON", tr._student_shadows), ("AN", tr._teacher_shadows)):
        for i, s in enumerate(sh.shadows):
            out[f"shadow.{tag}.{i}"] = s.clone()
    return out


def _assert_same_state(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k


@functools.lru_cache(maxsize=None)
def _plain_run():
    """six steps without the flag -> (losses [6][5], state after 6)"""
    tr = _trainer()
    assert tr.teacher_check_state is None and tr.model_CK is None and tr.teacher_check() is None
    losses = torch.stack([_step(tr, k) for k in range(1, STEPS + 1)])
    assert tr._graph is not None, "the teacher's graph must have been captured: the run under test replays it"
    return losses, _state(tr)


def _hand_check(tr, teacher_before, batch, counters):
    """the two passes of one check by hand, on copies of the teacher taken before the step, one per mode -> `counters` (a host copy of the
    trainer's before the step) advanced by seg_helper.teacher_check_torch.  Library workspaces of its own, like the trainer's check pass:
    the captured graph keeps the addresses of the default ones."""
    from cosa_amd import _C
    from cosa_amd.train_step import teacher_products
    from cosa_amd.utils import seg_helper
    wimg, simg, cls_label, img_box = batch
    args = tr.args
    thresholds = ((args.high_thre, args.low_thre), (args.high_thre_aux, args.low_thre_aux))
    out = []
    with _C.workspace_scope("by_hand"):
        for mode in (args.teacher_precision, args.teacher_check_mode):
            m = copy.deepcopy(teacher_before).set_nograd_precision(mode)
            (cam, aux), (mask, mask_aux), tgt = teacher_products(m, args, wimg, simg, img_box, cls_label, thresholds, True, (4, 4), {}, None)
            out.append([t.cpu().clone() for t in (cam, aux, mask, mask_aux, tgt)])
    a, b = out
    seg_helper.teacher_check_torch((a[0], b[0]), (a[1], b[1]), (a[4], b[4]), (a[2], b[2]), (a[3], b[3]), cls_label.cpu(), img_box, counters)
    return counters


@functools.lru_cache(maxsize=None)
def _checked_run(directory):
    """six steps with --teacher_check_iters 2 against bf16, a state file after the third, the fifth (the last check step) repeated by hand
    -> dict"""
    tr = _trainer(teacher_check_iters=2, teacher_check_mode="bf16")
    assert tr.args.teacher_precision == "fp16x3" and tr.model_CK is not None
    assert not {id(p) for p in tr.model_CK.parameters()} & {id(p) for p in tr.model_AN.parameters()}
    assert tr._checks["teacher_check"].shadows is not tr._teacher_shadows and not tr._checks["teacher_check"].shadows.optimizer_owned
    losses, counters = [], {}
    for k in range(1, STEPS + 1):
        if k == 5:
            before, teacher_before = tr.teacher_check_state.cpu().clone(), copy.deepcopy(tr.model_AN)
        losses.append(_step(tr, k))
        counters[k] = tr.teacher_check_state.cpu().numpy().copy()
        if k == 3:
            path = os.path.join(directory, "state_00000003.cosa")
            tr.save_state(path, n_iter=tr.args.warmup_iters + 3)
            tr.wait_state()
        if k == 5:
            by_hand = _hand_check(tr, teacher_before, _batch(tr, 5), before).numpy().copy()
    assert tr._graph is not None
    return dict(losses=torch.stack(losses), state=_state(tr), counters=counters, by_hand=by_hand, path=path, summary=tr.teacher_check())


@pytest.fixture(scope="module")
def checked_run(tmp_path_factory):
    return _checked_run(str(tmp_path_factory.mktemp("teacher_check")))


def test_the_flag_changes_no_bit_of_the_run(checked_run):
    """(a) weights, moments, EMA teacher, shadows and the five losses of six steps, the teacher's graph and side stream on"""
    losses, state = _plain_run()
    assert torch.equal(losses.view(torch.int32), checked_run["losses"].view(torch.int32))
    _assert_same_state(state, checked_run["state"])


def test_a_check_against_the_teachers_own_mode_finds_nothing():
    """(b) fails when model_CK is stale by one EMA step or reads another model's buffers"""
    from cosa_amd.utils import seg_helper
    tr = _trainer(teacher_check_iters=2, teacher_check_mode="fp16x3")
    for k in range(1, STEPS + 1):
        _step(tr, k)
    s = tr.teacher_check()
    assert s["checks"] == 3 and s["conforms"] is True
    for name in seg_helper.TEACHER_CHECK_SETS:
        assert s[name]["planes"] > 0 and s[name]["worst_bits"] == 0 and s[name]["over"] == 0 and s[name]["hist"][0] == s[name]["planes"], (name, s[name])
        assert s[name]["nonfinite_a"] == s[name]["nonfinite_b"] == 0
    for name in seg_helper.TEACHER_CHECK_PAIRS:
        assert s[name]["pix"] > 0 and s[name]["agree"] == 1.0 and s[name]["miou"] == 1.0, (name, s[name])


def test_a_check_against_bf16_equals_the_two_passes_run_by_hand(checked_run):
    """(c)"""
    from cosa_amd.utils import seg_helper
    off, _ = seg_helper.teacher_check_layout(21)
    c = checked_run["counters"]
    assert [int(c[k][off["checks"]]) for k in range(1, STEPS + 1)] == [1, 1, 2, 2, 3, 3]
    s = checked_run["summary"]
    assert s["checks"] == 3 and s["cam"]["worst_bits"] > 0 and s["aux"]["worst_bits"] > 0 and s["tgt"]["planes"] == s["cam"]["planes"] > 0
    assert s["main"]["pix"] == s["aux_label"]["pix"] > 0
    assert np.array_equal(c[5], checked_run["by_hand"]), np.nonzero(c[5] != checked_run["by_hand"])[0]
    assert np.array_equal(c[6], c[5])                                                   # step 6 is no check step


def test_two_identical_runs_give_identical_counters(checked_run):
    """(d)"""
    tr = _trainer(teacher_check_iters=2, teacher_check_mode="bf16")
    for k in (1, 2, 3):
        _step(tr, k)
    assert np.array_equal(tr.teacher_check_state.cpu().numpy(), checked_run["counters"][3])


def test_counters_and_weights_resume_with_the_run(checked_run):
    """(e) saved after step 3 (two checks counted), resumed in a fresh trainer, finished at step 6"""
    tr = _trainer(seed=77, teacher_check_iters=2, teacher_check_mode="bf16")            # another seed: nothing of its own survives the load
    assert tr.load_state(checked_run["path"])["n_iter"] == tr.args.warmup_iters + 3
    assert np.array_equal(tr.teacher_check_state.cpu().numpy(), checked_run["counters"][3])
    losses = torch.stack([_step(tr, k) for k in (4, 5, 6)])
    assert torch.equal(losses.view(torch.int32), checked_run["losses"][3:].view(torch.int32))
    assert np.array_equal(tr.teacher_check_state.cpu().numpy(), checked_run["counters"][6])
    _assert_same_state(_state(tr), checked_run["state"])


def test_accum_steps_checks_once_per_check_step_on_the_closing_micro_batch():
    """(f) two optimizer steps of two micro-batches, every optimizer step a check step"""
    from cosa_amd.utils import seg_helper
    off, _ = seg_helper.teacher_check_layout(21)
    tr = _trainer(teacher_check_iters=1, teacher_check_mode="bf16", accum_steps=2)
    seen = []
    for it in (1, 2):
        for micro in (0, 1):
            _step(tr, 2 * it + micro, n_iter=tr.args.warmup_iters + it)
            seen.append(int(tr.teacher_check_state[off["checks"]]))
    assert seen == [0, 1, 1, 2]


def test_usegmm_queues_and_trackers_keep_their_bytes():
    """(g) the check reads the threshold VALUES of its step; the queues and trackers are the run's"""
    def run(**over):
        tr = _trainer(usegmm=True, queue_update_ratio=4, gmmscale=4, **over)
        for k in (1, 2, 3, 4):
            _step(tr, k)
        out = {"q": tr.cam_queue.queue.clone(), "q_aux": tr.camaux_queue.queue.clone(),
               "ptr": torch.tensor([tr.cam_queue.ptr, tr.camaux_queue.ptr])}
        for n in ("ema_lowthre", "ema_highthre", "ema_auxlowthre", "ema_auxhighthre"):
            out[n] = torch.as_tensor(getattr(tr, n).get()).detach().clone().cpu().double()
        for n, p in tr.model_AN.named_parameters():
            out["AN." + n] = p.detach().clone()
        return out, tr.teacher_check()
    plain, none = run()
    checked, s = run(teacher_check_iters=2, teacher_check_mode="bf16")
    assert none is None and s["checks"] == 2 and s["cam"]["planes"] > 0
    _assert_same_state(plain, checked)


def test_the_tool_prints_one_json_line_with_the_summary():
    """tools/teacher_check.py --synthetic at crop 64, in a fresh child process"""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "teacher_check.py"), "--synthetic", "--crop_size", "64", "--batch_size", "2", "--batches", "2",
           "--mode", "fp16x3", "--check_mode", "bf16"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    for key in ("checks", "cam", "aux", "tgt", "main", "aux_label", "conforms", "exemption_evaluated", "criterion", "mode", "check_mode"):
        assert key in rec, key
    assert rec["checks"] == 2 and rec["mode"] == "fp16x3" and rec["check_mode"] == "bf16" and rec["exemption_evaluated"] is False
    assert rec["cam"]["planes"] > 0 and rec["cam"]["worst_bits"] > 0 and rec["main"]["pix"] > 0
