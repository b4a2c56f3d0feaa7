"""The --student_check monitor on the GPU: cosa_student_check against the NumPy restatement of its rules
(tests/student_check_ref.py) -- every counter an integer, every comparison exact equality --, then the trainer at crop 64: the flag changes no
bit of the run (alone and next to --teacher_check_iters), the counters equal the restatement applied to the training outputs and to a
forward the test makes itself, a corrupted 16-bit shadow shows, the check runs once per optimizer step under --accum_steps, and the counters
travel in a state file; then the tool."""
import copy
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import student_check_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -0x0123456789abcdef


@functools.lru_cache(maxsize=None)
def _case_and_ref(name, seed=0):
    d = ref.make_case(name, seed)
    return d, ref.ref_of_case(d)


def _dev_tensors(d, dev):
    t = lambda p: tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in p)
    return [t(d[k]) for k in ("seg", "cam", "cam_aux", "cls", "cls_aux", "losses")], torch.from_numpy(d["cls_label"]).to(dev)


def _call(d, counters, dev):
    from cosa_amd.utils import seg_helper
    pairs, lab = _dev_tensors(d, dev)
    return seg_helper.student_check(*pairs, lab, counters)


@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_kernel_counters_equal_the_restatement(name):
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    d, want = _case_and_ref(name)
    off, n = seg_helper.student_check_layout(d["K"])
    assert all(v > 0 for v in want[off["flip_hist"]:off["flip_hist"] + 4]) and want[off["flags"]] == 0b11111      # the case hits what it was built to hit
    counters = seg_helper.new_student_check(d["K"], dev)
    assert _call(d, counters, dev) is counters
    got = counters.cpu().tolist()
    assert got == want, [(k, got[v], want[v]) for k, v in off.items() if got[v] != want[v]]


def test_two_calls_accumulate_and_two_runs_give_identical_bytes():
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    (d0, w0), (d1, _) = _case_and_ref("blocks"), _case_and_ref("blocks", 1)
    want = ref.ref_of_case(d1, w0)
    runs = []
    for _ in range(2):
        counters = seg_helper.new_student_check(d0["K"], dev)
        _call(d0, counters, dev)
        _call(d1, counters, dev)
        runs.append(counters.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes() and runs[0].tolist() == want and want[0] == 2


def _raw_call(d, counters, dev, null=None, **over):
    from cosa_amd import _C
    pairs, lab = _dev_tensors(d, dev)
    ts = [t for p in pairs for t in p] + [lab]
    ptrs = [_C.ptr(None if i == null else t) for i, t in enumerate(ts)]
    B, K, h, w = d["seg"][0].shape
    dims = dict(B=B, K=K, h=h, w=w)
    dims.update(over)
    rc = _C.lib().cosa_student_check(*ptrs, _C.ptr(counters), dims["B"], dims["K"], dims["h"], dims["w"], _C.stream_ptr())
    torch.cuda.synchronize()
    return rc


def test_a_sentinel_border_around_the_counters_survives():
    dev = torch.device("cuda", 0)
    for name in ("small", "wide"):
        d, want = _case_and_ref(name)
        n = len(want)
        buf = torch.full((n + 16,), SENTINEL, dtype=torch.int64, device=dev)
        buf[8:8 + n] = 0
        assert _raw_call(d, buf[8:8 + n], dev) == 0
        c = buf.cpu().tolist()
        assert c[8:8 + n] == want and all(v == SENTINEL for v in c[:8] + c[8 + n:])


def test_outside_the_envelope_returns_einval_and_touches_nothing():
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    L = _C.lib()
    d, want = _case_and_ref("small")
    n = len(want)
    COSA_EINVAL = 1
    for kw, word in ((dict(B=0), b"positive"), (dict(h=0), b"positive"), (dict(w=-1), b"positive"), (dict(K=1), b"K must be"),
                     (dict(K=257), b"K must be"), (dict(null=0), b"null"), (dict(null=5), b"null"), (dict(null=11), b"null"), (dict(null=12), b"null")):
        counters = torch.full((n,), 3, dtype=torch.int64, device=dev)
        assert _raw_call(d, counters, dev, **kw) == COSA_EINVAL and word in L.cosa_last_error(), kw
        assert bool((counters == 3).all())
    pairs, lab = _dev_tensors(d, dev)
    assert L.cosa_student_check(*[_C.ptr(t) for p in pairs for t in p], _C.ptr(lab), _C.ptr(None), 2, 6, 4, 4, _C.stream_ptr()) == COSA_EINVAL
    assert L.cosa_student_check_counters(1) == 0 and L.cosa_student_check_counters(257) == 0 and L.cosa_student_check_counters(81) == 62 + 162
    with pytest.raises(ValueError):                                                     # the wrapper's shape checks
        seg_helper.student_check(*pairs, lab, torch.zeros(n - 1, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        seg_helper.student_check(pairs[0], pairs[0], *pairs[2:], lab, seg_helper.new_student_check(6, dev))
    with pytest.raises(_C.CosaError):                                                   # host tensors raise as everywhere
        seg_helper.student_check(*[tuple(t.cpu() for t in p) for p in pairs], lab.cpu(), seg_helper.new_student_check(6, "cpu"))


# ---- the trainer --------------------------------------------------------------------------------------------------------------------------
LOSSES = ("cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")
STEPS = 5


def _trainer(seed=3, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, **over)              # (teacher graph and side stream on: the defaults)
    return CoSATrainer(args, torch.device("cuda", 0), seed=seed)


def _batch(tr, k):
    from cosa_amd.train_step import synthetic_batch
    return synthetic_batch(2, 64, 20, tr.device, seed=700 + k)


def _step(tr, k, n_iter=None):
    """step k = 1.. of the fixed batch sequence, past warm-up; with --student_check_iters 2 the even ones are check steps"""
    logs = tr.step(*_batch(tr, k), n_iter=tr.args.warmup_iters + 1 + k if n_iter is None else n_iter)
    return torch.stack([logs[n].reshape(()).float() for n in LOSSES]).clone()


def _state(tr):
    """clones of what a step writes: the student's weights, the AdamW moments, the teacher's weights"""
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
def _plain_run():
    """five steps without the flag -> (losses [5][5], state after 5)"""
    tr = _trainer()
    assert tr.student_check_state is None and tr.model_SK is None and tr.student_check() is None
    losses = torch.stack([_step(tr, k) for k in range(1, STEPS + 1)])
    assert tr._graph is not None, "the teacher's graph must have been captured: the run under test replays it"
    return losses, _state(tr)


def _hand_forward(tr, weights, simg):
    """a model_SK-style forward the test makes itself: a fresh network in fp32 mode with the student's weights of before the step"""
    from cosa_amd import _C
    from cosa_amd.models import build_model
    m = build_model(tr.args)
    m.load_state_dict(weights)
    m = m.to(tr.device)
    for p in m.parameters():
        p.requires_grad = False
    m.set_nograd_precision("fp32")
    with torch.no_grad(), _C.workspace_scope("by_hand"):
        cls, cls_aux, _f, seg, cam, cam_aux = m(simg)
    return dict(seg=seg, cam=cam, cam_aux=cam_aux, cls=cls, cls_aux=cls_aux)


@functools.lru_cache(maxsize=None)
def _checked_run(directory):
    """five steps with --student_check_iters 2, the fourth (the second check step) repeated by hand, a state file after it -> dict"""
    from cosa_amd import nn_ops
    assert nn_ops._reference_ops is None                                                # no reference operators: reaching reference_op raises
    tr = _trainer(student_check_iters=2)
    assert tr.args.student_check_mode == "fp32" and tr.model_SK is not None and tr.model_CK is None and tr._checks["student_check"].shadows is None
    assert not {id(p) for p in tr.model_SK.parameters()} & {id(p) for p in tr.student.parameters()}
    losses, counters = [], {}
    for k in range(1, STEPS + 1):
        if k == 4:
            before = tr.student_check_state.cpu().tolist()
            weights = copy.deepcopy(tr.student.state_dict())
        losses.append(_step(tr, k))
        counters[k] = tr.student_check_state.cpu().tolist()
        if k == 4:
            last = {k_: ({n: t.cpu().clone() for n, t in v.items()} if isinstance(v, dict) else v.cpu().clone()) for k_, v in tr.student_check_last.items()}
            mine = {n: t.float().cpu() for n, t in _hand_forward(tr, weights, _batch(tr, 4)[1]).items()}
            path = os.path.join(directory, "state_00000004.cosa")
            tr.save_state(path, n_iter=tr.args.warmup_iters + 5)
            tr.wait_state()
    assert tr._graph is not None
    return dict(losses=torch.stack(losses), state=_state(tr), counters=counters, before=before, last=last, mine=mine, path=path,
                summary=tr.student_check(), labels=_batch(tr, 4)[2].cpu())


@pytest.fixture(scope="module")
def checked_run(tmp_path_factory):
    return _checked_run(str(tmp_path_factory.mktemp("student_check")))


def test_the_flag_changes_no_bit_of_the_run(checked_run):
    """1: the losses of every step, the student's weights, the moments and the teacher's weights after five steps; two checks counted"""
    from cosa_amd.utils import seg_helper
    losses, state = _plain_run()
    assert torch.equal(losses.view(torch.int32), checked_run["losses"].view(torch.int32))
    _assert_same_state(state, checked_run["state"])
    off, _ = seg_helper.student_check_layout(21)
    assert [checked_run["counters"][k][off["checks"]] for k in range(1, STEPS + 1)] == [0, 1, 1, 2, 2]
    assert checked_run["summary"]["checks"] == 2


def test_the_counters_equal_the_restatement_on_the_training_outputs_and_an_independent_forward(checked_run):
    """2: `student_check_last` is the documented hook: a = the training forward's outputs, b = the check pass's, loss_a / loss_b"""
    last, mine = checked_run["last"], checked_run["mine"]
    for n in ref.TENSORS:
        assert torch.equal(last["b"][n], mine[n]), n                                     # the check pass is that forward, bit for bit
        assert last["a"][n].shape == mine[n].shape and not torch.equal(last["a"][n], mine[n]), n
    assert last["a"]["seg"].shape == (2, 21, 4, 4)
    # the two classification losses of the check pass, against torch on the independent forward's logits (fp32 sums of 40 terms: 1e-5)
    lab = checked_run["labels"]
    for j, n in ((0, "cls"), (1, "cls_aux")):
        want = torch.nn.functional.multilabel_soft_margin_loss(mine[n].double(), lab.double())
        assert abs(float(last["loss_b"][j]) - float(want)) <= 1e-5 * abs(float(want)), (n, float(last["loss_b"][j]), float(want))
    assert torch.equal(last["loss_a"].cpu(), checked_run["losses"][3][:4].cpu())        # the step's own four losses
    assert bool(torch.isfinite(last["loss_b"]).all()) and bool((last["loss_b"] != last["loss_a"]).any())
    pair = lambda n: (last["a"][n].numpy(), mine[n].numpy())
    want = ref.student_check_ref(pair("seg"), pair("cam"), pair("cam_aux"), pair("cls"), pair("cls_aux"),
                                 (last["loss_a"].numpy(), last["loss_b"].numpy()), lab.numpy(), checked_run["before"])
    got = checked_run["counters"][4]
    off, _ = ref.layout(21)
    assert got == want, [(k, got[v], want[v]) for k, v in off.items() if got[v] != want[v]]
    assert checked_run["counters"][5] == got                                             # step 5 is no check step
    s = checked_run["summary"]
    assert s["flags"] == 0 and s["seg"]["rel_l2"] > 0 and s["seg"]["nonfinite_a"] == s["seg"]["nonfinite_b"] == 0 and s["cells"] == 2 * 2 * 16


@pytest.mark.parametrize("flags", [dict(student_check_iters=2, teacher_check_iters=2),
                                   dict(student_check_iters=2, teacher_check_iters=2, act_stats_iters=2, grad_check_iters=2)],
                         ids=["student_teacher", "all_four"])
def test_both_monitors_on_change_no_bit_of_the_run(flags):
    """6: next to --teacher_check_iters, and with all four monitors that keep a network of their own (the gradient check at its defaults: fp64,
    one direction)"""
    losses, state = _plain_run()
    tr = _trainer(**flags)
    all_four = len(flags) == 4
    assert len(tr._checks) == len(flags) and tr.model_SK is not None and tr.model_CK is not None
    assert (tr.model_AK is not None) == all_four and (tr.model_GK is not None) == all_four
    nets = [tr.student, tr.model_AN, tr.model_SK, tr.model_CK] + ([tr.model_AK, tr.model_GK] if all_four else [])
    ids = [{id(p) for p in net.parameters()} for net in nets]
    assert all(not a & b for i, a in enumerate(ids) for b in ids[i + 1:])              # no parameter object is shared, pairwise
    buffers = [tr._cam_buffers] + [ck.buffers for ck in tr._checks.values()]
    assert len({id(b) for b in buffers}) == len(buffers)                                # nor a CAM-buffer dict
    got, popped = [], []
    for k in range(1, STEPS + 1):
        got.append(_step(tr, k))
        popped.append(tr.pop_grad_check())
    assert torch.equal(losses.view(torch.int32), torch.stack(got).view(torch.int32))
    _assert_same_state(state, _state(tr))
    assert tr.student_check()["checks"] == 2 and tr.teacher_check()["checks"] == 2
    if all_four:
        assert int(tr.act_stats_state[-1]) == 2
        assert [p is not None for p in popped] == [False, True, False, True, False]
        assert all(d["flags"] == 0 for p in popped if p is not None for d in p)
    else:
        assert popped == [None] * STEPS


def test_a_stale_weight_shadow_shows():
    """3: one block's fc1 16-bit shadow scaled by 1.5, its fp32 master untouched: the training forward reads the shadow, the check the master"""
    from cosa_amd import nn_ops
    figs = {}
    for tag in ("clean", "stale"):
        tr = _trainer(student_check_iters=1)
        for k in (1, 2, 3):                                                             # (the third call captures the teacher's graph)
            _step(tr, k)
        tr.student_check_state.zero_()
        if tag == "stale":
            w = tr.student.encoder.blocks[0].mlp.fc1.weight
            master = w.detach().clone()
            nn_ops.shadow_of(w).mul_(1.5)
        logs = _step(tr, 4)
        s = tr.student_check()
        assert s["checks"] == 1 and bool(torch.isfinite(logs).all())
        if tag == "stale":
            assert not torch.equal(master, w.detach())                                  # (the optimizer moved it: the step went through)
        figs[tag] = s["seg"]["rel_l2"]
    print("seg rel_l2: clean %.4e, stale shadow %.4e" % (figs["clean"], figs["stale"]))
    assert figs["clean"] > 0 and figs["stale"] >= 10 * figs["clean"], figs


def test_accum_steps_checks_on_the_closing_micro_batch_only():
    """4: two optimizer steps of two micro-batches, every optimizer step a check step"""
    from cosa_amd.utils import seg_helper
    off, _ = seg_helper.student_check_layout(21)
    tr = _trainer(student_check_iters=1, accum_steps=2)
    seen = []
    for it in (1, 2):
        for micro in (0, 1):
            _step(tr, 2 * it + micro, n_iter=tr.args.warmup_iters + it)
            seen.append(int(tr.student_check_state[off["checks"]]))
    assert seen == [0, 1, 1, 2]


def test_a_state_file_restores_the_counters(checked_run):
    """5: written after the fourth step (two checks counted), read by a fresh trainer"""
    tr = _trainer(seed=77, student_check_iters=2)                                        # another seed: nothing of its own survives the load
    assert tr.load_state(checked_run["path"])["n_iter"] == tr.args.warmup_iters + 5
    assert tr.student_check_state.cpu().tolist() == checked_run["counters"][4]
    assert tr.extra_state["student_check.counters"] is tr.student_check_state


def test_the_tool_prints_one_json_line_with_the_summary():
    """tools/student_check.py --synthetic at crop 64 against the no-grad bf16 path, in a fresh child process"""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "student_check.py"), "--synthetic", "--crop_size", "64", "--batch_size", "2", "--batches", "2",
           "--check_mode", "bf16"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    for key in ("checks", "flags", "seg", "cam", "cam_aux", "cls", "cls_aux", "seg_agree", "flip_hist", "class_agree", "losses", "mode", "check_mode"):
        assert key in rec, key
    assert rec["checks"] == 2 and rec["mode"] == "bf16" and rec["check_mode"] == "bf16" and rec["batches"] == 2 and rec["flags"] == 0
    assert rec["cells"] == 2 * 2 * 16 and rec["seg"]["n"] > 0 and 0 < rec["seg"]["rel_l2"] < 0.1 and rec["losses"]["seg_loss"]["n"] == 2
