"""The --grad_check_iters check on the GPU: the two kernels of csrc/grad_check_kernels.hip against the float64
restatement (tests/grad_check_ref.py) -- dst bit for bit, sums to 1e-12 relative --, their sentinels, refusals and run-to-run bytes; the
trainer at crop 64, b = 2 (no bit of training changes, a doubled site gradient halves the site's figure exactly, --accum_steps, the tool);
and the figure against oracle/cpu_step.py's gradient."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import grad_check_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -77.25                       # the sentinel around every output
PAD = 64                            # floats of border on each side (a multiple of 4: a view's alignment is its tensor's)
RHO = 1e-3


def _dev():
    return torch.device("cuda", 0)


def _framed(a, off4, fill=None):
    """a device copy of the fp32 array `a` (or `fill` everywhere) inside a sentinel frame; off4: the view starts 4 bytes off a 16-byte boundary"""
    n, lead = a.size, PAD + (1 if off4 else 0)
    buf = torch.full((lead + n + PAD,), SENT, dtype=torch.float32, device=_dev())
    view = buf[lead:lead + n]
    view.copy_(torch.from_numpy(a) if fill is None else torch.full((n,), fill))
    assert view.data_ptr() % 16 == (4 if off4 else 0)
    return buf, view


class _Case:
    """ref.make_case() on the device: w, g and dst framed by sentinels, the record and the workspace with sentinels behind them"""

    def __init__(self, seed=0):
        from cosa_amd.utils import grad_check as gc
        self.gc, self.np = gc, ref.make_case(seed)
        c = self.np
        self.dirs, self.n_dirs = c["dirs"], c["n_dirs"]
        off = set(c["off4"])
        self.w = [_framed(a, i in off) for i, a in enumerate(c["ws"])]
        self.g = [None if a is None else _framed(a, i in off) for i, a in enumerate(c["gs"])]
        self.dst = [_framed(a, i in off, fill=5.5) for i, a in enumerate(c["ws"])]
        self.table = gc.Table([a.size for a in c["ws"]], _dev())
        need = self.table.workspace.numel()
        self.ws_buf = torch.full((need + 256,), 0x5a, dtype=torch.uint8, device=_dev())
        self.table.workspace = self.ws_buf[:need]
        self.rec_buf = torch.full(((self.n_dirs + 2) * gc.RECORD,), SENT, dtype=torch.float64, device=_dev())
        self.rows = self.rec_buf[gc.RECORD:(self.n_dirs + 1) * gc.RECORD].view(self.n_dirs, gc.RECORD)
        self.fill()

    def fill(self):
        self.table.fill([v for _, v in self.w], [None if p is None else p[1] for p in self.g], [v for _, v in self.dst], self.dirs)
        torch.cuda.synchronize()

    def frames_intact(self):
        for buf, view in self.w + [p for p in self.g if p is not None] + self.dst:
            lead = (view.data_ptr() - buf.data_ptr()) // 4
            if not (bool((buf[:lead] == SENT).all()) and bool((buf[lead + view.numel():] == SENT).all())):
                return False
        gc = self.gc
        return bool((self.rec_buf[:gc.RECORD] == SENT).all()) and bool((self.rec_buf[(self.n_dirs + 1) * gc.RECORD:] == SENT).all()) and \
            bool((self.ws_buf[self.table.workspace.numel():] == 0x5a).all())

    def inputs_intact(self):
        c = self.np
        return all(np.array_equal(v.cpu().numpy().view(np.uint32), a.view(np.uint32)) for (_, v), a in zip(self.w, c["ws"])) and \
            all(p is None or np.array_equal(p[1].cpu().numpy().view(np.uint32), a.view(np.uint32)) for p, a in zip(self.g, c["gs"]))


def _run_all(case):
    """norms, then every (direction, step): -> (rows after norms, {(d, slot): ([dst bits per tensor], t_c)}, the workspace bytes at the end)"""
    gc = case.gc
    gc.norms(case.table, case.n_dirs, RHO, case.rows)
    after_norms = case.rows.cpu().numpy().copy()
    out = {}
    for d in range(case.n_dirs):
        for k, c in enumerate(gc.STEPS):
            gc.perturb(case.table, case.n_dirs, d, c, k, case.rows)
            out[(d, k)] = ([v.cpu().numpy().view(np.uint32).copy() for _, v in case.dst], float(case.rows[d, gc.T + k]))
    return after_norms, out, case.table.workspace.cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def _kernel_run():
    case = _Case()
    return (case,) + _run_all(case)


def test_norms_equal_the_restatement():
    case, rows, _, _ = _kernel_run()
    c = case.np
    want = ref.norms(c["ws"], c["gs"], c["dirs"], c["n_dirs"], RHO)
    cols = [ref.S, ref.FLAGS, ref.BAD_G, ref.BAD_W]
    assert np.array_equal(rows[:, cols], want[:, cols]), (rows[:, cols], want[:, cols])
    np.testing.assert_allclose(rows[:3, [ref.G2, ref.W2]], want[:3, [ref.G2, ref.W2]], rtol=1e-12, atol=0)
    # G2 = 0 (direction 2), planted inf / NaN (3: both counted, G2 not finite), no tensor at all (4): flagged, s = 0
    assert rows[:, ref.FLAGS].tolist() == [0, 0, 1, 2, 1] and rows[3, ref.BAD_G] == 2 and not np.isfinite(rows[3, ref.G2])
    assert (rows[2:, ref.S] == 0).all() and (rows[:2, ref.S] > 0).all() and rows[4, ref.W2] == 0


def test_perturb_equals_the_restatement_bit_for_bit():
    case, rows, runs, _ = _kernel_run()
    c, gc = case.np, case.gc
    for (d, k), (bits, t) in runs.items():
        wp, t_want = ref.perturb(c["ws"], c["gs"], c["dirs"], d, gc.STEPS[k], rows[d, ref.S])
        for i, (a, b) in enumerate(zip(bits, wp)):
            assert np.array_equal(a, b.view(np.uint32)), (d, k, i)              # (every size, the 4-byte-off views, the tensors in no direction)
            if c["dirs"][i] != d or d >= 2:
                assert np.array_equal(a, c["ws"][i].view(np.uint32)), (d, k, i)  # outside the direction, or s = 0: dst = w
            elif c["ws"][i].size > 3:
                assert not np.array_equal(a, c["ws"][i].view(np.uint32)), (d, k, i)
        assert t == pytest.approx(t_want, rel=1e-12, abs=0), (d, k)
        assert d < 2 or t == 0.0
    assert case.frames_intact() and case.inputs_intact()


def test_two_runs_give_identical_bytes():
    _, rows, runs, ws = _kernel_run()
    other = _Case()
    rows2, runs2, ws2 = _run_all(other)
    assert rows.tobytes() == rows2.tobytes() and ws.tobytes() == ws2.tobytes()
    for key, (bits, t) in runs.items():
        assert np.float64(t).tobytes() == np.float64(runs2[key][1]).tobytes(), key
        assert all(np.array_equal(a, b) for a, b in zip(bits, runs2[key][0])), key


def test_every_refusal_returns_einval_and_touches_nothing():
    from cosa_amd import _C
    case = _Case(seed=1)
    gc, t, L = case.gc, case.table, _C.lib()
    stream = _C.stream_ptr()
    before = (case.rec_buf.clone(), case.ws_buf.clone(), [b.clone() for b, _ in case.dst])

    def untouched():
        torch.cuda.synchronize()
        return torch.equal(case.rec_buf, before[0]) and torch.equal(case.ws_buf, before[1]) and \
            all(torch.equal(b, x) for (b, _), x in zip(case.dst, before[2]))

    def norms(host=None, dev=None, n_tensors=None, n_chunks=None, n_dirs=None, rho=RHO, rec=None, ws=None, ws_bytes=None):
        pick = lambda v, d: d if v is None else v
        return L.cosa_grad_check_norms(pick(host, t.host.data_ptr()), pick(dev, t.dev.data_ptr()), pick(n_tensors, t.n_tensors),
                                       pick(n_chunks, t.n_chunks), pick(n_dirs, case.n_dirs), rho, pick(rec, case.rows.data_ptr()),
                                       pick(ws, t.workspace.data_ptr()), pick(ws_bytes, t.workspace.numel()), stream)

    def perturb(host=None, dev=None, n_dirs=None, d=0, c=1.0, slot=0, rec=None, ws=None, ws_bytes=None):
        pick = lambda v, dflt: dflt if v is None else v
        return L.cosa_grad_check_perturb(pick(host, t.host.data_ptr()), pick(dev, t.dev.data_ptr()), t.n_tensors, t.n_chunks,
                                         pick(n_dirs, case.n_dirs), d, c, slot, pick(rec, case.rows.data_ptr()),
                                         pick(ws, t.workspace.data_ptr()), pick(ws_bytes, t.workspace.numel()), stream)

    bad_calls = [lambda: norms(host=0), lambda: norms(dev=0), lambda: norms(rec=0), lambda: norms(ws=0), lambda: norms(n_tensors=0),
                 lambda: norms(n_chunks=0), lambda: norms(n_dirs=0), lambda: norms(n_dirs=3),              # (a record says dir 3: outside [-1, 3))
                 lambda: norms(ws_bytes=t.workspace.numel() - 1), lambda: norms(n_chunks=t.n_chunks - 1),
                 lambda: norms(rho=float("nan")), lambda: norms(rho=float("inf")), lambda: norms(rho=0.0), lambda: norms(rho=-1e-3),
                 lambda: perturb(host=0), lambda: perturb(dev=0), lambda: perturb(rec=0), lambda: perturb(ws=0),
                 lambda: perturb(ws_bytes=8 * t.n_chunks - 1), lambda: perturb(d=-1), lambda: perturb(d=case.n_dirs),
                 lambda: perturb(slot=-1), lambda: perturb(slot=4), lambda: perturb(c=float("nan")), lambda: perturb(c=float("inf"))]
    for i, call in enumerate(bad_calls):
        assert call() == 1, i                                                   # COSA_EINVAL
        assert L.cosa_last_error(), i
    assert untouched()
    # a bad record or chunk in the table itself (the host copy is what the envelope reads)
    recs, chunks = t.recs, t.host.numpy()[t.n_tensors * 40:].view("<i4").reshape(-1, 2)
    for field, i, value in (("n", 2, -1), ("dir", 0, case.n_dirs), ("dir", 0, -2), ("w", 3, 0), ("dst", 3, 0), ("g", 1, 0), ("w", 4, recs["w"][4] + 2)):
        held = recs[field][i]
        recs[field][i] = value
        assert norms() == 1 and perturb() == 1, (field, i, value)
        recs[field][i] = held
    for row, col, value in ((5, 1, 7), (0, 0, 1), (t.n_chunks - 1, 0, -1), (3, 1, -1)):
        held = chunks[row, col]
        chunks[row, col] = value
        assert norms() == 1 and perturb() == 1, (row, col, value)
        chunks[row, col] = held
    assert untouched()
    assert norms() == 0 and perturb() == 0                                      # the table as it was is accepted
    torch.cuda.synchronize()
    assert case.frames_intact()
    with pytest.raises(ValueError):
        case.table.fill([v for _, v in case.w], [None] * len(case.w), [v for _, v in case.dst], case.dirs)


# ---- the trainer at crop 64, b = 2 ------------------------------------------------------------------------------------------------------
LOSSES = ("cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")


def _trainer(seed=3, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, **over)
    return CoSATrainer(args, _dev(), seed=seed)


def _batch(tr, k):
    from cosa_amd.train_step import synthetic_batch
    return synthetic_batch(2, 64, 20, tr.device, seed=700 + k)


def _step(tr, k, n_iter=None):
    logs = tr.step(*_batch(tr, k), n_iter=tr.args.warmup_iters + 1 + k if n_iter is None else n_iter)
    return torch.stack([logs[n].reshape(()).float() for n in LOSSES]).clone()


def _state(tr):
    out = {}
    for tag, net in (("ON", tr.student), ("AN", tr.model_AN)):
        for n, p in net.named_parameters():
            out[f"{tag}.{n}"] = p.detach().clone()
    names = {id(p): n for n, p in tr.student.named_parameters()}
    for p, st in tr.optimizer.state.items():
        for k in ("exp_avg", "exp_avg_sq"):
            out[f"opt.{names[id(p)]}.{k}"] = st[k].clone()
    return out


def test_the_flag_changes_no_bit_of_three_steps():
    a = _trainer()
    assert a.model_GK is None and a.grad_check_state is None and a.grad_check() is None
    la = torch.stack([_step(a, k) for k in (1, 2, 3)])
    b = _trainer(grad_check_iters=1)
    assert b.args.grad_check_mode == "fp64" and b.model_GK is not None
    assert not {id(p) for p in b.model_GK.parameters()} & {id(p) for p in b.student.parameters()}
    lb, seen = [], []
    for k in (1, 2, 3):
        lb.append(_step(b, k))
        seen.append(b.pop_grad_check())
    assert torch.equal(la.view(torch.int32), torch.stack(lb).view(torch.int32))
    sa, sb = _state(a), _state(b)
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k].reshape(-1).view(torch.uint8), sb[k].reshape(-1).view(torch.uint8)), k
    for s in seen:
        assert [d["dir"] for d in s] == ["all"] and s[0]["flags"] == 0 and s[0]["s"] > 0 and np.isfinite(s[0]["r_star"])
        print("r*", s[0]["r_star"], "r1", s[0]["r1"], "r_half", s[0]["r_half"], "curv", s[0]["curv"])
    assert not hasattr(b, "extra_state")


def test_doubling_a_sites_gradient_halves_its_figure_exactly():
    from cosa_amd import nn_ops
    tr = _trainer(grad_check_iters=1, grad_check_dirs="sites")
    batch, n_iter = _batch(tr, 1), tr.args.warmup_iters + 2
    recs = []
    for scale in (1.0, 2.0):
        loss, _ = tr.forward_losses(*batch, n_iter)
        tr.optimizer.zero_grad(set_to_none=True)
        nn_ops.wgrad_arena_begin(tr.device)
        loss.backward()
        with torch.no_grad():
            for n, p in tr.student.named_parameters():
                if n.startswith("encoder.blocks.3.") and p.grad is not None:
                    p.grad.mul_(scale)
        tr._grad_check()
        recs.append(({d["dir"]: d for d in tr.grad_check()}, tr.grad_check_record.clone()))
    (one, rec1), (two, rec2) = recs
    gc = __import__("cosa_amd.utils.grad_check", fromlist=["x"])
    names = [d for d in one]
    i = names.index("block3")
    assert names[:2] == ["all", "embed"] and names[-3:] == ["norm", "decoder", "heads"] and len(names) == 17
    # s halves and s g is unchanged: the four weight sets, hence the 25 losses and t_c, are the same bits; r* = dL / t ... with t halved twice over g
    assert two["block3"]["s"] == one["block3"]["s"] / 2 and two["block3"]["G2"] == pytest.approx(4 * one["block3"]["G2"], rel=1e-12)
    assert torch.equal(rec1[i, gc.LOSS:gc.LOSS + 25], rec2[i, gc.LOSS:gc.LOSS + 25])
    assert torch.equal(rec1[i, gc.T:gc.T + 4] * 2, rec2[i, gc.T:gc.T + 4])
    assert two["block3"]["r_star"] == one["block3"]["r_star"] / 2 and two["block3"]["r1"] == one["block3"]["r1"] / 2
    for d in one.values():
        print(d["dir"], "r*", d["r_star"], "rough", d["rough"], "|g|", d["G2"] ** 0.5)
    for k in names:
        if k not in ("all", "block3"):
            assert two[k]["r_star"] == one[k]["r_star"] and torch.equal(rec1[names.index(k)], rec2[names.index(k)]), k
    assert two["all"]["r_star"] < one["all"]["r_star"]


def test_accum_steps_checks_the_closing_micro_batch_only():
    tr = _trainer(grad_check_iters=1, accum_steps=2)
    seen = []
    for it in (1, 2):
        for micro in (0, 1):
            _step(tr, 2 * it + micro, n_iter=tr.args.warmup_iters + it)
            seen.append(tr.pop_grad_check() is not None)
    assert seen == [False, True, False, True]
    assert np.isfinite(tr.grad_check()[0]["r_star"])


def test_the_tool_prints_one_json_line():
    cmd = [sys.executable, os.path.join(ROOT, "tools", "grad_check.py"), "--synthetic", "--crop_size", "64", "--batch_size", "2", "--batches", "2",
           "--mode", "fp32", "--dirs", "sites"]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.strip().splitlines()
    rec = json.loads(lines[-1])
    assert sum(1 for x in lines if x.startswith("{")) == 1
    assert rec["mode"] == "fp32" and rec["dirs"] == "sites" and len(rec["batches"]) == 2 and rec["synthetic"] is True
    assert [d["dir"] for d in rec["batches"][0]][:2] == ["all", "embed"] and len(rec["batches"][0]) == 17
    assert all(d["flags"] == 0 and d["r_star"] is not None for b in rec["batches"] for d in b)
    assert lines[0] == "batch 0:" and lines[1].split()[:2] == ["dir", "r_star"]


# ---- against the reference's gradient --------------------------------------------------------------------------------------------------
ORACLE_S = 64                       # the smallest of 64, 128, 224 where the label agreement holds (measured 0.99988, 1.0, 1.0 for the seeds below)
# |r* - q| <= three times the worst value seen over seeds 3, 7, 11 at the default rho (9.49e-4, 3.27e-4, 4.7e-6), under the cap of 2e-2
ORACLE_BAR = 2.85e-3


@functools.lru_cache(maxsize=None)
def _oracle_run(seed):
    from cosa_amd import nn_ops
    from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch
    from oracle.cpu_step import CpuStep
    S, b, C = ORACLE_S, 2, 20
    args = default_args("VOC12", crop_size=S, teacher_precision="fp16c8", teacher_graph=False, teacher_async=False, grad_check_iters=1)
    tr = CoSATrainer(args, _dev(), seed=seed)
    sd = {k: v.detach().cpu().clone() for k, v in tr.student.state_dict().items()}
    wimg, simg, lab, box = synthetic_batch(b, S, C, _dev(), seed=seed + 2)
    n_iter = args.warmup_iters + 1
    loss, logs = tr.forward_losses(wimg, simg, lab, box, n_iter)
    tr.optimizer.zero_grad(set_to_none=True)
    nn_ops.wgrad_arena_begin(tr.device)
    loss.backward()
    tr._grad_check()
    summary = tr.grad_check()[0]
    torch.set_num_threads(max(1, min(16, torch.get_num_threads())))
    cpu = CpuStep(sd, num_classes=21, aux_layer=-4)
    closs, clogs = cpu.losses(wimg.cpu(), simg.cpu(), lab.cpu(), box.numpy(), n_iter)
    agree = float((logs["mask"].cpu().numpy() == clogs["mask"].numpy()).mean())
    cpu.opt.zero_grad(set_to_none=True)
    closs.backward()
    dot = gg = 0.0
    for n, p in tr.student.named_parameters():
        if p.grad is not None:
            g, go = p.grad.detach().double().cpu().flatten(), cpu.student.p(n).grad.double().flatten()
            dot += float(go @ g)
            gg += float(g @ g)
    return dict(agree=agree, q=dot / gg, r_star=summary["r_star"], rough=summary["rough"], flags=summary["flags"])


@pytest.mark.parametrize("seed", [3, 7, 11])
def test_r_star_equals_the_oracles_projection(seed):
    """q = <g_oracle, g> / <g, g> from oracle/cpu_step.py (fp32 CPU autograd) on identical weights, batch and labels against r_star of
    direction `all`, mode fp64, the default rho (1e-5), S = 64, b = 2.  Measured on one MI355X (r_star | q | difference): seed 3 0.997600 |
    0.998548 | 9.49e-4, seed 7 0.999473 | 0.999146 | 3.27e-4, seed 11 1.000466 | 1.000461 | 4.7e-6; at rho 1e-4 the differences are 3.3e-3,
    3.7e-4, 3.6e-3 and at 1e-3 (r(1) and r(1/2) 0.12 apart) 6.5e-2, 5.0e-2, 8.4e-2: the step, not the gradient."""
    r = _oracle_run(seed)
    print("seed", seed, r, "|r* - q|", abs(r["r_star"] - r["q"]))
    assert r["agree"] >= 0.999, r
    assert r["flags"] == 0
    assert abs(r["r_star"] - r["q"]) <= ORACLE_BAR, r
