"""The --grad_check_iters check without a GPU: the host maths on planted records, the torch composition of the two
kernels against the float64 restatement (tests/grad_check_ref.py), the site map on the real parameter names, the whole check on the toy host
trainer (torch operators: autograd is the truth), and the refusals."""
import json
import math

import numpy as np
import pytest
import torch

import grad_check_ref as ref
import test_student_check_cpu as SC

# |r* - 1| on the toy trainer against autograd: three times the worst value seen over the five directions and seeds 3, 7, 11 of the test
# below (measured: fp64 5.01e-5 at seed 11 `norm`, fp32 9.67e-5 at seed 11 `decoder`; in both modes the five terms leave the forward as
# float32, which is most of the fp64 figure), far under the cap of 1e-2
CPU_BAR = {"fp64": 1.5e-4, "fp32": 2.9e-4}
# the toy trainer's step: its five terms are O(1) numbers that leave as float32, so a difference over the default relative step of 1e-5
# (chosen on the real network at 448^2, whose curvature along g is 75) is mostly their rounding (measured 2.5e-3 / 6.5e-3); the toy's
# curvature is small and 1e-3 resolves it
TOY_RHO = 1e-3
WEIGHTS = [1.0, 1.0, 0.1, 0.05, 0.05]


def test_summary_on_an_exactly_quadratic_loss():
    from cosa_amd.utils import grad_check as gc
    g2, s = 4.0, 0.5
    t = [c * s * g2 for c in gc.STEPS]                              # 2, -2, 1, -1
    L = lambda x: 3.0 + 1.0 * x + 0.3 * x * x                       # slope 1 along g: r(1) = r(1/2) = 1; curvature 0.6 per unit t^2
    row = [0.0] * gc.RECORD
    row[gc.G2], row[gc.W2], row[gc.S], row[gc.FLAGS] = g2, 9.0, s, 0
    row[gc.T:gc.T + 4] = t
    for j, x in enumerate([0.0] + t):                                # the objective split over the terms: 2 x (cls) + 10 x (seg) x 0.1 weights
        vals = [L(x) / 4, L(x) / 4, 2.5 * L(x), 0.0, 5.0 * L(x)]
        row[gc.LOSS + 5 * j:gc.LOSS + 5 * j + 5] = vals
    (d,) = gc.summarize([row], ["all"], WEIGHTS)
    assert d["r1"] == pytest.approx(1.0, abs=1e-14) and d["r_half"] == pytest.approx(1.0, abs=1e-14) and d["r_star"] == pytest.approx(1.0, abs=1e-14)
    assert d["rough"] < 1e-14 and d["flags"] == 0 and d["flag_names"] == []
    # L(2) + L(-2) - 2 L(0) = 2 x 0.3 x 4 = 2.4 over s^2 G2 = 1
    assert d["curv"] == pytest.approx(2.4, rel=1e-13)
    assert d["terms"]["cls"] == pytest.approx(0.25, rel=1e-13) and d["terms"]["seg"] == pytest.approx(2.5, rel=1e-13) and d["terms"]["cam"] == 0.0
    want = ref.figures([L(x) for x in [0.0] + t], t, s, g2)
    assert (d["r1"], d["r_half"], d["r_star"], d["rough"], d["curv"]) == pytest.approx(want, rel=1e-13, abs=1e-14)
    # a cubic term leaves r(1) != r(1/2) and cancels in r_star
    for j, x in enumerate([0.0] + t):
        row[gc.LOSS + 5 * j:gc.LOSS + 5 * j + 5] = [L(x) + 0.01 * x ** 3, 0.0, 0.0, 0.0, 0.0]
    (d,) = gc.summarize([row], ["all"], WEIGHTS)
    assert d["r1"] == pytest.approx(1.04, rel=1e-12) and d["r_half"] == pytest.approx(1.01, rel=1e-12) and d["r_star"] == pytest.approx(1.0, abs=1e-12)
    # a flagged direction (s = 0, no step taken): NaN figures, None in a JSON record, `-` never a crash
    row[gc.S], row[gc.FLAGS] = 0.0, gc.FLAG_ZERO_GRAD
    row[gc.T:gc.T + 4] = [0.0] * 4
    (d,) = gc.summarize([row], ["all"], WEIGHTS)
    assert math.isnan(d["r_star"]) and d["flag_names"] == ["zero_grad"]
    assert json.loads(json.dumps(gc.jsonable(d)))["r_star"] is None
    assert gc.line([d], "fp64").startswith(" gcheck[fp64]: r nan")


def test_log_fragment_and_worst_site():
    from cosa_amd.utils import grad_check as gc
    mk = lambda name, r: dict(dir=name, r_star=r, curv=3.1)
    s = [mk("all", 0.9871), mk("embed", 1.001), mk("block7", 0.912), mk("heads", float("nan"))]
    assert gc.line(s, "fp64") == " gcheck[fp64]: r 0.987 (worst 0.912 block7), curv 3.1e+00"
    assert gc.line(s[:1], "fp32") == " gcheck[fp32]: r 0.987, curv 3.1e+00"


def _t(a):
    return None if a is None else torch.from_numpy(a.copy())


def test_torch_composition_equals_the_restatement():
    from cosa_amd.utils import grad_check as gc
    case = ref.make_case()
    ws, gs, dirs, n_dirs = [_t(a) for a in case["ws"]], [_t(a) for a in case["gs"]], case["dirs"], case["n_dirs"]
    rho = 1e-3
    want = ref.norms(case["ws"], case["gs"], dirs, n_dirs, rho)
    rows = torch.zeros((n_dirs, gc.RECORD), dtype=torch.float64)
    gc.norms_torch(ws, gs, dirs, n_dirs, rho, rows)
    got = rows.numpy()
    assert np.array_equal(got[:, [gc.S, gc.FLAGS, gc.BAD_G, gc.BAD_W]], want[:, [ref.S, ref.FLAGS, ref.BAD_G, ref.BAD_W]])
    assert want[:, ref.FLAGS].tolist() == [0, 0, 1, 2, 1] and want[3, ref.BAD_G] == 2 and (want[2:, ref.S] == 0).all() and (want[:2, ref.S] > 0).all()
    np.testing.assert_allclose(got[:2, [gc.G2, gc.W2]], want[:2, [ref.G2, ref.W2]], rtol=1e-12)
    dsts = [torch.full_like(w, 7.0) for w in ws]
    for d in range(n_dirs):
        for k, c in enumerate(gc.STEPS):
            gc.perturb_torch(ws, gs, dsts, dirs, d, c, k, rows)
            wp, t = ref.perturb(case["ws"], case["gs"], dirs, d, c, want[d, ref.S])
            for i, (a, b) in enumerate(zip(dsts, wp)):
                assert np.array_equal(a.numpy().view(np.uint32), b.view(np.uint32)), (d, c, i)
                if dirs[i] != d or d >= 2:
                    assert np.array_equal(b.view(np.uint32), case["ws"][i].view(np.uint32))
            assert float(rows[d, gc.T + k]) == pytest.approx(t, rel=1e-12, abs=0)
            if d < 2:                                               # the realised step is c s G2 up to the weights' own rounding
                assert t == pytest.approx(c * want[d, ref.S] * want[d, ref.G2], rel=1e-4)
    with pytest.raises(ValueError):
        gc.norms_torch(ws, gs, dirs, n_dirs, float("nan"), rows)
    with pytest.raises(ValueError):
        gc.perturb_torch(ws, gs, dsts, dirs, 0, float("inf"), 0, rows)


def test_site_map_on_the_real_parameter_names():
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    from cosa_amd.utils import grad_check as gc
    net = build_model(default_args())
    names = [n for n, _ in net.named_parameters()]
    depth = len(net.encoder.blocks)
    sites = {n: gc.site_of(n) for n in names}
    assert "other" not in sites.values()
    assert {n for n, s in sites.items() if s == "embed"} == {"encoder.cls_token", "encoder.pos_embed", "encoder.patch_embed.proj.weight",
                                                            "encoder.patch_embed.proj.bias"}
    assert {n for n, s in sites.items() if s == "norm"} == {"encoder.norm.weight", "encoder.norm.bias"}
    assert {n for n, s in sites.items() if s == "heads"} == {"classifier.weight", "aux_classifier.weight", "encoder.head.weight", "encoder.head.bias"}
    assert {n for n, s in sites.items() if s == "decoder"} == {n for n in names if n.startswith("decoder.")}
    for i in range(depth):
        assert sum(s == f"block{i}" for s in sites.values()) == 12
    assert gc.site_of("encoder.blocks.11.mlp.fc2.bias") == "block11" and gc.site_of("something.else") == "other"
    # frozen / gradient-less tensors belong to no direction; `sites` is `all` plus the sites in network order
    in_play = [n not in ("encoder.pos_embed", "encoder.head.weight", "encoder.head.bias") for n in names]
    dir_names, passes = gc.plan(names, in_play, "sites")
    assert dir_names == ["all", "embed"] + [f"block{i}" for i in range(depth)] + ["norm", "decoder", "heads"]
    (r0, n0, d0), (r1, n1, d1) = passes
    assert (r0, n0, r1, n1) == (0, 1, 1, len(dir_names) - 1)
    assert all((a == 0) == ok and (b >= 0) == ok for a, b, ok in zip(d0, d1, in_play))
    assert d1[names.index("encoder.blocks.3.attn.qkv.weight")] == dir_names.index("block3") - 1
    assert gc.plan(names, in_play, "all") == (["all"], [passes[0]])
    with pytest.raises(ValueError):
        gc.plan(names, in_play, "blocks")


# ---- the toy host trainer -------------------------------------------------------------------------------------------------------------
def _terms(m, x, y):
    """five smooth loss terms on the toy network, in the network's own dtype"""
    dt = next(m.parameters()).dtype
    h = m.norm(torch.tanh(m.encoder.proj(x.to(dt))))
    o = m.decoder(h)
    return torch.stack([m.classifier(h[:, :, None, None]).square().mean(), (o - y.to(dt)).square().mean(), 0.1 * torch.tanh(o).sum(),
                        h.pow(3).mean(), torch.cos(m.classifier.weight.sum() * h).mean()])


def _trainer(monkeypatch, seed=3, **over):
    if over.get("grad_check_iters"):
        over.setdefault("grad_check_rho", TOY_RHO)
    tr = SC._host_trainer(monkeypatch, seed, **over)

    def forward_losses(wimg, simg, cls_label, img_box, n_iter):
        loss = torch.dot(_terms(tr.student, simg, cls_label), torch.tensor(WEIGHTS))
        if tr.model_GK is not None and tr._is_check_step(n_iter, "grad"):
            tr._step_ctx = dict(x=simg, y=cls_label, weights=[float(np.float32(w)) for w in WEIGHTS])
        return loss, dict(overall_loss=loss.detach())

    monkeypatch.setattr(tr, "forward_losses", forward_losses)
    monkeypatch.setattr(tr, "_check_objective", lambda net, ctx: _terms(net, ctx["x"], ctx["y"]).float())
    return tr


def _batch(k, b=4):
    g = torch.Generator().manual_seed(500 + k)
    return torch.randn(b, 5, generator=g), torch.randn(b, 5, generator=g), torch.randn(b, 3, generator=g), None


def _backward(tr, batch, n_iter=0):
    loss, _ = tr.forward_losses(*batch, n_iter)
    tr.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    return {n: (p.grad.clone() if p.grad is not None else None) for n, p in tr.student.named_parameters()}


@pytest.mark.parametrize("mode", ["fp64", "fp32"])
def test_r_star_is_one_for_autograd_gradients_on_the_toy_trainer(monkeypatch, mode):
    from cosa_amd.utils import grad_check as gc
    worst = 0.0
    for seed in (3, 7, 11):
        tr = _trainer(monkeypatch, seed, grad_check_iters=1, grad_check_mode=mode, grad_check_dirs="sites")
        before = [p.detach().clone() for p in tr.student.parameters()]
        _backward(tr, _batch(seed))
        tr._grad_check()
        summary = tr.grad_check()
        assert [d["dir"] for d in summary] == ["all", "norm", "decoder", "heads", "other"]          # (encoder.head is frozen: in none)
        assert all(torch.equal(a, b) for a, b in zip(before, tr.student.parameters()))
        for d in summary:
            assert d["flags"] == 0 and d["s"] > 0
            print(mode, seed, d["dir"], "r*", d["r_star"], "|r*-1|", abs(d["r_star"] - 1), "rough", d["rough"])
            worst = max(worst, abs(d["r_star"] - 1))
        # G2 of `all` is the sum of the sites'; the terms' own figures add up to the objective's
        assert summary[0]["G2"] == pytest.approx(sum(d["G2"] for d in summary[1:]), rel=1e-12)
        assert sum(w * summary[0]["terms"][k] for w, k in zip(WEIGHTS, gc.TERMS)) == pytest.approx(summary[0]["r_star"], rel=1e-9)
    print("worst |r* - 1|", mode, worst)
    assert worst <= CPU_BAR[mode]


@pytest.mark.parametrize("plant", ["zeroed", "doubled"])
def test_a_planted_error_is_seen(monkeypatch, plant):
    tr = _trainer(monkeypatch, 5, grad_check_iters=1, grad_check_dirs="sites")
    full = _backward(tr, _batch(1))
    params = dict(tr.student.named_parameters())
    with torch.no_grad():
        for n in ("decoder.weight", "decoder.bias"):
            params[n].grad.mul_(0.0 if plant == "zeroed" else 2.0)
    planted = {n: p.grad for n, p in params.items() if p.grad is not None}
    dot = sum(float((full[n].double() * g.double()).sum()) for n, g in planted.items())
    want = dot / sum(float(g.double().square().sum()) for g in planted.values())
    tr._grad_check()
    summary = {d["dir"]: d for d in tr.grad_check()}
    print(plant, "want", want, "r*", summary["all"]["r_star"])
    assert summary["all"]["r_star"] == pytest.approx(want, abs=CPU_BAR["fp64"])
    if plant == "zeroed":                                           # the error is orthogonal to what is left: the figure stays 1 and the site is flagged
        assert want == pytest.approx(1.0, abs=1e-12) and summary["decoder"]["flag_names"] == ["zero_grad"] and math.isnan(summary["decoder"]["r_star"])
    else:                                                           # twice the gradient: r of the site halves, `all` drops below 1
        assert want < 0.95 and summary["decoder"]["r_star"] == pytest.approx(0.5, abs=CPU_BAR["fp64"])
    assert summary["norm"]["r_star"] == pytest.approx(1.0, abs=CPU_BAR["fp64"])


def _state(tr):
    out = [p.detach().clone() for p in tr.student.parameters()] + [p.detach().clone() for p in tr.model_AN.parameters()]
    for grp in tr.optimizer.param_groups:
        for p in grp["params"]:
            st = tr.optimizer.state.get(p, {})
            out += [st[k].clone() for k in ("exp_avg", "exp_avg_sq") if k in st]
    return out


@pytest.mark.parametrize("accum", [1, 2])
def test_training_is_untouched_and_the_check_runs_on_the_closing_micro_batch(monkeypatch, accum):
    a = _trainer(monkeypatch, 3, accum_steps=accum)
    b = _trainer(monkeypatch, 3, accum_steps=accum, grad_check_iters=2)
    assert a.model_GK is None and a.grad_check_state is None and a.grad_check() is None
    calls = []
    inner = b._grad_check
    monkeypatch.setattr(b, "_grad_check", lambda: (calls.append((n_iter, b._micro_k)), inner())[1])
    k = 0
    for n_iter in range(4):
        for _ in range(accum):
            la, lb = a.step(*_batch(k), n_iter=n_iter), b.step(*_batch(k), n_iter=n_iter)
            assert torch.equal(la["overall_loss"], lb["overall_loss"])
            k += 1
        got = b.pop_grad_check()
        assert (got is not None) == (n_iter % 2 == 1) and b.pop_grad_check() is None
    assert calls == [(1, accum - 1), (3, accum - 1)]
    sa, sb = _state(a), _state(b)
    assert len(sa) == len(sb) and all(torch.equal(x, y) for x, y in zip(sa, sb))
    assert abs(b.grad_check()[0]["r_star"] - 1) <= CPU_BAR["fp64"]                 # (with accum 2: the micro-batch's own gradient and loss)
    assert "grad_check" not in "".join(getattr(b, "extra_state", {}))


def test_refusals(monkeypatch):
    from cosa_amd import args as cosa_args
    from cosa_amd import main as launcher
    from cosa_amd import monitors, train_step
    from cosa_amd.utils import grad_check as gc
    d = train_step.default_args()
    assert (d.grad_check_iters, d.grad_check_mode, d.grad_check_dirs, d.grad_check_rho) == (0, "fp64", "all", gc.DEFAULT_RHO)
    a, _ = cosa_args.parse(["EXP"])
    assert (a.grad_check_iters, a.grad_check_mode, a.grad_check_dirs, a.grad_check_rho) == (0, "fp64", "all", gc.DEFAULT_RHO)
    a, _ = cosa_args.parse(["EXP", "--grad_check_iters", "50", "--grad_check_mode", "fp32", "--grad_check_dirs", "sites", "--grad_check_rho", "1e-4"])
    assert (a.grad_check_iters, a.grad_check_mode, a.grad_check_dirs, a.grad_check_rho) == (50, "fp32", "sites", 1e-4)
    launcher.check_supported(a)
    for bad in (["--grad_check_iters", "-1"], ["--grad_check_iters", "5", "--grad_check_mode", "bf16"],
                ["--grad_check_iters", "5", "--grad_check_dirs", "layers"], ["--grad_check_iters", "5", "--grad_check_rho", "0"]):
        a, _ = cosa_args.parse(["EXP"] + bad)
        with pytest.raises(ValueError):
            launcher.check_supported(a)
    with pytest.raises(ValueError):
        SC._host_trainer(monkeypatch, 1, grad_check_iters=-2)
    for mode in ("bf16", "fp16", "fp16x3", "auto"):                # a 16-bit forward is too noisy to difference
        with pytest.raises(ValueError):
            SC._host_trainer(monkeypatch, 1, grad_check_iters=2, grad_check_mode=mode)
    with pytest.raises(ValueError):
        SC._host_trainer(monkeypatch, 1, grad_check_iters=2, grad_check_rho=float("nan"))
    monkeypatch.setattr(train_step, "build_model", lambda args: SC._TinyNet())
    args = train_step.default_args("VOC12", crop_size=48, batch_size=3, num_classes=6, max_iters=100, grad_check_iters=2)
    with pytest.raises(NotImplementedError, match="data parallelism"):
        train_step.CoSATrainer(args, torch.device("cpu"), ddp=True, seed=1)
    # the check is no monitor row and no state entry
    assert "grad_check" not in monitors.BY_NAME
    tr = SC._host_trainer(monkeypatch, 1, grad_check_iters=2)
    assert monitors.active(tr) == [] and not hasattr(tr, "extra_state")


def test_jsonl_record(tmp_path):
    from types import SimpleNamespace
    from cosa_amd import main as launcher
    from cosa_amd.utils import grad_check as gc
    row = [0.0] * gc.RECORD
    row[gc.G2], row[gc.W2], row[gc.S] = 4.0, 9.0, 0.5
    row[gc.T:gc.T + 4] = [2.0, -2.0, 1.0, -1.0]
    for j, x in enumerate([0.0, 2.0, -2.0, 1.0, -1.0]):
        row[gc.LOSS + 5 * j] = 1.0 + 0.9 * x
    summary = gc.summarize([row, [0.0] * gc.RECORD], ["all", "heads"], WEIGHTS)
    targs = SimpleNamespace(grad_check_mode="fp64", grad_check_rho=1e-3)
    launcher.append_grad_check(tmp_path, summary, 20, targs)
    launcher.append_grad_check(tmp_path, summary, 40, targs)
    recs = [json.loads(x) for x in (tmp_path / "grad_check.jsonl").read_text().splitlines()]
    assert [r["iters"] for r in recs] == [20, 40] and recs[0]["mode"] == "fp64" and recs[0]["rho"] == 1e-3
    d = recs[0]["dirs"][0]
    assert d["dir"] == "all" and d["r_star"] == pytest.approx(0.9) and d["r1"] == pytest.approx(0.9) and d["rough"] < 1e-12
    assert set(d) >= {"r1", "r_half", "r_star", "rough", "curv", "G2", "W2", "s", "flags", "terms"} and set(d["terms"]) == set(gc.TERMS)
    assert recs[0]["dirs"][1]["r_star"] is None
