"""The "fp32" operand mode of the no-grad passes end to end: the network against the reference's golden and the
float64 oracle, the multi-scale products, batch invariance, the captured teacher, and fp32 as the check mode of --teacher_check_iters.
Measured figures go on record in profiles/fp32_teacher_parity.txt (tests/test_f32_kernels_gpu.py: record)."""
import os

import numpy as np
import pytest
import torch

from test_f32_kernels_gpu import record

pytestmark = pytest.mark.gpu

OUTPUTS = ("cls", "cls_aux", "x4", "seg", "cam", "cam_aux")
LOSSES = ("cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")
FACTOR = 10.0          # a sequential MFMA chain sits up to ~6u sum|ab| from exact at K = 4096 where a blocked CPU sum is about 1u


def test_fp32_network_vs_float64_oracle_on_the_reference_golden(golden):
    """the reference's fp32 outputs (tests/golden/vit_base_d2.npz) sit about 1e-6 of range from the float64 evaluation of the same network; the
    HIP network in mode "fp32" must sit within 10 x that distance, for each of the six outputs, `seg` included (the decoder runs fp32 too)"""
    from test_network_gpu import _vit_b_width_model
    from oracle import torch_oracle as to
    from oracle.gen_golden import recipe_state, VIT_BASE_CFG as cfg
    net, g = _vit_b_width_model(golden)
    net.set_nograd_precision("fp32")
    x = torch.from_numpy(g["x"])
    with torch.no_grad():
        assert net.encoder.use_fused(x.cuda()), "the fused HIP path must be the one that runs"
        out = [o.double().cpu().numpy() for o in net(x.cuda())]
    assert "_weight_shadows" not in net.__dict__, "an fp32 pass makes no 16-bit copy of a weight"
    shapes = {str(k): tuple(int(d) for d in str(s_).split(",")) for k, s_ in zip(g["shape_keys"], g["shape_dims"])}
    sd, _ = recipe_state(shapes)
    m = to.OracleViT(num_classes=cfg["num_classes"], embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"],
                     aux_layer=cfg["aux_layer"])
    m.load_named(sd)
    with torch.no_grad():
        ref64 = [o.numpy() for o in m.double()(x.double())]
    fails = []
    for name, o, r64 in zip(OUTPUTS, out, ref64):
        assert o.shape == r64.shape == g[name].shape, name
        rng = np.abs(r64).max()
        e_hip, e_ref = np.abs(o - r64).max() / rng, np.abs(g[name].astype(np.float64) - r64).max() / rng
        record(f"golden vit_base_d2 {name}", f"hip_vs_f64={e_hip:.3e} golden_vs_f64={e_ref:.3e} ratio={e_hip / e_ref:.2f}")
        if not e_hip <= FACTOR * e_ref:
            fails.append((name, e_hip, e_ref))
    assert not fails, fails


_DRAW = {}


def _draw(oracle_c):
    """S = 64, b = 2, default pseudo_scales, fixed seeds: the fp32 HIP network's multi-scale products and the oracle's in float64 and fp32"""
    if not _DRAW:
        from oracle import torch_oracle as to
        from cosa_amd.models import build_model
        from cosa_amd.train_step import default_args, synthetic_batch
        from cosa_amd.utils import seg_helper
        S = 64
        args = default_args("VOC12", crop_size=S, batch_size=2)
        torch.manual_seed(7)
        net = build_model(args).eval()
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        wimg, _, lab, box = synthetic_batch(2, S, 20, torch.device("cpu"), seed=9)
        m = to.OracleViT(num_classes=21, aux_layer=args.aux_layer)
        m.load_named(sd)
        with torch.no_grad():
            c32, a32, _ = to.multi_scale_camseg(m, wimg, list(args.pseudo_scales))
            c64, a64, _ = to.multi_scale_camseg(m.double(), wimg.double(), list(args.pseudo_scales))
        bx = np.asarray(box.numpy(), np.int32)
        masks32 = [oracle_c.cam2mask(None, bx, c.numpy(), lab.numpy(), 0.7, 0.25, 2, par=None) for c in (c32, a32)]
        net = net.cuda().set_nograd_precision("fp32")
        _DRAW.update(args=args, net=net, wimg=wimg, lab=lab, box=box, o32=(c32, a32), o64=(c64, a64), masks32=masks32)
    return _DRAW


def test_fp32_multi_scale_cams_vs_the_float64_oracle(oracle_c):
    """normalised CAMs of `multi_scale_camseg`: max over the active planes of |HIP - float64| <= 10 x the same maximum for the oracle run in
    fp32; the label maps of cam2mask agree >= 0.999 with the fp32 oracle's"""
    from cosa_amd.utils import seg_helper
    d = _draw(oracle_c)
    wimg, lab, box = d["wimg"].cuda(), d["lab"].cuda(), d["box"]
    with torch.no_grad():
        cam, aux, _ = seg_helper.multi_scale_camseg(d["net"], wimg, d["args"].pseudo_scales)
        masks = [seg_helper.cam2mask(wimg, box, c * lab[:, :, None, None], lab, 0.7, 0.25).cpu().numpy() for c in (cam, aux)]
    act = d["lab"].bool()
    assert int(act.sum()) > 0
    fails = []
    for name, hip, o32, o64, mg, mo in zip(("cam", "cam_aux"), (cam, aux), d["o32"], d["o64"], masks, d["masks32"]):
        e_hip = float((hip.cpu().double() - o64).abs().amax(dim=(2, 3))[act].max())
        e_ref = float((o32.double() - o64).abs().amax(dim=(2, 3))[act].max())
        agree = float(np.mean(mg == mo))
        record(f"multi_scale S=64 b=2 {name}", f"hip_vs_f64={e_hip:.3e} oracle_fp32_vs_f64={e_ref:.3e} ratio={e_hip / e_ref:.2f} label_agreement={agree:.5f}")
        if not (e_hip <= FACTOR * e_ref and agree >= 0.999):
            fails.append((name, e_hip, e_ref, agree))
    assert not fails, fails


def test_fp32_pass_is_batch_invariant(oracle_c):
    """image 0's CAMs and seg from a batch of 2 == from a batch of 1, bit for bit (every GEMM row and attention slice is computed alone)"""
    from cosa_amd.utils import seg_helper
    d = _draw(oracle_c)
    wimg = d["wimg"].cuda()
    with torch.no_grad():
        two = [t.clone() for t in seg_helper.multi_scale_camseg(d["net"], wimg, d["args"].pseudo_scales)]
        one = seg_helper.multi_scale_camseg(d["net"], wimg[:1].contiguous(), d["args"].pseudo_scales)
    for name, a, b in zip(("cam", "cam_aux", "seg"), two, one):
        assert torch.isfinite(a).all() and float(a.abs().max()) > 0, name
        assert torch.equal(a[:1].view(torch.int32), b.view(torch.int32)), (name, float((a[:1] - b).abs().max()))


def test_fp32_teacher_graph_every_replay_equals_the_eager_pass():
    """the captured fp32 teacher pass gives the eager pass's bits on every replay (the pattern of tests/test_stream_gpu.py for the other modes)"""
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args, synthetic_batch
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    wimg, _, lab, _ = synthetic_batch(2, 64, 20, dev, seed=100)
    args = default_args("VOC12", crop_size=64, batch_size=2)
    torch.manual_seed(0)
    net = build_model(args).to(dev).eval().set_nograd_precision("fp32")
    bufs = {}
    run = lambda: seg_helper.multi_scale_camseg(net, wimg, args.pseudo_scales, _active_labels=lab, _seg_scales=True, _buffers=bufs)
    with torch.no_grad():
        for _ in range(2):
            e = run()
        torch.cuda.synchronize()
        ref = [e[0].clone(), e[1].clone()] + [t.clone() for t in e[2]]
        assert all(torch.isfinite(t).all() for t in ref)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            out = run()
        for rep in range(3):
            g.replay()
            torch.cuda.synchronize()
            for name, c, r in zip(("cam", "cam_aux", "seg0", "seg1", "seg2"), [out[0], out[1]] + list(out[2]), ref):
                assert torch.equal(c, r), (rep + 1, name, float((c - r).abs().max()))
    assert "_weight_shadows" not in net.__dict__


def _trainer(seed=3, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    return CoSATrainer(default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, **over), torch.device("cuda", 0), seed=seed)


def _run(tr, steps=3):
    from cosa_amd.train_step import synthetic_batch
    losses = []
    for k in range(1, steps + 1):
        logs = tr.step(*synthetic_batch(2, 64, 20, tr.device, seed=500 + k), n_iter=tr.args.warmup_iters + k)
        losses.append(torch.stack([logs[n].reshape(()).float() for n in LOSSES]).clone())
    torch.cuda.synchronize()
    return torch.stack(losses)


def _weights(tr):
    return {f"{tag}.{n}": p.detach().clone() for tag, net in (("ON", tr.student), ("AN", tr.model_AN)) for n, p in net.named_parameters()}


def test_trainer_with_the_fp32_teacher():
    """--teacher_precision fp32: three steps past warm-up with the teacher captured in its hipGraph; losses finite; the teacher has no 16-bit
    shadows and its EMA update still moves its fp32 masters"""
    tr = _trainer(teacher_precision="fp32")
    assert tr.args.teacher_precision == "fp32" and tr._teacher_shadows is None and tr.model_AN.encoder.precision == "f32"
    before = [p.detach().clone() for p in tr.model_AN.parameters()]
    losses = _run(tr)
    assert tr._graph is not None and tr.graph_error is None, tr.graph_error
    assert torch.isfinite(losses).all(), losses
    assert any(not torch.equal(a, b) for a, b in zip(before, tr.model_AN.parameters()))
    assert "_weight_shadows" not in tr.model_AN.__dict__


def test_fp32_check_mode_changes_no_bit_of_the_run_and_counts_its_checks():
    """--teacher_check_iters 1 --teacher_check_mode fp32 on the default teacher: student and teacher weights after three steps are those of the
    run without the flags, bit for bit; 3 checks, planes > 0, nothing non-finite.  The `worst` figure goes on record and is not asserted: nobody
    has measured fp16x3 against fp32 at S = 64."""
    from cosa_amd.utils import seg_helper
    plain = _trainer()
    l0 = _run(plain)
    w0 = _weights(plain)
    del plain
    tr = _trainer(teacher_check_iters=1, teacher_check_mode="fp32")
    assert tr.args.teacher_precision == "fp16x3" and tr.args.teacher_check_mode == "fp32"
    assert tr.model_CK is not None and tr.model_CK.encoder.precision == "f32" and tr._checks["teacher_check"].shadows is None
    l1 = _run(tr)
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32))
    w1 = _weights(tr)
    assert w0.keys() == w1.keys()
    for k in w0:
        assert torch.equal(w0[k].view(torch.int32), w1[k].view(torch.int32)), k
    s = tr.teacher_check()
    assert s["checks"] == 3
    for name in seg_helper.TEACHER_CHECK_SETS:
        assert s[name]["planes"] > 0 and s[name]["nonfinite_a"] == s[name]["nonfinite_b"] == 0, (name, s[name])
        record(f"teacher_check S=64 b=2 fp16x3 vs fp32 {name}", f"worst={s[name]['worst']:.3e} over={s[name]['over']}/{s[name]['planes']}")
    for name in seg_helper.TEACHER_CHECK_PAIRS:
        record(f"teacher_check S=64 b=2 fp16x3 vs fp32 {name}", f"agree={s[name]['agree']:.5f} miou={s[name]['miou']:.5f}")


def test_an_fp32_teacher_checked_in_fp32_finds_nothing():
    from cosa_amd.utils import seg_helper
    tr = _trainer(teacher_precision="fp32", teacher_check_iters=1, teacher_check_mode="fp32")
    _run(tr)
    s = tr.teacher_check()
    assert s["checks"] == 3
    for name in seg_helper.TEACHER_CHECK_SETS:
        assert s[name]["planes"] > 0 and s[name]["worst_bits"] == 0 and s[name]["over"] == 0, (name, s[name])
        assert s[name]["nonfinite_a"] == s[name]["nonfinite_b"] == 0
    for name in seg_helper.TEACHER_CHECK_PAIRS:
        assert s[name]["pix"] > 0 and s[name]["agree"] == 1.0 and s[name]["miou"] == 1.0, (name, s[name])
