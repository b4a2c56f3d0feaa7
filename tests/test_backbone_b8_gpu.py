"""The DINO ViT-B/8 encoder (`dino_base_patch8_224`) on the MI355X: the patch-projection weight gradient at K = 192, the fp16x3 teacher
against the fp32 CPU oracle with patch 8, the student step against oracle/cpu_step.py with patch 8, replay == eager for the captured teacher,
run-to-run determinism, one full-size step (448^2 x 16) and evaluate() against the oracle's composition."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B8 = "dino_base_patch8_224"
# the pre-registered per-plane criterion of tests/test_precision_gpu.py (kept equal there, in bench.py and in tests/test_boundary.py)
CAM_BAR, COND_MAX, FP64_FACTOR, AGREE_BAR, MIOU_BAR = 1e-3, 50.0, 4.0, 0.999, 0.999
# tests/test_losses_gpu.py:STUDENT_BARS["fp32"] (the default fp32 residual stream)
STUDENT_BARS = dict(enc=0.995, enc224=0.992, qk=0.99, dec=0.999, loss=1e-3)


def _args(**kw):
    from cosa_amd.train_step import default_args
    return default_args("VOC12", backbone=B8, **kw)


@pytest.mark.parametrize("M", [1000, 50176])
def test_patch_projection_weight_gradient_vs_float64(M):
    from cosa_amd import nn_ops
    g = torch.Generator(device="cuda").manual_seed(M)
    dy = torch.randn(M, 768, device="cuda", generator=g).to(torch.bfloat16)
    x = torch.randn(M, 192, device="cuda", generator=g).to(torch.bfloat16)
    dw, db = nn_ops.patch_wgrad(dy, x)
    dw, db = dw.clone(), db.clone()
    ref = dy.double().t() @ x.double()
    refb = dy.double().sum(0)
    assert float((dw.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()) + 1e-4
    assert float((db.double() - refb).abs().max()) <= 1e-5 * float(refb.abs().max()) + 1e-4
    dw2, db2 = nn_ops.patch_wgrad(dy, x)
    assert torch.equal(dw2, dw) and torch.equal(db2, db)


_ORACLE = {}


def _oracle(S, seed, b=2):
    if (S, seed, b) not in _ORACLE:
        _ORACLE.clear()
        from oracle import c_oracle, torch_oracle as to
        from cosa_amd.models import build_model
        from cosa_amd.train_step import synthetic_batch
        torch.manual_seed(seed)
        net = build_model(_args(crop_size=S, compute_dtype=torch.float32))
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        wimg, _, lab, box = synthetic_batch(b, S, 20, torch.device("cpu"), seed=seed + 2)
        m = to.OracleViT(num_classes=21, aux_layer=_args().aux_layer, patch=8)
        m.load_named(sd)
        torch.set_num_threads(16)
        with torch.no_grad():
            cam, cam_aux, _, sc_cam, sc_aux = to.multi_scale_camseg(m, wimg, [1.0, 0.5, 1.5], return_scale=True)
        bx = np.asarray(box.numpy(), np.int32)
        masks = [c_oracle.cam2mask(None, bx, c.numpy(), lab.numpy(), 0.7, 0.25, 2, par=None) for c in (cam, cam_aux)]
        _ORACLE[(S, seed, b)] = (sd, wimg, lab, box, cam, cam_aux, masks, (sc_cam, sc_aux), m)
    return _ORACLE[(S, seed, b)]


_POOL = {}


@pytest.mark.parametrize("S,seed", [(224, 3), (224, 11), (224, 29), (448, 3)])
def test_fp16x3_teacher_at_patch_8_vs_fp32_cpu_oracle(S, seed):
    """per active CAM plane: normalised-CAM |delta| <= CAM_BAR, or -- planes of conditioning > COND_MAX only -- own-scale err <= CAM_BAR and
    |HIP - float64| <= CAM_BAR + FP64_FACTOR x |fp32 - float64|; label agreement >= AGREE_BAR per draw; mIoU pooled over the draws >= MIOU_BAR"""
    from oracle import torch_oracle as to
    from cosa_amd.models import build_model
    from cosa_amd.utils import seg_helper
    sd, wimg, lab, box, cam_o, aux_o, masks_o, scales_o, m = _oracle(S, seed)
    args = _args(crop_size=S)
    net = build_model(args).cuda().eval()
    net.load_state_dict(sd)
    net.set_nograd_precision("fp16x3")
    with torch.no_grad():
        cam, cam_aux, _ = seg_helper.multi_scale_camseg(net, wimg.cuda(), args.pseudo_scales)
        masks = [seg_helper.cam2mask(wimg.cuda(), box, c * lab.cuda()[:, :, None, None], lab.cuda(), 0.7, 0.25).cpu().numpy() for c in (cam, cam_aux)]
    assert cam.shape[-1] == S
    act = lab.bool()
    o64 = None
    fails = []
    for k, (name, g, o, mg, mo, (peak, rawmax)) in enumerate((("cam", cam.cpu(), cam_o, masks[0], masks_o[0], scales_o[0]),
                                                              ("cam_aux", cam_aux.cpu(), aux_o, masks[1], masks_o[1], scales_o[1]))):
        d = (g - o).abs().amax(dim=(2, 3))
        lit = d / o.abs().amax(dim=(2, 3)).clamp_min(1e-6)
        own = d * peak / rawmax.clamp_min(1e-30)
        cond = rawmax / peak
        for i, c in zip(*torch.nonzero(act & (lit > CAM_BAR), as_tuple=True)):
            i, c = int(i), int(c)
            if float(cond[i, c]) <= COND_MAX:
                fails.append((name, i, c, float(lit[i, c]), float(cond[i, c])))
                continue
            if o64 is None:
                with torch.no_grad():
                    o64 = to.multi_scale_camseg(m.double(), wimg.double(), [1.0, 0.5, 1.5])[:2]
                m.float()
            p64 = o64[k][i, c]
            bound = CAM_BAR + FP64_FACTOR * float((o[i, c].double() - p64).abs().max())
            if not (float(own[i, c]) <= CAM_BAR and float((g[i, c].double() - p64).abs().max()) <= bound):
                fails.append((name, i, c, float(lit[i, c]), float(cond[i, c]), "fp64 leg"))
        agree = float(np.mean(mg == mo))
        assert agree >= AGREE_BAR, (name, agree)
        pool = _POOL.setdefault(name, {})
        for cl in list(range(21)) + [255]:
            P, T = mg == cl, mo == cl
            v = [int((P & T).sum()), int((P & ~T).sum()), int((~P & T).sum())]
            pool[cl] = [a + b for a, b in zip(pool.get(cl, [0, 0, 0]), v)]
    assert not fails, fails
    for name, pool in _POOL.items():
        ious = [v[0] / (v[0] + v[1] + v[2]) for v in pool.values() if v[0] + v[2] > 0]
        assert float(np.mean(ious)) >= MIOU_BAR, (name, float(np.mean(ious)))


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-300))


def test_student_step_at_patch_8_vs_cpu_oracle():
    from cosa_amd.train_step import CoSATrainer, synthetic_batch
    from oracle.cpu_step import CpuStep
    dev = torch.device("cuda", 0)
    S, b, C = 128, 2, 20
    args = _args(crop_size=S, teacher_graph=False, teacher_async=False)
    tr = CoSATrainer(args, dev, seed=3)
    assert args.teacher_precision == "fp16x3"
    sd = {k: v.detach().cpu().clone() for k, v in tr.student.state_dict().items()}
    wimg, simg, lab, box = synthetic_batch(b, S, C, dev, seed=5)
    n_iter = args.warmup_iters + 1
    loss, logs = tr.forward_losses(wimg, simg, lab, box, n_iter)
    torch.set_num_threads(16)
    cpu = CpuStep(sd, num_classes=21, aux_layer=-4, vit_kwargs={"patch": 8})
    closs, clogs = cpu.losses(wimg.cpu(), simg.cpu(), lab.cpu(), box.numpy(), n_iter)
    agree = (logs["mask"].cpu().numpy() == clogs["mask"].numpy()).mean()
    assert agree >= 0.999, agree
    for k in ("cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss", "overall_loss"):
        assert float(logs[k]) == pytest.approx(float(clogs[k]), rel=STUDENT_BARS["loss"], abs=2e-5), (k, float(logs[k]), float(clogs[k]))
    tr.optimizer.zero_grad(set_to_none=True)
    loss.backward()
    cpu.opt.zero_grad(set_to_none=True)
    closs.backward()
    named = dict(tr.student.named_parameters())
    assert tuple(named["encoder.patch_embed.proj.weight"].grad.shape) == (768, 3, 8, 8)
    for name in ("encoder.patch_embed.proj.weight", "encoder.patch_embed.proj.bias", "encoder.blocks.0.attn.proj.weight",
                 "encoder.blocks.5.mlp.fc1.weight", "encoder.blocks.11.mlp.fc2.weight", "decoder.conv6.weight", "decoder.conv8.weight",
                 "classifier.weight", "aux_classifier.weight"):
        gg, gc = named[name].grad.float().cpu(), cpu.student.p(name).grad
        cs, ratio = _cos(gg, gc), float(gg.norm() / (gc.norm() + 1e-30))
        bar = STUDENT_BARS["enc224"] if name.startswith("encoder.") else STUDENT_BARS["dec"]
        assert cs >= bar and 0.95 <= ratio <= 1.05, (name, cs, ratio)


def test_training_step_at_patch_8_is_bit_identical_run_to_run():
    from cosa_amd.train_step import CoSATrainer, synthetic_batch
    dev = torch.device("cuda", 0)
    args = _args(crop_size=128, batch_size=2, teacher_graph=False, teacher_async=False)
    tr = CoSATrainer(args, dev, seed=7)
    wimg, simg, lab, box = synthetic_batch(2, 128, 20, dev, seed=9)
    runs = []
    for _ in range(2):
        tr.optimizer.zero_grad(set_to_none=True)
        loss, _ = tr.forward_losses(wimg, simg, lab, box, args.warmup_iters + 1)
        loss.backward()
        runs.append((loss.detach().clone(), {n: p.grad.detach().clone() for n, p in tr.student.named_parameters() if p.grad is not None}))
    assert "encoder.patch_embed.proj.weight" in runs[0][1] and len(runs[0][1]) > 100
    assert torch.equal(runs[0][0], runs[1][0])
    for n, g in runs[0][1].items():
        assert torch.equal(runs[1][1][n], g), n


@pytest.mark.parametrize("S", [64, 224])
def test_captured_patch_8_teacher_every_replay_equals_the_eager_pass(S):
    from cosa_amd import nn_ops
    from cosa_amd.models import build_model
    from cosa_amd.train_step import synthetic_batch
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    wimg, _, lab, _ = synthetic_batch(2, S, 20, dev, seed=100)
    args = _args(crop_size=S, batch_size=2)
    torch.manual_seed(0)
    net = build_model(args).to(dev).eval()
    net.set_nograd_precision("fp16x3")
    nn_ops.ensure_shadows(net, net.compute_dtype)
    bufs = {}
    run = lambda: seg_helper.multi_scale_camseg(net, wimg, args.pseudo_scales, _active_labels=lab, _seg_scales=True, _buffers=bufs)
    with torch.no_grad():
        for _ in range(2):
            e = run()
        torch.cuda.synchronize()
        ref = [e[0].clone(), e[1].clone()] + [t.clone() for t in e[2]]
        assert all(torch.isfinite(t).all() for t in ref) and ref[2].shape[-1] == S // 8
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            out = run()
        for rep in range(3):
            g.replay()
            torch.cuda.synchronize()
            for name, c, r in zip(("cam", "cam_aux", "seg0", "seg1", "seg2"), [out[0], out[1]] + list(out[2]), ref):
                assert torch.equal(c, r), (rep + 1, name)


def test_full_size_step_448_b16_runs_on_own_kernels():
    """one step of the default configuration (captured fp16x3 teacher, 351 328 teacher token rows, N = 7057 attention at scale 1.5) with every
    ATen fallback an error (nn_ops.reference_op raises in the product)"""
    from cosa_amd.train_step import CoSATrainer, synthetic_batch
    dev = torch.device("cuda", 0)
    args = _args(crop_size=448, batch_size=16)
    tr = CoSATrainer(args, dev, seed=0)
    wimg, simg, lab, box = synthetic_batch(16, 448, 20, dev, seed=1)
    for it in range(2):                                      # (the second step replays the captured teacher)
        logs = tr.step(wimg, simg, lab, box, n_iter=args.warmup_iters + 1 + it)
        torch.cuda.synchronize()
        for k in ("seg_loss", "cam_loss", "reg_loss", "cls_loss"):
            assert np.isfinite(float(logs[k])), (it, k)
    assert tr.graph_error is None
    assert all(torch.isfinite(p).all() for p in tr.student.parameters())


def test_evaluate_with_the_patch_8_network_vs_oracle_composition(oracle_c):
    from cosa_amd import evaluation_engine as ee
    from cosa_amd.models import build_model
    from cosa_amd.utils import seg_helper
    torch.manual_seed(0)
    C, S = 4, 64
    args = _args(crop_size=S, batch_size=1)
    args.num_classes, args.bkg_thre = C + 1, 0.5
    model = build_model(args).cuda().eval()
    rng = np.random.default_rng(3)
    loader = []
    for (H, W) in [(50, 70), (64, 64), (81, 47), (64, 64)]:
        img = torch.from_numpy(rng.standard_normal((1, 3, H, W)).astype(np.float32))
        lab = torch.from_numpy(rng.integers(0, C + 1, (1, H, W)).astype(np.int64))
        lab[0, :3] = 255
        cls = torch.zeros(1, C)
        cls[0, rng.choice(C, 2, replace=False)] = 1
        loader.append(("img", img, lab, cls))
    tab, seg_miou, cam_miou, df, cls_aps = ee.evaluate(model, loader, args, epoch=3, s_or_t='s', get_camiou=True)
    model.batch_invariant_heads = model.decoder.batch_invariant = True
    hist = {k: np.zeros((C + 1, C + 1), np.int64) for k in ("cam", "aux", "vd")}
    with torch.no_grad():
        for _, img, lab, cls in loader:
            x = torch.nn.functional.interpolate(img.cuda(), size=[S, S], mode="bilinear", align_corners=False)
            cam, aux, seg, cf, ca = seg_helper.multi_scale_camsegv3(model, x, ee.EVAL_SCALES, getcls=True)
            assert seg.shape[-1] == S // 8 or seg.shape[-1] == S
            H, W = lab.shape[1:]
            a, _, c = oracle_c.eval_labels(cam[0].cpu().numpy(), seg[0].cpu().numpy(), cls[0].numpy(), H, W, 0.5)
            a2, _, _ = oracle_c.eval_labels(aux[0].cpu().numpy(), seg[0].cpu().numpy(), cls[0].numpy(), H, W, 0.5)
            gt = lab[0].numpy().astype(np.uint8)
            for k, p in (("cam", a), ("aux", a2), ("vd", c)):
                hist[k] += oracle_c.confusion([gt], [p], C + 1)
    model.batch_invariant_heads = model.decoder.batch_invariant = False
    ref = [oracle_c.scores_from_hist(hist[k]) for k in ("cam", "aux", "vd")]
    ref_miou = [np.round(np.array(list(r["iou"].values())) * 100, 2).mean() for r in ref]
    assert abs(cam_miou - ref_miou[0]) < 1e-9 and abs(seg_miou - ref_miou[2]) < 1e-9
    np.testing.assert_allclose(df["mIoU"], ref_miou, atol=1e-9)
