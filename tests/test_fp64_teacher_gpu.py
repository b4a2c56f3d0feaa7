"""The "fp64" mode of the no-grad passes end to end: the network against the float64 oracle on the reference's golden,
the multi-scale products with their scale figures on both patch sizes, batch invariance through the whole network, the criterion's per-plane
reduction against its numpy restatement (tests/conformance_ref.py) and end to end, and fp64 as the check mode of --teacher_check_iters /
--student_check_iters.  The rule everywhere: distance of the float64 path from the float64 oracle <= 64 x 2^-29 x the distance the fp32 path
measures from the same oracle in the same test.  Measured figures go on record in profiles/fp64_teacher_parity.txt."""
import numpy as np
import pytest
import torch

import conformance_ref as cref
from test_f64_kernels_gpu import RULE, record

pytestmark = pytest.mark.gpu

OUTPUTS = ("cls", "cls_aux", "x4", "seg", "cam", "cam_aux")
LOSSES = ("cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")
SCALES = [1.0, 0.5, 1.5]
B8 = "dino_base_patch8_224"


def _bits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def test_fp64_network_vs_float64_oracle_on_the_reference_golden(golden):
    """tests/golden/vit_base_d2.npz: the six outputs of mode "fp64" (float64 tensors) against OracleViT(...).double(), each within 64 x 2^-29 x the
    distance mode "fp32" measures from the same oracle here"""
    from test_network_gpu import _vit_b_width_model
    from oracle import torch_oracle as to
    from oracle.gen_golden import recipe_state, VIT_BASE_CFG as cfg
    net, g = _vit_b_width_model(golden)
    x = torch.from_numpy(g["x"])
    out = {}
    with torch.no_grad():
        for mode in ("fp32", "fp64"):
            net.set_nograd_precision(mode)
            assert net.encoder.use_fused(x.cuda()), "the fused HIP path must be the one that runs"
            out[mode] = [o.cpu() for o in net(x.cuda())]
    assert all(o.dtype == torch.float64 for o in out["fp64"]) and "_weight_shadows" not in net.__dict__
    shapes = {str(k): tuple(int(d) for d in str(s_).split(",")) for k, s_ in zip(g["shape_keys"], g["shape_dims"])}
    sd, _ = recipe_state(shapes)
    m = to.OracleViT(num_classes=cfg["num_classes"], embed_dim=cfg["embed_dim"], depth=cfg["depth"], num_heads=cfg["num_heads"],
                     aux_layer=cfg["aux_layer"])
    m.load_named(sd)
    with torch.no_grad():
        ref64 = m.double()(x.double())
    fails = []
    for name, o64, o32, r in zip(OUTPUTS, out["fp64"], out["fp32"], ref64):
        assert o64.shape == r.shape == g[name].shape, name
        d64, d32 = float((o64 - r).abs().max()), float((o32.double() - r).abs().max())
        record(f"golden vit_base_d2 {name}", f"d64={d64:.3e} d32={d32:.3e} ratio_to_rule={d64 / (RULE * d32):.4f}")
        if not (torch.isfinite(o64).all() and d64 <= RULE * d32):
            fails.append((name, d64, d32))
    assert not fails, fails


def test_fp64_image_alone_has_the_bits_it_has_in_a_batch_of_three():
    """the whole network at S = 32, all six outputs, bit for bit: every GEMM row, attention slice and conv image is computed alone"""
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    torch.manual_seed(11)
    net = build_model(default_args("VOC12", crop_size=32, batch_size=3)).cuda().eval().set_nograd_precision("fp64")
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(12)).cuda()
    with torch.no_grad():
        three = [o.clone() for o in net(x)]
        one = net(x[1:2].contiguous())
    for name, a, b in zip(OUTPUTS, three, one):
        assert a.dtype == torch.float64 and torch.isfinite(a).all() and float(a.abs().max()) > 0, name
        assert torch.equal(_bits(a[1:2]), _bits(b)), (name, float((a[1:2] - b).abs().max()))


def test_fp64_pass_walked_in_image_chunks_moves_no_bit():
    """VITNetwork.forward_multi walks a float64 batch in chunks of F64_CHUNK images (memory): three images in chunks of 2 + 1 give the bits of
    the pass in one go, for the CAMs, the seg sum and the scale figures"""
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    from cosa_amd.utils import seg_helper
    torch.manual_seed(13)
    net = build_model(default_args("VOC12", crop_size=32, batch_size=3)).cuda().eval().set_nograd_precision("fp64")
    x = torch.randn(3, 3, 32, 32, generator=torch.Generator().manual_seed(14)).cuda()
    flat = lambda out: list(out[:3]) + list(out[3]) + list(out[4])
    with torch.no_grad():
        assert net.F64_CHUNK >= 3
        whole = flat(seg_helper.multi_scale_camseg(net, x, SCALES, _return_scale=True))
        net.F64_CHUNK = 2
        parts = flat(seg_helper.multi_scale_camseg(net, x, SCALES, _return_scale=True))
    for i, (a, b) in enumerate(zip(whole, parts)):
        assert a.dtype == torch.float64 and torch.isfinite(a).all() and torch.equal(_bits(a), _bits(b)), i


_DRAW = {}


def _draw(backbone, oracle_c=None):
    """S = 64, b = 2, scales [1.0, 0.5, 1.5], fixed seeds, one backbone: the oracle's multi-scale products in float64 and fp32 with their scale
    figures, and the HIP network's in the modes fp32 and fp64 (two networks on the same weights) -- computed once, shared, left unchanged"""
    if backbone not in _DRAW:
        from oracle import torch_oracle as to
        from cosa_amd.models import build_model
        from cosa_amd.train_step import default_args, synthetic_batch
        from cosa_amd.utils import seg_helper
        S = 64
        args = default_args("VOC12", crop_size=S, batch_size=2, backbone=backbone)
        torch.manual_seed(7)
        net = build_model(args).eval()
        sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
        wimg, _, lab, box = synthetic_batch(2, S, 20, torch.device("cpu"), seed=9)
        m = to.OracleViT(num_classes=21, aux_layer=args.aux_layer, patch=net.encoder.patch_size)
        m.load_named(sd)
        with torch.no_grad():
            o32 = to.multi_scale_camseg(m, wimg, SCALES, return_scale=True)
            o64 = to.multi_scale_camseg(m.double(), wimg.double(), SCALES, return_scale=True)
        nets = {}
        for mode in ("fp32", "fp64"):
            n = build_model(args).eval()
            n.load_state_dict(sd)
            nets[mode] = n.cuda().set_nograd_precision(mode)
        with torch.no_grad():
            h32 = seg_helper.multi_scale_camseg(nets["fp32"], wimg.cuda(), SCALES)
            h64 = seg_helper.multi_scale_camseg(nets["fp64"], wimg.cuda(), SCALES, _return_scale=True)
        _DRAW[backbone] = dict(args=args, nets=nets, sd=sd, wimg=wimg, lab=lab, box=box, o32=o32, o64=o64, h32=h32, h64=h64)
    return _DRAW[backbone]


@pytest.mark.parametrize("backbone", ["vit_base_patch16_224", B8], ids=["p16", "p8"])
def test_fp64_multi_scale_cams_and_scale_figures_vs_the_float64_oracle(backbone):
    """normalised cam and cam_aux (every plane), seg, peak and rawmax of both CAM sets against to.multi_scale_camseg(m.double(), ...,
    return_scale=True): each within 64 x 2^-29 x its fp32 counterpart's distance from the same oracle -- the HIP network in mode fp32 for the
    maps; for peak / rawmax, which no fp32 HIP path returns, the oracle run in fp32.  The label maps of cam2mask on the fp32-rounded float64
    CAMs are those of mode fp32: agreement 1.0."""
    from cosa_amd.utils import seg_helper
    d = _draw(backbone)
    tag = "p8" if backbone == B8 else "p16"
    cam, aux, seg, (pk, rw), (pk_a, rw_a) = d["h64"]
    assert all(t.dtype == torch.float64 for t in (cam, aux, seg, pk, rw, pk_a, rw_a))
    o64, o32, h32 = d["o64"], d["o32"], d["h32"]
    pairs = [("cam", cam, h32[0], o64[0]), ("cam_aux", aux, h32[1], o64[1]), ("seg", seg, h32[2], o64[2]),
             ("peak", pk, o32[3][0], o64[3][0]), ("rawmax", rw, o32[3][1], o64[3][1]),
             ("peak_aux", pk_a, o32[4][0], o64[4][0]), ("rawmax_aux", rw_a, o32[4][1], o64[4][1])]
    fails = []
    for name, got, yard, ref in pairs:
        d64, d32 = float((got.cpu() - ref).abs().max()), float((yard.cpu().double() - ref).abs().max())
        record(f"multi_scale {tag} S=64 b=2 {name}", f"d64={d64:.3e} d32={d32:.3e} ratio_to_rule={d64 / max(RULE * d32, 1e-300):.4f}")
        if not (torch.isfinite(got).all() and d64 <= RULE * d32):
            fails.append((name, d64, d32))
    d.setdefault("d32", {"cam": float((h32[0].cpu().double() - o64[0]).abs().max()), "cam_aux": float((h32[1].cpu().double() - o64[1]).abs().max())})
    wimg, lab, box = d["wimg"].cuda(), d["lab"].cuda(), d["box"]
    with torch.no_grad():
        for name, c64, c32 in (("cam", cam, h32[0]), ("cam_aux", aux, h32[1])):
            m64, m32 = (seg_helper.cam2mask(wimg, box, c.float() * lab[:, :, None, None], lab, 0.7, 0.25).cpu().numpy() for c in (c64, c32))
            agree = float(np.mean(m64 == m32))
            record(f"multi_scale {tag} S=64 b=2 {name} labels", f"agreement_with_fp32_mode={agree:.6f}")
            if agree != 1.0:
                fails.append((name, "label agreement", agree))
    assert not fails, fails


# ---- the criterion per plane ---------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """distance in units of the last place of float64 (same sign, finite)"""
    return np.abs(np.asarray(a, np.float64).view(np.int64) - np.asarray(b, np.float64).view(np.int64))


@pytest.mark.parametrize("S", [7, 24])
def test_conformance_planes_equals_the_numpy_restatement_on_hand_built_planes(S):
    """every branch (ok; over at cond 49.9; exempt; own over; e_hip just over / just under its bound; inactive; a NaN element): verdicts, counts
    and non-finite counts equal the reference exactly, every figure to 1 ulp of float64; two runs give identical bytes"""
    from cosa_amd.utils import seg_helper
    hb = cref.hand_built(S)
    dev = torch.device("cuda", 0)
    t = lambda k, dt: torch.from_numpy(np.ascontiguousarray(hb[k])).to(dt).to(dev)
    run = lambda: seg_helper.conformance_planes(t("camA", torch.float32), t("cam32", torch.float32), t("cam64", torch.float64), t("active", torch.float32),
                                                t("peak", torch.float64), t("rawmax", torch.float64))
    tab, again = run(), run()
    for k in ("fig", "verdict", "nonfinite"):
        assert torch.equal(tab[k], again[k]) and (k != "fig" or torch.equal(_bits(tab[k]), _bits(again[k]))), k
    fig, vd, bad = cref.planes(hb["camA"], hb["cam32"], hb["cam64"], hb["active"], hb["peak"], hb["rawmax"], seg_helper.CAM_BAR, seg_helper.COND_MAX,
                               seg_helper.FP64_FACTOR)
    assert (vd == hb["verdict"]).all()
    assert (tab["verdict"].cpu().numpy() == vd).all() and (tab["nonfinite"].cpu().numpy() == bad).all()
    assert int(_ulps(tab["fig"].cpu().numpy(), fig).max()) <= 1
    s = seg_helper.conformance_summary({"cam": tab})["cam"]
    assert {k: s[k] for k in ("planes", "literal_ok", "exempt", "failed")} == cref.counts(vd)
    # active = None: every plane counts (the inactive one is then scored like any other)
    all_on = seg_helper.conformance_planes(t("camA", torch.float32), t("cam32", torch.float32), t("cam64", torch.float64), None,
                                           t("peak", torch.float64), t("rawmax", torch.float64))
    assert int((all_on["verdict"] >= 0).sum()) == 8 and int(all_on["verdict"][1, 2]) == 2


SEED_BF16 = 9          # synthetic_batch seed of the S = 64 draw: bf16 as mode A leaves planes over the literal bar there (asserted below on both sides)


def test_criterion_end_to_end_bf16_has_planes_over_the_bar_and_fp32_has_none():
    """S = 64, b = 2, the draw's weights and images (seed 9): with bf16 as mode A at least one active plane is over the literal bar -- by the
    kernel AND by the numpy restatement on the same tensors; with fp32 as mode A none is, and e_hip = e_ref on every plane (A IS the fp32
    pass)"""
    from cosa_amd.models import build_model
    from cosa_amd.utils import seg_helper
    d = _draw("vit_base_patch16_224")
    wimg, lab = d["wimg"].cuda(), d["lab"].cuda()
    n16 = build_model(d["args"]).eval()
    n16.load_state_dict(d["sd"])
    n16 = n16.cuda().set_nograd_precision("bf16")
    with torch.no_grad():
        c16 = seg_helper.multi_scale_camseg(n16, wimg, SCALES, _active_labels=lab)[:2]
        c32 = seg_helper.multi_scale_camseg(d["nets"]["fp32"], wimg, SCALES, _active_labels=lab)[:2]
        c32b = [c.clone() for c in seg_helper.multi_scale_camseg(d["nets"]["fp32"], wimg, SCALES, _active_labels=lab)[:2]]
        c64, a64, _, sc, sa = seg_helper.multi_scale_camseg(d["nets"]["fp64"], wimg, SCALES, _active_labels=lab, _return_scale=True)
    assert int(lab.sum()) > 0
    over_any = 0
    for name, A, F32, F32b, F64, (pk, rw) in (("cam", c16[0], c32[0], c32b[0], c64, sc), ("cam_aux", c16[1], c32[1], c32b[1], a64, sa)):
        tab = seg_helper.conformance_planes(A, F32, F64, lab, pk, rw)
        s = seg_helper.conformance_summary({name: tab})[name]
        fig, vd, _ = cref.planes(A.cpu().numpy(), F32.cpu().numpy(), F64.cpu().numpy(), lab.cpu().numpy(), pk.cpu().numpy(), rw.cpu().numpy(),
                                 seg_helper.CAM_BAR, seg_helper.COND_MAX, seg_helper.FP64_FACTOR)
        assert (tab["verdict"].cpu().numpy() == vd).all() and int(_ulps(tab["fig"].cpu().numpy(), fig).max()) <= 1
        assert s["planes"] == int(lab.sum()) and len(s["over"]) == int((vd > 0).sum())
        record(f"criterion S=64 b=2 seed={SEED_BF16} bf16 {name}", seg_helper.conformance_line(s))
        over_any += len(s["over"])
        same = seg_helper.conformance_planes(F32b, F32, F64, lab, pk, rw)
        ss = seg_helper.conformance_summary({name: same})[name]
        f = same["fig"].cpu().numpy()
        assert ss["literal_ok"] == ss["planes"] and not ss["over"] and (f[:, :, cref.FIGS.index("d")] == 0).all()
        assert (f[:, :, cref.FIGS.index("e_hip")] == f[:, :, cref.FIGS.index("e_ref")]).all()
    assert over_any >= 1


# ---- fp64 as the check mode inside a run ---------------------------------------------------------------------------------------------------
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


def _state(tr):
    """weights of student and EMA teacher, and the optimizer's moments"""
    st = {f"{tag}.{n}": p.detach().clone() for tag, net in (("ON", tr.student), ("AN", tr.model_AN)) for n, p in net.named_parameters()}
    for gi, grp in enumerate(tr.optimizer.param_groups):
        for pi, p in enumerate(grp["params"]):
            for k, v in tr.optimizer.state.get(p, {}).items():
                if torch.is_tensor(v):
                    st[f"opt.{gi}.{pi}.{k}"] = v.detach().clone()
    return st


_PLAIN = {}


def _plain():
    if not _PLAIN:
        tr = _trainer()
        _PLAIN.update(losses=_run(tr), state=_state(tr))
        del tr
    return _PLAIN


def _same_run(tr, losses):
    ref = _plain()
    assert torch.equal(ref["losses"].view(torch.int32), losses.view(torch.int32))
    st = _state(tr)
    assert st.keys() == ref["state"].keys() and any(k.startswith("opt.") for k in st)
    for k in st:
        assert torch.equal(st[k], ref["state"][k]) and st[k].dtype == ref["state"][k].dtype, k


def test_fp64_teacher_check_changes_no_bit_of_the_run_and_counts_its_checks():
    """--teacher_check_iters 1 --teacher_check_mode fp64 on the default teacher: weights, moments, EMA teacher and losses after three steps are
    those of the run without the flags, bit for bit; 3 checks, planes > 0, nothing non-finite"""
    from cosa_amd.utils import seg_helper
    tr = _trainer(teacher_check_iters=1, teacher_check_mode="fp64")
    assert tr.args.teacher_precision == "fp16x3" and tr.model_CK.encoder.precision == "f64" and tr._checks["teacher_check"].shadows is None
    _same_run(tr, _run(tr))
    s = tr.teacher_check()
    assert s["checks"] == 3
    for name in seg_helper.TEACHER_CHECK_SETS:
        assert s[name]["planes"] > 0 and s[name]["nonfinite_a"] == s[name]["nonfinite_b"] == 0, (name, s[name])
        record(f"teacher_check S=64 b=2 fp16x3 vs fp64 {name}", f"worst={s[name]['worst']:.3e} over={s[name]['over']}/{s[name]['planes']}")
    assert "_weight_shadows" not in tr.model_CK.__dict__


def test_fp64_student_check_changes_no_bit_of_the_run_and_counts_its_checks():
    from cosa_amd.utils import seg_helper
    tr = _trainer(student_check_iters=1, student_check_mode="fp64")
    assert tr.model_SK.encoder.precision == "f64" and tr._checks["student_check"].shadows is None
    _same_run(tr, _run(tr))
    s = tr.student_check()
    assert s["checks"] == 3
    for name in seg_helper.STUDENT_CHECK_TENSORS:
        assert s[name]["n"] > 0 and s[name]["nonfinite_a"] == s[name]["nonfinite_b"] == 0, (name, s[name])
        record(f"student_check S=64 b=2 bf16 vs fp64 {name}", f"rel_l2={s[name]['rel_l2']:.3e}")


def test_an_fp32_teacher_checked_in_fp64_sits_within_four_times_the_measured_fp32_distance():
    """--teacher_precision fp32 --teacher_check_mode fp64: the literal figure (max |fp32 - fp64| per active plane of the normalised CAMs) <= 4 x
    the distance the multi-scale test measures between the fp32 mode and the float64 oracle on the same geometry"""
    d = _draw("vit_base_patch16_224")
    if "d32" not in d:
        d["d32"] = {k: float((d["h32"][i].cpu().double() - d["o64"][i]).abs().max()) for i, k in enumerate(("cam", "cam_aux"))}
    tr = _trainer(teacher_precision="fp32", teacher_check_iters=1, teacher_check_mode="fp64")
    _run(tr)
    s = tr.teacher_check()
    assert s["checks"] == 3
    for name, key in (("cam", "cam"), ("aux", "cam_aux")):
        worst, yard = float(s[name]["worst"]), d["d32"][key]
        record(f"teacher_check S=64 b=2 fp32 vs fp64 {name}", f"worst={worst:.3e} fp32_vs_f64_oracle={yard:.3e} ratio={worst / yard:.3f}")
        assert s[name]["planes"] > 0 and s[name]["over"] == 0 and worst <= 4 * yard, (name, worst, yard)
