"""The host logic of evaluation_engine's export (DESIGN.md sections 8, 22, 23, 26, 27) without a device: the per-image record plan against
the layout rules restated here, every refusal of the request check, and the score files' local records."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest

ALL_BITS = 127                         # seg | pseudo | pseudo_aux | rawcam | rawcam_aux | pseudo_par | pseudo_aux_par
EXTRA_ORDER = ("seg_crf", "overlay", "camheat", "camheat_aux", "panel")


def up16(n):
    return (n + 15) // 16 * 16


@pytest.mark.parametrize("C", [4, 20])
@pytest.mark.parametrize("k_live", [0, 1, 3])
@pytest.mark.parametrize("H,W", [(3, 5), (50, 70), (375, 500)])
def test_record_plan_follows_the_layout_rules(H, W, k_live, C):
    from cosa_amd import evaluation_engine as ee
    from cosa_amd.utils import seg_helper
    core, core_end = seg_helper.export_record_layout(C, H, W, k_live, ALL_BITS)
    for getcrf, overlay, camheat, camheat_aux, panel_cols in itertools.product((False, True), (False, True), (False, True), (False, True), (0, 3, 4)):
        pictures = tuple(p for p, on in (("camheat", camheat), ("camheat_aux", camheat_aux), ("panel", panel_cols)) if on)
        plan = ee._RecordPlan(C, H, W, k_live, ALL_BITS, getcrf, overlay, pictures, panel_cols or 3)
        assert {p: plan.offsets[p] for p in core} == core
        sizes = {"seg_crf": H * W, "overlay": 3 * H * W, "camheat": 3 * k_live * H * W, "camheat_aux": 3 * k_live * H * W,
                 "panel": 3 * k_live * H * panel_cols * W}
        asked = {"seg_crf": getcrf, "overlay": overlay, "camheat": camheat and k_live, "camheat_aux": camheat_aux and k_live,
                 "panel": panel_cols and k_live}
        end = core_end
        for p in EXTRA_ORDER:                                          # in this order, each from the 16-byte boundary behind the one before
            if not asked[p]:
                assert p not in plan.offsets                           # k_live == 0: no picture slot
                continue
            assert plan.offsets[p] == up16(end) and plan.offsets[p] >= end          # no overlap with anything in front
            end = plan.offsets[p] + sizes[p]
        assert sorted(plan.offsets) == sorted(list(core) + [p for p in EXTRA_ORDER if asked[p]])
        assert plan.copy_bytes == (up16(end) if end != core_end else core_end) and plan.reserve_bytes >= plan.copy_bytes
        heat = {p: plan.offsets[p] for p in ("camheat", "camheat_aux") if asked[p]}
        if asked["panel"] and not asked["camheat"]:                    # the panel's first column: a scratch plane behind what is copied
            heat["camheat"] = plan.copy_bytes
            assert plan.copy_bytes + 3 * k_live * H * W <= plan.reserve_bytes
        assert plan.heat_at == heat
        rec = np.zeros(plan.reserve_bytes, np.uint8)
        for p in plan.offsets:                                         # every view lies inside the copied bytes and has its product's shape
            v = plan.view(rec, p)
            lo = v.__array_interface__["data"][0] - rec.__array_interface__["data"][0] if v.size else plan.offsets[p]
            assert lo == plan.offsets[p] and lo + v.nbytes <= plan.copy_bytes
        if asked["panel"]:
            assert plan.view(rec, "panel").shape == (k_live, H, panel_cols * W, 3) and plan.view(rec, "rawcam").shape == (k_live, H, W)
            assert plan.view(rec, "rawcam").dtype == np.float32 and plan.view(rec, "rawcam_idx").dtype == np.int32


def _args(**kw):
    return SimpleNamespace(**dict(dict(num_classes=5, high_thre=0.7, low_thre=0.25), **kw))


def _check(what=("seg",), classes=None, cls_thre=0.5, cls_min=1, overlay_alpha=0.5, scores=False, boundary=False, getcrf=False, writers=4,
           args=None):
    from cosa_amd import evaluation_engine as ee
    return ee.check_export_request(what, classes, cls_thre, cls_min, overlay_alpha, scores, boundary, getcrf, writers, args or _args())


@pytest.mark.parametrize("kw,exc,match", [
    (dict(what=("seg", "heatmap")), ValueError, "export products"),
    (dict(what=("seg", "overlay", "overlay")), ValueError, "named twice"),
    (dict(what=("panel", "seg", "panel")), ValueError, "named twice"),
    (dict(classes="guessed"), ValueError, "classes must be"),
    (dict(what=("seg", "pseudo"), classes="none"), ValueError, "classes='none'"),
    (dict(what=("seg", "camheat"), classes="none"), ValueError, "classes='none'"),                  # tests/test_camheat_gpu.py
    (dict(classes="predicted", cls_min=5), ValueError, "cls_min"),
    (dict(classes="predicted", cls_min=-1), ValueError, "cls_min"),
    (dict(classes="predicted", cls_thre=1.0), ValueError, "cls_thre"),
    (dict(classes="predicted", cls_thre=0.0), ValueError, "cls_thre"),
    (dict(what=("seg", "overlay"), overlay_alpha=1.5), ValueError, "alpha"),
    (dict(what=("seg", "overlay"), overlay_alpha=-0.1), ValueError, "alpha"),
    (dict(writers=9), ValueError, "writers"),
    (dict(args=_args(usepar=True)), NotImplementedError, "PAR"),                                    # tests/test_export_gpu.py
    (dict(what=("pseudo_par",), args=_args(usepar=True)), NotImplementedError, "pseudo_par"),      # tests/test_export_par_gpu.py
    (dict(what=("pseudo_par",), args=_args(par_downscale=4)), ValueError, "par_downscale"),        # tests/test_export_par_gpu.py
    (dict(what=("rawcam",), scores=True), ValueError, "scores=True needs a label-map product"),
    (dict(what=("rawcam",), boundary=True), ValueError, "boundary=True needs a label-map product"),
])
def test_request_check_refuses(kw, exc, match):
    with pytest.raises(exc, match=match):
        _check(**kw)


def test_request_check_reads_the_request():
    from cosa_amd.utils.seg_helper import EXPORT_BITS as B
    r = _check(what=("pseudo",), args=_args(par_downscale=4))                    # the other products do not read par_downscale
    assert (r.mask, r.par_mask, r.products, r.pictures, r.overlay, r.predicted, r.scored) == (B["pseudo"], 0, ("pseudo",), (), False, False, ["pseudo"])
    r = _check(what=("overlay",), classes="none", getcrf=True, scores=True, writers=2)
    assert (r.mask, r.products, r.overlay, r.writers, r.scored) == (B["seg"], ("overlay", "seg_crf"), True, 2, ["seg_crf"])
    # a picture's source slots are computed even where no file of them is asked for
    assert _check(what=("camheat",)).mask == B["rawcam"] and _check(what=("camheat_aux",)).mask == B["rawcam_aux"]
    r = _check(what=("panel", "camheat_aux", "pseudo_aux_par"), classes="predicted", cls_min=0, args=_args(par_downscale=0))
    assert r.mask == B["seg"] | B["rawcam"] | B["rawcam_aux"] | B["pseudo_aux_par"] and r.pictures == ("camheat_aux", "panel")
    assert (r.par_mask, r.par_downscale, r.predicted, r.scored) == (B["pseudo_aux_par"], 0, True, ["pseudo_aux_par"])
    with pytest.raises(ValueError, match="classes='none'"):                       # picture products need the class row
        _check(what=("panel",), classes="none")


def test_eval_pass_restores_the_model_on_every_path():
    """evaluate() and export_predictions() run inside it: an exception in either leaves mode and flags as they were"""
    import torch
    from cosa_amd import evaluation_engine as ee

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.decoder = torch.nn.Linear(2, 2)
            self.batch_invariant_heads = self.decoder.batch_invariant = False

    def state(m):
        return m.training, m.batch_invariant_heads, m.decoder.batch_invariant, torch.is_grad_enabled()

    for net, training in ((Net().train(), True), (Net().eval(), False)):
        with ee._eval_pass(net, use_graph=False) as camseg:
            assert isinstance(camseg, ee._GraphedCamSeg) and not camseg.enabled and camseg.scales == ee.EVAL_SCALES
            assert state(net) == (False, True, True, False) and not net.decoder.training
        assert state(net) == (training, False, False, True)
        with pytest.raises(KeyError):
            with ee._eval_pass(net, use_graph=True):
                raise KeyError("inside the pass")
        assert state(net) == (training, False, False, True) and net.decoder.training is training
    plain = torch.nn.Linear(2, 2).train()                                      # a model without the flags: only the mode
    with ee._eval_pass(plain, use_graph=False):
        assert not plain.training and not hasattr(plain, "batch_invariant_heads")
    assert plain.training


def test_local_score_records():
    import torch
    from cosa_amd.utils import evaluation
    rows = np.arange(3 * 6, dtype=np.int64).reshape(3, 6)
    meta = [("a", torch.tensor([0.0, 1.0, 0.0, 1.0]), 5, 7), ("b", np.zeros(4, np.float32), 3, 3), ("c", torch.tensor([[1, 1, 1, 1]]), 9, 2)]
    local = evaluation.local_score_records(meta, rows, 1, 3)
    assert [pos for pos, _ in local] == [1, 4, 7]
    assert [r["present"] for _, r in local] == [[2, 4], [], [1, 2, 3, 4]]
    assert [(r["name"], r["h"], r["w"]) for _, r in local] == [("a", 5, 7), ("b", 3, 3), ("c", 9, 2)]
    assert all(np.array_equal(r["row"], rows[k]) and "d" not in r for k, (_, r) in enumerate(local))
    band = evaluation.local_score_records(meta, rows, 0, 1, widths={0: 2, 1: 1, 2: 4})
    assert [pos for pos, _ in band] == [0, 1, 2] and [r["d"] for _, r in band] == [2, 1, 4]
