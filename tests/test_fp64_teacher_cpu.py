"""The "fp64" mode's host side: mode strings and refusals, the operand map, the criterion's constants in ONE place of the
product, the numpy restatement of the criterion (tests/conformance_ref.py) on hand-built planes and on a line of the committed accuracy
record, and tools/teacher_check.py --criterion as far as it goes without a device."""
import os
import re

import numpy as np
import pytest
import torch

import conformance_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _net():
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    torch.manual_seed(0)
    return build_model(default_args("VOC12", crop_size=64, batch_size=2))


def test_mode_string_fp64_and_the_refused_suffixes():
    from cosa_amd.train_step import NOGRAD_PRECISIONS
    assert "fp64" in NOGRAD_PRECISIONS
    net = _net().set_nograd_precision("fp16x3")
    before = (net.compute_dtype, net.encoder.precision, net.encoder.x3_dtype)
    for bad in ("fp64-3", "fp64-x2", "fp64x3", "fp64-", "fp64-9m7"):
        with pytest.raises(AssertionError):
            net.set_nograd_precision(bad)
        assert (net.compute_dtype, net.encoder.precision, net.encoder.x3_dtype) == before, bad
    net.check_nograd_precision("fp64")
    assert net.set_nograd_precision("fp64") is net
    assert net.compute_dtype == net.encoder.compute_dtype == torch.float64 and net.encoder.precision == "f64"
    net.refresh_shadows()                                   # no 16-bit copy of anything: a no-op
    assert "_weight_shadows" not in net.__dict__
    net.set_nograd_precision("fp32")
    assert net.compute_dtype == torch.float32 and net.encoder.precision == "f32"


def test_operand_map_of_the_mode_is_f64_all_or_none():
    net = _net().set_nograd_precision("fp64")
    fmap = net.encoder._operand_map()
    depth = len(net.encoder.blocks)
    assert fmap.patch == "f64" and fmap.attn == ("f64",) * depth and fmap.mlp == ("f64",) * depth and fmap.dt16 is None and fmap.hdt is None
    assert all(fmap.of(i, n) == "f64" for i in range(depth) for n in ("qkv", "proj", "fc1", "fc2")) and fmap.uses("f64") and not fmap.uses("f32")
    for other in ("fp32", "fp16x3", "fp16c8-x2", "bf16"):
        assert not net.set_nograd_precision(other).encoder._operand_map().uses("f64"), other


def test_teacher_precision_fp64_is_refused_with_the_reason():
    from cosa_amd import args as cosa_args
    from cosa_amd import main as launcher
    from cosa_amd.train_step import CoSATrainer, default_args
    for flags in (["--teacher_check_iters", "5", "--teacher_check_mode", "fp64"], ["--student_check_iters", "5", "--student_check_mode", "fp64"],
                  ["--teacher_precision", "fp32"]):
        launcher.check_supported(cosa_args.parse(["EXP"] + flags)[0])
    with pytest.raises(ValueError, match="fp32 IS the reference's arithmetic"):
        launcher.check_supported(cosa_args.parse(["EXP", "--teacher_precision", "fp64"])[0])
    with pytest.raises(ValueError, match="check mode, not a training teacher"):
        CoSATrainer(default_args("VOC12", crop_size=64, batch_size=2, teacher_precision="fp64"), torch.device("cpu"))


def test_the_criterions_constants_live_in_one_place_and_equal_the_pre_registered_ones():
    """seg_helper's CAM_BAR / COND_MAX / FP64_FACTOR / AGREE_BAR / MIOU_BAR == the assignments at the top of tests/test_precision_gpu.py (read
    as text: that module needs a device to import its fixtures' targets) == bench.py's"""
    from cosa_amd.utils import seg_helper
    import bench
    src = open(os.path.join(ROOT, "tests", "test_precision_gpu.py")).read()
    for name in ("CAM_BAR", "COND_MAX", "FP64_FACTOR", "AGREE_BAR", "MIOU_BAR"):
        m = re.search(rf"^{name} = ([0-9.e+-]+)$", src, re.M)
        assert m, name
        assert getattr(seg_helper, name) == float(m.group(1)), name
        if hasattr(bench, name):
            assert getattr(seg_helper, name) == getattr(bench, name), name
    assert (seg_helper.CAM_BAR, seg_helper.COND_MAX, seg_helper.FP64_FACTOR) == (1e-3, 50.0, 4.0)
    assert seg_helper.TEACHER_CHECK_BAR == seg_helper.CAM_BAR and tuple(seg_helper.CONFORMANCE_FIGS) == tuple(cref.FIGS)


@pytest.mark.parametrize("S", [7, 24])
def test_conformance_ref_on_the_hand_built_planes(S):
    from cosa_amd.utils import seg_helper
    hb = cref.hand_built(S)
    fig, vd, bad = cref.planes(hb["camA"], hb["cam32"], hb["cam64"], hb["active"], hb["peak"], hb["rawmax"], seg_helper.CAM_BAR, seg_helper.COND_MAX,
                               seg_helper.FP64_FACTOR)
    assert (vd == hb["verdict"]).all(), vd
    assert cref.counts(vd) == {"planes": 7, "literal_ok": 1, "exempt": 2, "failed": 4}
    assert bad[1, 3] == 1 and bad.sum() == 1 and (fig[1, 2] == 0).all()
    col = lambda k: fig[:, :, cref.FIGS.index(k)]
    assert abs(col("cond")[0, 1] - 49.9) < 1e-12 and col("lit")[0, 1] > 1e-3 and col("own")[0, 3] > 1e-3 >= col("own")[0, 2]
    assert col("e_hip")[1, 0] > col("bound")[1, 0] and col("e_hip")[1, 1] <= col("bound")[1, 1]
    assert abs(col("e_hip")[1, 0] / col("bound")[1, 0] - 1) < 1e-2 and abs(col("e_hip")[1, 1] / col("bound")[1, 1] - 1) < 1e-2          # "just"
    # the summary and the record-format line of the product, fed the reference's table
    s = seg_helper.conformance_summary({"cam": {"fig": fig, "verdict": vd}})["cam"]
    assert {k: s[k] for k in ("planes", "literal_ok", "exempt", "failed")} == cref.counts(vd) and len(s["over"]) == 6
    line = seg_helper.conformance_line(s)
    assert line.startswith("planes 7 literal-ok 1 exempt 2 fail 4 [img 0 cls 1: cond 49.9 lit ") and line.count("FAIL]") == 4 and line.count(" ok]") == 2


def test_conformance_ref_reproduces_a_bracket_of_the_committed_accuracy_record():
    """profiles/r06_accuracy_teacher.txt carries `[img 3 cls 13: cond 158.5 lit 1.405e-03 own 8.861e-06 fp64 1.407e-03 bound 1.034e-03 FAIL]` (fp16c8-x2,
    S = 448, b = 16, seed 8, cam): a plane built to those figures gets them back from the restatement, and the verdict.  (The record holds no
    bracket that ends in `ok`: the exempt branch rests on the hand-built planes alone.)"""
    from cosa_amd.utils import seg_helper
    rec = open(os.path.join(ROOT, "profiles", "r06_accuracy_teacher.txt")).read()
    m = re.search(r"\[img 3 cls 13: cond ([0-9.]+) lit ([0-9.e-]+) own ([0-9.e-]+) fp64 ([0-9.e-]+) bound ([0-9.e-]+) FAIL\]", rec)
    assert m, "the committed record no longer carries the bracket this test was written against"
    cond, lit, own, e_hip, bound = (float(v) for v in m.groups())
    assert not re.search(r"bound [0-9.e-]+ ok\]", rec)
    S = 8
    c32 = np.zeros((1, 1, S, S), np.float32)
    c32[0, 0, -1, -1] = 1.0
    A, c64 = c32.copy(), c32.astype(np.float64)
    A[0, 0, 1, 1] = np.float32(lit)                               # d = lit (max |c32| = 1)
    c64[0, 0, 1, 1] = np.float64(np.float32(lit)) - e_hip         # e_hip at that element (e_ref there: |e_hip - lit| ~ 2e-6)
    c64[0, 0, 2, 2] = (bound - seg_helper.CAM_BAR) / seg_helper.FP64_FACTOR          # e_ref = 8.5e-6 at another one
    fig, vd, _ = cref.planes(A, c32, c64, None, np.ones((1, 1)), np.full((1, 1), cond), seg_helper.CAM_BAR, seg_helper.COND_MAX, seg_helper.FP64_FACTOR)
    got = dict(zip(cref.FIGS, fig[0, 0]))
    assert vd[0, 0] == 2
    for k, want in (("cond", cond), ("lit", lit), ("own", own), ("e_hip", e_hip), ("bound", bound)):
        assert abs(got[k] / want - 1) < 2e-3, (k, got[k], want)          # (the record prints 4 digits; cond 158.5 is printed with 1 decimal)


def test_teacher_check_tool_parses_criterion_and_is_unchanged_without_it(capsys):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import teacher_check as tool
    p = tool.get_parser()
    a = p.parse_args(["X", "--synthetic", "--criterion", "--mode", "bf16"])
    assert a.criterion is True and a.mode == "bf16" and a.check_mode == "auto"
    a = p.parse_args(["X", "--synthetic", "--mode", "fp64", "--check_mode", "fp64"])
    assert a.criterion is False and a.mode == "fp64" and a.check_mode == "fp64"
    for argv in (["--synthetic", "--criterion", "--check_mode", "fp16x3"], ["--synthetic", "--criterion", "--use_cammix", "true"]):
        with pytest.raises(SystemExit):
            tool.main(argv)
    assert "--criterion" in capsys.readouterr().err
    # without the flag the tool's output is the summary it always printed: the code path that adds keys is behind `if args.criterion`
    src = open(os.path.join(ROOT, "tools", "teacher_check.py")).read()
    tail = src[src.index("res = dict(seg_helper.teacher_check_summary"):]
    assert re.search(r"\n    if args\.criterion:\n(?:        .*\n|\s*\n)+    print\(json\.dumps\(res\), flush=True\)\n    return res\n", tail)
    assert src.count("print(") == 2 and "if args.criterion:\n            with _C.workspace_scope" in src
