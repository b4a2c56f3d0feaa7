"""The --act_stats_iters monitor without a GPU: the flag, the counters' layout, the summary of a hand-filled table through
the launcher's interval read and the jsonl writer (a fixed-point word above 2^53 included), the monitor table's three tuples, and the
--qk_gain knob of the two tools."""
import importlib.util
import json
import os
from types import SimpleNamespace

import pytest
import torch

import act_stats_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_parses_and_a_negative_interval_is_refused():
    from cosa_amd import args as cosa_args
    from cosa_amd import main as launcher
    from cosa_amd.train_step import check_iters, default_args
    a, changed = cosa_args.parse(["EXP"])
    assert a.act_stats_iters == 0 and "act_stats_iters" not in changed and default_args().act_stats_iters == 0
    a, changed = cosa_args.parse(["EXP", "--act_stats_iters", "50"])
    assert a.act_stats_iters == 50 and changed["act_stats_iters"] == 50 and check_iters(a, "act_stats") == 50
    launcher.check_supported(a)
    a, _ = cosa_args.parse(["EXP", "--act_stats_iters", "-1"])
    with pytest.raises(ValueError, match="act_stats_iters"):
        launcher.check_supported(a)
    with pytest.raises(ValueError, match="act_stats_iters"):
        check_iters(SimpleNamespace(act_stats_iters=-3), "act_stats")


def test_layout_offsets_are_as_documented():
    from cosa_amd.utils import seg_helper
    off, n = seg_helper.act_stats_layout(12, 12)
    W = 6 * 6 + 12 * 7
    assert off["width"] == W == 120 and n == 12 * W + 1 and off["checks"] == 12 * W
    assert [off[f"0.{s}.finite"] for s in ("q", "k", "v", "o", "h", "x")] == [0, 6, 12, 18, 24, 30]
    assert [off[f"0.h.{f}"] for f in ("finite", "absmax", "over", "near", "tiny", "nonfinite")] == list(range(24, 30))
    assert [off[f"0.head0.{f}"] for f in ("rows", "ent_fix", "top1_fix", "peaked", "smax", "sharp", "nonfinite_rows")] == list(range(36, 43))
    assert off["3.head5.smax"] == 3 * W + 36 + 7 * 5 + 4 and off["11.head11.nonfinite_rows"] == 12 * W - 1
    slots = [v for k, v in off.items() if k != "width"]
    assert sorted(slots) == list(range(n))                                            # every element has exactly one name
    assert seg_helper.ACT_STATS_SITES == ref.SITES and seg_helper._AS_RANGE_FIELDS == ref.RANGE_FIELDS and seg_helper._AS_HEAD_FIELDS == ref.HEAD_FIELDS
    t = seg_helper.new_act_stats(2, 3, "cpu")
    view = seg_helper.act_stats_table(t, 2, 3)
    assert t.shape == (2 * 57 + 1,) and t.dtype == torch.int64 and view.shape == (2, 57) and view.data_ptr() == t.data_ptr()
    with pytest.raises(ValueError):
        seg_helper.act_stats_layout(0, 12)
    with pytest.raises(ValueError):
        seg_helper.act_stats_summary([0] * 5, 2, 3)


ROWS_PER_HEAD = 1 << 22
LINE = " act: headroom 9.3b (h L1), max|s| 41.2 (L1 h1), ent 0.62 (min 0.31 L1 h1), over 0"


def _hand_table():
    """depth 2, two heads: h of block 1 peaks at 104 (9.3 bits under 65504), head (1, 1) holds the largest logit, 41.2, and the lowest mean
    entropy, 0.31; the other three heads sit at 0.72333.. so that the mean over all rows is 0.62; three passes"""
    from cosa_amd.utils import seg_helper
    off, n = seg_helper.act_stats_layout(2, 2)
    c = [0] * n
    c[off["checks"]] = 3
    for i in range(2):
        for s, amax in zip(ref.SITES, (3.0, 5.0, 2.0, 1.5, 20.0 + 84.0 * i, 400000.0)):
            c[off[f"{i}.{s}.finite"]] = 1000
            c[off[f"{i}.{s}.absmax"]] = ref.f32_bits(amax)
        c[off[f"{i}.x.over"]] = 7                                                      # the fp32 stream is no fp16-stored site: not in `over`
        c[off[f"{i}.x.near"]] = 9
        c[off[f"{i}.q.tiny"]] = 11
        for h in range(2):
            low = (i, h) == (1, 1)
            ent = 0.31 if low else (4 * 0.62 - 0.31) / 3
            c[off[f"{i}.head{h}.rows"]] = ROWS_PER_HEAD
            c[off[f"{i}.head{h}.ent_fix"]] = ROWS_PER_HEAD * round(ent * 2 ** 32) + (0 if low else 1)          # (odd, above 2^53)
            c[off[f"{i}.head{h}.top1_fix"]] = ROWS_PER_HEAD * round(0.25 * 2 ** 32)
            c[off[f"{i}.head{h}.peaked"]] = ROWS_PER_HEAD // 8
            c[off[f"{i}.head{h}.smax"]] = ref.f32_bits(41.2 if low else 7.5 + h)
            c[off[f"{i}.head{h}.sharp"]] = ref.f32_bits(0.75 if low else 0.5)
    return c, off


def test_summary_log_line_and_jsonl_record_through_the_interval_read(tmp_path):
    from cosa_amd import main as launcher
    from cosa_amd import monitors
    from cosa_amd.utils import seg_helper
    c, off = _hand_table()
    assert max(c) > 2 ** 53 and c[off["0.head0.ent_fix"]] % 2 == 1
    m = monitors.BY_NAME["act_stats"]
    t = torch.tensor(c, dtype=torch.int64)
    acc = torch.arange(8, dtype=torch.float64) * 20
    vals, host = launcher.read_interval(acc, 20, [(m, t)])
    assert vals == [float(i) for i in range(8)] and host["act_stats"] == c              # exact: the words travel as 32-bit halves
    assert int(t.abs().sum()) == 0                                                      # an interval's: zeroed after the read
    trainer, targs = SimpleNamespace(act_stats_shape=(2, 2)), SimpleNamespace()
    s = m.summary(trainer, targs, host["act_stats"])
    assert s == seg_helper.act_stats_summary(c, 2, 2) and m.gate(s) and not m.gate(dict(s, checks=0))
    assert m.line(s, targs) == LINE
    assert s["checks"] == 3 and s["headroom_at"] == ["h", 1] and s["smax_at"] == [1, 1] and s["ent_min_at"] == [1, 1] and s["over"] == 0
    assert s["nonfinite"] == 0 and abs(s["ent_mean"] - 0.62) < 1e-9 and abs(s["ent_min"] - 0.31) < 1e-9
    assert s["layers"][0]["sites"]["x"] == dict(absmax=400000.0, over=7, near=9, tiny=0, nonfinite=0, finite=1000)
    assert s["layers"][1]["sites"]["q"]["tiny"] == 11 and s["layers"][1]["sites"]["h"]["absmax"] == 104.0
    h = s["layers"][1]["heads"][1]
    assert h["rows"] == ROWS_PER_HEAD and h["peaked"] == 0.125 and abs(h["top1"] - 0.25) < 1e-9 and h["sharpest"] == 0.25
    assert h["smax"] == ref.bits_f32(ref.f32_bits(41.2))
    # the restatement of the globals, from the same words
    layers = [({n: [c[off[f"{i}.{n}.{f}"]] for f in ref.RANGE_FIELDS] for n in ref.SITES},
               [ref.head_words_decoded([c[off[f"{i}.head{k}.{f}"]] for f in ref.HEAD_FIELDS]) for k in range(2)]) for i in range(2)]
    g = ref.summary_globals(layers)
    assert all(s[k] == g[k] for k in ("headroom_at", "smax_at", "ent_min_at", "over", "nonfinite", "smax", "nonfinite_rows"))
    assert all(abs(s[k] - g[k]) < 1e-12 for k in ("headroom_bits", "ent_mean", "ent_min"))
    monitors.append_monitor(tmp_path, m, s, 20, targs)
    monitors.append_monitor(tmp_path, m, s, 40, targs)
    recs = [json.loads(x) for x in (tmp_path / "act_stats.jsonl").read_text().splitlines()]
    assert [r["iters"] for r in recs] == [20, 40] and recs[0]["mode"] == "fp32" and recs[0]["checks"] == 3
    assert recs[0]["layers"][1]["heads"][1]["smax"] == h["smax"] and recs[0]["headroom_at"] == ["h", 1]


def test_summary_of_an_empty_table_and_of_overflowing_sites():
    from cosa_amd.utils import seg_helper
    off, n = seg_helper.act_stats_layout(2, 2)
    s = seg_helper.act_stats_summary([0] * n, 2, 2)
    assert s["checks"] == 0 and s["headroom_bits"] is None and s["smax_at"] is None and s["ent_mean"] is None
    assert seg_helper.act_stats_line(s) == " act: headroom -, max|s| -, ent -, over 0"
    c = [0] * n
    c[off["1.v.absmax"]], c[off["1.v.over"]], c[off["1.v.nonfinite"]], c[off["0.head1.nonfinite_rows"]] = ref.f32_bits(131008.0), 4, 2, 5
    s = seg_helper.act_stats_summary(c, 2, 2)
    assert s["headroom_bits"] == -1.0 and s["headroom_at"] == ["v", 1] and s["over"] == 4 and s["nonfinite"] == 2 and s["nonfinite_rows"] == 5
    assert seg_helper.act_stats_line(s) == " act: headroom -1.0b (v L1), max|s| -, ent -, over 4"


def test_the_monitor_table_keeps_its_pinned_tuples_and_ends_with_the_new_row():
    from cosa_amd import checkpoint, monitors
    assert [m.name for m in monitors.MONITORS] == ["guard", "label_stats", "tensor_stats", "teacher_check", "student_check", "gt_stats", "act_stats"]
    assert monitors.MONITORS[-1].state_name == "aux.act_stats.counters"
    assert set(monitors.BY_NAME) == {m.name for m in monitors.MONITORS} and all(monitors.BY_NAME[m.name] is m for m in monitors.MONITORS)
    on = SimpleNamespace(guard_state=None, label_stats_state=None, tensor_stats_table=None, tensor_stats_state=None, teacher_check_state=None,
                         student_check_state=None, gt_stats_state=None, act_stats_state=torch.zeros(3, dtype=torch.int64))
    assert [m.name for m, _ in monitors.active(on)] == ["act_stats"]
    assert monitors.active(SimpleNamespace(**dict(vars(on), act_stats_state=None))) == []
    assert checkpoint.MONITORS is monitors.MONITORS


def _tool(name):
    spec = importlib.util.spec_from_file_location("cosa_tool_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("tool", ["act_stats", "teacher_check"])
def test_qk_gain_scales_exactly_the_q_and_k_rows(tool):
    from cosa_amd.models.vit import VisionTransformer
    mod = _tool(tool)
    assert mod.get_parser().parse_args(["EXP"]).qk_gain == 1.0 and mod.get_parser().parse_args(["EXP", "--qk_gain", "8"]).qk_gain == 8.0
    torch.manual_seed(0)
    net = VisionTransformer(img_size=32, patch_size=16, embed_dim=64, depth=2, num_heads=1, num_classes=0)
    for blk in net.blocks:
        torch.nn.init.normal_(blk.attn.qkv.bias)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    mod.scale_qk(net, 1.0)
    after = net.state_dict()
    assert before.keys() == after.keys() and all(before[k].numpy().tobytes() == after[k].numpy().tobytes() for k in before)
    mod.scale_qk(net, 4.0)
    after = net.state_dict()
    touched = 0
    for k, v in before.items():
        if k.endswith("attn.qkv.weight") or k.endswith("attn.qkv.bias"):
            assert torch.equal(after[k][:128], 2.0 * v[:128]) and torch.equal(after[k][128:], v[128:]) and bool((v[:128] != 0).all()), k
            touched += 1
        else:
            assert torch.equal(after[k], v), k
    assert touched == 4
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            mod.scale_qk(net, bad)
