"""The optional run-time monitors as ONE table: the gradient guard, --label_stats, --tensor_stats, --teacher_check_iters,
--student_check_iters, --gt_stats and --act_stats_iters (section 21).  A row says what the launcher's log interval
(main.read_interval and the log block), the jsonl files and the state files (checkpoint.TrainState) need to know about a monitor; the kernels, their torch partners and the summaries are the monitors' own
and live where they always did (utils/seg_helper.py, utils/torch_helper.py, CoSATrainer).  Adding a monitor is adding a row."""
import json
from pathlib import Path
from typing import Callable, NamedTuple, Optional, Tuple

from .utils import seg_helper, torch_helper


class Monitor(NamedTuple):
    name: str                             # also the stem of <output_dir>/<name>.jsonl
    tensors: Callable                     # (trainer) -> the monitor's device tensor(s), None when it is off
    pack: Callable                        # (tensors) -> [float64 vectors] for the interval's one transfer
    unpack: Callable                      # (tensors, flat) -> host values from its slice of that transfer, a list of Python floats
    zero: Callable                        # (tensors): what is an interval's is zeroed after the read, what is the run's stays
    summary: Optional[Callable]           # (trainer, args, host values) -> summary; None: the host values are shown as they are
    line: Callable                        # (summary, targs) -> what the monitor adds to the interval's log line
    record_extra: Optional[Callable]      # (targs) -> the jsonl record's keys beside the summary and `iters`; None: no jsonl file
    gate: Callable                        # (summary) -> whether this interval shows the monitor at all
    state_name: str                       # its optional entry of a state file
    notes: Tuple[str, str]                # (note when a file has the entry and the run does not, note when only the run has it)


# a vector of integer counters: counts and 32-bit patterns are exact in a double (an interval's stay far below 2^53)
_counts_pack = lambda t: [t.double()]
_counts_unpack = lambda t, flat: [int(v) for v in flat]
_zero = lambda t: t.zero_()                           # an interval's
_keep = lambda t: None                                # the run's
_always = lambda summary: True
_held_a_check = lambda summary: summary["checks"] > 0      # (an interval without a check step: the line as ever)


def _guard_pack(g):
    return [torch_helper.guard_norm(g).double().reshape(1), g[3:5].double()]


def _guard_line(g, targs):
    return " grad_norm: %.4f, skipped: %d, clipped: %d" % (g[0], int(g[1]), int(g[2]))


def _label_stats_line(summary, targs):
    return " ignore: %.3f, fg: %.3f, aux_agree: %.3f, student_miou: %.3f, teacher_nonfinite: %d" % (
        summary["ignore_frac"], summary["fg_frac"], summary["aux_agree"], summary["student_miou"], summary["teacher_nonfinite"])


def _tensor_stats_tensors(trainer):
    return None if trainer.tensor_stats_table is None else (trainer.tensor_stats_table, trainer.tensor_stats_state)


def _tensor_stats_pack(pair):
    table, blame = pair
    return [torch_helper.tensor_stats_values(table).reshape(-1)] + ([blame.double()] if blame is not None else [])


def _tensor_stats_unpack(pair, flat):
    """-> (the table's values as [T][W] floats, the blame counters as ints or None)"""
    (T, W), blame = pair[0].shape, pair[1]
    return [flat[i * W:(i + 1) * W] for i in range(T)], [int(v) for v in flat[T * W:]] if blame is not None else None


def _tensor_stats_line(summary, targs):
    """the global relative EMA gap, and the blamed / non-finite tensor's name or -"""
    return " ema_gap: %.3e, worst: %s" % (summary["global"]["ema_gap_rel"], summary["worst"] if summary["worst"] is not None else "-")


def _teacher_check_line(summary, targs):
    """the worst figure over the map sets, the planes over the literal bar, the lowest agreement and mIoU over the label pairs"""
    w = seg_helper.teacher_check_worst(summary)
    return " tcheck[%s]: worst %.1e, over %d/%d, agree %.5f, miou %.5f" % (
        targs.teacher_check_mode, w["worst"], w["over"], w["planes"], w["agree"], w["miou"])


def _student_check_pack(t):
    return [(t >> 32).double(), (t & 0xffffffff).double()]     # its fixed-point sums may pass 2^53: each travels as its high and low 32 bits


def _student_check_unpack(t, flat):
    m = len(flat) // 2
    return [(int(h) << 32) | int(l) for h, l in zip(flat[:m], flat[m:])]


def _student_check_line(summary, targs):
    """` scheck[MODE]: seg rel 1.2e-03, agree 0.99987, flips>=1e-1 0, loss rel 3.1e-04` -- the seg logits' relative L2 difference, the share of
    cells with the same argmax, the differing cells whose check-pass margin is at least 1e-1 (real flips, not near-ties), and the largest
    relative difference over the four loss terms"""
    return " scheck[%s]: seg rel %.1e, agree %.5f, flips>=1e-1 %d, loss rel %.1e" % (
        targs.student_check_mode, summary["seg"]["rel_l2"], summary["seg_agree"], summary["flip_hist"][3], summary["loss_rel"])


def _gt_stats_line(summary, targs):
    """` gt: main 0.412 (lab 0.731), aux 0.388, student 0.295`: the mIoUs against ground truth as fractions -- the main labels' over the
    pixels that carry one, with the share of ground-truth pixels that do; `-` for the auxiliary map where the run has none"""
    aux = "%.3f" % summary["aux"]["miou"] if summary["aux"]["pixels"] else "-"
    return " gt: main %.3f (lab %.3f), aux %s, student %.3f" % (summary["main"]["miou"], summary["main"]["labelled"], aux,
                                                                 summary["student"]["miou"])


def _act_stats_summary(trainer, args, values):
    depth, heads = trainer.act_stats_shape
    return seg_helper.act_stats_summary(values, depth, heads)


# in the order in which the log line shows them
MONITORS = (
    Monitor("guard", lambda tr: tr.guard_state, _guard_pack, lambda g, flat: list(flat), _keep, None, _guard_line, None, _always,
            "guard.state",
            ("the file holds a gradient guard's counters and this run has no guard (--clip_grad_norm 0, --skip_nonfinite false): the entry "
             "is ignored",
             "written without a gradient guard: this run's guard counters start at zero")),
    Monitor("label_stats", lambda tr: tr.label_stats_state, _counts_pack, _counts_unpack, _zero,
            lambda tr, args, v: seg_helper.label_stats_summary(v, args.num_classes), _label_stats_line, lambda targs: {}, _always,
            "aux.label_stats.counters",
            ("the file holds pseudo-label statistics and this run does not collect them (--label_stats false): the entry is ignored",
             "written without pseudo-label statistics: this run's label counters start at zero")),
    # the table is the sample of the interval's last step and is not accumulated; the blame counters are the run's: neither is zeroed
    Monitor("tensor_stats", _tensor_stats_tensors, _tensor_stats_pack, _tensor_stats_unpack, _keep,
            lambda tr, args, v: tr.tensor_stats(v), _tensor_stats_line, lambda targs: {}, _always,
            "aux.tensor_stats.blame",
            ("the file holds per-tensor blame counters and this run does not keep them (--tensor_stats false, or no gradient guard): the "
             "entry is ignored",
             "written without per-tensor blame counters: this run's blame counters start at zero")),
    Monitor("teacher_check", lambda tr: tr.teacher_check_state, _counts_pack, _counts_unpack, _zero,
            lambda tr, args, v: seg_helper.teacher_check_summary(v, args.num_classes), _teacher_check_line,
            lambda targs: dict(mode=targs.teacher_precision, check_mode=targs.teacher_check_mode), _held_a_check,
            "aux.teacher_check.counters",
            ("the file holds a teacher check's counters and this run makes no checks (--teacher_check_iters 0): the entry is ignored",
             "written without a teacher check: this run's check counters start at zero")),
    Monitor("student_check", lambda tr: tr.student_check_state, _student_check_pack, _student_check_unpack, _zero,
            lambda tr, args, v: seg_helper.student_check_summary(v, args.num_classes), _student_check_line,
            lambda targs: dict(mode="bf16", check_mode=targs.student_check_mode), _held_a_check,      # (`mode`: the training forward's)
            "aux.student_check.counters",
            ("the file holds a student check's counters and this run makes no checks (--student_check_iters 0): the entry is ignored",
             "written without a student check: this run's check counters start at zero")),
    Monitor("gt_stats", lambda tr: getattr(tr, "gt_stats_state", None), _counts_pack, _counts_unpack, _zero,
            lambda tr, args, v: seg_helper.gt_stats_summary(v, args.num_classes), _gt_stats_line, lambda targs: {}, _always,
            "aux.gt_stats.counters",
            ("the file holds ground-truth statistics and this run does not collect them (--gt_stats false): the entry is ignored",
             "written without ground-truth statistics: this run's ground-truth counters start at zero")),
    # its fixed-point sums (2^-32 units, one term per attention row) pass 2^53 within an interval: they travel as --student_check_iters' do
    Monitor("act_stats", lambda tr: getattr(tr, "act_stats_state", None), _student_check_pack, _student_check_unpack, _zero,
            _act_stats_summary, lambda summary, targs: seg_helper.act_stats_line(summary), lambda targs: dict(mode="fp32"), _held_a_check,
            "aux.act_stats.counters",
            ("the file holds activation statistics and this run collects none (--act_stats_iters 0): the entry is ignored",
             "written without activation statistics: this run's activation counters start at zero")),
)
BY_NAME = {m.name: m for m in MONITORS}


def active(trainer):
    """[(Monitor, its tensors)] of the monitors `trainer` has on, in the table's order: what main.read_interval takes"""
    return [(m, t) for m, t in ((m, m.tensors(trainer)) for m in MONITORS) if t is not None]


def monitor_record(m, summary, n_iter, targs):
    """one line of <output_dir>/<name>.jsonl: the full summary of an interval and, for the two checks, the operand modes compared"""
    return json.dumps(dict(summary, iters=int(n_iter), **m.record_extra(targs)))


def append_monitor(output_dir, m, summary, n_iter, targs):
    with (Path(output_dir) / (m.name + ".jsonl")).open("a") as f:
        f.write(monitor_record(m, summary, n_iter, targs) + "\n")
