"""What --student_check_iters costs on one MI355X: ONE trainer of the default workload (b = 16 x 448^2, K = 21;
tools/bench_teacher_check.py's set-up) timed in blocks of 10 steps, host clock around a synchronised block -> one JSON line.

    python tools/bench_student_check.py LABEL N [blocks=5] [check_mode=fp32]

N = 0: the flag off; N = 1: every step a check step; N = 1000000: the flag on and no timed step a check step (the ordinary step with
the monitor armed).  The cost of one check is the difference of the medians of two such runs, and whether the ordinary step moved is the
N = 1000000 run against N = 0 -- or against the parent commit's tree, which this file runs on unchanged (COSA_TREE=<its root>; a tree
without the flag ignores it).  Runs to compare are started in turn, one process each, several rounds, so that a drift of the box shows as spread of
the repeated reference run and not as a difference (profiles/student_check.json holds the record)."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("COSA_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch

STEPS = 10
B, S, K = 16, 448, 21
label, n_check = sys.argv[1], int(sys.argv[2])
blocks = int(sys.argv[3]) if len(sys.argv) > 3 else 5
mode = sys.argv[4] if len(sys.argv) > 4 else "fp32"
dev = torch.device("cuda", 0)
batch = synthetic_batch(B, S, K - 1, dev, seed=1234)
tr = CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, student_check_iters=n_check, student_check_mode=mode), dev, seed=0)
n_iter = tr.args.warmup_iters + 1                # (n_iter + 1) % 1000000 != 0: no check step unless N = 1
for _ in range(5):                               # the teacher's graph is captured in the third call: every timed step replays it
    tr.step(*batch, n_iter)
torch.cuda.synchronize()
ms = []
for _ in range(blocks):
    t0 = time.perf_counter()
    for _ in range(STEPS):
        tr.step(*batch, n_iter)
    torch.cuda.synchronize()
    ms.append((time.perf_counter() - t0) * 1e3 / STEPS)
summary = tr.student_check() if getattr(tr, "student_check_state", None) is not None else None
print(json.dumps({"label": label, "student_check_iters": n_check, "check_mode": mode if n_check else None, "blocks": blocks,
                  "steps_per_block": STEPS, "step_ms_blocks": ms, "step_ms_median": statistics.median(ms), "step_ms_min": min(ms),
                  "step_ms_max": max(ms), "checks_counted": summary["checks"] if summary else 0,
                  "tree": os.path.dirname(os.path.abspath(sys.modules["cosa_amd"].__file__))}), flush=True)
