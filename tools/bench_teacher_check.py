"""What --teacher_check_iters costs on one MI355X -> profiles/teacher_check_cost.txt (one JSON document).

Two trainers of the default workload (b = 16 x 448^2, K = 21, default teacher fp16x3; tools/bench_label_stats.py's set-up) live in ONE process,
same seed, same batch: one with the flag off (the step as it was, call for call) and one with --teacher_check_iters 1, so that EVERY step
of it is a check step (check mode: auto = bf16x3).
(a) the reduction alone (cosa_teacher_check: the memset node and both launches; HIP events, 5 warm-up + 30 timed, median) on what the
    flag-on trainer's last step left behind -- the teacher's CAM buffers against the check network's, the step's label map against a
    perturbed copy, random targets -- beside its byte floor at 8 TB/s: both passes' planes of the present classes of two CAM sets, four
    label maps, the targets;
(b) step time: interleaved blocks of 10 steps of either trainer, host clock around a synchronised block; the difference of the medians is
    the cost of one check, and / 100 its amortised share at --teacher_check_iters 100;
(c) final weights of the two runs compared bit for bit (expected identical: the check only reads).
usage: python tools/bench_teacher_check.py [out=profiles/teacher_check_cost.txt] [blocks=5]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch
from cosa_amd.utils import seg_helper

HBM_PEAK_GBS = 8000.0
STEPS = 10
B, S, K = 16, 448, 21
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "teacher_check_cost.txt")
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda", 0)
batch = synthetic_batch(B, S, K - 1, dev, seed=1234)
trainers = {"off": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B), dev, seed=0),
            "on": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, teacher_check_iters=1), dev, seed=0)}
n_iter = trainers["off"].args.warmup_iters + 1
for _ in range(5):                      # the teacher's graph is captured in the third call: every timed step replays it
    for tr in trainers.values():
        logs = tr.step(*batch, n_iter)
torch.cuda.synchronize()

# (a) the reduction alone
on = trainers["on"]
_, _, cls_label, img_box = batch
cam_a, aux_a = on._s_out[0], on._s_out[1]
ent = next(iter(on._checks["teacher_check"].buffers.values()))
cam_b, aux_b = ent["cam"], ent["aux"]
mask_a = logs["mask"].contiguous().float()
mask_b = torch.where(torch.rand(mask_a.shape, device=dev) < 0.01, torch.zeros_like(mask_a), mask_a)
h = S // 16
tgt_a = torch.rand(B, K - 1, h, h, device=dev)
tgt_b = tgt_a + 1e-4 * torch.rand_like(tgt_a)
counters = seg_helper.new_teacher_check(K, dev)
kernel_ms = []
for i in range(35):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    seg_helper.teacher_check((cam_a, cam_b), (aux_a, aux_b), (tgt_a, tgt_b), (mask_a, mask_b), (mask_a, mask_b), cls_label, img_box, counters)
    b.record()
    b.synchronize()
    if i >= 5:
        kernel_ms.append(a.elapsed_time(b))
present = int((cls_label != 0).sum())
kernel_bytes = (2 * 2 * present * S * S + 4 * B * S * S + 2 * present * h * h) * 4

# (b) step time, interleaved
ms = {"off": [], "on": []}
for _ in range(blocks):
    for name, tr in trainers.items():
        t0 = time.perf_counter()
        for _ in range(STEPS):
            tr.step(*batch, n_iter)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3 / STEPS)

# (c)
same = True
for (n, p), (_, q) in zip(list(trainers["off"].student.named_parameters()) + list(trainers["off"].model_AN.named_parameters()),
                          list(trainers["on"].student.named_parameters()) + list(trainers["on"].model_AN.named_parameters())):
    if not torch.equal(p.view(torch.int32), q.view(torch.int32)):
        same = False
        print("weights differ:", n)

med = statistics.median(kernel_ms)
off_med, on_med = statistics.median(ms["off"]), statistics.median(ms["on"])
summary = on.teacher_check()
res = {
    "workload": "b=16 x 448^2, VOC12 (K = 21), vit_base_patch16_224, teacher %s (captured), check mode %s, one MI355X"
                % (on.args.teacher_precision, on.args.teacher_check_mode),
    "blocks": blocks, "steps_per_block": STEPS,
    "kernel_ms_median": med, "kernel_ms_min": min(kernel_ms), "kernel_ms_max": max(kernel_ms),
    "kernel_note": "one C call = a memset node + the reduction + the finish launch, timed together with HIP events (launch gaps included)",
    "present_cam_planes_per_set": present, "kernel_bytes": kernel_bytes,
    "kernel_floor_ms_at_8TBs": kernel_bytes / (HBM_PEAK_GBS * 1e9) * 1e3, "kernel_achieved_GBs": kernel_bytes / (med * 1e-3) / 1e9,
    "step_ms_flag_off": {"median": off_med, "min": min(ms["off"]), "max": max(ms["off"]), "blocks": ms["off"]},
    "step_ms_every_step_a_check": {"median": on_med, "min": min(ms["on"]), "max": max(ms["on"]), "blocks": ms["on"]},
    "check_step_cost_ms": on_med - off_med, "check_step_cost_share_of_a_step": (on_med - off_med) / off_med,
    "amortised_cost_ms_at_N_100": (on_med - off_med) / 100, "amortised_share_at_N_100": (on_med - off_med) / 100 / off_med,
    "flag_off_block_spread_ms": max(ms["off"]) - min(ms["off"]),
    "final_weights_bit_identical": same, "checks_counted_by_the_trainer": summary["checks"],
    "monitor_figures_of_the_run": {k: summary[k] for k in ("cam", "aux", "tgt", "conforms")}
    | {p: {k: summary[p][k] for k in ("pix", "agree", "miou")} for p in ("main", "aux_label")},
}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
