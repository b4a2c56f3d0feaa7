"""What --label_stats costs on one MI355X -> profiles/r12_label_stats.json.

Two trainers of the default workload (b = 16 x 448^2, K = 21, tools/bench_grad_guard.py's set-up) live in ONE process, same seed, same
batch: one with the flag off (the step as it was, call for call) and one with it on.
(a) the kernel alone (cosa_label_stats: the memset node and both launches; HIP events, 5 warm-up + 30 timed, median) on the tensors of
    the flag-on trainer's last step -- its label map, the teacher's CAM buffers, the batch's labels and boxes -- beside its byte floor at
    8 TB/s: the two masks plus the CAM planes of the present classes, the only full-resolution streams;
(b) step time: interleaved blocks of 10 steps of either trainer, host clock around a synchronised block; the block-to-block spread of the
    flag-off blocks is the yardstick for the difference;
(c) final weights of the two runs compared bit for bit (expected identical: the flag only reads).
usage: python tools/bench_label_stats.py [out=profiles/r12_label_stats.json] [blocks=6]"""
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
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r12_label_stats.json")
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 6
dev = torch.device("cuda", 0)
batch = synthetic_batch(B, S, K - 1, dev, seed=1234)
trainers = {"off": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B), dev, seed=0),
            "on": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, label_stats=True), dev, seed=0)}
n_iter = trainers["off"].args.warmup_iters + 1
for _ in range(5):                      # the teacher's graph is captured in the third call: every timed step replays it
    for tr in trainers.values():
        logs = tr.step(*batch, n_iter)
torch.cuda.synchronize()

# (a) the kernel alone, first: on what the flag-on trainer's last step left behind
on = trainers["on"]
_, _, cls_label, img_box = batch
mask_main = logs["mask"].contiguous().float()
mask_aux = torch.where(torch.rand(mask_main.shape, device=dev) < 0.1, torch.zeros_like(mask_main), mask_main)
cam, cam_aux = on._s_out[0], on._s_out[1]
h = S // 16
seg = torch.randn(B, K, h, h, device=dev) * 4
counters = seg_helper.new_label_stats(K, dev)
scale = torch.ones(1, device=dev)
kernel_ms = []
for i in range(35):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    seg_helper.label_stats(mask_main, mask_aux, seg, cls_label, img_box, cam, cam_aux, counters, step_scale=scale)
    b.record()
    b.synchronize()
    if i >= 5:
        kernel_ms.append(a.elapsed_time(b))
summary = seg_helper.label_stats_summary(counters, K)
present_planes = int((cls_label != 0).sum())
kernel_bytes = (2 * B + 2 * present_planes) * S * S * 4

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
res = {
    "workload": "b=16 x 448^2, VOC12 (K = 21), vit_base_patch16_224, teacher fp16x3 (captured), one MI355X", "blocks": blocks,
    "steps_per_block": STEPS,
    "kernel_ms_median": med, "kernel_ms_min": min(kernel_ms), "kernel_ms_max": max(kernel_ms),
    "kernel_note": "one C call = a memset node + the reduction + the one-thread finish, timed together with HIP events (launch gaps included)",
    "present_cam_planes_per_set": present_planes, "kernel_bytes": kernel_bytes,
    "kernel_floor_ms_at_8TBs": kernel_bytes / (HBM_PEAK_GBS * 1e9) * 1e3, "kernel_achieved_GBs": kernel_bytes / (med * 1e-3) / 1e9,
    "step_ms_flag_off": {"median": off_med, "min": min(ms["off"]), "max": max(ms["off"]), "blocks": ms["off"]},
    "step_ms_flag_on": {"median": on_med, "min": min(ms["on"]), "max": max(ms["on"]), "blocks": ms["on"]},
    "step_ms_difference_of_medians": on_med - off_med, "flag_off_block_spread_ms": max(ms["off"]) - min(ms["off"]),
    "difference_exceeds_spread": (on_med - off_med) > (max(ms["off"]) - min(ms["off"])),
    "final_weights_bit_identical": same, "steps_counted_by_the_trainer": trainers["on"].label_stats()["steps"],
    "kernel_run_summary": {k: summary[k] for k in ("steps", "pix", "ignore_frac", "bg_frac", "fg_frac", "aux_agree", "student_miou", "teacher_nonfinite")},
}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
