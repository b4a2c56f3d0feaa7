"""What the gradient guard costs on one MI355X -> profiles/r11_grad_guard.json.

Two trainers of the default workload (b = 16 x 448^2, tools/step_only.py's step) live in ONE process, same seed, same batch: one without a
guard (the unguarded step, call for call) and one behind a guard that never fires (clip_grad_norm 1e9, skip_nonfinite).
(a) step time: interleaved blocks of 10 steps of either trainer, host clock around a synchronised block; the block-to-block spread of the
    guard-off blocks is the yardstick for the difference;
(b) final weights of the two runs compared bit for bit (expected identical: coef == 1 is an exact product);
(c) the kernels on their own, afterwards, on the guarded trainer's record table (HIP events, 5 warm-up + 30 timed, median): the norm
    reduction (both of its launches) as GB/s of the gradient bytes beside the HBM floor, the unguarded and the guarded optimizer kernel.
usage: python tools/bench_grad_guard.py [out=profiles/r11_grad_guard.json] [blocks=6]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd import _C
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch

HBM_PEAK_GBS = 8000.0
STEPS = 10
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r11_grad_guard.json")
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 6
dev = torch.device("cuda", 0)
batch = synthetic_batch(16, 448, 20, dev, seed=1234)
trainers = {"off": CoSATrainer(default_args("VOC12", crop_size=448, batch_size=16), dev, seed=0),
            "on": CoSATrainer(default_args("VOC12", crop_size=448, batch_size=16, clip_grad_norm=1e9, skip_nonfinite=True), dev, seed=0)}
n_iter = trainers["off"].args.warmup_iters + 1
for _ in range(5):                      # the teacher's graph is captured in the third call: every timed step replays it
    for tr in trainers.values():
        tr.step(*batch, n_iter)
torch.cuda.synchronize()

ms = {"off": [], "on": []}
for _ in range(blocks):
    for name, tr in trainers.items():
        t0 = time.perf_counter()
        for _ in range(STEPS):
            tr.step(*batch, n_iter)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3 / STEPS)

same = True
for (n, a), (_, b) in zip(list(trainers["off"].student.named_parameters()) + list(trainers["off"].model_AN.named_parameters()),
                          list(trainers["on"].student.named_parameters()) + list(trainers["on"].model_AN.named_parameters())):
    if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
        same = False
        print("weights differ:", n)
counters = trainers["on"].guard_counters()
norm = float(trainers["on"].guard_state.view(torch.float32)[0])

# (c) the kernels alone, on the record table of the guarded trainer's last step (its gradients are still in place)
fs = trainers["on"]._fused_step
L = _C.lib()
d_rec = fs.d_recs[(fs.slot - 1) % fs.kRing]
grad_elems = sum(p.numel() for p in fs.student if p.grad is not None)
state_elems = sum(p.numel() for p in fs.student)
b1, b2 = fs.opt.param_groups[0]["betas"]
eps, step = float(fs.opt.param_groups[0]["eps"]), int(fs.opt.global_step)
calls = {
    "grad_norm": lambda: L.cosa_grad_norm(_C.ptr(d_rec), _C.ptr(fs.d_chunks), fs.n_chunks, fs.max_norm, int(fs.skip_nonfinite), _C.ptr(fs.norm_ws),
                                          fs.norm_ws.numel(), _C.ptr(fs.guard), _C.stream_ptr()),
    "adamw_ema": lambda: L.cosa_fused_adamw_ema(_C.ptr(d_rec), _C.ptr(fs.d_chunks), fs.n_chunks, float(b1), float(b2), eps, step, fs.momentum,
                                                _C.stream_ptr()),
    "adamw_ema_guarded": lambda: L.cosa_fused_adamw_ema_guarded(_C.ptr(d_rec), _C.ptr(fs.d_chunks), fs.n_chunks, float(b1), float(b2), eps, step,
                                                                fs.momentum, _C.ptr(fs.guard), _C.stream_ptr()),
}
kernel_ms = {k: [] for k in calls}
for i in range(35):
    for k, fn in calls.items():         # alternating, so that all three see the same machine
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _C.check(fn(), k)
        b.record()
        b.synchronize()
        if i >= 5:
            kernel_ms[k].append(a.elapsed_time(b))

med = {k: statistics.median(v) for k, v in kernel_ms.items()}
grad_bytes = grad_elems * 4
res = {
    "workload": "b=16 x 448^2, VOC12, vit_base_patch16_224, teacher fp16x3 (captured), one MI355X", "blocks": blocks, "steps_per_block": STEPS,
    "step_ms_guard_off": {"median": statistics.median(ms["off"]), "min": min(ms["off"]), "max": max(ms["off"]), "blocks": ms["off"]},
    "step_ms_guard_on": {"median": statistics.median(ms["on"]), "min": min(ms["on"]), "max": max(ms["on"]), "blocks": ms["on"]},
    "step_ms_difference_of_medians": statistics.median(ms["on"]) - statistics.median(ms["off"]),
    "final_weights_bit_identical": same, "guard_counters": counters, "last_grad_norm": norm,
    "n_chunks": fs.n_chunks, "gradient_elements": grad_elems, "parameter_elements": state_elems,
    "kernel_ms_median": med, "kernel_ms_min": {k: min(v) for k, v in kernel_ms.items()},
    "grad_norm_bytes": grad_bytes, "grad_norm_floor_ms_at_8TBs": grad_bytes / (HBM_PEAK_GBS * 1e9) * 1e3,
    "grad_norm_achieved_GBs": grad_bytes / (med["grad_norm"] * 1e-3) / 1e9,
    "guarded_minus_unguarded_kernel_ms": med["adamw_ema_guarded"] - med["adamw_ema"],
    "note": "grad_norm: one C call = the per-chunk reduction + the one-block finalize, timed together with HIP events (launch gaps included)",
}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
