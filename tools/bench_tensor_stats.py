"""What --tensor_stats costs on one MI355X -> profiles/r13_tensor_stats.json.

Four trainers of the default workload (b = 16 x 448^2, tools/bench_label_stats.py's set-up) live in ONE process, same seed, same batch:
"off" (the step as it was, call for call: the yardstick) and "on" (--tensor_stats true), neither behind a gradient guard, so "on" has no
per-step work; and "guard_off" (--skip_nonfinite true) and "guard_on" (--skip_nonfinite true --tensor_stats true), the configuration that
adds one blame launch to every step.  The flag-on trainers arm the sample on the step that closes each log_iters interval, as the launcher
does.
(a) step time: interleaved blocks of 10 steps of each trainer, host clock around a synchronised block; the block-to-block spread of the
    flag-off blocks is the yardstick for on - off, that of the guard_off blocks for guard_on - guard_off;
(b) the sample call alone (cosa_tensor_stats: both launches and the read-back of first_chunk; HIP events, 5 warm-up + 30 timed, median)
    on the flag-on trainer's last record table, beside its byte floor at 8 TB/s -- 12 B per parameter, g, p and tp read once -- and beside
    the norm reduction's figure of profiles/r11_grad_guard.json;
(c) the blame launch alone (cosa_grad_blame over the guard's partials), timed the same way;
and the final weights of each pair compared bit for bit (expected identical: the flag only reads).
usage: python tools/bench_tensor_stats.py [out=profiles/r13_tensor_stats.json] [blocks=6]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd import _C
from cosa_amd import args as cosa_args
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch

HBM_PEAK_GBS = 8000.0
STEPS = 10
B, S, K = 16, 448, 21
LOG_ITERS = {f: d for f, _t, d in cosa_args.EXTRA}["log_iters"]           # the launcher's default
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r13_tensor_stats.json")
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 6
dev = torch.device("cuda", 0)
batch = synthetic_batch(B, S, K - 1, dev, seed=1234)
CONFIGS = {"off": {}, "on": dict(tensor_stats=True), "guard_off": dict(skip_nonfinite=True),
           "guard_on": dict(skip_nonfinite=True, tensor_stats=True)}
trainers = {k: CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, **over), dev, seed=0) for k, over in CONFIGS.items()}
n_iter = trainers["off"].args.warmup_iters + 1
count = {k: 0 for k in CONFIGS}


def step(name):
    tr = trainers[name]
    count[name] += 1
    if "tensor_stats" in CONFIGS[name] and count[name] % LOG_ITERS == 0:           # the launcher's cadence: the step that closes an interval samples
        tr.request_tensor_stats()
    tr.step(*batch, n_iter)


for _ in range(5):                      # the teacher's graph is captured in the third call: every timed step replays it
    for name in trainers:
        step(name)
torch.cuda.synchronize()

# (a) step time, interleaved
ms = {k: [] for k in CONFIGS}
for _ in range(blocks):
    for name in trainers:
        t0 = time.perf_counter()
        for _ in range(STEPS):
            step(name)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3 / STEPS)


def same_weights(a, b):
    same = True
    for (n, p), (_, q) in zip(list(trainers[a].student.named_parameters()) + list(trainers[a].model_AN.named_parameters()),
                              list(trainers[b].student.named_parameters()) + list(trainers[b].model_AN.named_parameters())):
        if not torch.equal(p.view(torch.int32), q.view(torch.int32)):
            same = False
            print("weights differ:", a, b, n)
    return same


same = same_weights("off", "on")
same_guarded = same_weights("guard_off", "guard_on")


def timed(fn):
    out = []
    for i in range(35):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= 5:
            out.append(a.elapsed_time(b))
    return out


# (b) the sample alone, on the record table of the flag-on trainer's last step (its gradients are still alive)
fused = trainers["on"]._fused_step
sample_ms = timed(fused.sample)
host_ms = []                            # what the host spends inside the call (the read-back it waits for, both launches), device idle
for _ in range(30):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fused.sample()
    host_ms.append((time.perf_counter() - t0) * 1e3)
summary = trainers["on"].tensor_stats()
n_params = sum(fused.sizes)
n_grad = sum(s for s, gi in zip(fused.sizes, fused.group_idx) if gi >= 0)
sample_bytes = 4 * (2 * n_params + n_grad)

# (c) the blame launch alone, over the partials the guard_on trainer's last step left
guarded = trainers["guard_on"]
gf = guarded._fused_step
L = _C.lib()
blame_ms = timed(lambda: _C.check(L.cosa_grad_blame(_C.ptr(gf.norm_ws), _C.ptr(gf.d_first_chunk), len(gf.student), gf.n_chunks,
                                                    _C.ptr(gf.blame), _C.stream_ptr()), "cosa_grad_blame"))
blamed_total = int(gf.blame.sum())

guard_ref = None
ref_path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r11_grad_guard.json")
if os.path.exists(ref_path):
    with open(ref_path) as f:
        r11 = json.load(f)
    guard_ref = {"grad_norm_ms_median": r11["kernel_ms_median"]["grad_norm"], "grad_norm_bytes": r11["grad_norm_bytes"],
                 "grad_norm_achieved_GBs": r11["grad_norm_achieved_GBs"]}

med = statistics.median(sample_ms)
off_med, on_med = statistics.median(ms["off"]), statistics.median(ms["on"])
spread = max(ms["off"]) - min(ms["off"])
goff_med, gon_med = statistics.median(ms["guard_off"]), statistics.median(ms["guard_on"])
gspread = max(ms["guard_off"]) - min(ms["guard_off"])
res = {
    "workload": "b=16 x 448^2, VOC12 (K = 21), vit_base_patch16_224, teacher fp16x3 (captured), one MI355X", "blocks": blocks,
    "steps_per_block": STEPS, "log_iters": LOG_ITERS, "samples_taken_by_the_flag_on_trainer": count["on"] // LOG_ITERS,
    "step_ms_flag_off": {"median": off_med, "min": min(ms["off"]), "max": max(ms["off"]), "blocks": ms["off"]},
    "step_ms_flag_on": {"median": on_med, "min": min(ms["on"]), "max": max(ms["on"]), "blocks": ms["on"]},
    "step_ms_difference_of_medians": on_med - off_med, "flag_off_block_spread_ms": spread,
    "difference_exceeds_spread": (on_med - off_med) > spread,
    "final_weights_bit_identical": same,
    "step_ms_guard_flag_off": {"median": goff_med, "min": min(ms["guard_off"]), "max": max(ms["guard_off"]), "blocks": ms["guard_off"]},
    "step_ms_guard_flag_on": {"median": gon_med, "min": min(ms["guard_on"]), "max": max(ms["guard_on"]), "blocks": ms["guard_on"]},
    "guarded_step_ms_difference_of_medians": gon_med - goff_med, "guard_flag_off_block_spread_ms": gspread,
    "guarded_difference_exceeds_spread": (gon_med - goff_med) > gspread,
    "guarded_final_weights_bit_identical": same_guarded, "guard_counters": guarded.guard_counters(),
    "tensors": len(fused.sizes), "n_chunks": fused.n_chunks, "parameter_elements": n_params, "gradient_elements": n_grad,
    "sample_ms_median": med, "sample_ms_min": min(sample_ms), "sample_ms_max": max(sample_ms),
    "sample_note": "one C call = the read-back of first_chunk on the library's own stream + the per-chunk reduction + the per-tensor "
                   "finalize, timed together with HIP events (launch gaps and the host's wait for the read-back included)",
    "sample_host_ms_median": statistics.median(host_ms), "sample_host_ms_max": max(host_ms),
    "sample_bytes": sample_bytes, "sample_floor_ms_at_8TBs": sample_bytes / (HBM_PEAK_GBS * 1e9) * 1e3,
    "sample_achieved_GBs": sample_bytes / (med * 1e-3) / 1e9,
    "sample_ms_amortised_per_step": med / LOG_ITERS,
    "norm_reduction_r11": guard_ref,
    "blame_ms_median": statistics.median(blame_ms), "blame_ms_min": min(blame_ms), "blame_ms_max": max(blame_ms),
    "blame_counters_after_the_timed_calls": blamed_total,
    "sample_summary_global": summary["global"], "sample_worst": summary["worst"],
}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
