"""What --accum_steps costs on one MI355X -> profiles/r13_accum.json.

(a) cosa_grad_accumulate alone, each mode, on the record table of the default trainer (vit_base_patch16_224, crop 448): HIP events, 5 warm-up
    + 30 timed calls, median, beside its byte count (mode 0: 4 B read + 4 B written per trainable element, modes 1 and 2: 8 + 4) and the
    achieved GB/s;
(b) the time of one optimizer step at the same 16 images: b = 16 x N = 1 (the default workload, the step as it was), b = 8 x N = 2 and
    b = 2 x N = 8 (the reference's per-process batch), each trainer alone in its turn, HIP events around the N calls of step(), 5 warm-up
    + 30 timed optimizer steps, median.
usage: python tools/bench_accum.py [out=profiles/r13_accum.json]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd import _C
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch
from cosa_amd.utils import torch_helper

HBM_PEAK_GBS = 8000.0
WARM, TIMED = 5, 30
S, K, IMAGES = 448, 21, 16
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r13_accum.json")
dev = torch.device("cuda", 0)


def timed(fn):
    out = []
    for i in range(WARM + TIMED):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= WARM:
            out.append(a.elapsed_time(b))
    return out


def figures(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


steps, kernel, table = {}, {}, {}
for b, n in ((16, 1), (8, 2), (2, 8)):
    assert b * n == IMAGES
    tr = CoSATrainer(default_args("VOC12", crop_size=S, batch_size=b, accum_steps=n), dev, seed=0)
    batches = [synthetic_batch(b, S, K - 1, dev, seed=1234 + k) for k in range(n)]
    n_iter = tr.args.warmup_iters + 1

    def opt_step():
        for x in batches:
            tr.step(*x, n_iter)

    ms = timed(opt_step)                    # (the teacher's graph is captured in the third call of step(): inside the warm-up)
    steps[f"b{b}_N{n}"] = dict(figures(ms), batch_size=b, accum_steps=n, img_per_s=IMAGES / (statistics.median(ms) * 1e-3))
    if n == 2:                              # (a) on this trainer's table: the gradients of its last micro-step are still alive
        f = tr._fused_step
        d_rec = f._last_rec.clone()         # the step's table points at the accumulator: point it at the live gradients again
        rec = f.recs[0].copy()
        for i, p in enumerate(f.student):
            rec[i]["g"] = p.grad.data_ptr() if (f.group_idx[i] >= 0 and p.grad is not None) else 0
        d_rec.copy_(torch.from_numpy(rec.view("u1").copy()))
        n_grad = sum(sz for sz, p, gi in zip(f.sizes, f.student, f.group_idx) if gi >= 0 and p.grad is not None)
        table = {"tensors": len(f.sizes), "n_chunks": f.n_chunks, "gradient_elements": n_grad, "accumulator_bytes": f.acc.numel() * 4}
        for mode in (0, 1, 2):
            call = lambda: _C.check(_C.lib().cosa_grad_accumulate(_C.ptr(d_rec), _C.ptr(f.d_chunks), f.n_chunks, _C.ptr(f.d_acc_ptrs), mode,
                                                                  torch_helper.accum_scale(2), _C.stream_ptr()), "cosa_grad_accumulate")
            kms = timed(call)
            nbytes = n_grad * (8 if mode == 0 else 12)
            med = statistics.median(kms)
            kernel[f"mode{mode}"] = dict(figures(kms), bytes=nbytes, floor_ms_at_8TBs=nbytes / (HBM_PEAK_GBS * 1e9) * 1e3,
                                         achieved_GBs=nbytes / (med * 1e-3) / 1e9)
    del tr
    torch.cuda.empty_cache()

base = steps["b16_N1"]["median"]
res = {"workload": f"{IMAGES} images x {S}^2 per optimizer step, VOC12 (K = {K}), vit_base_patch16_224, teacher fp16x3 (captured), one MI355X",
       "warm_up": WARM, "timed": TIMED, "record_table": table, "grad_accumulate_ms": kernel, "optimizer_step_ms": steps,
       "optimizer_step_vs_b16_N1": {k: v["median"] / base for k, v in steps.items()}}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
