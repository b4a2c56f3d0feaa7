"""What the "fp32" operand mode of the no-grad passes costs on one MI355X -> profiles/fp32_teacher.json.

(a) the four block GEMMs (cosa_gemm_f32) at the default workload's token count M = 87 904 (b = 16 x 448^2, three scales, mirror images) and
    the attention (cosa_attn_fwd_f32) at its largest scale, N = 1765, B = 32, H = 12: HIP events around `iters` calls after `warm` warm-up
    calls, median; TF/s = algorithmic flops (2 M N K; 4 B H N^2 64) over that time; share of the 157.3 TF f32-MFMA peak beside it;
(b) step time of three trainers of the default workload in ONE process, same seed, same batch, interleaved blocks, host clock around a
    synchronised block: the default teacher (fp16x3), --teacher_precision fp32, and the default teacher with --teacher_check_iters 1
    --teacher_check_mode fp32 (every step a check step); the difference of the medians of the last and the first is the cost of one fp32 check.
usage: python tools/bench_fp32_teacher.py [out=profiles/fp32_teacher.json] [blocks=3]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd import nn_ops
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch

F32_MFMA_PEAK_TF = 157.3
VALU_GEMM_TF = 52.0          # an f32 VALU (v_pk_fma_f32) GEMM at 4096^3 on this part: the figure a matrix-core GEMM must not fall below
B, S, K = 16, 448, 21
M = 87904
STEPS = 5
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "fp32_teacher.json")
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda", 0)


def timed(fn, warm=2, iters=7):
    ms = []
    for i in range(warm + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= warm:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


res = {"workload": f"b={B} x {S}^2, VOC12 (K = {K}), vit_base_patch16_224, one MI355X", "f32_mfma_peak_TF": F32_MFMA_PEAK_TF}

# (a) kernels
g = torch.Generator(device=dev).manual_seed(0)
rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
D, Hd = 768, 3072
x768, x3072, stream = rnd(M, D), rnd(M, Hd), rnd(M, D)
kern = {}
for name, N_, K_, epi, x in (("qkv", 3 * D, D, nn_ops.EPI_BIAS, x768), ("proj", D, D, nn_ops.EPI_RESIDUAL, x768), ("fc1", Hd, D, nn_ops.EPI_GELU, x768),
                             ("fc2", D, Hd, nn_ops.EPI_RESIDUAL, x3072)):
    w, bias = rnd(N_, K_) * 0.03, rnd(N_)
    out = stream if epi == nn_ops.EPI_RESIDUAL else torch.empty((M, N_), device=dev)
    med, lo, hi = timed(lambda: nn_ops.gemm_f32(x, w, bias, M, N_, K_, epi, residual=stream if epi == nn_ops.EPI_RESIDUAL else None, out=out))
    tf = 2.0 * M * N_ * K_ / (med * 1e-3) / 1e12
    kern[name] = {"M": M, "N": N_, "K": K_, "epilogue": epi, "ms_median": med, "ms_min": lo, "ms_max": hi, "TFs": tf, "share_of_f32_mfma_peak": tf / F32_MFMA_PEAK_TF,
                  "below_the_VALU_gemm_figure": tf < VALU_GEMM_TF}
    del w, bias, out
Ba, Na, H = 32, 1765, 12
qkv, o = rnd(Ba * Na, 3 * D), torch.empty((Ba * Na, D), device=dev)
med, lo, hi = timed(lambda: nn_ops.attn_fwd_f32(qkv, Ba, Na, H, o))
tf = 4.0 * Ba * H * Na * Na * 64 / (med * 1e-3) / 1e12
kern["attention"] = {"B": Ba, "N": Na, "H": H, "ms_median": med, "ms_min": lo, "ms_max": hi, "TFs": tf, "share_of_f32_mfma_peak": tf / F32_MFMA_PEAK_TF}
res["kernels"] = kern
del x768, x3072, stream, qkv, o
torch.cuda.empty_cache()

# (b) step time
batch = synthetic_batch(B, S, K - 1, dev, seed=1234)
mk = lambda **kw: CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, **kw), dev, seed=0)
trainers = {"default": mk(), "teacher_fp32": mk(teacher_precision="fp32"), "check_fp32_every_step": mk(teacher_check_iters=1, teacher_check_mode="fp32")}
n_iter = trainers["default"].args.warmup_iters + 1
for _ in range(5):                      # the teacher's graph is captured in the third call: every timed step replays it
    for tr in trainers.values():
        tr.step(*batch, n_iter)
torch.cuda.synchronize()
ms = {k: [] for k in trainers}
for _ in range(blocks):
    for name, tr in trainers.items():
        t0 = time.perf_counter()
        for _ in range(STEPS):
            tr.step(*batch, n_iter)
        torch.cuda.synchronize()
        ms[name].append((time.perf_counter() - t0) * 1e3 / STEPS)
med = {k: statistics.median(v) for k, v in ms.items()}
res["step_ms"] = {k: {"median": med[k], "min": min(v), "max": max(v), "blocks": v} for k, v in ms.items()}
res["teachers"] = {k: (tr.args.teacher_precision, "graph" if tr._graph is not None else "eager: " + str(tr.graph_error)) for k, tr in trainers.items()}
res["fp32_teacher_step_cost_ms"] = med["teacher_fp32"] - med["default"]
res["fp32_check_cost_ms"] = med["check_fp32_every_step"] - med["default"]
res["fp32_check_amortised_share_at_N_100"] = res["fp32_check_cost_ms"] / 100 / med["default"]
s = trainers["check_fp32_every_step"].teacher_check()
res["monitor_fp16x3_vs_fp32"] = {k: {f: s[k][f] for f in ("worst", "over", "planes")} for k in ("cam", "aux", "tgt")} | \
    {p: {f: s[p][f] for f in ("pix", "agree", "miou")} for p in ("main", "aux_label")} | {"checks": s["checks"], "conforms_without_tgt": s["conforms_without_tgt"]}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
