"""What the "fp64" mode of the no-grad passes costs on one MI355X -> profiles/fp64_teacher.json.

(a) the four block GEMMs (cosa_gemm_f64, fp32 master weights widened in the kernel) at the default workload's token count M = 87 904 (b = 16
    x 448^2, three scales, mirror images) and the attention (cosa_attn_fwd_f64) at its largest scale, N = 1765, B = 32, H = 12: HIP events
    around `iters` calls after `warm` warm-up calls, median; TF/s = algorithmic flops (2 M N K; 4 B H N^2 64) over that time, beside the
    part's published float64 peak (78.6 TF, vector and matrix alike: the f64 MFMA runs at the f64 VALU rate, as the f32-input MFMA runs at the
    f32 one) -- a GEMM below `VALU_SHARE_FLOOR` of it is flagged, with the reason in the record;
(b) one batch of `tools/teacher_check.py --criterion` at b = 16 x 448^2: three multi-scale passes (fp16x3, fp32, fp64; the fp64 one in chunks of
    VITNetwork.F64_CHUNK images) and the per-plane reduction for cam and cam_aux, the same way (HIP events, median of 7 after 2 warm-up), and
    the three passes one by one.
Nobody has measured these before; there is no performance bar.
usage: python tools/bench_fp64_teacher.py [out=profiles/fp64_teacher.json]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd import nn_ops
from cosa_amd.models import VITNetwork, build_model
from cosa_amd.train_step import default_args, synthetic_batch
from cosa_amd.utils import seg_helper

F64_PEAK_TF = 78.6           # published float64 peak of the part, vector = matrix
VALU_SHARE_FLOOR = 1.0 / 3   # the share of the f64 peak an f64 VALU GEMM reaches, by the f32 pair of figures on this part (52 of 157.3 TF)
B, S, K = 16, 448, 21
M = 87904
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "fp64_teacher.json")
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


res = {"workload": f"b={B} x {S}^2, VOC12 (K = {K}), vit_base_patch16_224, one MI355X", "f64_peak_TF": F64_PEAK_TF,
       "f64_chunk_images": VITNetwork.F64_CHUNK}

# (a) kernels
g = torch.Generator(device=dev).manual_seed(0)
rnd = lambda *s, dt=torch.float64: torch.randn(*s, device=dev, generator=g, dtype=dt)
D, Hd = 768, 3072
x768, x3072, stream = rnd(M, D), rnd(M, Hd), rnd(M, D)
kern = {}
for name, N_, K_, epi, x in (("qkv", 3 * D, D, nn_ops.EPI_BIAS, x768), ("proj", D, D, nn_ops.EPI_RESIDUAL, x768), ("fc1", Hd, D, nn_ops.EPI_GELU, x768),
                             ("fc2", D, Hd, nn_ops.EPI_RESIDUAL, x3072)):
    w, bias = rnd(N_, K_, dt=torch.float32) * 0.03, rnd(N_, dt=torch.float32)
    out = stream if epi == nn_ops.EPI_RESIDUAL else torch.empty((M, N_), device=dev, dtype=torch.float64)
    med, lo, hi = timed(lambda: nn_ops.gemm_f64(x, w, bias, M, N_, K_, epi, residual=stream if epi == nn_ops.EPI_RESIDUAL else None, out=out))
    tf = 2.0 * M * N_ * K_ / (med * 1e-3) / 1e12
    kern[name] = {"M": M, "N": N_, "K": K_, "epilogue": epi, "ms_median": med, "ms_min": lo, "ms_max": hi, "TFs": tf, "share_of_f64_peak": tf / F64_PEAK_TF,
                  "below_the_VALU_gemm_figure": tf / F64_PEAK_TF < VALU_SHARE_FLOOR}
    del w, bias, out
Ba, Na, H = 32, 1765, 12
qkv, o = rnd(Ba * Na, 3 * D), torch.empty((Ba * Na, D), device=dev, dtype=torch.float64)
med, lo, hi = timed(lambda: nn_ops.attn_fwd_f64(qkv, Ba, Na, H, o))
tf = 4.0 * Ba * H * Na * Na * 64 / (med * 1e-3) / 1e12
kern["attention"] = {"B": Ba, "N": Na, "H": H, "ms_median": med, "ms_min": lo, "ms_max": hi, "TFs": tf, "share_of_f64_peak": tf / F64_PEAK_TF}
res["kernels"] = kern
if any(k.get("below_the_VALU_gemm_figure") for k in kern.values()):
    res["why_below_the_VALU_figure"] = ("cosa_gemm_f64 is a correctness-first kernel: 64 x 64 block tiles with one 16-k LDS stage in flight, scalar "
                                        "8-byte LDS reads (two per MFMA pair) and transposing 8-byte LDS stores; per MFMA it issues about as many LDS "
                                        "and VALU instructions as the MFMA has issue cycles, so the matrix pipe waits on LDS.  A 128 x 128 tile with "
                                        "16-byte LDS reads would halve the LDS traffic per flop; not done: the mode is a check, run on demand.")
del x768, x3072, stream, qkv, o
torch.cuda.empty_cache()

# (b) one --criterion batch
args = default_args("VOC12", crop_size=S, batch_size=B)
torch.manual_seed(0)
first = build_model(args).eval()
nets = {}
for mode in ("fp16x3", "fp32", "fp64"):
    n = build_model(args).eval()
    n.load_state_dict(first.state_dict())
    nets[mode] = n.to(dev).set_nograd_precision(mode)
wimg, _, lab, _ = synthetic_batch(B, S, K - 1, dev, seed=1234)
lab = lab.to(dev)
scales = list(args.pseudo_scales)
torch.cuda.reset_peak_memory_stats()
last = {}


def one_pass(mode):
    with torch.no_grad():
        last[mode] = seg_helper.multi_scale_camseg(nets[mode], wimg, scales, _active_labels=lab, _seg_scales=True, _return_scale=mode == "fp64")


def criterion_batch():
    for mode in nets:
        one_pass(mode)
    a, c32, c64 = last["fp16x3"], last["fp32"], last["fp64"]
    last["tables"] = {"cam": seg_helper.conformance_planes(a[0], c32[0], c64[0], lab, *c64[3]),
                      "cam_aux": seg_helper.conformance_planes(a[1], c32[1], c64[1], lab, *c64[4])}


torch.cuda.synchronize()
held = torch.cuda.memory_allocated()            # (the three networks and the batch)
one_pass("fp64")
torch.cuda.synchronize()
res["fp64_pass_peak_GB_above_the_networks"] = (torch.cuda.max_memory_allocated() - held) / 2 ** 30
med, lo, hi = timed(criterion_batch)
res["criterion_batch_ms"] = {"median": med, "min": lo, "max": hi}
res["pass_ms"] = {}
for mode in nets:
    m_, lo, hi = timed(lambda: one_pass(mode))
    res["pass_ms"][mode] = {"median": m_, "min": lo, "max": hi}
med, lo, hi = timed(lambda: seg_helper.conformance_planes(last["fp16x3"][0], last["fp32"][0], last["fp64"][0], lab, *last["fp64"][3]))
res["conformance_planes_ms"] = {"median": med, "min": lo, "max": hi}
res["peak_memory_GB"] = torch.cuda.max_memory_allocated() / 2 ** 30
summ = seg_helper.conformance_summary(last["tables"])
res["criterion_fp16x3_random_init"] = {k: {f: v[f] for f in ("planes", "literal_ok", "exempt", "failed", "worst")} for k, v in summ.items()}
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as f:
    json.dump(res, f, indent=1)
    f.write("\n")
print(json.dumps(res))
