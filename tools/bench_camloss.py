"""What --camloss_version v1 | v2 | v3 cost on the fused kernels and on the torch compositions -> profiles/camloss.json.

b = 16, C = 20, CAM grid 28 x 28, S = 448, three teacher scales (28, 14, 42 cells), one MI355X, all in one process:
(a) loss level: per version, forward + backward of the fused form (targets / label map given) and of the torch composition (the refined
    full-resolution teacher probabilities / the label map given) on the same device tensors, interleaved in blocks of ITER calls, HIP events
    around a block; per variant the median block's ms per call with the spread over the blocks, and the peak allocated memory of a block above
    what was resident when it began;
(b) what feeds them: cam_loss_targets, the label kernel (cam_label_from_scales), and the torch label map (sum of up-sampled scales ->
    seg_refine_by_label -> max) on their own, the same way;
(c) step level: fused trainers of one seed at v1 / v2 / v3, 5 warm-up steps each (the teacher's graph is captured in the third), then
    interleaved blocks of ten steps.
A `defaults_vs_parent` entry of an existing output file (bench.py at default flags, parent commit and this one interleaved) is kept.
usage: python tools/bench_camloss.py [out=profiles/camloss.json] [nosteps]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch
from cosa_amd.utils import seg_helper as sh

B, C, G, S, SIZES = 16, 20, 28, 448, (28, 14, 42)
T, THRE = 0.01, 0.25
ITER, BLOCKS, WARM, STEP_BLOCK, STEP_BLOCKS = 20, 7, 5, 10, 5
args_cli = [a for a in sys.argv[1:] if a != "nosteps"]
out_path = args_cli[0] if args_cli else os.path.join("profiles", "camloss.json")
dev = torch.device("cuda", 0)


def timed(fn, n):
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n, torch.cuda.max_memory_allocated(dev) - resident


def interleaved(variants, n, blocks):
    """{name: callable} -> {name: median / min / max ms per call over the blocks, peak bytes above resident}"""
    for fn in variants.values():
        for _ in range(3):
            fn()
    rows = {k: [] for k in variants}
    for _ in range(blocks):
        for k, fn in variants.items():
            rows[k].append(timed(fn, n))
    return {k: {"median_ms": statistics.median(x[0] for x in r), "min_ms": min(x[0] for x in r), "max_ms": max(x[0] for x in r),
                "blocks_ms": [x[0] for x in r], "peak_above_resident_bytes": max(x[1] for x in r)} for k, r in rows.items()}


g = torch.Generator(device="cpu").manual_seed(24)
cam = torch.randn(B, C, G, G, generator=g).to(dev).requires_grad_(True)
scales = [torch.randn(2 * B, C + 1, s, s, generator=g).to(dev) for s in SIZES]
cls = (torch.rand(B, C, generator=g) < 0.1).float().to(dev)


def full_res():
    tot = None
    for s in scales:
        up = F.interpolate(s, size=(S, S), mode="bilinear", align_corners=False)
        v = up[:B] + up[B:].flip(-1)
        tot = v if tot is None else tot + v
    return tot


with torch.no_grad():
    seg_ps = sh.seg_refine_by_label(full_res(), cls, T)
    tgt = sh.cam_loss_targets(scales, cls, S, (G, G), T)
    label = sh.cam_label_from_scales(scales, cls, S, T, THRE)
    label_t = sh._cam_label_torch(seg_ps, THRE)
agree = float((label.long() == label_t).float().mean())


def fb(fn):
    def run():
        cam.grad = None
        fn().backward()
    return run


res = {"workload": f"b = {B}, C = {C}, CAM grid {G} x {G}, S = {S}, teacher scales {list(SIZES)}, T = {T}, segconf_thre = {THRE}, one MI355X",
       "calls_per_block": ITER, "blocks": BLOCKS, "label_kernel_agrees_with_torch_label_share": agree,
       "label_shares": {"ignore": float((label == 255).float().mean()), "background": float((label == 0).float().mean())}}
res["loss_forward_backward"] = interleaved({
    "v1_fused": fb(lambda: sh.cam_loss_from_targets(cam, tgt)), "v1_torch": fb(lambda: sh.cam_loss(cam, seg_ps)),
    "v2_fused": fb(lambda: sh.cam_lossv2_from_targets(cam, tgt)),
    "v2_torch": fb(lambda: sh._cam_lossv2_torch(cam, F.interpolate(seg_ps[:, 1:], size=[G, G], mode="bilinear", align_corners=False))),
    "v3_fused": fb(lambda: sh.cam_lossv3(cam, label)), "v3_torch": fb(lambda: sh._cam_lossv3_torch(cam, label_t))}, ITER, BLOCKS)
print(json.dumps(res["loss_forward_backward"]), flush=True)
with torch.no_grad():
    res["targets_and_labels"] = interleaved({
        "cam_loss_targets": lambda: sh.cam_loss_targets(scales, cls, S, (G, G), T),
        "cam_label_from_scales": lambda: sh.cam_label_from_scales(scales, cls, S, T, THRE),
        "cam_label_from_scales_after_softmax": lambda: sh.cam_label_from_scales(scales, cls, S, T, THRE, True),
        "torch_full_res_refine_and_label": lambda: sh._cam_label_torch(sh.seg_refine_by_label(full_res(), cls, T), THRE)}, ITER, BLOCKS)
print(json.dumps(res["targets_and_labels"]), flush=True)
del seg_ps, label_t
torch.cuda.empty_cache()

if "nosteps" not in sys.argv:
    batch = synthetic_batch(B, S, C, dev, seed=1234)
    trainers = {v: CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, camloss_version=v), dev, seed=0) for v in ("v1", "v2", "v3")}
    n_iter = trainers["v1"].args.warmup_iters + 1
    for tr in trainers.values():
        assert tr.fused_losses
        for _ in range(WARM):
            tr.step(*batch, n_iter)
    steps = {v: (lambda tr=tr: tr.step(*batch, n_iter)) for v, tr in trainers.items()}
    rows = {v: [] for v in steps}
    for _ in range(STEP_BLOCKS):
        for v, fn in steps.items():
            rows[v].append(timed(fn, STEP_BLOCK))
    res["step_ms"] = {v: {"median": statistics.median(x[0] for x in r), "min": min(x[0] for x in r), "max": max(x[0] for x in r),
                          "blocks": [x[0] for x in r], "img_per_s": B / (statistics.median(x[0] for x in r) * 1e-3),
                          "peak_above_resident_bytes": max(x[1] for x in r)} for v, r in rows.items()}
    res["step_blocks"], res["block_steps"], res["warm_up_steps"] = STEP_BLOCKS, STEP_BLOCK, WARM
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
if os.path.exists(out_path):                # bench.py's parent / this figures at default flags are entered by hand: keep them
    with open(out_path) as fh:
        kept = json.load(fh)
    for key in ("defaults_vs_parent", "measured_errors"):
        if kept.get(key) is not None:
            res[key] = kept[key]
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
