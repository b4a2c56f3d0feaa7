"""What the torch path of the dense losses costs at non-default loss flags, and whether it is reproducible
-> profiles/r15_loss_flags.json.

Per flag setting (--segfg_alpha 0.3, and the same with --after_softmax true) two trainers of one seed at b = 16 x 448^2, K = 21: one with
`fused_losses=False` (the op-by-op torch path every non-default setting took before) and the fused one.
(a) step time: after 5 warm-up steps each (the teacher's graph is captured in the third), the two are interleaved in one process in blocks of
    ten steps, six blocks each; HIP events around a block; per trainer the median block's ms per step and the spread over the blocks; peak
    allocated memory of a block, absolute and above what was allocated when the block began (both trainers are resident throughout);
(b) reproducibility: on the fresh trainers, three forward + backward passes on the same weights and batch; how many parameters' gradients
    differ in any bit from the first pass, and the largest difference (the weight gradients are formed from bf16 operands, which hide
    most last-bit differences of d loss / d seg_pred).  A finding, not an assertion.
A `defaults_vs_parent` entry of an existing output file (bench.py at default flags, parent commit and this one interleaved) is kept.
usage: python tools/bench_loss_flags.py [out=profiles/r15_loss_flags.json]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd import nn_ops
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch

WARM, BLOCK, BLOCKS, PASSES = 5, 10, 6, 3
S, K, B = 448, 21, 16
SETTINGS = {"segfg_alpha_0.3": dict(segfg_alpha=0.3), "segfg_alpha_0.3_after_softmax": dict(segfg_alpha=0.3, after_softmax=True)}
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r15_loss_flags.json")
dev = torch.device("cuda", 0)


def gradient_passes(tr, batch, n_iter):
    """PASSES x (forward, backward) without an optimizer step -> per pass {name: gradient clone}"""
    runs = []
    for _ in range(PASSES):
        tr.optimizer.zero_grad(set_to_none=True)
        loss, _ = tr.forward_losses(*batch, n_iter)
        nn_ops.wgrad_arena_begin(dev)
        loss.backward()
        runs.append({n: p.grad.detach().clone() for n, p in tr.student.named_parameters() if p.grad is not None})
    torch.cuda.synchronize()
    return runs


def differing(runs):
    bits = lambda t: t.reshape(-1).view(torch.uint8)
    names = [n for n in runs[0] if any(not torch.equal(bits(r[n]), bits(runs[0][n])) for r in runs[1:])]
    worst = max((float((r[n].float() - runs[0][n].float()).abs().max()) for n in names for r in runs[1:]), default=0.0)
    top = max(float(g.float().abs().max()) for g in runs[0].values())
    return {"parameters": len(runs[0]), "parameters_differing_in_any_bit": len(names), "max_abs_difference": worst, "max_abs_gradient": top,
            "examples": names[:6]}


def block(tr, batch, n_iter):
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(BLOCK):
        tr.step(*batch, n_iter)
    b.record()
    b.synchronize()
    peak = torch.cuda.max_memory_allocated(dev)
    return a.elapsed_time(b) / BLOCK, peak, peak - resident


res = {"workload": f"b = {B} x {S}^2, VOC12 (K = {K}), vit_base_patch16_224, teacher fp16x3 (captured), one MI355X",
       "warm_up_steps": WARM, "block_steps": BLOCK, "blocks": BLOCKS, "gradient_passes": PASSES, "settings": {}}
batch = synthetic_batch(B, S, K - 1, dev, seed=1234)
for name, flags in SETTINGS.items():
    trainers = {"torch_path": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, fused_losses=False, **flags), dev, seed=0),
                "fused": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, **flags), dev, seed=0)}
    assert trainers["fused"].fused_losses and not trainers["torch_path"].fused_losses
    n_iter = trainers["fused"].args.warmup_iters + 1
    entry = {"flags": flags, "reproducibility": {}, "step_ms": {}}
    for tag, tr in trainers.items():
        entry["reproducibility"][tag] = differing(gradient_passes(tr, batch, n_iter))
    for tr in trainers.values():
        for _ in range(WARM):
            tr.step(*batch, n_iter)
    torch.cuda.synchronize()
    rows = {tag: [] for tag in trainers}
    for _ in range(BLOCKS):
        for tag, tr in trainers.items():
            rows[tag].append(block(tr, batch, n_iter))
    for tag, r in rows.items():
        ms = [x[0] for x in r]
        entry["step_ms"][tag] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "blocks": ms,
                                 "img_per_s": B / (statistics.median(ms) * 1e-3), "peak_allocated_bytes": max(x[1] for x in r),
                                 "peak_above_resident_bytes": max(x[2] for x in r)}
    entry["torch_path_over_fused"] = entry["step_ms"]["torch_path"]["median"] / entry["step_ms"]["fused"]["median"]
    res["settings"][name] = entry
    print(name, json.dumps(entry), flush=True)
    del trainers, tr
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
if os.path.exists(out_path):                # bench.py's parent / this figures at default flags are entered by hand: keep them
    with open(out_path) as fh:
        kept = json.load(fh).get("defaults_vs_parent")
    if kept is not None:
        res["defaults_vs_parent"] = kept
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
