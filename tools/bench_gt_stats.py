"""What --gt_stats true adds to a training step, next to what --label_stats true adds -> profiles/gt_stats.json.

Three trainers of one seed at b = 16 x 448^2, K = 21: flags off, --gt_stats true, --label_stats true (the yardstick: the same upsample-argmax
pass over the student's logits, one map fewer).  Synthetic batches plus a synthetic uint8 ground truth (32 x 32 patches of the classes,
runs of 255; the kernel alone also on 4 x 4 patches, where a wavefront meets some twenty classes at once).  The method of tools/bench_loss_flags.py: after 5 warm-up steps each (the teacher's graph is captured in the third), the trainers
are interleaved in one process in blocks of ten steps, six blocks each; HIP events around a block; per trainer the median block's ms per
step and the spread over the blocks.  Then the two kernels alone, 50 launches each between a pair of events: cosa_gt_stats on the last
step's own tensors (and at COCO's K = 81, the global-atomics path, on synthetic ones), cosa_augment_labels on 16 maps of 375 x 500.
usage: python tools/bench_gt_stats.py [out=profiles/gt_stats.json]"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from cosa_amd import _C
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch
from cosa_amd.utils import seg_helper

WARM, BLOCK, BLOCKS, REPS = 5, 10, 6, 50
S, K, B = 448, 21, 16
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "gt_stats.json")
dev = torch.device("cuda", 0)


def synthetic_gt(b, s, k, seed, cell=32):
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, k, (b, s // cell, s // cell), generator=g).repeat_interleave(cell, 1).repeat_interleave(cell, 2).to(torch.uint8)
    gt[:, ::9, s // 8:s // 2] = 255
    return gt.to(dev)


def block(tr, batch, n_iter, kw):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(BLOCK):
        tr.step(*batch, n_iter, **kw)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / BLOCK


def kernel_ms(fn):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS


res = {"workload": f"b = {B} x {S}^2, VOC12 (K = {K}), vit_base_patch16_224, teacher fp16x3 (captured), one MI355X",
       "warm_up_steps": WARM, "block_steps": BLOCK, "blocks": BLOCKS, "kernel_launches_timed": REPS}
batch = synthetic_batch(B, S, K - 1, dev, seed=1234)
gt = synthetic_gt(B, S, K, 99)
flags = {"off": {}, "gt_stats": dict(gt_stats=True), "label_stats": dict(label_stats=True)}
trainers = {tag: CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, **f), dev, seed=0) for tag, f in flags.items()}
kws = {tag: (dict(gt=gt) if tag == "gt_stats" else {}) for tag in flags}
n_iter = trainers["off"].args.warmup_iters + 1
seen = []
plain = trainers["gt_stats"].update_gt_stats
trainers["gt_stats"].update_gt_stats = lambda *a: (seen.append(a), plain(*a))[1]          # the step's own tensors, for the kernel alone
for tag, tr in trainers.items():
    for _ in range(WARM):
        tr.step(*batch, n_iter, **kws[tag])
torch.cuda.synchronize()
rows = {tag: [] for tag in trainers}
for _ in range(BLOCKS):
    for tag, tr in trainers.items():
        rows[tag].append(block(tr, batch, n_iter, kws[tag]))
res["step_ms"] = {tag: {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "blocks": ms} for tag, ms in rows.items()}
med = {tag: res["step_ms"][tag]["median"] for tag in rows}
res["added_ms_per_step"] = {"gt_stats": med["gt_stats"] - med["off"], "label_stats": med["label_stats"] - med["off"]}
res["spread_of_off_ms"] = res["step_ms"]["off"]["max"] - res["step_ms"]["off"]["min"]
res["gt_summary_of_the_run"] = {k: v for k, v in trainers["gt_stats"].gt_stats().items() if k in ("steps", "pix", "valid_frac")}

# the kernels alone
a = [t.detach().contiguous().float() if torch.is_tensor(t) and t.dtype != torch.uint8 else t for t in seen[-1]]
counters = seg_helper.new_gt_stats(K, dev)
res["kernel_ms"] = {"cosa_gt_stats_K21_lds": kernel_ms(lambda: seg_helper.gt_stats(*a, counters))}
speckled = synthetic_gt(B, S, K, 98, cell=4)
res["kernel_ms"]["cosa_gt_stats_K21_lds_4x4_patches"] = kernel_ms(lambda: seg_helper.gt_stats(speckled, *a[1:], counters))
ls_counters = seg_helper.new_label_stats(K, dev)
res["kernel_ms"]["cosa_label_stats_K21_no_cams"] = kernel_ms(lambda: seg_helper.label_stats(a[1], a[2], a[3], a[4], a[5], None, None, ls_counters))
K2 = 81
g = torch.Generator().manual_seed(5)
m2 = torch.randint(0, K2, (B, S // 4, S // 4), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2).float().to(dev)
seg2, cls2 = torch.randn(B, K2, S // 16, S // 16, generator=g).to(dev), torch.ones(B, K2 - 1, device=dev)
c2 = seg_helper.new_gt_stats(K2, dev)
assert _C.lib().cosa_gt_stats_uses_lds(K) == 1 and _C.lib().cosa_gt_stats_uses_lds(K2) == 0
res["kernel_ms"]["cosa_gt_stats_K81_global"] = kernel_ms(lambda: seg_helper.gt_stats(gt, m2, m2, seg2, cls2, batch[3], c2))
h, w = 375, 500
raw = torch.randint(0, 21, (B * h * w,), dtype=torch.uint8, device=dev)
maps = torch.tensor([[i * h * w, w, h] for i in range(B)], dtype=torch.int64, device=dev)
tab = torch.from_numpy(np.stack([np.stack([np.arange(S) * h // S, np.arange(S) * w // S]) for _ in range(B)]).astype(np.int32)).to(dev)
out = torch.empty(B, S, S, dtype=torch.uint8, device=dev)
L = _C.lib()
res["kernel_ms"]["cosa_augment_labels"] = kernel_ms(lambda: _C.check(L.cosa_augment_labels(_C.ptr(raw), raw.numel(), _C.ptr(maps), _C.ptr(tab), B, S, _C.ptr(out),
                                                                                              _C.stream_ptr()), "cosa_augment_labels"))
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
if os.path.exists(out_path):                # bench.py's parent / this figures at default flags are entered by hand: keep them
    with open(out_path) as fh:
        kept = json.load(fh).get("defaults_vs_parent")
    if kept is not None:
        res["defaults_vs_parent"] = kept
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
