"""What the supervised-contrastive token loss costs -> profiles/token_contrast.json.  One MI355X:
(a) with parent=<dir of a built checkout of the parent commit>: `bench.py --gpus 1` at default flags (the term off), parent and this tree in
    interleaved processes, RUNS each, before this process opens the device -> `off_vs_parent` (images/s per run; "inside" says whether this
    tree's median lies inside the parent's own min..max);
(b) kernel times: cosa_token_contrast_fwd and cosa_token_contrast_bwd on their own at b = 16, n = 784 and b = 4, n = 3136 (60 % of the tokens
    labelled over four classes, tau 0.5), HIP events around blocks of ITER calls, the median block; the products' FLOPs (forward: S = Z Z^T,
    2 B n^2 768; backward: S again and W Z, 4 B n^2 768) over the time as a share of the 157 TF/s f32-MFMA peak;
(c) the training step at b = 16 x 448^2 with the term off and on (weight 0.1, tau 0.5, purity 1.0): two fused trainers of one seed, WARM
    warm-up steps each, then interleaved blocks of ten steps; the term's cost in ms and as a share of the on step; cosa_token_labels on
    its own at that size.
usage: python tools/bench_token_contrast.py [out=profiles/token_contrast.json] [parent=DIR] [nosteps]"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F32_MFMA = 157e12
ITER, BLOCKS, WARM, STEP_BLOCK, STEP_BLOCKS, RUNS = 20, 7, 5, 10, 5, 3
cli = [a for a in sys.argv[1:] if a != "nosteps" and not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out_path = cli[0] if cli else os.path.join(ROOT, "profiles", "token_contrast.json")
res = {}


def bench_once(tree):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10"], cwd=tree, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed in {tree}: {r.stderr[-2000:]}")
    return float(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])["value"])


if parent is not None:                      # (a), before torch opens the device here
    rows = {"parent": [], "this": []}
    for _ in range(RUNS):
        for name, tree in (("parent", parent), ("this", ROOT)):
            rows[name].append(bench_once(tree))
            print(name, rows[name][-1], flush=True)
    med = {k: statistics.median(v) for k, v in rows.items()}
    res["off_vs_parent"] = {"command": "bench.py --gpus 1 --steps 50 --warmup 10, interleaved processes", "images_per_s": rows, "median": med,
                            "parent_spread": [min(rows["parent"]), max(rows["parent"])],
                            "inside": min(rows["parent"]) <= med["this"] <= max(rows["parent"]) or med["this"] >= med["parent"]}

import torch                                                            # noqa: E402
from cosa_amd import _C                                                 # noqa: E402
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch          # noqa: E402
from cosa_amd.utils import seg_helper as sh                             # noqa: E402

dev = torch.device("cuda", 0)


def timed(fn, n):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def blocks_of(fn, n=ITER, blocks=BLOCKS):
    for _ in range(3):
        fn()
    ms = [timed(fn, n) for _ in range(blocks)]
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


res["kernels"] = {}
L = _C.lib()
for B, n in ((16, 784), (4, 3136)):
    g = torch.Generator().manual_seed(28)
    x = torch.randn(B, n, 768, generator=g).to(torch.bfloat16).to(dev)
    y = torch.randint(0, 4, (B, n), generator=g)
    y[torch.rand(B, n, generator=g) > 0.6] = 255
    y = y.to(torch.uint8).to(dev)
    rows = torch.empty((2, B, n), device=dev)
    counts = torch.empty(B * 256 + 1, device=dev, dtype=torch.int32)
    loss, up, dx = torch.empty(1, device=dev), torch.ones(1, device=dev), torch.empty_like(x)
    ws = _C.workspace(L.cosa_token_contrast_workspace_bytes(B, n), dev, "token_contrast")
    fwd = lambda: _C.check(L.cosa_token_contrast_fwd(_C.ptr(x), _C.ptr(y), _C.ptr(rows), _C.ptr(counts), _C.ptr(loss), B, n, 768, 0.5, _C.ptr(ws),
                                                     ws.numel(), _C.stream_ptr()), "fwd")
    bwd = lambda: _C.check(L.cosa_token_contrast_bwd(_C.ptr(x), _C.ptr(y), _C.ptr(rows), _C.ptr(counts), _C.ptr(up), _C.ptr(dx), B, n, 768, 0.5,
                                                     _C.ptr(ws), ws.numel(), _C.stream_ptr()), "bwd")
    entry = {"forward": blocks_of(fwd), "backward": blocks_of(bwd), "anchors": int(counts[-1]), "loss": float(loss),
             "workspace_bytes": int(ws.numel())}
    flops = 2.0 * B * n * n * 768
    entry["forward"].update(flops=flops, share_of_f32_mfma_peak=flops / (entry["forward"]["median_ms"] * 1e-3) / PEAK_F32_MFMA)
    entry["backward"].update(flops=2 * flops, share_of_f32_mfma_peak=2 * flops / (entry["backward"]["median_ms"] * 1e-3) / PEAK_F32_MFMA)
    res["kernels"][f"b{B}_n{n}"] = entry
    print(json.dumps({f"b{B}_n{n}": entry}), flush=True)
    del x, y, rows, dx

mask = torch.randint(0, 21, (16, 28, 28), device=dev).repeat_interleave(16, 1).repeat_interleave(16, 2).contiguous()
res["token_labels_b16_448"] = blocks_of(lambda: sh.token_labels(mask, 16))
del mask

if "nosteps" not in sys.argv:
    B, S = 16, 448
    batch = synthetic_batch(B, S, 20, dev, seed=1234)
    trainers = {"off": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B), dev, seed=0),
                "on": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, tokcon_weight=0.1), dev, seed=0)}
    n_iter = trainers["off"].args.warmup_iters + 1
    last = {}
    for k, tr in trainers.items():
        for _ in range(WARM):
            last[k] = tr.step(*batch, n_iter)
    steps = {k: (lambda tr=tr: tr.step(*batch, n_iter)) for k, tr in trainers.items()}
    rows = {k: [] for k in steps}
    for _ in range(STEP_BLOCKS):
        for k, fn in steps.items():
            rows[k].append(timed(fn, STEP_BLOCK))
    med = {k: statistics.median(r) for k, r in rows.items()}
    res["step_ms"] = {k: {"median": med[k], "min": min(r), "max": max(r), "blocks": r, "img_per_s": B / (med[k] * 1e-3)} for k, r in rows.items()}
    res["step_ms"]["term_cost_ms"] = med["on"] - med["off"]
    res["step_ms"]["term_share_of_on_step"] = (med["on"] - med["off"]) / med["on"]
    res["step_ms"]["tok_loss_at_last_warm_up_step"] = float(last["on"]["tok_loss"])
    res["step_blocks"], res["block_steps"], res["warm_up_steps"] = STEP_BLOCKS, STEP_BLOCK, WARM

if os.path.exists(out_path):                # a part not measured in this call keeps its earlier figures
    with open(out_path) as fh:
        kept = json.load(fh)
    for key in ("off_vs_parent", "step_ms", "measured_e32"):
        if key not in res and kept.get(key) is not None:
            res[key] = kept[key]
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
