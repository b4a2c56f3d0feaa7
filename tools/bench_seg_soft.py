"""What the soft-label seg loss costs -> profiles/seg_soft.json.  One MI355X:
(a) with parent=<dir of a built checkout of the parent commit>: `bench.py --gpus 1` at default flags (the term off), parent and this tree in
    interleaved processes, RUNS each, before this process opens the device -> `off_vs_parent` (images/s per run; "inside" says whether this
    tree's median lies inside the parent's own min..max, or above its median);
(b) kernel times at b = 16 x 448^2 with the teacher's scales (1, 0.5, 1.5) of the 16-pixel-patch encoder (28, 14, 42 cells a side), at K = 21
    (VOC) and K = 81 (COCO), three present classes per image, full boxes: cosa_seg_soft_forward / _backward beside cosa_seg_loss_forward_w /
    _backward_w on the same student logits (two label maps, the regulariser's outputs and inputs included: the yardstick does the same
    student-side work), the four taking turns block by block; and the soft pair again with ONE scale, which shows the teacher taps' share;
(c) the training step at b = 16 x 448^2 with the term off and on (weight 0.1, T 1, no gate): two fused trainers of one seed, WARM warm-up
    steps each, then interleaved blocks of ten steps.
usage: python tools/bench_seg_soft.py [out=profiles/seg_soft.json] [parent=DIR] [nosteps]"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ITER, BLOCKS, WARM, STEP_BLOCK, STEP_BLOCKS, RUNS = 20, 7, 5, 10, 5, 3
cli = [a for a in sys.argv[1:] if a != "nosteps" and not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out_path = cli[0] if cli else os.path.join(ROOT, "profiles", "seg_soft.json")
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

import ctypes                                                           # noqa: E402
import torch                                                            # noqa: E402
from cosa_amd import _C                                                 # noqa: E402
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch          # noqa: E402

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


def blocks_of(fns, n=ITER, blocks=BLOCKS):
    """{name: fn} -> {name: median / min / max ms per call}; the functions take turns block by block"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    ms = {k: [] for k in fns}
    for _ in range(blocks):
        for k, fn in fns.items():
            ms[k].append(timed(fn, n))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}


def kernels_at(K):
    B, S, hs, ths = 16, 448, 28, (28, 14, 42)
    L, p = _C.lib(), _C.ptr
    g = torch.Generator().manual_seed(30 + K)
    labels = torch.zeros(B, K - 1)
    for b in range(B):
        labels[b, torch.randperm(K - 1, generator=g)[:3]] = 1
    labels = labels.to(dev)
    seg = torch.randn(B, K, hs, hs, generator=g).to(dev)
    scales = [(torch.randn(2 * B, K, n, n, generator=g) * 2).to(dev) for n in ths]
    box = torch.tensor([[0, S, 0, S]] * B, dtype=torch.int32, device=dev)
    # the yardstick's inputs: two label maps of the present classes, background and ignore
    present = [[0] + (torch.nonzero(labels[b])[:, 0] + 1).tolist() + [255] for b in range(B)]
    masks = [torch.stack([torch.tensor(present[b], dtype=torch.float32)[torch.randint(0, 5, (S // 8, S // 8), generator=g)]
                          .repeat_interleave(8, 0).repeat_interleave(8, 1) for b in range(B)]).contiguous().to(dev) for _ in range(2)]
    simg = torch.randn(B, 3, S, S, generator=g).to(dev)
    AS = (torch.randn(B, K, S // 2, S // 2, generator=g) * 1e4).to(dev)
    sums8, sums4, loss, grad = torch.empty(8, device=dev), torch.empty(4, device=dev), torch.empty(1, device=dev), torch.empty_like(seg)
    s_seg, s_img = torch.empty((B, K, S // 2, S // 2), device=dev), torch.empty((B, 3, S // 2, S // 2), device=dev)
    roi, unl = torch.empty((B, S // 2, S // 2), device=dev), torch.empty((B, S // 2, S // 2), device=dev, dtype=torch.uint8)
    gs, gr = torch.tensor([0.1], device=dev), torch.tensor([0.05e-7], device=dev)
    ws = _C.workspace(max(L.cosa_seg_loss_workspace_bytes(B, K, hs, hs), L.cosa_seg_soft_workspace_bytes(B, K, hs, hs)), dev, "bench_seg_soft")
    fargs = (p(seg), p(masks[0]), p(masks[1]), p(simg), p(box), p(sums8), p(s_seg), p(s_img), p(roi), p(unl), B, K, hs, hs, S, p(ws), ws.numel(),
             _C.stream_ptr())
    bargs = (p(seg), p(masks[0]), p(masks[1]), p(sums8), p(AS), p(roi), p(gs), p(gr), p(grad), 0.25, 0.25, 0.25, 0.25, B, K, hs, hs, S, p(ws), ws.numel(),
             _C.stream_ptr())

    def soft(n):
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in scales[:n]])
        hh = _C.int_array([t.shape[2] for t in scales[:n]])
        head = (p(seg), ptrs, hh, hh, n, p(labels), p(box))
        tail = (B, K, hs, hs, S, 1.0, 0.0, 0.5, p(ws), ws.numel(), _C.stream_ptr())
        return (lambda: _C.check(L.cosa_seg_soft_forward(*head, p(sums4), p(loss), *tail), "soft_fwd"),
                lambda: _C.check(L.cosa_seg_soft_backward(*head, p(sums4), p(gs), p(grad), *tail), "soft_bwd"))
    (f3, b3), (f1, b1) = soft(3), soft(1)
    out = {"forward": blocks_of({"seg_loss_w": lambda: _C.check(L.cosa_seg_loss_forward_w(*fargs), "fwd_w"), "seg_soft": f3, "seg_soft_one_scale": f1})}
    _C.check(L.cosa_seg_loss_forward_w(*fargs), "fwd_w")       # (the yardstick's backward reads its own forward's sums)
    bw = blocks_of({"seg_loss_w": lambda: _C.check(L.cosa_seg_loss_backward_w(*bargs), "bwd_w")})
    f3()
    bw.update(blocks_of({"seg_soft": b3}))
    f1()
    bw.update(blocks_of({"seg_soft_one_scale": b1}))
    out["backward"] = bw
    for d in ("forward", "backward"):
        out[d]["soft_over_seg_loss"] = out[d]["seg_soft"]["median_ms"] / out[d]["seg_loss_w"]["median_ms"]
        out[d]["teacher_taps_share_of_soft"] = 1.0 - out[d]["seg_soft_one_scale"]["median_ms"] / out[d]["seg_soft"]["median_ms"]
    out["shape"] = {"B": B, "K": K, "S": S, "student": hs, "teacher_scales": list(ths), "present_classes": 3}
    return out


res["kernels"] = {}
for K in (21, 81):
    res["kernels"]["K%d" % K] = kernels_at(K)
    print(json.dumps({"K%d" % K: res["kernels"]["K%d" % K]}), flush=True)

if "nosteps" not in sys.argv:
    B, S = 16, 448
    batch = synthetic_batch(B, S, 20, dev, seed=1234)
    trainers = {"off": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B), dev, seed=0),
                "on": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, seg_soft_weight=0.1), dev, seed=0)}
    n_iter = trainers["off"].args.warmup_iters + 1
    last = {}
    for k_, tr in trainers.items():
        for _ in range(WARM):
            last[k_] = tr.step(*batch, n_iter)
    steps = {k_: (lambda tr=tr: tr.step(*batch, n_iter)) for k_, tr in trainers.items()}
    rows = {k_: [] for k_ in steps}
    for _ in range(STEP_BLOCKS):
        for k_, fn in steps.items():
            rows[k_].append(timed(fn, STEP_BLOCK))
    med = {k_: statistics.median(r) for k_, r in rows.items()}
    res["step_ms"] = {k_: {"median": med[k_], "min": min(r), "max": max(r), "blocks": r, "img_per_s": B / (med[k_] * 1e-3)} for k_, r in rows.items()}
    res["step_ms"]["term_cost_ms"] = med["on"] - med["off"]
    res["step_ms"]["term_share_of_on_step"] = (med["on"] - med["off"]) / med["on"]
    res["step_ms"]["soft_loss_at_last_warm_up_step"] = float(last["on"]["soft_loss"])
    res["step_blocks"], res["block_steps"], res["warm_up_steps"] = STEP_BLOCKS, STEP_BLOCK, WARM

if os.path.exists(out_path):                # a part not measured in this call keeps its earlier figures
    with open(out_path) as fh:
        kept = json.load(fh)
    for key in ("off_vs_parent", "step_ms"):
        if key not in res and kept.get(key) is not None:
            res[key] = kept[key]
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
