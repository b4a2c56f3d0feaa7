"""What the reliability-weighted seg loss costs -> profiles/seg_reliability.json.  One MI355X:
(a) with parent=<dir of a built checkout of the parent commit>: `bench.py --gpus 1` at default flags (the switch off), parent and this tree in
    interleaved processes, RUNS each, before this process opens the device -> `off_vs_parent` (images/s per run; "inside" says whether this
    tree's median lies inside the parent's own min..max);
(b) the weight kernel's accuracy at tests/test_seg_reliability_gpu.py's middle shape (B, C, S) = (3, 20, 37): per power beta and floor the
    largest error e32 of the numpy-float32 formula against float64 and the kernel's own (tests/seg_weight_ref.py) -> `measured_e32`;
(c) kernel times at b = 16 x 448^2, C = 20 (K = 21), two present classes per image: cosa_label_reliability for G = 2 on its own, with the bytes
    it must move (per set and pixel: the label, the weight, one plane per present class; 4 bytes each) over the 8.0 TB/s HBM peak and the
    6.3 TB/s a float4 copy reaches; cosa_seg_loss_forward_rw / _backward_rw against _w, the pairs taking turns block by block;
(d) the training step at b = 16 x 448^2 with the switch off and on (beta 1, floor 0): two fused trainers of one seed, WARM warm-up steps each,
    then interleaved blocks of ten steps.
usage: python tools/bench_seg_reliability.py [out=profiles/seg_reliability.json] [parent=DIR] [nosteps]"""
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12
ITER, BLOCKS, WARM, STEP_BLOCK, STEP_BLOCKS, RUNS = 20, 7, 5, 10, 5, 3
cli = [a for a in sys.argv[1:] if a != "nosteps" and not a.startswith("parent=")]
parent = next((a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("parent=")), None)
out_path = cli[0] if cli else os.path.join(ROOT, "profiles", "seg_reliability.json")
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

import numpy as np                                                      # noqa: E402
import torch                                                            # noqa: E402
import seg_weight_ref as R                                              # noqa: E402
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


# (b) the weight kernel against its restatements
rng = np.random.default_rng(29)
B, C, S = 3, 20, 37
cam = rng.uniform(0, 1, (B, C, S, S)).astype(np.float32)
y = np.zeros((B, C), np.float32)
y[1, :] = 1
y[2, [3, 11]] = 1
mask = rng.choice(np.array([0, 1, 2, 4, 12, C, 255], np.float32), size=(B, S, S)).astype(np.float32)
t = lambda a: torch.from_numpy(a).to(dev)
res["measured_e32"] = {"shape_BCS": [B, C, S], "thresholds": [0.7, 0.25], "rows": []}
for beta in (0.5, 2.0, 8.0):
    for floor in (0.0, 0.25):
        w = sh.label_reliability([t(cam)], t(y), [t(mask)], [0.7], [0.25], beta=beta, floor=floor)[0].cpu().numpy().astype(np.float64)
        w64 = R.weight_f64(cam, y, mask, 0.7, 0.25, beta, floor)
        e32 = float(np.abs(R.weight_f32(cam, y, mask, 0.7, 0.25, beta, floor).astype(np.float64) - w64).max())
        res["measured_e32"]["rows"].append({"beta": beta, "floor": floor, "e32": e32, "kernel": float(np.abs(w - w64).max()),
                                            "bar": 4 * e32 + 2.0 ** -24})
print(json.dumps(res["measured_e32"]), flush=True)

# (c) kernels at the workload's size
B, C, S, hs = 16, 20, 448, 28
K = C + 1
g = torch.Generator().manual_seed(29)
labels = torch.zeros(B, C)
for b in range(B):
    labels[b, torch.randperm(C, generator=g)[:2]] = 1
labels = labels.to(dev)



def smooth_cams():
    """CAM-like planes: 28 x 28 noise up-sampled to the crop and stretched to [0, 1] per plane (noise at full resolution would leave
    cam2mask's half-resolution argmax almost nothing but ignored pixels, whose threads read no plane)"""
    c = torch.nn.functional.interpolate(torch.rand(B, C, hs, hs, generator=g), size=(S, S), mode="bilinear", align_corners=False)
    lo_, hi_ = c.amin(dim=(2, 3), keepdim=True), c.amax(dim=(2, 3), keepdim=True)
    return ((c - lo_) / (hi_ - lo_)).contiguous().to(dev)


cams = [smooth_cams() for _ in range(2)]
masks = sh.cam2mask_multi(torch.zeros(B, 3, S, S, device=dev), torch.tensor([[0, S, 0, S]] * B), cams, labels, [0.7, 0.7], [0.25, 0.25],
                          _fold_validation=True)          # (no refine model: the image is not read)
stats = sh.new_reliability_stats(2, dev)
rel = sh.label_reliability(cams, labels, masks, [0.7, 0.7], [0.25, 0.25], stats=stats)
summary = sh.reliability_summary(stats)
labelled = sum(s_["n_bg"] + s_["n_fg"] for s_ in summary) / (2.0 * B * S * S)
bytes_moved = 2 * B * S * S * 4 * (2 + 2)            # per set and pixel: label + weight + two present planes
arr = lambda ts: (ctypes.c_void_p * 2)(*[t_.data_ptr() for t_ in ts])
thr = (ctypes.c_float * 2)(0.7, 0.7), (ctypes.c_float * 2)(0.25, 0.25)
raw_args = (arr(cams), _C.ptr(labels), arr(masks), arr(rel), thr[0], thr[1], None, 2, B, C, S, 1.0, 0.0, _C.ptr(stats), _C.stream_ptr())
raw = lambda: _C.check(_C.lib().cosa_label_reliability(*raw_args), "cosa_label_reliability")          # (the entry point alone: no allocation)
k = blocks_of({"label_reliability_G2": raw})["label_reliability_G2"]
k.update(bytes=bytes_moved, labelled_share=labelled, ms_at_hbm_peak=bytes_moved / HBM_PEAK * 1e3, ms_at_hbm_copy_rate=bytes_moved / HBM_COPY * 1e3,
         share_of_hbm_peak=bytes_moved / (k["median_ms"] * 1e-3) / HBM_PEAK, share_of_hbm_copy_rate=bytes_moved / (k["median_ms"] * 1e-3) / HBM_COPY,
         mean_weights=summary)
res["kernels"] = {"label_reliability_G2": k}
print(json.dumps(res["kernels"]), flush=True)

L = _C.lib()
seg = torch.randn(B, K, hs, hs, generator=g).to(dev)
simg = torch.randn(B, 3, S, S, generator=g).to(dev)
box = torch.tensor([[0, S, 0, S]] * B, dtype=torch.int32, device=dev)
AS = (torch.randn(B, K, S // 2, S // 2, generator=g) * 1e4).to(dev)
sums, grad = torch.empty(8, device=dev), torch.empty_like(seg)
s_seg, s_img = torch.empty((B, K, S // 2, S // 2), device=dev), torch.empty((B, 3, S // 2, S // 2), device=dev)
roi, unl = torch.empty((B, S // 2, S // 2), device=dev), torch.empty((B, S // 2, S // 2), device=dev, dtype=torch.uint8)
gs, gr = torch.tensor([0.1], device=dev), torch.tensor([0.05e-7], device=dev)
ws = _C.workspace(L.cosa_seg_loss_workspace_bytes(B, K, hs, hs), dev, "seg_loss")
p = _C.ptr
fargs = (p(seg), p(masks[0]), p(masks[1]), p(simg), p(box), p(sums), p(s_seg), p(s_img), p(roi), p(unl), B, K, hs, hs, S, p(ws), ws.numel(), _C.stream_ptr())
bargs = (p(seg), p(masks[0]), p(masks[1]), p(sums), p(AS), p(roi), p(gs), p(gr), p(grad), 0.25, 0.25, 0.25, 0.25, B, K, hs, hs, S, p(ws), ws.numel(),
         _C.stream_ptr())
tail = (p(rel[0]), p(rel[1]))
res["kernels"]["seg_loss_forward"] = blocks_of({"w": lambda: _C.check(L.cosa_seg_loss_forward_w(*fargs), "fwd_w"),
                                                "rw": lambda: _C.check(L.cosa_seg_loss_forward_rw(*fargs, *tail), "fwd_rw")})
res["kernels"]["seg_loss_backward"] = blocks_of({"w": lambda: _C.check(L.cosa_seg_loss_backward_w(*bargs), "bwd_w"),
                                                 "rw": lambda: _C.check(L.cosa_seg_loss_backward_rw(*bargs, *tail), "bwd_rw")})
print(json.dumps({k_: res["kernels"][k_] for k_ in ("seg_loss_forward", "seg_loss_backward")}), flush=True)
del cams, masks, rel, seg, simg, AS, s_seg, s_img

if "nosteps" not in sys.argv:
    B, S = 16, 448
    batch = synthetic_batch(B, S, 20, dev, seed=1234)
    trainers = {"off": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B), dev, seed=0),
                "on": CoSATrainer(default_args("VOC12", crop_size=S, batch_size=B, seg_reliability=True), dev, seed=0)}
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
    res["step_ms"]["switch_cost_ms"] = med["on"] - med["off"]
    res["step_ms"]["switch_share_of_on_step"] = (med["on"] - med["off"]) / med["on"]
    res["step_ms"]["seg_loss_at_last_warm_up_step"] = {k_: float(v["seg_loss"]) for k_, v in last.items()}
    res["step_ms"]["mean_weights"] = trainers["on"].seg_reliability()
    res["step_blocks"], res["block_steps"], res["warm_up_steps"] = STEP_BLOCKS, STEP_BLOCK, WARM

if os.path.exists(out_path):                # a part not measured in this call keeps its earlier figures
    with open(out_path) as fh:
        kept = json.load(fh)
    for key in ("off_vs_parent", "step_ms", "loss_kernels_ab"):
        if key not in res and kept.get(key) is not None:
            res[key] = kept[key]
os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
with open(out_path, "w") as fh:
    json.dump(res, fh, indent=1)
print(json.dumps(res))
