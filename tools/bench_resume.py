"""What a full-state checkpoint costs on one MI355X -> profiles/r10_resume.json.

(a) state capture: the snapshot and restore launches (HIP events, 5 warm-up + 30 timed, median) as GB/s of 2 x state bytes, and interleaved in
    the same process the state-gathering work of the torch route -- the per-tensor .detach().cpu() copies torch_helper.save_best makes,
    extended to all state -- WITHOUT torch.save's file write (wall clock around a synchronised block);
(b) step time: the training step of tools/step_only.py (b = 16 x 448^2) in interleaved blocks of 10 steps without a save, with one
    save_state per block, and with the complete torch route (copies + torch.save) per block; the run-to-run spread of the no-save blocks
    is the yardstick.
usage: python tools/bench_resume.py [out=profiles/r10_resume.json] [blocks=6] [dir=<tmp>]"""
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch

HBM_PEAK_GBS = 8000.0
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join("profiles", "r10_resume.json")
blocks = int(sys.argv[2]) if len(sys.argv) > 2 else 6
work = sys.argv[3] if len(sys.argv) > 3 else tempfile.mkdtemp(prefix="cosa_resume_")
dev = torch.device("cuda", 0)
args = default_args("VOC12", crop_size=448, batch_size=16, keep_states=2)
tr = CoSATrainer(args, dev, seed=0)
batch = synthetic_batch(16, 448, 20, dev, seed=1234)
n_iter = args.warmup_iters + 1
for _ in range(4):
    tr.step(*batch, n_iter)
st = tr.train_state()
st._ensure_buffers()
torch.cuda.synchronize()


def timed_launch(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def torch_gather():
    """the copies of the torch route: every state tensor through .detach().cpu()"""
    t0 = time.perf_counter()
    sd = {n: t.detach().cpu() for n, t in zip(st.names, st.tensors)}
    return (time.perf_counter() - t0) * 1e3, sd


snap, verify, scatter, gather = [], [], [], []
arena, sums = st._arenas[0], st._sums[0]
for i in range(35):
    s_ms = timed_launch(lambda: st._table.snapshot(arena, sums))
    v_ms = timed_launch(lambda: st._table.restore(arena, sums, False))
    r_ms = timed_launch(lambda: st._table.restore(arena, sums, True))       # (writes back the bytes just taken: the state is unchanged)
    g_ms = torch_gather()[0] if i % 5 == 0 or i >= 30 else None             # the torch route is ~1000x slower: sampled, not run 35 times
    if i >= 5:
        snap.append(s_ms), verify.append(v_ms), scatter.append(r_ms)
    if g_ms is not None and i >= 5:
        gather.append(g_ms)
gbs = lambda ms, passes: round(passes * st.state_bytes / (ms * 1e-3) / 1e9, 1)
part_a = {"state_bytes": st.state_bytes, "tensors": len(st.tensors), "hbm_peak_GBs": HBM_PEAK_GBS,
          "snapshot_ms": round(statistics.median(snap), 4), "snapshot_GBs_of_2x_state": gbs(statistics.median(snap), 2),
          "verify_ms": round(statistics.median(verify), 4), "verify_GBs_of_1x_state": gbs(statistics.median(verify), 1),
          "restore_ms": round(statistics.median(scatter), 4), "restore_GBs_of_2x_state": gbs(statistics.median(scatter), 2),
          "torch_cpu_copies_ms": round(statistics.median(gather), 2), "torch_cpu_copies_samples": len(gather)}


def block(kind, idx):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        tr.step(*batch, n_iter)
    if kind == "state":
        tr.save_state(os.path.join(work, f"state_{idx:08d}.cosa"), n_iter=idx)
    elif kind == "torch":
        torch.save({"state": torch_gather()[1]}, os.path.join(work, "torch_route.pth"))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e2            # ms per step


res = {"none": [], "state": [], "torch": []}
for i in range(blocks):
    for kind in ("none", "state", "torch"):
        res[kind].append(block(kind, i + 1))
tr.wait_state()
med = {k: statistics.median(v) for k, v in res.items()}
part_b = {"steps_per_block": 10, "blocks": blocks, "ms_per_step_no_save": round(med["none"], 3),
          "no_save_spread_ms": round(max(res["none"]) - min(res["none"]), 3),
          "ms_per_step_save_state_every_10": round(med["state"], 3), "ms_per_step_torch_route_every_10": round(med["torch"], 3),
          "save_state_overhead_ms_per_step": round(med["state"] - med["none"], 3),
          "torch_route_overhead_ms_per_step": round(med["torch"] - med["none"], 3),
          "per_block_ms_per_step": {k: [round(v, 3) for v in vs] for k, vs in res.items()}}
for f in os.listdir(work):
    if f.startswith("state_") or f == "torch_route.pth":
        os.remove(os.path.join(work, f))
report = {"device": torch.cuda.get_device_name(0), "capture": part_a, "step": part_b}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(report, f, indent=1)
print(json.dumps(report))
