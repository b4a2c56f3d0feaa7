"""Training-step throughput of one encoder at the benchmark's shape (bench.py measures ViT-B/16 and stays as it is):

    python tools/bench_backbone.py [--backbone dino_base_patch8_224] [--crop 448] [--batch 16] [--steps 20] [--warmup 3]

The default training step (captured teacher in the trainer's default operand mode, own kernels end to end) on a synthetic batch; every timed
step is closed by a device synchronisation.  Prints one JSON line: img/s, ms/step (mean, median, min), peak device memory."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbone", default="dino_base_patch8_224")
    ap.add_argument("--crop", type=int, default=448)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--teacher-precision", default="auto")
    opt = ap.parse_args()
    assert opt.steps >= 1 and opt.warmup >= 2, "the first two steps capture the teacher graph"
    import torch
    from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch
    dev = torch.device("cuda", 0)
    args = default_args("VOC12", backbone=opt.backbone, crop_size=opt.crop, batch_size=opt.batch, teacher_precision=opt.teacher_precision)
    tr = CoSATrainer(args, dev, seed=0)
    wimg, simg, lab, box = synthetic_batch(opt.batch, opt.crop, 20, dev, seed=1)
    n_iter = args.warmup_iters + 1
    for i in range(opt.warmup):
        tr.step(wimg, simg, lab, box, n_iter + i)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    times = []
    for i in range(opt.steps):
        t0 = time.perf_counter()
        logs = tr.step(wimg, simg, lab, box, n_iter + opt.warmup + i)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    losses = {k: float(logs[k]) for k in ("seg_loss", "cam_loss", "reg_loss", "cls_loss")}
    ms = sorted(1e3 * t for t in times)
    mean = sum(ms) / len(ms)
    print(json.dumps({"backbone": opt.backbone, "crop": opt.crop, "batch": opt.batch, "teacher_precision": args.teacher_precision,
                      "steps": opt.steps, "warmup": opt.warmup, "img_per_s": round(opt.batch * 1e3 / mean, 2), "ms_per_step": round(mean, 2),
                      "ms_median": round(ms[len(ms) // 2], 2), "ms_min": round(ms[0], 2),
                      "peak_mem_gib": round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2), "teacher_graph": tr._graph is not None,
                      "graph_error": tr.graph_error, "losses_finite": all(v == v and abs(v) != float("inf") for v in losses.values())}))


if __name__ == "__main__":
    main()
