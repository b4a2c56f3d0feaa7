"""Rate of prediction export next to evaluate() on the same loader.

    python tools/bench_export.py --mode evaluate|seg|all_crf [--writers N] [--items 200] [--out profiles/r08_export.json]

One mode per process (run each under its own time limit); the result is merged into the JSON file under the key `evaluate` or
`<mode>_w<writers>`.  The loader is synthetic: `--items` images of VOC-like sizes (around 375 x 500, both orientations) with two
present classes each, a seeded ViT-B/16 CoSA network at crop_size 448.  evaluate() is the comparison point: the same forward, the label
maps folded into confusion matrices on the device instead of being copied out and encoded."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(375, 500), (500, 375), (333, 500), (375, 500), (500, 334), (281, 500), (366, 500), (375, 500)]
ALL = ("seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux")


def loader(n, C, seed=0):
    rng = np.random.default_rng(seed)
    base = []
    for H, W in SIZES:
        img = torch.from_numpy(rng.standard_normal((1, 3, H, W)).astype(np.float32))
        lab = torch.from_numpy(rng.integers(0, C + 1, (1, H, W)).astype(np.int64))
        cls = torch.zeros(1, C)
        cls[0, rng.choice(C, 2, replace=False)] = 1
        base.append((img, lab, cls))
    return [(f"item_{i:04d}",) + base[i % len(base)] for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("evaluate", "seg", "all_crf"), required=True)
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--items", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "r08_export.json"))
    opt = ap.parse_args()
    from cosa_amd import evaluation_engine as ee
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    torch.manual_seed(0)
    args = default_args("VOC12", crop_size=448, batch_size=1)
    model = build_model(args).cuda().eval()
    items = loader(opt.items, args.num_classes - 1)
    warm = items[:8]
    tmp = tempfile.mkdtemp(prefix="cosa_export_")
    try:
        if opt.mode == "evaluate":
            ee.evaluate(model, warm, args, epoch=0, getcrf=False)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ee.evaluate(model, items, args, epoch=0, getcrf=False)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            res, key = {"images": len(items), "seconds": dt, "img_per_s": len(items) / dt}, "evaluate"
        else:
            what, crf = (("seg",), False) if opt.mode == "seg" else (ALL, True)
            ee.export_predictions(model, warm, args, os.path.join(tmp, "warm"), what=what, getcrf=crf, writers=opt.writers)
            res = ee.export_predictions(model, items, args, os.path.join(tmp, "run"), what=what, getcrf=crf, writers=opt.writers)
            res["writers"], key = opt.writers, f"{opt.mode}_w{opt.writers}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res["device"] = torch.cuda.get_device_name(0)
    doc = {}
    if os.path.exists(opt.out):
        with open(opt.out) as f:
            doc = json.load(f)
    doc[key] = res
    os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({key: res}), flush=True)


if __name__ == "__main__":
    main()
