"""Rate of prediction export next to evaluate() on the same loader.

    python tools/bench_export.py --mode evaluate|seg|all_crf|pseudo|pseudo_par|refine_time|given|predicted|predicted_overlay|camheat|kernel_time \
        [--writers N] [--items 200] [--out FILE]

One mode per process (run each under its own time limit); the result is merged into the JSON file under the key `evaluate` or
`<mode>_w<writers>`.  The loader is synthetic: `--items` images of VOC-like sizes (around 375 x 500, both orientations) with two
present classes each, a seeded ViT-B/16 CoSA network at crop_size 448.  evaluate() is the comparison point: the same forward, the label
maps folded into confusion matrices on the device instead of being copied out and encoded.
`pseudo` (seg,pseudo,pseudo_aux) and `pseudo_par` (seg,pseudo_par,pseudo_aux_par) are the pair that shows what PAR refinement costs an
export run.  `refine_time` is no export run: the device time per image of `seg_helper.export_refine` (both CAM sets) against the generic
way to the same two maps -- two `_cam2mask_generic(..., refine_model=PAR(...))` calls on resized, validated CAMs -- interleaved in one
process after warm-up, HIP events around each call, median over `--reps` repetitions per size.
`given`, `predicted` and `predicted_overlay` are `seg` with the class row given, taken from the model's own head, and that plus the
overlay product; `kernel_time` times `cosa_predict_classes` and `cosa_export_overlay` alone.
`camheat` is seg,camheat,panel: per item two heat maps and two four-column panels on top of `seg`."""
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


def refine_time(reps, warmup=5):
    """per size: median device ms of the fused path and of the generic path, same inputs, calls interleaved"""
    import torch.nn.functional as F
    from cosa_amd.models.PAR import PAR
    from cosa_amd.utils import seg_helper, torch_helper
    par = PAR(num_iter=seg_helper.PAR_NUM_ITER, dilations=list(seg_helper.PAR_DILATIONS))
    C, S, hi, lo = 20, 448, 0.7, 0.25
    rng = np.random.default_rng(0)
    rows = []
    for (H, W) in sorted(set(SIZES)):
        img01 = torch_helper.denormalize_img(torch.from_numpy(rng.standard_normal((1, 3, H, W)).astype(np.float32)).cuda())
        cam, aux = (torch.from_numpy(rng.random((C, S, S), dtype=np.float32)).cuda() for _ in range(2))
        cls = torch.zeros(C, device="cuda")
        cls[[3, 11]] = 1
        rec = torch.empty(seg_helper.export_record_layout(C, H, W, 2, PAR_WHAT)[1], device="cuda", dtype=torch.uint8)

        def fused():
            return seg_helper.export_refine(img01, cam, aux, cls, PAR_WHAT, hi, lo, out=rec, k_live=2)

        def generic():
            out = []
            for c in (cam, aux):
                v = cls[None, :, None, None] * F.interpolate(c[None], size=(H, W), mode="bilinear", align_corners=False)
                out.append(seg_helper._cam2mask_generic(img01, [[0, H, 0, W]], v, cls[None], hi, lo, par, 255, 2))
            return out

        times = {"fused": [], "generic": []}
        for r in range(warmup + reps):
            for name, fn in (("fused", fused), ("generic", generic)):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                if r >= warmup:
                    times[name].append(a.elapsed_time(b))
        f, g = float(np.median(times["fused"])), float(np.median(times["generic"]))
        rows.append({"H": H, "W": W, "fused_ms": f, "generic_ms": g, "ratio": g / f, "fused_ms_min_max": [min(times["fused"]), max(times["fused"])],
                     "generic_ms_min_max": [min(times["generic"]), max(times["generic"])]})
    return {"reps": reps, "warmup": warmup, "C": C, "S": S, "present": 2, "downscale": 2, "sizes": rows,
            "fused_ms_mean_of_medians": float(np.mean([r["fused_ms"] for r in rows])),
            "generic_ms_mean_of_medians": float(np.mean([r["generic_ms"] for r in rows])),
            "ratio_of_means": float(np.mean([r["generic_ms"] for r in rows]) / np.mean([r["fused_ms"] for r in rows])),
            "note": "device time between HIP events on the launch stream; the generic path's host-side Python (torch.nonzero, .tolist) "
                    "waits for the device inside the interval, as it does in use"}


def kernel_time(reps, warmup=10):
    """median device ms of the two kernels of label-free export at the sizes an export run gives them: the class rows of one group
    (G = 4 images, C = 20) and the overlay of one image per VOC-like size"""
    from cosa_amd.utils import seg_helper
    rng = np.random.default_rng(0)

    def timed(fn):
        ts = []
        for r in range(warmup + reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= warmup:
                ts.append(a.elapsed_time(b))
        return {"median_ms": float(np.median(ts)), "min_ms": float(min(ts)), "max_ms": float(max(ts))}

    logits = torch.from_numpy(rng.standard_normal((4, 20)).astype(np.float32) - 2).cuda()
    out = seg_helper.predict_classes(logits)
    res = {"reps": reps, "warmup": warmup, "predict_classes_G4_C20": timed(lambda: seg_helper.predict_classes(logits, 0.5, 1, out=out)),
           "predict_classes_G4_C20_cls_min20": timed(lambda: seg_helper.predict_classes(logits - 50, 0.5, 20, out=out)), "overlay": [],
           "note": "HIP events around the Python wrapper on the launch stream: launch overhead included"}
    for (H, W) in sorted(set(SIZES)):
        img = torch.from_numpy(rng.standard_normal((3, H, W)).astype(np.float32)).cuda()
        seg = torch.from_numpy(rng.integers(0, 21, (H, W)).astype(np.uint8)).cuda()
        rgb = torch.empty(3 * H * W, device="cuda", dtype=torch.uint8)
        res["overlay"].append(dict(timed(lambda: seg_helper.export_overlay(img, seg, 0.5, out=rgb)), H=H, W=W, bytes_moved=H * W * (12 + 1 + 3)))
    return res


PAR_WHAT = ("pseudo_par", "pseudo_aux_par")
EXPORT_MODES = {"seg": (("seg",), False), "all_crf": (ALL, True), "pseudo": (("seg", "pseudo", "pseudo_aux"), False),
                "pseudo_par": (("seg",) + PAR_WHAT, False),
                # where the class row comes from: `given` is `seg` with the argument spelled out
                "camheat": (("seg", "camheat", "panel"), False),         # the CAM pictures
                "given": (("seg",), False), "predicted": (("seg",), False), "predicted_overlay": (("seg", "overlay"), False)}
CLASSES = {"given": "given", "predicted": "predicted", "predicted_overlay": "predicted"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("evaluate",) + tuple(EXPORT_MODES) + ("refine_time", "kernel_time"), required=True)
    ap.add_argument("--reps", type=int, default=30, help="refine_time: timed repetitions per size")
    ap.add_argument("--writers", type=int, default=4)
    ap.add_argument("--items", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "r08_export.json"))
    opt = ap.parse_args()
    from cosa_amd import evaluation_engine as ee
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    if opt.mode == "refine_time":
        res = refine_time(opt.reps)
        res["device"] = torch.cuda.get_device_name(0)
        merge(opt.out, "refine_time", res)
        return
    if opt.mode == "kernel_time":
        res = kernel_time(opt.reps)
        res["device"] = torch.cuda.get_device_name(0)
        merge(opt.out, "kernel_time", res)
        return
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
            what, crf = EXPORT_MODES[opt.mode]
            kw = {"classes": CLASSES[opt.mode]} if opt.mode in CLASSES else {}
            ee.export_predictions(model, warm, args, os.path.join(tmp, "warm"), what=what, getcrf=crf, writers=opt.writers, **kw)
            res = ee.export_predictions(model, items, args, os.path.join(tmp, "run"), what=what, getcrf=crf, writers=opt.writers, **kw)
            res["writers"], key = opt.writers, f"{opt.mode}_w{opt.writers}"
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    res["device"] = torch.cuda.get_device_name(0)
    merge(opt.out, key, res)


def merge(path, key, res):
    doc = {}
    if os.path.exists(path):
        with open(path) as f:
            doc = json.load(f)
    doc[key] = res
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({key: res}), flush=True)


if __name__ == "__main__":
    main()
