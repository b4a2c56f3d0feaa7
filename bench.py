#!/usr/bin/env python
"""bench.py -- training images/sec of the CoSA hot path on N MI355X GPUs (one process per GPU, RCCL).

    python bench.py --gpus 1 --steps 10 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one full training iteration (main.py:106-252): teacher 3 scales x 2 flips forward,
student forward+backward, CAM -> label maps (x2), the five losses incl. the bilateral dense-energy
regulariser, AdamW, EMA -- on one synthetic batch per rank, post-warm-up loss
weights so every loss is live.  Workload = BASELINE.json configs[1]: VOC 21-class, ViT-B bf16,
batch 16 x 448 x 448 per GPU (weak scaling).

The headline `value` is measured in the trainer's default mode -- the cheapest teacher-operand mode with no failed plane on the committed
accuracy record under the pre-registered criterion (`conformance()` below; since round 6: fp16x3, hi + lo fp16 halves and three MFMA terms per
product), student on an fp32 residual stream: with --full, `tolerance_met` is read from that record and confirmed in the run.  `fast_mode` = the
same step with the bf16-operand teacher of configs[1] read literally (faster, out of tolerance); `other_modes`: fp16c8-x2 (round 5's default:
25 % faster, fails the float64-bounded exemption on planes of conditioning > 100), uniform fp16c8, bf16x3.

Rank 0 prints ONE JSON line: the headline (`metric`, `value`, `unit`, `higher_is_better`, `dtype`, `ms_per_step`) and the run's `config`.
A plain run does nothing else: set-up, W warm-up steps, K timed steps, the line.  With --full the line also carries, among others:
  roofline      the dominant hand-written kernel, device-clock spans of its launches inside the timed steps
  tolerance_met the accuracy record of the benchmarked mode and the in-run check (`accuracy_vs_fp32_cpu_oracle`, `accuracy_live`)
  par_refine, bilateral, vit_forward, teacher_attention, evaluation, input_pipeline   stand-alone timings of their own
  fast_mode, other_modes   the same step with other teacher-operand modes (N=1 only)
  cpu_baseline  the CPU oracle's step on a bounded sample (N=1 only), timed on the host cores
--dump-outputs DIR writes what the last timed step computed as DIR/<name>.npy (dump_outputs below).
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FLOP_PER_IMG_448 = 1.782e12        # teacher 1282.9 G + student fwd+bwd 498.9 G
PEAK_BF16 = 2.5e15                 # dense bf16 MFMA peak (MI355X_MICROARCH.md)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50, help="timed steps (SURVEY d-1: >= 50)")
    ap.add_argument("--warmup", type=int, default=10, help="untimed warm-up steps (SURVEY d-1: >= 10)")
    ap.add_argument("--batch", type=int, default=16, help="per-GPU batch (BASELINE configs[1]: 16)")
    ap.add_argument("--crop", type=int, default=448)
    ap.add_argument("--dataset", default="VOC12", choices=["VOC12", "COCO"])
    ap.add_argument("--usepar", action="store_true", help="PAR(T=10, 6 dilations) as cam2mask's refine_model")
    ap.add_argument("--usegmm", action="store_true", help="adaptive thresholds: 3-component mixture fitted to the CAM queue every step")
    ap.add_argument("--full", action="store_true",
                    help="measure everything beyond the headline as well: kernel rooflines, the accuracy record and in-run check, PAR / bilateral / "
                         "evaluation / input-pipeline timings, the other teacher-operand modes and the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32; at most 64 MB)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--teacher-precision", default="auto", type=_mode_arg,
                    metavar="{auto,bf16,fp16,bf16x3,fp16x3,fp16c8[-N[mK]|-xN[mK]],fp16c4[...]}",
                    help="MFMA operand precision of the teacher's no-grad passes in the HEADLINE run (DESIGN.md section 3).  The default (`auto`) is the "
                         "cheapest mode with no failed plane on the committed accuracy record under the pre-registered criterion of "
                         "tests/test_precision_gpu.py (literal normalised-CAM bar 1e-3; float64-bounded exemption above conditioning 50; pooled mask "
                         "mIoU >= 0.999; >= 64 draws): train_step.resolve_teacher_precision; "
                         "`bf16` is BASELINE configs[1] read literally and does not meet it (measured beside the headline as `fast_mode`)")
    ap.add_argument("--no-secondary", "--no-parity-grade", dest="no_secondary", action="store_true",
                    help="with --full: skip the secondary measurements (`fast_mode`: bf16-operand teacher; `other_modes`)")
    ap.add_argument("--student-stream", default="fp32", choices=["fp32", "bf16"],
                    help="residual stream of the student's training path: fp32 like the reference (default) or the bf16 stream of rounds 1-3")
    ap.add_argument("--defer-groups", type=int, default=0,
                    help="weight gradients of the student's blocks in this many batched launches (0: the trainer's choice -- 1 on one GPU, 6 under "
                         "data parallelism so that the gradient buckets fill while the backward pass is still running)")
    ap.add_argument("--grid-policy", type=int, default=-1, choices=[-1, 0, 1],
                    help="persistent-GEMM grid under DDP: 1 = balanced over the rounds (leaves CUs to RCCL's channels; the trainer's default when "
                         "world > 1), 0 = full grid, -1 = the trainer's choice; lets the first multi-GPU run A/B the policy")
    ap.add_argument("--teacher-sync", action="store_true",
                    help="replay the teacher graph on the main stream (default: on a side stream, overlapping the student's forward); "
                         "kernel spans in `roofline` are then undisturbed by co-running kernels")
    ap.add_argument("--cpu-batch", type=int, default=2, help="batch of the CPU-baseline sample (configs[0]: 2)")
    ap.add_argument("--cpu-steps", type=int, default=5, help="timed CPU-baseline steps after one warm-up step (BASELINE.md: >= 5)")
    opt = ap.parse_args()
    if opt.teacher_precision == "auto":          # the trainer's rule (train_step.resolve_teacher_precision; margins: DESIGN.md section 3)
        sys.path.insert(0, ROOT)
        from cosa_amd.train_step import resolve_teacher_precision
        opt.teacher_precision = resolve_teacher_precision("auto", opt.crop, opt.usepar)
    return opt


def newest_profile(name):
    """newest committed summary profiles/rNN_<name> (the evidence files are named per round)"""
    for rnd in range(9, 0, -1):
        f = os.path.join(ROOT, "profiles", f"r{rnd:02d}_{name}")
        if os.path.exists(f):
            return f
    return None


TEACHER_CSRC = ("gemm_kernels.hip", "attn_kernels.hip", "split_kernels.hip", "vit_kernels.hip", "label_kernels.hip", "c4.hpp", "c8.hpp",
                "op16.hpp", "common.hpp", "kernels.hpp")          # (= tests/test_precision_gpu.py:TEACHER_CSRC; tests/test_boundary.py checks)
TEACHER_HOST = ("build.py", "models/vit.py")          # compiler flags and the block -> operand-format map are part of "the kernels the record was taken with"


def teacher_csrc_hash():
    import hashlib
    h = hashlib.sha256()
    for f in TEACHER_CSRC:
        h.update(open(os.path.join(ROOT, "cosa_amd", "csrc", f), "rb").read())
    for f in TEACHER_HOST:
        h.update(open(os.path.join(ROOT, "cosa_amd", f), "rb").read())
    return h.hexdigest()[:16]


# the pre-registered conformance criterion (= the constants at the top of tests/test_precision_gpu.py; tests/test_boundary.py checks they agree)
CAM_BAR, COND_MAX, FP64_FACTOR, AGREE_BAR, MIOU_BAR, MIN_DRAWS = 1e-3, 50.0, 4.0, 0.999, 0.999, 64


def parse_accuracy_record(path):
    """lines of an accuracy record (tests/test_precision_gpu.py:_check_teacher) -> (rows, csrc hash).  Round-6 lines carry the per-plane
    bookkeeping (`| planes N literal-ok L exempt E fail F [...]`) and the confusion counts (`| conf class:tp/fp/fn,...`)."""
    import re
    rows, rec_hash = [], None
    pat = re.compile(r"teacher (\S+)\s+S=(\d+) b=(\d+) seed=(\d+)\s+(\S+)\s*: normalised-CAM rel err (\S+)\s+label agreement (\S+)\s+mask mIoU (\S+)"
                     r"(?:\s+own-scale err (\S+)\s+worst conditioning (\S+))?(?:\s+\| planes (\d+) literal-ok (\d+) exempt (\d+) fail (\d+)([^|]*)\| conf (\S*))?")
    for ln in open(path):
        if ln.startswith("#") and "csrc_sha256_16=" in ln:
            rec_hash = ln.split("csrc_sha256_16=")[1].split()[0]
        m = pat.match(ln)
        if not m:
            continue
        r = dict(mode=m.group(1), S=int(m.group(2)), b=int(m.group(3)), seed=int(m.group(4)), set=m.group(5), rel=float(m.group(6)),
                 agree=float(m.group(7)), iou=float(m.group(8)), own=float(m.group(9)) if m.group(9) else None,
                 cond=float(m.group(10)) if m.group(10) else None, planes=None)
        if m.group(11) is not None:
            r.update(planes=int(m.group(11)), literal_ok=int(m.group(12)), exempt=int(m.group(13)), fail=int(m.group(14)), notes=m.group(15).strip(),
                     conf={int(c): [int(x) for x in v.split("/")] for c, v in (e.split(":") for e in m.group(16).split(",") if e)})
        rows.append(r)
    return rows, rec_hash


def pooled_miou(conf):
    """{class: [tp, fp, fn]} summed over draws -> (mean IoU over the classes the oracle's masks contain, min class IoU) -- the reference's
    scoring (utils/evaluation.py:17-35: one confusion matrix over the set, iu = diag / (row + col - diag), mean over the rows that are present)"""
    ious = [v[0] / (v[0] + v[1] + v[2]) for v in conf.values() if v[0] + v[2] > 0]
    return (sum(ious) / len(ious), min(ious)) if ious else (1.0, 1.0)


def conformance(mode, crop):
    """Does teacher-operand mode `mode` meet BASELINE.json's tolerance ("1e-3 relative on fp32 CAMs ... mask IoU >= 0.999") at this crop?  Read
    from the newest committed profiles/rNN_accuracy_teacher.txt (written on the GPU by tests/test_precision_gpu.py: fused HIP teacher vs the fp32
    CPU oracle, which asserts the same rule per draw), by the criterion PRE-REGISTERED at the top of that test file:
      (a) every active (image, class) plane: max |delta| of the min-max NORMALISED plane <= 1e-3 (the literal bar), or
      (b) -- only for a plane whose conditioning (class-logit magnitude / what the normalisation divides by, from the oracle) is > 50 -- the
          exemption: own-scale err <= 1e-3 AND |HIP - float64 oracle| <= 1e-3 + 4 x |fp32 oracle - float64 oracle| on that plane;
      (c) label agreement >= 0.999 on every draw, and mask mIoU >= 0.999 from ONE confusion matrix pooled over all draws (per CAM set), the way
          the reference scores IoU (utils/evaluation.py:17-35); the per-draw minimum is reported as a diagnostic;
      (d) at least 64 draws of the mode on record (8 at this crop).
    `planes_exempt` / `planes_failed` count the planes that took (b) / failed it.  The record names the sources it was taken with (sha256 over the
    teacher's kernel files, the build flags and the block -> format map): a record of another tree does not count."""
    f = newest_profile("accuracy_teacher.txt")
    if f is None:
        return {"tolerance_met": False, "note": "no committed accuracy file"}
    rows_all, rec_hash = parse_accuracy_record(f)
    rows_mode = [r for r in rows_all if r["mode"] == mode]
    rows = [r for r in rows_mode if r["S"] == crop]
    if not rows:
        return {"tolerance_met": False, "note": f"no line for mode {mode} at S={crop} in {os.path.basename(f)}"}
    if any(r["planes"] is None for r in rows):
        return {"tolerance_met": False, "note": f"{os.path.basename(f)} predates the pre-registered criterion (no per-plane bookkeeping): re-take the record"}
    draws, draws_mode = {(r["seed"], r["b"]) for r in rows}, {(r["S"], r["seed"], r["b"]) for r in rows_mode}
    pooled = {}
    for r in rows:
        acc = pooled.setdefault(r["set"], {})
        for c, v in r["conf"].items():
            acc[c] = [x + y for x, y in zip(acc.get(c, [0, 0, 0]), v)]
    pm = {k: pooled_miou(v) for k, v in pooled.items()}
    failed = [f"seed {r['seed']} b={r['b']} {r['set']}: {r['notes']}" for r in rows if r["fail"]]
    out = {"planes": sum(r["planes"] for r in rows), "planes_exempt": sum(r["exempt"] for r in rows), "planes_failed": sum(r["fail"] for r in rows),
           "normalised_cam_rel_err_max": max(r["rel"] for r in rows),
           "normalised_cam_rel_err_max_non_exempt": max([r["rel"] for r in rows if not r["exempt"] and not r["fail"]] or [0.0]),
           "cam_rel_err_own_scale_max": max(r["own"] for r in rows), "worst_conditioning": max(r["cond"] for r in rows),
           "label_agreement_min": min(r["agree"] for r in rows),
           "mask_miou_pooled": {k: round(v[0], 6) for k, v in pm.items()}, "mask_iou_pooled_min_class": {k: round(v[1], 6) for k, v in pm.items()},
           "mask_miou_per_draw_min": min(r["iou"] for r in rows),
           "draws": len(draws), "draws_all_crops": len(draws_mode), "lines": len(rows), "seeds": len({r["seed"] for r in rows}),
           "batch_sizes": sorted({r["b"] for r in rows})}
    ok = (out["planes_failed"] == 0 and out["label_agreement_min"] >= AGREE_BAR and min(v[0] for v in pm.values()) >= MIOU_BAR
          and len(draws_mode) >= MIN_DRAWS and len(draws) >= 8)
    out = {"tolerance_met": bool(ok), **out,
           "bars": f"per plane: normalised-CAM |delta| <= {CAM_BAR:g}, or (conditioning > {COND_MAX:g}: own-scale err <= {CAM_BAR:g} and |HIP - fp64| <= {CAM_BAR:g} + "
                   f"{FP64_FACTOR:g} x |fp32 - fp64|); label agreement >= {AGREE_BAR} per draw; pooled-confusion mask mIoU >= {MIOU_BAR}; >= {MIN_DRAWS} draws "
                   "(pre-registered: tests/test_precision_gpu.py)",
           "source": "profiles/" + os.path.basename(f) + " (tests/test_precision_gpu.py, fused HIP teacher vs fp32 / float64 CPU oracle)"}
    if failed:
        out["failed_planes"] = failed[:8]
    out["kernels_match_record"] = rec_hash == teacher_csrc_hash()
    if not out["kernels_match_record"]:
        out["tolerance_met"] = False
        out["note"] = f"the accuracy record was taken with another tree (source hash {rec_hash}, tree {teacher_csrc_hash()}): re-run tools/accuracy_evidence.sh"
    return out


def usable_cores():
    """host cores this process may really use: min(affinity mask, cgroup CPU quota, the pool's 16-core share per GPU box)"""
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, min(n, int(os.environ.get("COSA_CPU_THREADS", "16"))))


def cpu_baseline(opt, state_dict, C):
    """one step of the CPU oracle at configs[0] (b=2, 448^2, fp32) on all host cores"""
    from oracle import c_oracle
    from oracle.cpu_step import CpuStep
    from cosa_amd.train_step import synthetic_batch
    c_oracle.build()
    cores = usable_cores()
    torch.set_num_threads(cores)
    sd = {k: v.detach().float().cpu() for k, v in state_dict.items()}
    step = CpuStep(sd, num_classes=C + 1, aux_layer=-4 if opt.dataset == "VOC12" else -3,
                   args=dict(max_iters=32000 if opt.dataset == "VOC12" else 60000, par=([1, 2, 4, 8, 12, 24], 10) if opt.usepar else None))
    b = opt.cpu_batch
    wimg, simg, lab, box = synthetic_batch(b, opt.crop, C, torch.device("cpu"), seed=1234, dataset=opt.dataset)
    step.step(wimg, simg, lab, box.numpy(), n_iter=10 ** 6)                      # 1 untimed warm-up step
    timers = {}
    n_steps = opt.cpu_steps
    t0 = time.perf_counter()
    for _ in range(n_steps):
        logs = step.step(wimg, simg, lab, box.numpy(), n_iter=10 ** 6, timers=timers)
    dt = time.perf_counter() - t0
    # PAR stage (second half of the metric): the four PAR(T=10, 6 dilations) calls per image (main / aux CAMs x hi / lo) on the same
    # sample, as the difference between the oracle's cam2mask with and without the refine model
    import numpy as np
    den = c_oracle.denormalize_img(simg.numpy())
    cams = [logs["cam_ps"].numpy(), logs["cam_aux_ps"].numpy()]
    bx = np.asarray(box.numpy(), np.int32)

    def lab_maps(par):
        t1 = time.perf_counter()
        for cm in cams:
            c_oracle.cam2mask(den, bx, cm, lab.numpy(), 0.7, 0.25, 2, par=par)
        return time.perf_counter() - t1
    t_plain, t_par = lab_maps(None), lab_maps(([1, 2, 4, 8, 12, 24], 10))
    return {"value": round(n_steps * b / dt, 4), "unit": "images/s", "cores": cores, "kind": "port",
            "sample": f"{n_steps} full training steps after 1 warm-up step, batch {b} x {opt.crop}x{opt.crop}, fp32, oracle/cpu_step.py "
                      f"({dt:.1f} s); PAR stage: oracle/cosa_oracle.c, 1 core, same sample",
            "stage_s": {k: round(v, 2) for k, v in timers.items()},
            "par_refine_ms_per_img": round((t_par - t_plain) / b * 1e3, 2), "par_cores": 1}


def par_refine_ms_per_img(trainer, simg, lab, box, dev, opt, C):
    """second half of BASELINE.json's metric: PAR refine ms/img = time of the hi+lo refinement of main+aux CAMs
    (4 PAR(T=10, dilations 1,2,4,8,12,24) calls per image at S/2) / images (SURVEY d-1), HIP events, resident inputs."""
    from cosa_amd.models.PAR import PAR
    from cosa_amd.utils import seg_helper, torch_helper
    b, S = opt.batch, opt.crop
    g = torch.Generator(device="cpu").manual_seed(7)
    cams = torch.nn.functional.interpolate(torch.rand(b, C, S // 8, S // 8, generator=g).to(dev), size=(S, S), mode="bilinear")
    cams_aux = torch.nn.functional.interpolate(torch.rand(b, C, S // 8, S // 8, generator=g).to(dev), size=(S, S), mode="bilinear")
    den = torch_helper.denormalize_img(simg)
    par = PAR(num_iter=10, dilations=[1, 2, 4, 8, 12, 24])

    def timed(refine, n=10, separate=False):
        # the training step's form: main + aux CAM sets of the same images through one pass (cam2mask_multi)
        if separate:
            f = lambda: (seg_helper.cam2mask(den, box, cams, lab, 0.7, 0.25, refine_model=refine, _fold_validation=True),
                         seg_helper.cam2mask(den, box, cams_aux, lab, 0.7, 0.25, refine_model=refine, _fold_validation=True))
        else:
            f = lambda: seg_helper.cam2mask_multi(den, box, [cams, cams_aux], lab, [0.7, 0.7], [0.25, 0.25], refine_model=refine,
                                                  _fold_validation=True)
        f()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            f()
        e.record()
        torch.cuda.synchronize()
        return a.elapsed_time(e) / n
    t0, t1 = timed(None), timed(par)
    t0s, t1s = timed(None, separate=True), timed(par, separate=True)

    # bilateral (dense-energy regulariser) ms/img: get_energy_loss forward + backward at S/2 on the same images (SURVEY d-1), and the
    # content-dependent worst case of both stages on uniform-noise images (d-2: noise inflates the lattice ~30x)
    layer = seg_helper.DenseEnergyLoss(weight=1e-7, sigma_rgb=15, sigma_xy=100, scale_factor=0.5)
    mask = torch.randint(0, C + 1, (b, S, S), generator=g).to(dev).float()

    def timed_bilateral(img, n=5):
        logit = torch.randn(b, C + 1, S, S, generator=g).to(dev).requires_grad_(True)

        def f():
            logit.grad = None                 # (as zero_grad(set_to_none=True) leaves it: the backward stores d logits, it does not add to an old one)
            loss = seg_helper.get_energy_loss(img, logit, mask, box, layer)
            loss.backward()
        for _ in range(3):                    # (allocator growth and the lattice workspace settle in the first calls)
            f()
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            f()
        e.record()
        torch.cuda.synchronize()
        return a.elapsed_time(e) / n
    tb = timed_bilateral(simg)
    noise = torch.rand(b, 3, S, S, generator=g).to(dev)
    mean = torch.tensor([123.675, 116.28, 103.53], device=dev).view(1, 3, 1, 1)
    std = torch.tensor([58.395, 57.12, 57.375], device=dev).view(1, 3, 1, 1)
    noise_norm = (noise * 255 - mean) / std
    den_keep, den = den, noise                       # `timed` closes over `den`
    t1n = timed(par, n=5)
    den = den_keep
    tbn = timed_bilateral(noise_norm, n=3)
    K = float((lab.sum(1) + 1).mean())
    s = S // 2
    alg = 4.0 * s * s * (3 + 2 * K * 10) * 4 * b            # bytes of the 4 PAR calls per image (main/aux x hi/lo), BASELINE.md §2
    per_pass = (t1 - t0) * 1e-3
    # bilateral (dense-energy regulariser) roofline, SURVEY d-3: compulsory I/O 4 (S/2)^2 (3 + 2 K) bytes per image (image once, K planes in
    # and out) over the forward + backward time; the lattice's own gather / scatter traffic is reported from the committed PMC passes
    comp = 4.0 * s * s * (3 + 2 * (C + 1))
    bil = {"fwd_bwd_ms_per_img": round(tb / b, 5), "noise_images_fwd_bwd_ms_per_img": round(tbn / b, 5),
           "roofline": {"bound": "hbm", "achieved": round(comp * b / (tb * 1e-3) / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                        "frac": round(comp * b / (tb * 1e-3) / 8e12, 5), "compulsory_MB_per_img": round(comp / 1e6, 2), "traffic": None,
                        "note": "gather / scatter through a hashed 5-D lattice: bound by the hash insertions (64-bit CAS, build) and random row "
                                "gathers (sorted splat, blur, slice), not by the compulsory bytes; no float atomics: the output is "
                                "bit-identical to the reference's"}}
    try:
        f = newest_profile("lattice_pmc.json")
        pmc = json.load(open(f))
        bil["roofline"]["traffic"] = pmc.get("hbm_bytes_per_forward_backward")
        bil["roofline"]["traffic_source"] = "profiles/" + os.path.basename(f)
    except Exception:
        pass
    par_traffic = None
    try:
        f = newest_profile("par_pmc.json")
        pmc = json.load(open(f))
        par_traffic = {"hbm_bytes_per_pass": pmc["hbm_bytes_per_pass"], "algorithmic_bytes_per_pass": pmc["algorithmic_bytes_per_pass"],
                       "ratio": round(pmc["hbm_bytes_per_pass"] / pmc["algorithmic_bytes_per_pass"], 2), "source": "profiles/" + os.path.basename(f)}
    except Exception:
        pass
    return {"bilateral": bil, "ms_per_img": round((t1 - t0) / b, 5), "cam2mask_no_par_ms_per_img": round(t0 / 2 / b, 5), "mean_K": round(K, 2),
            "separate_calls_ms_per_img": round((t1s - t0s) / b, 5),
            "bilateral_fwd_bwd_ms_per_img": round(tb / b, 5),
            "noise_images": {"par_ms_per_img": round((t1n - t0) / b, 5), "bilateral_fwd_bwd_ms_per_img": round(tbn / b, 5)},
            "roofline": {"bound": "hbm", "achieved": round(alg / per_pass / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
                         "frac": round(alg / per_pass / 8e12, 4), "algorithmic_MB_per_pass": round(alg / 1e6, 1), "traffic": par_traffic,
                         "note": "one pass = 4 PAR calls per image (main/aux CAMs x hi/lo thresholds), affinities shared"}}


def input_pipeline_images_per_s(dev, batch, crop):
    """SURVEY f-2: the training input pipeline (scale / flip / crop / blur / one-of-9 strong ops / normalise, Pillow-exact) on the
    device, from decoded VOC-sized uint8 images to (wimg, simg, img_box); wall clock including host packing and the H2D copy."""
    import random
    import numpy as np
    from cosa_amd.dataloaders import DeviceAugmenter, draw_params
    rng = np.random.default_rng(0)
    images = []
    for i in range(batch):
        h, w = [(375, 500), (500, 375), (333, 500), (500, 500)][i % 4]
        small = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
        images.append(np.ascontiguousarray(np.kron(small, np.ones((8, 8, 1), np.uint8))[:h, :w]))      # blocky 8x8 upsample
    random.seed(0)
    np.random.seed(0)
    params = [draw_params(im.shape[0], im.shape[1], crop_size=crop) for im in images]
    aug = DeviceAugmenter(crop, dev)
    for _ in range(3):
        aug(images, params)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        aug(images, params)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 20
    return {"images_per_s": round(batch / dt, 1), "ms_per_batch": round(dt * 1e3, 3), "batch": batch,
            "sample": "decoded 375x500-class uint8 images, all draws as the reference"}


def vit_forward_roofline(trainer, wimg, dev, crop):
    """north_star: ">= 40 % of CDNA4 bf16 MFMA peak on the ViT-B forward": the network forward alone (encoder + LargeFOV + heads,
    no gradients) on the teacher's scale-1.0 batch (images + flips) at the crop size, HIP events over 10 passes; 166.3 GFLOP per image
    at 448^2 (387.3 at 640^2)."""
    flop_img = {448: 166.3e9, 640: 387.3e9, 224: 37.5e9}.get(crop)
    if flop_img is None:
        return None
    x = torch.cat([wimg, wimg.flip(-1)], 0)
    net = trainer.model_AN
    with torch.no_grad():
        for _ in range(3):
            net(x)
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            net(x)
        e.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(e) / 10
    # issued MFMA work per algorithmic flop: bf16x3 3 terms everywhere; fp16c8 25 / 12 K-tiles in the projections (85 % of the forward's
    # flops at N = 785), attention 1x
    # fp16c4: qkv / fc1 / fc2 (per block 171 + 228 + 219 of 693 tile-units) at 19 / 12 resp. 73 / 48 tiles, proj at 25 / 12: 693 / 432 overall
    mult = {"bf16x3": 3.0, "fp16c8": 0.854 * 25 / 12 + 0.146, "fp16c4": 0.854 * 693 / 432 + 0.146}.get(trainer.model_AN.encoder.precision, 1.0)
    if trainer.model_AN.encoder.precision in ("fp16c8", "fp16c4") and trainer.model_AN.encoder.c8_plain_from is not None:
        pa, pm = trainer.model_AN.encoder._plain_from()
        frac8 = (pa + 2 * pm) / 36.0              # (an MLP half is two thirds of a block's projection work)
        mult = frac8 * mult + (1.0 - frac8)
    enc_ = trainer.model_AN.encoder
    if enc_.precision == "fp16c8" and enc_.c4_from is not None:          # mixed maps: the late blocks' qkv / fc1 / fc2 on fp16c4 operands
        fc = max(0, len(enc_.blocks) - enc_.c4_from) / len(enc_.blocks)
        mult = (1.0 - fc) * mult + fc * (0.854 * 693 / 432 + 0.146)
    xa, xm = trainer.model_AN.encoder._x3_until() if trainer.model_AN.encoder.precision in ("fp16c8", "fp16c4") else (0, 0)
    if xa or xm:                                  # mixed maps: the early blocks' halves on bf16x3 operands (3 MFMA terms)
        fx = (xa + 2 * xm) / 36.0
        mult = fx * 3.0 + (1.0 - fx) * mult
    ach = flop_img * x.shape[0] / (ms * 1e-3) / 1e12
    return {"bound": "mfma", "achieved": round(ach, 1), "peak": PEAK_BF16 / 1e12, "unit": "TFLOP/s", "frac": round(ach * 1e12 / PEAK_BF16, 4),
            "ms": round(ms, 3), "images": int(x.shape[0]), "flop_per_img": flop_img, "operands": trainer.args.teacher_precision,
            "issued_mfma_frac": round(ach * mult * 1e12 / PEAK_BF16, 4),
            "note": "algorithmic FLOPs of the fp32 reference / time; bf16x3 issues 3 MFMA terms per product, fp16c8 ~2.08 in the projections"}


def teacher_attention_roofline(dev, batch, crop, mode):
    """the attention kernel the teacher's default mode runs (attn_fwd_x3_kernel: hi + lo halves, three MFMA terms per product), stand-alone at
    the three sequence lengths of a step (B = 2 x batch images), HIP events on the launch stream; `achieved` counts ALGORITHMIC flops
    (4 N^2 64 per image and head), `issued_mfma_frac` the three terms.  (Inside the step these launches sit in the captured graph.)"""
    from cosa_amd import nn_ops
    if not mode.endswith("x3"):
        return None
    hdt = torch.float16 if mode == "fp16x3" else torch.bfloat16
    B, H, p = 2 * batch, 12, 16
    tot_fl = tot_s = 0.0
    per = {}
    for sc in (1.0, 0.5, 1.5):
        N = (int(crop * sc) // p) ** 2 + 1
        qkv = torch.randn(B * N, 3 * H * 64, device=dev) * 1.5
        qs = nn_ops.split_rows(qkv, dtype=hdt)[:, :6 * H * 64].contiguous()
        out = torch.zeros(B * N, 2 * H * 64 + 64, device=dev, dtype=hdt)
        for _ in range(3):
            nn_ops.attn_fwd_x3(qs, B, N, H, out)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(10):
            nn_ops.attn_fwd_x3(qs, B, N, H, out)
        b.record()
        torch.cuda.synchronize()
        sec = a.elapsed_time(b) * 1e-4
        fl = 4.0 * B * H * N * N * 64
        per[f"N={N}"] = {"us": round(sec * 1e6, 1), "algorithmic_TFLOPs": round(fl / sec / 1e12, 1)}
        tot_fl, tot_s = tot_fl + fl, tot_s + sec
    ach = tot_fl / tot_s / 1e12
    return {"kernel": "attn_fwd_x3_kernel (" + mode + " operands)", "bound": "mfma", "achieved": round(ach, 1), "peak": PEAK_BF16 / 1e12, "unit": "TFLOP/s",
            "frac": round(ach * 1e12 / PEAK_BF16, 4), "issued_mfma_frac": round(3 * ach * 1e12 / PEAK_BF16, 4), "launches": per,
            "ms_per_block": round(tot_s * 1e3, 3), "timer": "HIP events, stand-alone launches at the step's three sequence lengths"}


def live_accuracy_check(trainer, wimg, lab, box, n=16):
    """`tolerance_met` is read from the committed record (which must name this tree's kernel sources).  This is the same comparison made
    IN THE RUN: the teacher pass in the benchmarked mode against the bf16x3 pass (16 significant bits, on other kernels -- split-row GEMMs,
    attn_fwd_x3; 2.7e-5 from the fp32 CPU oracle on record) on the first n images of the bench batch -- CAM planes, label maps, masks.  A kernel
    regression, another ROCm or another GPU shows here.  It is a gross-error gate (`gross_error_ok`), not the tolerance: label agreement >= 0.999
    and mask mIoU over the masks of the whole batch >= 0.999; the normalised-plane figure is reported (it carries the conditioning of the planes).
    bench.py sets `tolerance_met` false when this check fails OR cannot run."""
    import numpy as np
    from cosa_amd.utils import seg_helper
    from cosa_amd.models import build_model
    args = trainer.args
    mode = args.teacher_precision
    # (a copy of the teacher: the trainer owns the 16-bit shadows and the captured graph of its own module, whose precision is fixed)
    net = build_model(args).to(wimg.device).eval()
    net.load_state_dict(trainer.model_AN.state_dict())
    x, lb, bx = wimg[:n], lab[:n], box[:n]
    res = {}
    with torch.no_grad():
        for m in (mode, "bf16x3"):
            net.set_nograd_precision(m)
            cam, cam_aux, _ = seg_helper.multi_scale_camseg(net, x, args.pseudo_scales)
            masks = [seg_helper.cam2mask(x, bx, c * lb[:, :, None, None], lb, 0.7, 0.25).cpu().numpy() for c in (cam, cam_aux)]
            res[m] = (cam.float().cpu(), cam_aux.float().cpu(), masks)
    del net
    act = lb.bool().cpu()
    out = {"vs": f"bf16x3 teacher pass, first {int(x.shape[0])} images of the bench batch", "mode": mode,
           "gate": "gross-error gate (NOT the tolerance: that is accuracy_vs_fp32_cpu_oracle): label agreement >= 0.999, mask mIoU over the batch's pooled masks >= 0.999"}
    rel, agree, iou = 0.0, 1.0, 1.0
    for k in (0, 1):
        g, o = res[mode][k], res["bf16x3"][k]
        d = (g - o).abs().amax(dim=(2, 3))
        rel = max(rel, float((d / o.abs().amax(dim=(2, 3)).clamp_min(1e-6))[act].max()))
        mg, mo = res[mode][2][k], res["bf16x3"][2][k]
        agree = min(agree, float(np.mean(mg == mo)))
        ious = []
        for c in np.union1d(np.unique(mg), np.unique(mo)):
            a_, b_ = mg == c, mo == c
            ious.append(float((a_ & b_).sum()) / float(max(1, (a_ | b_).sum())))
        iou = min(iou, float(np.mean(ious)))
    out.update({"normalised_cam_rel_err": float(f"{rel:.3e}"), "label_agreement": round(agree, 5), "mask_miou": round(iou, 5),
                "gross_error_ok": bool(agree >= 0.999 and iou >= 0.999)})
    return out


_BASE_TEXT = {
    "bf16": "bf16 operands (BASELINE configs[1] read literally; 8 significant bits)",
    "fp16": "fp16 operands (11 significant bits)",
    "bf16x3": "bf16x3 (hi + lo bf16 halves, 3 MFMA terms, fp32 accumulation: 16 significant bits)",
    "fp16x3": "fp16x3 (hi + lo fp16 halves, 3 MFMA terms, fp32 accumulation: 22 significant bits; attention included)",
    "fp16c8": "fp16c8 (fp16 x fp16 + two e5m2 correction terms on the block-scaled MFMA, fp32 accumulation; attention operands fp16, "
              "attention output fp16 + e5m2)",
    "fp16c4": "fp16c4 (fp16 x fp16 + both correction terms as FP4 (e2m1) MX blocks on the block-scaled MFMA at 4x the fp16 rate in qkv / fc1 / "
              "fc2, fp32 accumulation; output projection fp16c8, attention operands fp16)",
}


def mode_text(mode):
    """plain-words description of a teacher-operand mode string (VITNetwork.set_nograd_precision)"""
    import re
    base, _, tail = mode.partition("-")
    t = _BASE_TEXT[base]
    m = re.fullmatch(r"(\d+)(?:m(\d+))?(q?)", tail) if tail else None
    mx = re.fullmatch(r"(?:x(\d+)(?:m(\d+))?)?(?:c(\d+))?", tail) if tail and not m else None
    if m:
        a, k = int(m.group(1)), int(m.group(2)) if m.group(2) else int(m.group(1))
        t += f"; attention halves from block {a} on and MLP halves from block {k} on: plain fp16 operands" + ("; qkv projections plain fp16" if m.group(3) else "")
    if mx and mx.group(1):
        a, k = int(mx.group(1)), int(mx.group(2)) if mx.group(2) else int(mx.group(1))
        t += f"; attention halves of blocks 0-{a - 1} and MLP halves of blocks 0-{k - 1}: bf16x3 operands (hi + lo bf16 halves, 3 MFMA terms)"
    if mx and mx.group(3):
        t += f"; qkv / fc1 / fc2 of the blocks from {int(mx.group(3))} on: fp16c4 operands (FP4 MX-block correction terms)"
    return t


class _ModeText(dict):
    def __missing__(self, mode):
        return mode_text(mode)


MODE_TEXT = _ModeText()


def _mode_arg(v):
    import re
    if v == "auto" or v in _BASE_TEXT or re.fullmatch(r"fp16c[48]-(\d+(m\d+)?q?|x\d+(m\d+)?(c\d+)?|c\d+)", v):
        return v
    raise argparse.ArgumentTypeError(f"unknown teacher precision {v!r}")


def secondary_run(opt, dev, C, wimg, simg, lab, box, n_iter, mode):
    """the same training step with another teacher-operand mode, in a second trainer, timed like the headline: W untimed warm-up steps
    (at least the three calls after which the teacher pass is a hipGraph), then exactly K steps between two synchronisations"""
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args(opt.dataset, crop_size=opt.crop, batch_size=opt.batch, usepar=opt.usepar, usegmm=opt.usegmm,
                        teacher_precision=mode, teacher_async=not opt.teacher_sync)
    tr = CoSATrainer(args, dev, ddp=False, seed=0)
    configure_student(tr, opt)
    for _ in range(max(3, opt.warmup)):
        tr.step(wimg, simg, lab, box, n_iter)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(opt.steps):
        tr.step(wimg, simg, lab, box, n_iter)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / opt.steps
    out = {"teacher_operands": MODE_TEXT[mode], "images_per_s": round(opt.batch / dt, 2), "ms_per_step": round(dt * 1e3, 3),
           "steps": opt.steps, "warmup": max(3, opt.warmup), "accuracy_vs_fp32_cpu_oracle": conformance(mode, opt.crop)}
    out["tolerance_met"] = out["accuracy_vs_fp32_cpu_oracle"]["tolerance_met"]
    out["vit_forward"] = vit_forward_roofline(tr, wimg, dev, opt.crop)
    del tr
    torch.cuda.empty_cache()
    return out


def configure_student(trainer, opt):
    enc = trainer.student.encoder
    enc.residual_stream = opt.student_stream
    if opt.defer_groups > 0:
        enc.defer_groups = opt.defer_groups


def secondary_modes(opt, dev, C, wimg, simg, lab, box, n_iter):
    """`fast_mode`: the bf16-operand teacher (configs[1] literally; out of tolerance) -- or, when the headline itself is that mode, the
    conforming default; `other_modes`: round 5's default fp16c8-x2 and uniform fp16c8 (~14-bit products: faster, each with failed planes on
    record -- their own `tolerance_met` says so), fp16x3 / bf16x3 (three-term products with fp16 / bf16 halves)"""
    from cosa_amd import nn_ops
    st, gst = nn_ops.stamps, nn_ops.gemm_stamps
    nn_ops.stamps = nn_ops.gemm_stamps = None
    out = {}
    try:
        if opt.teacher_precision != "bf16":
            out["fast_mode"] = secondary_run(opt, dev, C, wimg, simg, lab, box, n_iter, "bf16")
        else:
            from cosa_amd.train_step import resolve_teacher_precision
            out["conforming_mode"] = secondary_run(opt, dev, C, wimg, simg, lab, box, n_iter, resolve_teacher_precision("auto", opt.crop, opt.usepar))
        others = [m for m in ("fp16c8-x2", "fp16c8", "fp16x3", "bf16x3") if m != opt.teacher_precision]
        out["other_modes"] = {m: {k: v for k, v in secondary_run(opt, dev, C, wimg, simg, lab, box, n_iter, m).items() if k != "vit_forward"}
                                         for m in others}
    finally:
        nn_ops.stamps, nn_ops.gemm_stamps = st, gst
    return out


def eval_images_per_s(trainer, dev, C, crop, n=20):
    """SURVEY f-1: the validation pass (batch 1, five scales x two flips, label maps + confusion matrices on the device) on synthetic
    VOC-val-shaped images with the teacher network; bounded sample."""
    import numpy as np
    from types import SimpleNamespace
    from cosa_amd import evaluation_engine as ee
    rng = np.random.default_rng(0)
    sizes = [(375, 500), (333, 500), (500, 375), (366, 500), (500, 281)]
    loader = []
    for i in range(n + 3):
        H, W = sizes[i % len(sizes)]
        cls = torch.zeros(1, C)
        cls[0, rng.choice(C, 2, replace=False)] = 1
        loader.append(("x", torch.randn(1, 3, H, W), torch.from_numpy(rng.integers(0, C + 1, (1, H, W))), cls))
    args = SimpleNamespace(num_classes=C + 1, crop_size=crop, bkg_thre=0.5)
    model = trainer.model_AN
    out = {}
    for key, grp in (("one_at_a_time", 1), ("default", 4)):               # default: four loader items share a multi-scale pass (same scores)
        ee.evaluate(model, loader[:12], args, epoch=0, eval_group=grp)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ee.evaluate(model, loader[3:], args, epoch=1, eval_group=grp)
        torch.cuda.synchronize()
        out[key] = time.perf_counter() - t0
    dt = out["default"]
    return {"images_per_s": round(n / dt, 2), "ms_per_img": round(dt / n * 1e3, 3),
            "images_per_s_one_at_a_time": round(n / out["one_at_a_time"], 2),
            "sample": f"{n} images ~375x500 from a batch-1 loader, 5 scales x 2 flips"}


DUMP_MAX_ELEMS = 1 << 22         # float32 entries per dumped array (16 MB): a larger output is written as a fixed, seeded sample
PARAM_SAMPLE = 1 << 20           # entries of the updated student parameters in the dump


def _seeded_sample(flat, n, seed):
    """n entries of the 1-D tensor `flat` at indices drawn from a CPU generator seeded with `seed`: the same for the same size and seed"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    idx = torch.randint(0, flat.numel(), (n,), generator=g).sort().values
    return flat[idx.to(flat.device)]


def dump_outputs(path, logs, student):
    """--dump-outputs: what the last timed step computed, as <path>/<name>.npy in float32 -- every tensor the step returns (the five losses
    and their sum, the label map `mask` of the main CAMs, the class logits) and `student_params_sample`, a seeded sample of the student's
    parameters after the step's AdamW update.  An array of more than DUMP_MAX_ELEMS entries is written as a seeded sample of its flattened
    values: the label map of the bench batch (16 x 448^2) is written whole, and the directory stays far below 64 MB at any batch."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    arrays = {k: v.detach() for k, v in logs.items() if torch.is_tensor(v)}
    flat = torch.cat([p.detach().reshape(-1).float() for p in student.parameters()])
    arrays["student_params_sample"] = _seeded_sample(flat, min(PARAM_SAMPLE, flat.numel()), 0)
    del flat
    for name, t in arrays.items():
        t = t.float()
        if t.numel() > DUMP_MAX_ELEMS:
            t = _seeded_sample(t.reshape(-1), DUMP_MAX_ELEMS, 1)
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())


_keep_stamp_buffers = []


def full_report(out, opt, trainer, prof, dt, ips, world, dev, C, wimg, simg, lab, box, n_iter):
    """--full: everything the line carries beyond the headline (module docstring), added to `out`"""
    from cosa_amd import nn_ops
    flop_img = FLOP_PER_IMG_448 if opt.crop == 448 else None
    # dominant hand-written kernels: the persistent projection GEMM (three epilogue instantiations of one kernel) and the
    # fused attention forward.  Their launches sit inside the teacher's hipGraph, where HIP events cannot be recorded
    # on ROCm, so every launch stamps the 100 MHz device clock itself (min start / max end over its workgroups); the
    # numbers below are the launches of the LAST timed step.  `roofline` is the family with the larger share of the step.
    def family(st, name, pmc_file, ev_key):
        n_launch, secs, flops = st.read()
        if not n_launch:
            return None
        traffic = None
        try:        # HBM bytes of the dominant launch shape from the newest committed PMC passes (profiles/, separate --pmc runs)
            f = newest_profile(pmc_file)
            pmc = json.load(open(f))
            traffic = {"hbm_bytes": pmc["hbm_bytes_per_launch"], "algorithmic_bytes": pmc["algorithmic_bytes_per_launch"],
                       "launch": pmc["launch"], "source": "profiles/" + os.path.basename(f)}
        except Exception:
            pass
        ev_n, ev_ms = prof.get(ev_key, (0, 0.0))     # HIP events around the eager (student) launches, for comparison
        ach = flops / secs / 1e12
        issued = getattr(st, "last_issued", flops)   # MFMA work issued: the correction terms of the fp16c8 / fp16c4 / bf16x3 operand formats on top
        return {"kernel": name, "bound": "mfma", "achieved": round(ach, 2), "peak": PEAK_BF16 / 1e12, "unit": "TFLOP/s",
                "frac": round(ach * 1e12 / PEAK_BF16, 4), "issued_mfma_frac": round(issued / secs / PEAK_BF16, 4),
                "note": "achieved / frac: ALGORITHMIC FLOPs (2 M N K per launch) over the launches' device time; issued_mfma_frac: the bf16-"
                        "equivalent MFMA work the launches issue (fp16c4: 19 K-tiles per 12, fp16c8: 25 per 12, fp16x3 / bf16x3: 37 per 12) over the same time",
                "traffic": traffic, "launches": n_launch,
                "avg_launch_ms": round(secs * 1e3 / n_launch, 4), "share_of_step": round(secs / (dt / opt.steps), 4),
                "timer": "device s_memrealtime spans, last timed step" + ("" if opt.teacher_sync else
                                                                               " (teacher graph on a side stream: spans include sharing the GPU with the student's forward)"),
                "hip_event_avg_ms_eager_launches": round(ev_ms / ev_n, 4) if ev_n else None}
    c4mode = opt.teacher_precision.startswith("fp16c4")
    fams = [family(nn_ops.gemm_stamps, "gemm_bf16_v6_kernel (persistent 256x256 MFMA GEMM: qkv / proj+residual / fc1+GELU / fc2+residual; teacher "
                   "launches on " + ("fp16c4" if c4mode else opt.teacher_precision.split("-")[0]) + " operands, student launches on bf16)",
                   "gemm_c4_pmc.json" if c4mode else ("gemm_c8_pmc.json" if opt.teacher_precision.startswith("fp16c8") else
                                                      ("gemm_x3_pmc.json" if opt.teacher_precision.endswith("x3") else "gemm_v6_pmc.json")), "gemm_bf16"),
            family(nn_ops.stamps, ("attn_fwd_x3_kernel (teacher, three-term operands) + attn_fwd2_kernel (student)" if opt.teacher_precision.endswith("x3")
                                   else "attn_fwd2_kernel (fused attention forward)"),
                   "attn_x3_pmc.json" if opt.teacher_precision.endswith("x3") else "attn_fwd_pmc.json", "attn_fwd")]
    fams = sorted([f for f in fams if f], key=lambda f: -f["share_of_step"])
    # the remaining legs time their own launches: stamping off (the buffers stay alive: the teacher's captured launches still write to them)
    _keep_stamp_buffers.extend([nn_ops.stamps, nn_ops.gemm_stamps])
    nn_ops.stamps = nn_ops.gemm_stamps = None
    # does the mode `value` was measured in meet BASELINE.json's tolerance (1e-3 relative on fp32 CAMs, mask IoU >= 0.999 against the
    # fp32 CPU oracle)?  Read from the committed accuracy record of that mode (worst over every draw on record; the GPU tests that write
    # it assert the same bars, and the record must name the kernel sources of this tree: conformance()).  The default headline mode
    # does; the bf16-operand teacher (`fast_mode`) does not.
    acc = conformance(opt.teacher_precision, opt.crop)
    out["tolerance_met"] = acc["tolerance_met"]          # (and the live check below: set after it ran)
    out["accuracy_vs_fp32_cpu_oracle"] = acc
    out["roofline"] = fams[0] if fams else None
    if len(fams) > 1:
        out["roofline_second"] = fams[1]
    if flop_img:
        out["step_mfma"] = {"achieved_TFLOPs": round(ips * flop_img / 1e12, 2), "peak_TFLOPs": PEAK_BF16 / 1e12 * world,
                            "frac": round(ips * flop_img / (PEAK_BF16 * world), 4), "flop_per_img": flop_img}
    out["tolerance_planes"] = {k: acc.get(k) for k in ("planes", "planes_exempt", "planes_failed", "draws")}          # how many planes took the conditioning exemption
    try:
        out["accuracy_live"] = live_accuracy_check(trainer, wimg, lab, box)
        out["tolerance_met"] = bool(out["tolerance_met"] and (out["accuracy_live"]["gross_error_ok"] or opt.teacher_precision == "bf16x3"))
    except Exception as e:          # (never lose the bench line to the side check -- but a check that could not run is not a pass: ADVICE r5)
        out["accuracy_live"] = {"error": repr(e)[:200]}
        out["tolerance_met"] = False
        out["tolerance_note"] = "the in-run accuracy check raised: tolerance not confirmed in this run"
    vf = vit_forward_roofline(trainer, wimg, dev, opt.crop)
    if vf:
        out["vit_forward"] = vf
    ta = teacher_attention_roofline(dev, opt.batch, opt.crop, opt.teacher_precision)
    if ta:
        out["teacher_attention"] = ta
    out["par_refine"] = par_refine_ms_per_img(trainer, simg, lab, box, dev, opt, C)
    out["bilateral"] = out["par_refine"].pop("bilateral")
    if world == 1 and not opt.no_secondary:
        out.update(secondary_modes(opt, dev, C, wimg, simg, lab, box, n_iter))
    if world == 1 and opt.crop == 448:
        out["evaluation"] = eval_images_per_s(trainer, dev, C, opt.crop)
        out["input_pipeline"] = input_pipeline_images_per_s(dev, opt.batch, opt.crop)
    if world == 1 and not opt.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(opt, trainer.student.state_dict(), C)


def main():
    opt = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs MI355X GPUs"
    ndev = torch.cuda.device_count()
    local = local % ndev                  # (rehearsals put several ranks on one card; a real node has one rank per GPU)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("COSA_DIST_BACKEND", "nccl")   # "nccl" == RCCL on ROCm; gloo only for single-card rehearsals
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        # fail loudly, before any timing, when the collective library does not see the world the driver asked for (a failed rank exits non-zero;
        # nothing is ever re-exec'ed from a process that has touched the GPU)
        if dist.get_world_size() != opt.gpus or world != opt.gpus:
            raise SystemExit(f"bench.py --gpus {opt.gpus}: launched with WORLD_SIZE={world}, the {backend} process group reports {dist.get_world_size()} ranks")
    elif opt.gpus != 1:
        raise SystemExit(f"bench.py --gpus {opt.gpus} needs one process per GPU: launch it with torch.distributed.run --nproc-per-node {opt.gpus} (WORLD_SIZE is {world})")

    from cosa_amd import _C, nn_ops
    from cosa_amd.train_step import CoSATrainer, default_args, rank_seed, synthetic_batch

    C = 20 if opt.dataset == "VOC12" else 80
    # several ranks on ONE card (single-GPU rehearsals only) time-slice the device between processes: two streams per process then
    # ping-pong across time slices (measured: 7 s/step), so the side-stream teacher is only used with a card per rank
    shared_card = world > ndev
    args = default_args(opt.dataset, crop_size=opt.crop, batch_size=opt.batch, usepar=opt.usepar, usegmm=opt.usegmm,
                        teacher_precision=opt.teacher_precision,
                        teacher_async=not (opt.teacher_sync or shared_card or os.environ.get("COSA_TEACHER_SYNC", "0") not in ("0", "")))
    if opt.full:
        nn_ops.stamps = nn_ops.KernelStamps(dev)          # device-side launch spans of the two dominant kernels (work inside hipGraphs)
        nn_ops.gemm_stamps = nn_ops.KernelStamps(dev)
    trainer = CoSATrainer(args, dev, ddp=world > 1, seed=0)
    configure_student(trainer, opt)
    if opt.grid_policy >= 0:
        _C.lib().cosa_gemm_set_grid_policy(opt.grid_policy)
        _C.lib().cosa_gemm_set_grid_policy_f16(opt.grid_policy)
    wimg, simg, lab, box = synthetic_batch(opt.batch, opt.crop, C, dev, seed=rank_seed(1234, rank), dataset=opt.dataset)
    n_iter = args.warmup_iters + 1            # post-warm-up: all five losses are live

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # set-up (untimed, not part of the W warm-up steps): the teacher pass becomes a hipGraph on its third call; make sure that
    # capture is over before the timed region whatever W the caller picks
    for _ in range(max(0, 3 - opt.warmup)):
        trainer.step(wimg, simg, lab, box, n_iter)
    for _ in range(opt.warmup):
        trainer.step(wimg, simg, lab, box, n_iter)
    sync()
    if opt.full:
        nn_ops._flops.clear()
        _C.profile_start()
    t0 = time.perf_counter()
    for _ in range(opt.steps):
        logs = trainer.step(wimg, simg, lab, box, n_iter)
    sync()
    dt = time.perf_counter() - t0
    prof = _C.profile_stop() if opt.full else None
    t = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    dt = float(t.item())
    loss = float(logs["overall_loss"])

    if rank == 0:
        if opt.dump_outputs:
            dump_outputs(opt.dump_outputs, logs, trainer.student)
        imgs = opt.batch * world * opt.steps
        ips = imgs / dt
        enc = trainer.student.encoder
        out = {
            "metric": "training images/sec at 448x448 ViT-B", "value": round(ips, 3), "unit": "images/s", "n_gpus": world,
            "steps": opt.steps, "warmup": opt.warmup, "ms_per_step": round(dt / opt.steps * 1e3, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",        # dtype: the student's MFMA operands (the teacher's: config.teacher_operands)
            "config": {"workload": f"{opt.dataset} {C + 1}-class, ViT-B/16 bf16, batch {opt.batch}/GPU x {opt.crop}x{opt.crop}, "
                                   f"teacher 3 scales x 2 flips + student fwd/bwd + cam2mask x2 + 5 losses + AdamW + EMA"
                                   f"{' + PAR' if opt.usepar else ''}{' + adaptive thresholds (GMM)' if opt.usegmm else ''}",
                       "global_batch": opt.batch * world, "parallelism": f"dp{world}", "final_loss": round(loss, 5),
                       "dist_backend": (dist.get_backend() + f" (world size seen by the collective library: {dist.get_world_size()})") if world > 1 else None,
                       "teacher_operands": opt.teacher_precision + ": " + MODE_TEXT[opt.teacher_precision],
                       "teacher_graph": {"captured": trainer._graph is not None, "side_stream": bool(trainer.teacher_async), "error": trainer.graph_error,
                                         "fallbacks": "COSA_TEACHER_SYNC=1 (replay on the main stream), COSA_TEACHER_GRAPH=0 (eager teacher)"},
                       "student": f"bf16 MFMA operands, {enc.residual_stream} residual stream and gradient sums, fp32 master weights / AdamW / EMA",
                       "defer_groups": enc._n_defer_groups() if enc.defer_wgrad else 0,
                       "grid_policy": opt.grid_policy if opt.grid_policy >= 0 else ("balanced (trainer default under DDP)" if world > 1 else "full grid"),
                       },
        }
        if opt.full:
            full_report(out, opt, trainer, prof, dt, ips, world, dev, C, wimg, simg, lab, box, n_iter)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
