"""One CoSA training iteration on MI355X (the hot path of main.py:106-252), data-parallel over RCCL.

`CoSATrainer.step()` is the reference loop body with the same call surface underneath
(models.build_model, utils.seg_helper.*, utils.torch_helper.PolyWarmupAdamW) and these deliberate
differences, none of which change the maths:
  * no per-iteration host syncs (the reference does 8 .item() + sklearn mAP per step, main.py:257-268);
    losses come back as device tensors
  * cam_validation is folded into the cam2mask kernel; the box ROI is one broadcast compare
  * EMA teacher update is two foreach launches instead of a ~150-tensor Python loop
  * the per-iteration barrier (main.py:385) is dropped: the gradient all-reduce already orders ranks
  * encoder.head (never used, vit.py:257,325) is frozen so DDP needs no find_unused_parameters
"""
import contextlib
import math
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from . import nn_ops
from .models import build_model
from .models.PAR import PAR
from .models.vit import ActProbe
from . import _C
from .utils import grad_check as gcheck
from .utils import seg_helper, torch_helper

IMAGENET_MEAN = (123.675, 116.28, 103.53)
IMAGENET_STD = (58.395, 57.12, 57.375)


def default_args(dataset="VOC12", **over):
    """Hot-path subset of args.py:3-79 / args_coco.py (values, not the argparse plumbing)."""
    a = dict(model='vit', backbone='vit_base_patch16_224', decoder='LargeFOV', pretrained=False, aux_layer=-3, isgap=False,
             crop_size=448, ignore_index=255, num_classes=21, batch_size=2, max_iters=40000, warmup_iters=6000, lr=6e-5,
             min_mult=0.0, wt_dec=1e-2, wt_dec_mult=1.0, lrscale=10.0, freeze_norm=False, momentum=0.9994, seg_weight=0.1,
             segfg_alpha=0.5, cam_weight=0.05, seg_softmaxtemp=0.01, reg_weight=0.05, pseudo_scales=[1.0, 0.5, 1.5],
             high_thre=0.7, high_thre_aux=0.7, low_thre=0.25, low_thre_aux=0.25, bkg_thre=0.5, par_downscale=2, usepar=False,
             aux_cam2seg=True, aux_cam2seg_alpha=0.5, aux_seg2cam=False, aux_seg2cam_alpha=0.5, after_softmax=False,
             detach='none', use_cammix=False, usegmm=False, usegmmaux=False, gmmscale=16, gmmfilter_thre=0.05, gmmemadecay=0.99,
             queue_update_ratio=100, compute_dtype=torch.bfloat16, teacher_precision="auto", teacher_graph=True, teacher_async=True, lattice_async=False, fused_losses=True, fused_optimizer=True,
             clip_grad_norm=0.0, skip_nonfinite=False, label_stats=False, tensor_stats=False, accum_steps=1,
             teacher_check_iters=0, teacher_check_mode="auto", student_check_iters=0, student_check_mode="fp32", gt_stats=False, gt_dir=None,
             act_stats_iters=0, camloss_version='v1', segconf_thre=0.25,
             grad_check_iters=0, grad_check_mode='fp64', grad_check_dirs='all', grad_check_rho=gcheck.DEFAULT_RHO,
             tokcon_weight=0.0, tokcon_temp=0.5, tokcon_purity=1.0,
             seg_reliability=False, seg_reliability_floor=0.0, camweight_beta=1.0,
             seg_soft_weight=0.0, seg_soft_temp=1.0, seg_soft_conf=0.0)
    if dataset == "VOC12":
        a.update(aux_layer=-4, max_iters=32000)            # run_voc.sh:9-11
    elif dataset == "COCO":
        a.update(num_classes=81, batch_size=4, max_iters=60000, warmup_iters=10000, high_thre=0.65)   # args_coco.py
    a.update(over)
    a["dataset"] = dataset
    return SimpleNamespace(**a)


CAMLOSS_VERSIONS = ("v1", "v2", "v3")          # --camloss_version (main.py:216-224)


def camloss_version(args):
    """--camloss_version of `args` ("v1" where the field is missing); an unknown one is refused"""
    v = str(getattr(args, "camloss_version", "v1") or "v1")
    if v not in CAMLOSS_VERSIONS:
        raise ValueError(f"camloss_version {v!r}: one of {', '.join(CAMLOSS_VERSIONS)}")
    if v == "v3" and not math.isfinite(float(getattr(args, "segconf_thre", 0.25))):
        raise ValueError(f"segconf_thre {getattr(args, 'segconf_thre')!r}: a finite probability threshold")
    return v


NOGRAD_PRECISIONS = ("bf16", "fp16", "fp32", "fp64", "bf16x3", "fp16x3", "fp16c8", "fp16c4")     # VITNetwork.set_nograd_precision's base names


def refuse_fp64_teacher(mode, flag=""):
    """"fp64" is a check mode (--teacher_check_mode, --student_check_mode, tools/teacher_check.py): as the training teacher it is refused,
    here for the trainer and, with flag="--", for the launcher's check_supported"""
    if str(mode).partition("-")[0] == "fp64":
        raise ValueError(f"{flag}teacher_precision {mode!r}: float64 is a check mode, not a training teacher -- fp32 IS the reference's arithmetic "
                         f"(--teacher_precision fp32), so a float64 teacher has no use and costs several times fp32's time; score a mode "
                         f"against float64 with --teacher_check_mode fp64, --student_check_mode fp64 or tools/teacher_check.py --criterion")


def wrap_ddp(module, device):
    """Student-only DDP (main.py:49-50): RCCL all-reduce of ~92.5 M fp32 grads, 64 MB buckets as gradient views,
    overlapped with backward.  find_unused_parameters is not needed (the dead encoder.head is frozen)."""
    ids = [device.index] if device.type == "cuda" else None
    return torch.nn.parallel.DistributedDataParallel(module, device_ids=ids, gradient_as_bucket_view=True, bucket_cap_mb=64)


def rank_seed(base, rank):
    """per-rank synthetic-data seed (SURVEY d-2): distinct shards, no data-path collective"""
    return base + rank


def resolve_teacher_precision(mode, crop_size, usepar=False):
    """"auto" -> the cheapest operand mode of the teacher's no-grad passes with NO failed plane on the committed accuracy record
    (profiles/r06_accuracy_teacher.txt, written by tests/test_precision_gpu.py) under the criterion pre-registered there: per active CAM plane
    the literal bar (normalised-CAM |delta| <= 1e-3), or -- only for planes of conditioning > 50 -- own-scale err <= 1e-3 AND |HIP - float64| <=
    1e-3 + 4 x |fp32 - float64|; label agreement >= 0.999 per draw; mask mIoU >= 0.999 from a confusion matrix pooled over the draws; >= 64
    draws.  Since round 6 that is "fp16x3": every MFMA operand as hi + lo fp16 halves (22 significant bits), three MFMA terms, attention
    included.  Round 5's default "fp16c8-x2" (fp16 + two e5m2 correction terms, blocks 0-1 on bf16x3: ~14 bits, 25 % faster) keeps the
    literal bar on every plane of conditioning <= 50 but fails the float64-bounded exemption on planes of conditioning > 100 (one of the
    260 planes of the b = 16 record; on such a plane its literal figure moves by 1e-3 with the last bit of the inputs): selectable, reported by
    bench.py as `other_modes`, not the default.  tests/test_boundary.py checks that the name returned here has no failed plane on record.
    "bf16" (configs[1] literally) is 1.9x faster and an order of magnitude out of tolerance."""
    if mode != "auto":
        return mode
    return "fp16x3"


def resolve_teacher_check_mode(mode, teacher_precision):
    """--teacher_check_mode: "auto" -> "bf16x3" against an "fp16x3" teacher -- the same three-term kernels on halves
    with fp32's exponent range, so an fp16 split that overflows (|t| > 65504: hi = inf) shows as a difference --, "fp16x3", the conforming
    default, against every other teacher mode.  Any other value is taken as it is (VITNetwork.set_nograd_precision's names); "fp32" makes the
    figure the criterion's own: the teacher's mode against the reference's arithmetic."""
    if mode != "auto":
        return mode
    return "bf16x3" if teacher_precision == "fp16x3" else "fp16x3"


def tokcon_settings(args, flag=""):
    """(weight, temp, purity) of the token contrast term from `args` (off where the fields are missing), refused when
    one is outside its range or when the term meets --grad_check_iters, whose five forward-only evaluators do not know a sixth term; here for
    the trainer and, with flag="--", for the launcher's check_supported"""
    w, t, p = (getattr(args, "tokcon_weight", 0.0) or 0.0, getattr(args, "tokcon_temp", 0.5), getattr(args, "tokcon_purity", 1.0))
    seg_helper.check_tokcon_settings(w, t, p, flag=flag)
    if float(w) > 0 and int(getattr(args, "grad_check_iters", 0) or 0) > 0:
        raise ValueError(f"{flag}tokcon_weight {w!r} with {flag}grad_check_iters: the gradient check differences the five terms of the "
                         f"reference's objective and has no evaluator for the token contrast term; run the check with {flag}tokcon_weight 0")
    return float(w), float(t), float(p)


def seg_soft_settings(args, flag=""):
    """(weight, temp, conf) of the soft-label seg loss from `args` (off where the fields are missing), refused when one is
    outside its range or when the term meets --grad_check_iters, as tokcon_settings refuses the token contrast term there; here for the
    trainer and, with flag="--", for the launcher's check_supported"""
    w, t, c = (getattr(args, "seg_soft_weight", 0.0) or 0.0, getattr(args, "seg_soft_temp", 1.0), getattr(args, "seg_soft_conf", 0.0))
    t, c = (1.0 if t is None else t), (0.0 if c is None else c)
    seg_helper.check_seg_soft_settings(w, t, c, flag=flag)
    if float(w) > 0 and int(getattr(args, "grad_check_iters", 0) or 0) > 0:
        raise ValueError(f"{flag}seg_soft_weight {w!r} with {flag}grad_check_iters: the gradient check differences the five terms of the "
                         f"reference's objective and has no evaluator for the soft-label seg term; run the check with {flag}seg_soft_weight 0")
    return float(w), float(t), float(c)


def reliability_settings(args, flag=""):
    """(on, beta, floor) of the reliability-weighted seg loss from `args` (off where the fields are missing): the
    switch, the reference's --camweight_beta and the floor, refused when one is outside its range -- with the switch off too, so that a
    typo does not wait for the run that turns it on; here for the trainer and, with flag="--", for the launcher's check_supported"""
    beta = getattr(args, "camweight_beta", 1.0)
    floor = getattr(args, "seg_reliability_floor", 0.0)
    beta, floor = (1.0 if beta is None else beta), (0.0 if floor is None else floor)
    seg_helper.check_reliability_settings(beta, floor, flag=flag)
    return bool(getattr(args, "seg_reliability", False)), float(beta), float(floor)


def check_iters(args, which, flag=""):
    """--<which>_check_iters of `args` (which: "teacher" / "student" / "grad"), or --act_stats_iters (which: "act_stats"), as an int; a negative one is
    refused, here for the trainer and, with flag="--", for the launcher's check_supported"""
    name = "act_stats_iters" if which == "act_stats" else which + "_check_iters"
    n = int(getattr(args, name, 0) or 0)
    if n < 0:
        raise ValueError(f"{flag}{name} {n!r}: 0 (off) or a positive number of optimizer steps")
    return n


@torch.no_grad()
def teacher_products(model, args, wimg, img_denorm, img_box, cls_label, thresholds, seg_scales, tgt_hw, buffers, refine_model=None):
    """What a training step derives from ONE teacher pass of `model` over `wimg`, by the step's own calls: -> ((cam, cam_aux) as cam2mask
    reads them, (main label map, auxiliary label map | None), cam-loss targets | None).  thresholds = ((high, low), (aux high, aux low)),
    floats or device scalars; tgt_hw: the targets' size, None for none (they need seg_scales); buffers: the caller's CAM-buffer dict for
    this model.  The --teacher_check pass (CoSATrainer._teacher_check) and tools/teacher_check.py; no host sync, no RNG."""
    cam, aux, seg = seg_helper.multi_scale_camseg(model, wimg, args.pseudo_scales, _active_labels=None if args.use_cammix else cls_label,
                                                  _seg_scales=seg_scales, _buffers=buffers)
    if cam.dtype == torch.float64:          # a network in mode "fp64": rounded to fp32 ONCE, here at the comparison boundary
        cam, aux, seg = cam.float(), aux.float(), ([s.float() for s in seg] if seg_scales else seg.float())
    if args.use_cammix:
        cam = (cam + aux) / 2
    (hi, lo), (hi_aux, lo_aux) = thresholds
    if args.aux_cam2seg:
        mask, mask_aux = seg_helper.cam2mask_multi(img_denorm, img_box, [cam, aux], cls_label, [hi, hi_aux], [lo, lo_aux],
                                                   refine_model=refine_model, downscale=args.par_downscale, _fold_validation=True)
    else:
        mask_aux = None
        mask = seg_helper.cam2mask(img_denorm, img_box, cam, cls_label, hi, lo, refine_model=refine_model, downscale=args.par_downscale,
                                   _fold_validation=True)
    tgt = None
    if tgt_hw is not None:
        tgt = seg_helper.cam_loss_targets(seg, cls_label, wimg.shape[-1], tuple(tgt_hw), args.seg_softmaxtemp, after_softmax=args.after_softmax)
    return (cam, aux), (mask, mask_aux), tgt


class CheckNetwork:
    """A monitor's network of its own (parameters, 16-bit shadows, operand and CAM buffers: nn_ops._owner_of is keyed by parameter) on
    `mode` operands, built without drawing from any RNG the run reads: it is initialised on the host and the host generators' states are
    put back.  Its initial weights never matter -- every check begins with load().  `params`: the fp32 tensors the weights are written to,
    in `src_params`' order -- the network's own parameters, which every family reads as they are; a host network in mode fp64 runs in
    torch.float64 and takes them from fp32 staging copies when a pass begins."""

    def __init__(self, name, args, device, mode, src_params):
        import random
        states = torch.get_rng_state(), np.random.get_state(), random.getstate()
        try:
            net = build_model(SimpleNamespace(**dict(vars(args), pretrained=False)))
        finally:
            torch.set_rng_state(states[0])
            np.random.set_state(states[1])
            random.setstate(states[2])
        net = net.to(device)
        for p in net.parameters():
            p.requires_grad = False
        if device.type == "cuda" or hasattr(net, "set_nograd_precision"):      # (a host trainer's toy network has torch operators only)
            net.set_nograd_precision(mode)
        params = list(net.parameters())
        assert len(params) == len(src_params) and all(a.shape == b.shape for a, b in zip(params, src_params))
        self._staged = device.type != "cuda" and mode == "fp64"
        if self._staged:
            net = net.double()
            params = [torch.empty_like(p, dtype=torch.float32) for p in net.parameters()]
        self.name, self.net, self.params = name, net, params
        # not optimizer-owned: refreshed at the entry of every pass ("fp32" / "fp64" and a host network: none, the fp32 parameters are read)
        self.shadows = nn_ops.ensure_shadows(net, net.compute_dtype) \
            if device.type == "cuda" and net.compute_dtype not in (torch.float32, torch.float64) else None
        self.buffers = {}                    # its CAM buffers (seg_helper.multi_scale_camseg, `_buffers`)

    def load(self, src_params):
        torch._foreach_copy_(self.params, src_params)

    @contextlib.contextmanager
    def run(self):
        """what a pass of the network runs inside: no kernel-span stamps (a benchmark's slots are the training kernels') and library
        workspaces of its own (_C.workspace_scope, named after the monitor)"""
        if self._staged:
            for p, s in zip(self.net.parameters(), self.params):
                p.copy_(s)
        held = nn_ops.stamps, nn_ops.gemm_stamps
        nn_ops.stamps = nn_ops.gemm_stamps = None
        try:
            with _C.workspace_scope(self.name):
                yield self.net
        finally:
            nn_ops.stamps, nn_ops.gemm_stamps = held


class CoSATrainer:
    def __init__(self, args, device, ddp=False, seed=0):
        self.args = args
        self.device = device
        self.camloss_version = camloss_version(args)      # (before anything is built: an unknown version costs nothing)
        self._tokcon = tokcon_settings(args)              # (likewise: the token contrast term; weight 0: off)
        self._seg_rel = reliability_settings(args)        # (likewise: the reliability-weighted seg loss)
        self._seg_soft = seg_soft_settings(args)          # (likewise: the soft-label seg loss; weight 0: off)
        # its counters, int64 [G][4] (seg_helper.new_reliability_stats): the run's, read and zeroed by seg_reliability(); None: the switch is off
        self.seg_rel_state = seg_helper.new_reliability_stats(2 if args.aux_cam2seg else 1, device) if self._seg_rel[0] else None
        if check_iters(args, "grad") > 0:                 # (--grad_check_iters, DESIGN.md section 25: refused before anything is built too)
            args.grad_check_mode = gcheck.check_mode(getattr(args, "grad_check_mode", "fp64"))
            args.grad_check_dirs = gcheck.check_dirs(getattr(args, "grad_check_dirs", "all"))
            args.grad_check_rho = gcheck.check_rho(getattr(args, "grad_check_rho", gcheck.DEFAULT_RHO))
            if ddp:
                raise NotImplementedError("grad_check_iters under data parallelism: the reduced gradient belongs to the mean of all ranks' "
                                          "losses, and averaging the check's loss slots across ranks is not built; run the check in a "
                                          "world of one (tools/grad_check.py)")
        torch_helper.setup_seed(seed)
        self.model_ON = build_model(args).to(device)
        self.model_AN = build_model(args).to(device)
        # same weights in student and teacher at step 0 (SURVEY d-2; the reference gets there through identical seeding)
        self.model_AN.load_state_dict(self.model_ON.state_dict())
        for m in (self.model_ON, self.model_AN):
            for p in m.encoder.head.parameters():
                p.requires_grad = False
        for p in self.model_AN.parameters():
            p.requires_grad = False
        groups = self.model_ON.get_param_groups()
        self.student = self.model_ON
        # Data parallelism (main.py:49-50).  On the GPU the teacher's hipGraph is captured BEFORE DistributedDataParallel exists (first step:
        # prepare_ddp): at that point the process group has no collective in flight, so RCCL's watchdog has no event to poll while the
        # capture is open and DDP's reducer / comm stream do not exist yet; the wrap's own parameter broadcast follows the capture.
        self._ddp_pending = False
        if ddp:
            if device.type == "cuda":        # leave CUs to RCCL's channels: persistent GEMM grids balanced over their rounds (include/cosa_hip.h)
                _C.lib().cosa_gemm_set_grid_policy(1)            # (before the capture: a captured launch keeps the grid it was recorded with)
                _C.lib().cosa_gemm_set_grid_policy_f16(1)
                self._ddp_pending = True
            else:
                self.model_ON = wrap_ddp(self.model_ON, device)
        self.optimizer = torch_helper.PolyWarmupAdamW(
            params=[
                {'params': [p for p in groups[0] if p.requires_grad], 'lr': args.lr, 'weight_decay': args.wt_dec},
                {'params': groups[1], 'lr': args.lr if not args.freeze_norm else 0,
                 'weight_decay': args.wt_dec * args.wt_dec_mult if not args.freeze_norm else 0},
                {'params': groups[2], 'lr': args.lrscale * args.lr, 'weight_decay': args.wt_dec},
                {'params': groups[3], 'lr': args.lrscale * args.lr, 'weight_decay': args.wt_dec},
            ],
            lr=args.lr, weight_decay=args.wt_dec, betas=(0.9, 0.999), warmup_iter=1500, max_iter=args.max_iters,
            warmup_ratio=1e-6, power=0.9, min_mult=args.min_mult)
        self.reg_layer = seg_helper.DenseEnergyLoss(weight=1e-7, sigma_rgb=15, sigma_xy=100, scale_factor=0.5)
        self.refine_model = PAR(num_iter=10, dilations=[1, 2, 4, 8, 12, 24]) if args.usepar else None
        # the regulariser's lattice depends on the strong image only and can be built on a side stream while the networks run
        # (args.lattice_async).  Measured neutral (334.2 vs 335.0 img/s: the CUs are already full), so it is off.
        self._lattice = seg_helper.PreparedLattice(self.reg_layer.sigma_rgb, self.reg_layer.sigma_xy * self.reg_layer.scale_factor) \
            if (getattr(args, "lattice_async", False) and device.type == "cuda") else None
        if args.usegmm:
            # main.py:94-103: queues of per-cell CAM maxima + EMA trackers of the fitted thresholds, all device-resident
            qdim = (args.crop_size // args.gmmscale) ** 2
            mk = lambda: seg_helper.DynamicQueue(args.batch_size * args.queue_update_ratio, dim=qdim, batch_size=args.batch_size,
                                                 device=device)
            self.cam_queue, self.camaux_queue = mk(), mk()
            self.ema_lowthre = torch_helper.EMAtracker(args.low_thre, decay=args.gmmemadecay)
            self.ema_highthre = torch_helper.EMAtracker(args.high_thre, decay=args.gmmemadecay)
            self.ema_auxlowthre = torch_helper.EMAtracker(args.low_thre_aux, decay=args.gmmemadecay)
            self.ema_auxhighthre = torch_helper.EMAtracker(args.high_thre_aux, decay=args.gmmemadecay)
        self._ema_pairs = (list(self.model_AN.parameters()), list(self.student.parameters()))
        # fixed-address 16-bit shadows of EVERY parameter of both networks (teacher: read by the six no-grad passes of a step and by
        # evaluation; student: the block projections of the training forward, everything in evaluation)
        on = args.compute_dtype == torch.bfloat16 and device.type == "cuda"
        # teacher_precision: operand precision of the teacher's no-grad passes (VITNetwork.set_nograd_precision).  The student, which
        # needs bf16's range for its gradients, stays bf16.
        tp = resolve_teacher_precision(getattr(args, "teacher_precision", "auto"), args.crop_size, bool(getattr(args, "usepar", False)))
        args.teacher_precision = tp
        refuse_fp64_teacher(tp)
        self.model_AN.check_nograd_precision(tp)          # (on the host too: a mode the encoder is not built for fails here, not in a step)
        if on:
            self.model_AN.set_nograd_precision(tp)
        tdt = self.model_AN.compute_dtype if on else args.compute_dtype
        # ("fp32": the teacher's passes read the fp32 masters themselves -- no 16-bit shadows exist, the fused optimizer step writes none)
        self._teacher_shadows = nn_ops.ensure_shadows(self.model_AN, tdt) if on and tdt != torch.float32 else None
        self._student_shadows = nn_ops.ensure_shadows(self.student) if on else None
        # AdamW + EMA + shadow refresh as one multi-tensor kernel: it rewrites every shadow each step, so the no-grad entry points
        # need not refresh them (nn_ops.ensure_shadows); without it they do
        # the gradient guard: off (None) unless --clip_grad_norm > 0 or --skip_nonfinite true
        self._max_norm = float(getattr(args, "clip_grad_norm", 0.0) or 0.0)
        self._skip_nonfinite = bool(getattr(args, "skip_nonfinite", False))
        if not self._max_norm >= 0:
            raise ValueError(f"clip_grad_norm {self._max_norm!r}: 0 (off) or a positive bound")
        guard_on = self._max_norm > 0 or self._skip_nonfinite
        self._tensor_stats = bool(getattr(args, "tensor_stats", False))
        # gradient accumulation: step() consumes one micro-batch, every accum_steps-th call applies the mean gradient
        self._accum_steps = int(getattr(args, "accum_steps", 1) or 1)
        if self._accum_steps < 1:
            raise ValueError(f"accum_steps {self._accum_steps!r}: a positive number of micro-batches per optimizer step")
        self._micro_k = 0                    # the micro-step the next step() call is (0: between optimizer steps)
        self._accum = None                   # the torch path's accumulator (fused_optimizer=False, host trainers)
        self._fused_step = None
        if on and getattr(args, "fused_optimizer", True):
            stats_kw = {}
            if self._tensor_stats:                       # (off: the constructor call as it always was)
                name_of = {id(p): n for n, p in self.student.named_parameters()}
                stats_kw = dict(tensor_stats=True, names=[name_of[id(p)] for p in self._ema_pairs[1]])
            if self._accum_steps > 1:                    # (1: the constructor call as it always was)
                stats_kw.update(accum_steps=self._accum_steps, names=[n for n, _ in self.student.named_parameters()])     # (_ema_pairs[1]'s order)
            self._fused_step = torch_helper.FusedAdamWEMAStep(self.optimizer, self._ema_pairs[1], self._ema_pairs[0], args.momentum,
                                                              shadow_of=nn_ops.shadow_of, max_norm=self._max_norm,
                                                              skip_nonfinite=self._skip_nonfinite, **stats_kw)
        # the guard record: the fused step's (written by its kernels) or, on the torch path, one of the same layout written by torch
        self.guard_state = None
        if guard_on:
            self.guard_state = self._fused_step.guard if self._fused_step is not None else torch_helper.new_guard_state(device)
        # per-tensor diagnostics: off unless --tensor_stats true.  The table is a sample of one step (the one after
        # request_tensor_stats()); `tensor_stats_state`, the blame counters, exists only behind a gradient guard, is state of the run and
        # travels in a state file as `aux.tensor_stats.blame`
        self.tensor_stats_state = self.tensor_stats_table = None
        if self._tensor_stats:
            if self._fused_step is not None:
                self._tensor_names, self._tensor_groups = self._fused_step.names, self._fused_step.group_idx
                self._tensor_sizes = self._fused_step.sizes
                self.tensor_stats_table = self._fused_step.stats_table
                self.tensor_stats_state = self._fused_step.blame
            else:
                group_of = {id(p): gi for gi, g in enumerate(self.optimizer.param_groups) for p in g["params"]}
                self._tensor_names = [n for n, _ in self.student.named_parameters()]
                self._tensor_groups = [group_of.get(id(p), -1) for p in self._ema_pairs[1]]
                self._tensor_sizes = [int(p.numel()) for p in self._ema_pairs[1]]
                self.tensor_stats_table = torch_helper.new_tensor_stats(len(self._tensor_names), device)
                if guard_on:
                    self.tensor_stats_state = torch.zeros(len(self._tensor_names), dtype=torch.int64, device=device)
            self._tensor_stats_armed = False
        # pseudo-label statistics and the teacher finite check: off (None) unless --label_stats true.  The counters
        # are state of the run: they travel in a state file as `label_stats.counters` of extra_state
        self.label_stats_state = None
        if bool(getattr(args, "label_stats", False)):
            self.label_stats_state = seg_helper.new_label_stats(args.num_classes, device)
            self._step_scale = torch.ones(1, device=device, dtype=torch.float32)
            self._add_extra_state("label_stats.counters", self.label_stats_state)
        # pseudo labels against ground truth: off (None) unless --gt_stats true.  The counters are state of the run
        # (`gt_stats.counters` of extra_state) and, under data parallelism, this rank's own, as --label_stats' are
        self.gt_stats_state = None
        if bool(getattr(args, "gt_stats", False)):
            self.gt_stats_state = seg_helper.new_gt_stats(args.num_classes, device)
            self._add_extra_state("gt_stats.counters", self.gt_stats_state)
        # The four monitors with a network of their own (_add_monitor): every N-th optimizer step (--<name>_iters N > 0; off: None) runs
        # one more pass on a CheckNetwork loaded from the checked network at that moment.  The counters are state of the run
        # (`<name>.counters` of extra_state); the networks are not: every pass overwrites them
        self._checks = {}
        self._check_iters = {which: check_iters(args, which) for which in ("teacher", "student", "act_stats", "grad")}
        # the teacher-precision monitor: the teacher's pass once more on `model_CK`, a third network on
        # --teacher_check_mode operands that takes the teacher's weights of that step; the two passes are scored against each other
        self.teacher_check_state = self.model_CK = None
        if self._check_iters["teacher"] > 0:
            cm = args.teacher_check_mode = resolve_teacher_check_mode(getattr(args, "teacher_check_mode", "auto"), tp)
            self.teacher_check_state, self.model_CK = self._add_monitor(
                "teacher_check", cm, 0, "the check compares 16-bit operand modes of the teacher's no-grad passes",
                lambda: seg_helper.new_teacher_check(args.num_classes, device))
        # the student-forward monitor: the student's weights of that step through `model_SK` on --student_check_mode
        # operands (fp32: the masters themselves on the fp32 family), over the batch the step trained on; the training forward is scored
        # against that pass
        self.student_check_state = self.model_SK = self.student_check_last = None
        if self._check_iters["student"] > 0:
            sm = args.student_check_mode = str(getattr(args, "student_check_mode", "fp32"))
            if sm.partition("-")[0] not in NOGRAD_PRECISIONS:
                raise ValueError(f"student_check_mode {sm!r}: one of {', '.join(NOGRAD_PRECISIONS)} (VITNetwork.set_nograd_precision's names)")
            self.student_check_state, self.model_SK = self._add_monitor(
                "student_check", sm, 1, "the check scores the 16-bit training forward",
                lambda: seg_helper.new_student_check(args.num_classes, device))
        # activation range and attention sharpness: the teacher's weights of that step through `model_AK` in mode
        # "fp32", whose encoder carries an ActProbe, over the weak images.  The counters (the probe's table and the number of passes) are,
        # under data parallelism, this rank's own
        self.act_stats_state = self.model_AK = self.act_stats_shape = None
        if self._check_iters["act_stats"] > 0:
            def new_act_stats():
                enc = self.model_AN.encoder
                self.act_stats_shape = (len(enc.blocks), enc.num_heads)
                return seg_helper.new_act_stats(*self.act_stats_shape, device)
            self.act_stats_state, self.model_AK = self._add_monitor(
                "act_stats", "fp32", 0, "the monitor runs the fp32 no-grad path of the HIP encoder", new_act_stats)
            if self.model_AK is not None:
                self.model_AK.encoder.act_probe = ActProbe(*self.act_stats_shape, table=seg_helper.act_stats_table(self.act_stats_state, *self.act_stats_shape))
        # the gradient check: differences the step's objective along the step's own raw gradient on `model_GK`, in
        # --grad_check_mode (fp32 | fp64), whose fp32 parameters the perturb kernel writes; built on a host trainer too.  Nothing
        # accumulates: `grad_check_state` is the record of ONE check (overwritten by the next), so the check is no row of
        # monitors.MONITORS and no entry of a state file
        self.grad_check_state = self.model_GK = self._gk_pending = self.grad_check_last = None
        self._step_ctx = {}                  # what forward_losses keeps of a step for the checks after its backward (_student_check, _grad_check)
        if self._check_iters["grad"] > 0:
            _, self.model_GK = self._add_monitor("grad_check", args.grad_check_mode, 1,
                                                 "the check runs the no-grad fp32 / fp64 path of the HIP encoder", host=True)
            self._gk_names = [n for n, _ in self.student.named_parameters()]
            self._gk_dirs = self._gk_plan = self._gk_tables = None                       # (made by the first check: which tensors hold a gradient)
            self.grad_check_state = True                                              # (the record itself: allocated with the plan)
        if on:
            for sh in (self._teacher_shadows, self._student_shadows):
                if sh is not None:
                    sh.optimizer_owned = self._fused_step is not None
            # bf16 W^T copies of the student's block projections (the input-gradient GEMMs run the forward kernel on them)
            ws = [self.student.encoder.patch_embed.proj.weight]
            for blk in self.student.encoder.blocks:
                ws += [blk.attn.qkv.weight, blk.attn.proj.weight, blk.mlp.fc1.weight, blk.mlp.fc2.weight]
            self._student_shadows.add_transposed(ws)
        # COSA_TEACHER_GRAPH=0 / COSA_TEACHER_SYNC=1: fallbacks reachable from any launcher's command line (first multi-GPU runs)
        self.use_graph = bool(getattr(args, "teacher_graph", True)) and on and os.environ.get("COSA_TEACHER_GRAPH", "1") != "0"
        self.graph_error = None              # why the capture was abandoned, if it was (the teacher then runs eagerly)
        # fused_losses: the dense losses on the HIP kernels, for every setting of --segfg_alpha / --aux_cam2seg_alpha / --aux_cam2seg /
        # --after_softmax.  False selects the op-by-op torch path (host trainers; the A/B partner of the fused one)
        self.fused_losses = bool(getattr(args, "fused_losses", True)) and device.type == "cuda"
        if self.fused_losses:               # (refuses an alpha outside [0, 1] here, not in the first step past warm-up)
            seg_helper.seg_blend_weights(args.segfg_alpha, args.aux_cam2seg_alpha, bool(args.aux_cam2seg))
        self._graph = None
        self._loss_weights = {}
        self._graph_calls = 0
        self._cam_buffers = {}               # this trainer's CAM buffers of the teacher passes (seg_helper.multi_scale_camseg, `_buffers`)
        self.teacher_async = bool(getattr(args, "teacher_async", True)) and self.use_graph and os.environ.get("COSA_TEACHER_SYNC", "0") in ("0", "")
        self._side = None
        self._teacher_pending = False

    # -- teacher pass: eager for the first calls (MIOpen/hipBLASLt pick their kernels), then captured and replayed --
    def _teacher(self, wimg, cls_label):
        args = self.args
        act = None if args.use_cammix else cls_label
        sts = [s_ for s_ in (nn_ops.stamps, nn_ops.gemm_stamps) if s_ is not None]
        for st in sts:                          # kernel-span slots are re-dealt every step: the teacher section's, then the eager ones
            st.begin_section()
        if not self.use_graph or (self._graph is None and self._graph_calls < 2):
            self._graph_calls += 1
            for st in sts:
                st.reset()
            out = seg_helper.multi_scale_camseg(self.model_AN, wimg, args.pseudo_scales, _active_labels=act,
                                                _seg_scales=self.fused_losses, _buffers=self._cam_buffers)
            for st in sts:
                st.begin_eager()
            return out
        if self._graph is None:
            self._s_wimg = wimg.clone()
            self._s_lab = cls_label.clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            try:
                # thread_local: a call another thread makes meanwhile (RCCL's watchdog polling an event) does not invalidate this capture
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    for st in sts:
                        st.reset()
                    self._s_out = seg_helper.multi_scale_camseg(self.model_AN, self._s_wimg, args.pseudo_scales,
                                                                _active_labels=None if args.use_cammix else self._s_lab,
                                                                _seg_scales=self.fused_losses, _buffers=self._cam_buffers)
            except Exception as e:          # a failed capture must not cost the run: eager teacher from here on, and the reason on record
                import sys
                self.graph_error = repr(e)[:300]
                self.use_graph = self.teacher_async = False
                print(f"[cosa_amd] teacher hipGraph capture failed ({self.graph_error}); the teacher runs eagerly", file=sys.stderr, flush=True)
                torch.cuda.synchronize()
                return self._teacher(wimg, cls_label)
            self._graph = g
            self._g_stamps = [(st.n, list(st.flops)) for st in sts]
        if self.teacher_async:
            # the teacher pass (no gradients, its own graph) and the student's forward are independent until the losses:
            # replay the graph on a side stream and let the student's kernels fill the CUs its tile rounds leave idle
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.device)
            self._side.wait_stream(torch.cuda.current_stream())        # after the previous step's EMA / shadow refresh
            with torch.cuda.stream(self._side):
                self._s_wimg.copy_(wimg, non_blocking=True)
                self._s_lab.copy_(cls_label, non_blocking=True)
                self._graph.replay()
            self._teacher_pending = True
        else:
            self._s_wimg.copy_(wimg)
            self._s_lab.copy_(cls_label)
            self._graph.replay()
        for st, (n_, fl_) in zip(sts, getattr(self, "_g_stamps", None) or []):
            st.n, st.flops = n_, list(fl_)
            st.begin_eager()
        return self._s_out

    def _add_monitor(self, name, mode, half, needs, new_counters=None, host=False):
        """set-up of the monitor --<name>_iters, whose CheckNetwork on `mode` operands shadows _ema_pairs[half] (0: teacher, 1: student)
        -> (its counters, entered into extra_state as `<name>.counters` | None without a constructor, its network | None).  A mode the
        encoder is not built for and a trainer without the 16-bit GPU path are refused here, on the host too, not in a step; the network
        is built on that path only, and with `host` on a host trainer as well."""
        on = self._student_shadows is not None
        (self.model_AN, self.student)[half].check_nograd_precision(mode)
        if self.device.type == "cuda" and not on:
            raise NotImplementedError(f"{name}_iters: {needs}; this trainer's compute dtype has none")
        counters = None
        if new_counters is not None:
            counters = new_counters()
            self._add_extra_state(name + ".counters", counters)
        if not (on or host):
            return counters, None
        ck = self._checks[name] = CheckNetwork(name, self.args, self.device, mode, self._ema_pairs[half])
        return counters, ck.net

    def _gk_make_plan(self, grads):
        args, dev = self.args, self.device
        self._gk_dirs, self._gk_plan = gcheck.plan(self._gk_names, [g is not None for g in grads], args.grad_check_dirs)
        self.grad_check_state = torch.zeros((len(self._gk_dirs), gcheck.RECORD), dtype=torch.float64, device=dev)
        self._gk_tables = None
        if dev.type == "cuda":
            sizes = [int(p.numel()) for p in self._ema_pairs[1]]
            self._gk_tables = [gcheck.Table(sizes, dev) for _ in self._gk_plan]     # (one per pass: a pinned table is read by an async copy)
            self._gk_host = torch.empty_like(self.grad_check_state, device="cpu").pin_memory()
            self._gk_event = torch.cuda.Event()
        self._gk_has_grad = [g is not None for g in grads]

    def _is_check_step(self, n_iter, which="teacher"):
        """the step that closes every N-th optimizer iteration (N: --<which>_check_iters); with --accum_steps its last micro-batch"""
        state = self.act_stats_state if which == "act_stats" else getattr(self, which + "_check_state")
        return state is not None and (n_iter + 1) % self._check_iters[which] == 0 and self._micro_k == self._accum_steps - 1

    def _add_extra_state(self, name, tensor):
        """`tensor` travels in a state file as `aux.<name>` (checkpoint.TrainState; `extra_state` exists only once something is in it)"""
        self.extra_state = dict(getattr(self, "extra_state", {}), **{name: tensor})

    def _summary_of(self, counters, summarise):
        """a monitor's summary of the counters accumulated since they were last zeroed (synchronises: for tests and the log interval); None
        when the monitor is off"""
        return None if counters is None else summarise(counters, self.args.num_classes)

    @torch.no_grad()
    def _student_check(self):
        """One check, eagerly on the current stream AFTER the step's backward and BEFORE its optimizer update: the
        student's fp32 masters of this step (the weights the training forward read through its shadows) into model_SK, its full no-grad
        forward over the step's strong images, the step's four losses on that pass's outputs against the step's own label maps, cam-loss
        targets, labels and blend weights (forward kernels only; the regulariser, whose forward owns per-step lattice state, is not
        re-evaluated), and the reduction.  No host sync, no RNG, and nothing the training path reads is written: model_SK's weights, shadows
        and operand buffers are its own, the library workspaces it needs are slots of their own (_C.workspace_scope), and the backward
        that read the training forward's workspaces has already run.  `student_check_last` keeps what went into the reduction."""
        ctx, ck = self._step_ctx, self._checks["student_check"]
        ck.load(self._ema_pairs[1])                                                  # (the unwrapped student's parameters, not DDP's)
        lab = ctx["cls_label"]
        with ck.run() as net:
            b, four = self._check_forward_losses(net, ctx)
            loss_b = torch.stack([t.reshape(()).float() for t in four])
        a, loss_a = ctx["outputs"], torch.stack([t.reshape(()).float() for t in ctx["losses"]])
        seg_helper.student_check(*[(a[k], b[k]) for k in seg_helper.STUDENT_CHECK_TENSORS], (loss_a, loss_b), lab, self.student_check_state)
        self.student_check_last = dict(a=a, b=b, loss_a=loss_a, loss_b=loss_b, cls_label=lab)

    def _check_forward_losses(self, net, ctx):
        """`net`'s full no-grad forward over the step's strong images and the step's four dense / classification losses on its outputs,
        forward kernels only, against what `ctx` kept of the step (label maps, cam-loss targets or v3's label map, labels, boxes) and the
        step's blend weights -> ({seg, cam, cam_aux, cls, cls_aux} as contiguous fp32, (cls, cls_aux, seg, cam) losses).  Both checks
        (_student_check, _grad_check) call it, inside their own CheckNetwork.run."""
        args = self.args
        lab, simg, masks, rels = ctx["cls_label"], ctx["simg"], ctx["masks"], ctx["rel"]
        cls_b, clsaux_b, _feat, seg_b, cam_b, aux_b = net(simg, cam_only=False, detach='none')
        cls_b, clsaux_b, seg_b, cam_b, aux_b = (t.float().contiguous() for t in (cls_b, clsaux_b, seg_b, cam_b, aux_b))
        l_cls = seg_helper.multilabel_soft_margin(cls_b, lab)
        l_cls_aux = seg_helper.multilabel_soft_margin(clsaux_b, lab)
        if self.fused_losses:                 # (rels: --seg_reliability's weight maps of the step, so the checks see the weighted term)
            l_seg = seg_helper.seg_loss_forward_only(seg_b, *masks, simg, ctx["img_box"], fg_alpha=args.segfg_alpha,
                                                     aux_alpha=args.aux_cam2seg_alpha, **self._rel_kw(*rels))
        else:
            l_seg = self._seg_loss_torch(F.interpolate(seg_b, size=masks[0].shape[1:], mode='bilinear', align_corners=False), masks, rels)
        l_cam = self._cam_loss(ctx["tgt"], cam_b, aux_b)
        return dict(seg=seg_b, cam=cam_b, cam_aux=aux_b, cls=cls_b, cls_aux=clsaux_b), (l_cls, l_cls_aux, l_seg, l_cam)

    def _check_objective(self, net, ctx):
        """the five float32 terms (cls, cls_aux, seg, cam, reg) of the step's objective on `net`, forward only, inside the caller's
        CheckNetwork.run.  The regulariser is get_energy_loss on this pass's up-sampled seg logits: its lattice is rebuilt from the same image
        (the training step's lattice state has been consumed by the backward)."""
        outs, four = self._check_forward_losses(net, ctx)
        mask = ctx["masks"][0]
        up = F.interpolate(outs["seg"], size=mask.shape[1:], mode='bilinear', align_corners=False)
        reg = seg_helper.get_energy_loss(img=ctx["simg"], logit=up, label=mask, img_box=ctx["img_box"], loss_layer=self.reg_layer)
        return torch.stack([t.reshape(()).float() for t in four + (reg,)])

    @torch.no_grad()
    def _grad_check(self):
        """One check, eagerly on the current stream AFTER the step's backward and BEFORE the weights move (with
        --accum_steps: before the closing micro-batch's gradient is folded): per direction the norms and the step length s (one reduction
        over the masters and their raw .grad), four perturbed weight sets w + fl32(c s g), c = +1, -1, +1/2, -1/2, written into model_GK by
        the perturb kernel (s is read on the device), and the step's objective evaluated forward-only at w and at each set.  The record
        [n_dirs][RECORD] is complete on the device when this returns and is on its way to the host; grad_check() waits for it -- the check's
        one sync.  No RNG, and nothing the training path reads is written: model_GK's weights and operand buffers are its own, the
        library workspaces it needs are slots of their own (_C.workspace_scope)."""
        ctx, ck = self._step_ctx, self._checks["grad_check"]
        args, rho, host = self.args, self.args.grad_check_rho, self.device.type != "cuda"
        ws = self._ema_pairs[1]                                                      # (the unwrapped student's parameters)
        grads = [p.grad if p.requires_grad else None for p in ws]
        if self._gk_plan is None or self._gk_has_grad != [g is not None for g in grads]:
            self._gk_make_plan(grads)
        rec = self.grad_check_state
        rec.zero_()

        def objective():
            with ck.run() as net:
                return self._check_objective(net, ctx).double()

        ck.load(ws)
        rec[:, gcheck.LOSS:gcheck.LOSS + 5] = objective()
        for p, (row0, n_dirs, dirs) in enumerate(self._gk_plan):
            rows = rec[row0:row0 + n_dirs]
            if host:
                gcheck.norms_torch(ws, grads, dirs, n_dirs, rho, rows)
            else:
                table = self._gk_tables[p].fill(ws, grads, ck.params, dirs)
                gcheck.norms(table, n_dirs, rho, rows)
            for d in range(n_dirs):
                for k, c in enumerate(gcheck.STEPS):
                    if host:
                        gcheck.perturb_torch(ws, grads, ck.params, dirs, d, c, k, rows)
                    else:
                        gcheck.perturb(table, n_dirs, d, c, k, rows)
                    at = gcheck.LOSS + 5 * (k + 1)
                    rows[d, at:at + 5] = objective()
        if host:
            self._gk_pending = rec.clone()
        else:
            self._gk_host.copy_(rec, non_blocking=True)
            self._gk_event.record()
            self._gk_pending = self._gk_host
        self._gk_weights = list(ctx["weights"])

    def grad_check(self):
        """the summary (utils.grad_check.summarize: one dict per direction) of the last check; waits for its record, the check's one sync.
        None when the check is off or none has run"""
        if self._gk_pending is not None:
            if self.device.type == "cuda":
                self._gk_event.synchronize()
            self.grad_check_last = gcheck.summarize(self._gk_pending.tolist(), self._gk_dirs, self._gk_weights)
            self.grad_check_record = self._gk_pending.clone()
            self._gk_pending = None
        return self.grad_check_last

    def grad_check_batch(self, wimg, simg, cls_label, img_box, n_iter, gt=None):
        """forward, backward and one check on a batch WITHOUT an optimizer update (the weights never move) -> the check's summary.  For
        tools/grad_check.py: a trainer built with grad_check_iters=1, so that every step is a check step."""
        if self.model_GK is None or self._check_iters["grad"] != 1 or self._accum_steps != 1:
            raise RuntimeError("grad_check_batch: build the trainer with grad_check_iters=1 and accum_steps=1")
        self._forward_backward(wimg, simg, cls_label, img_box, n_iter, gt)
        self._grad_check()
        self._step_ctx = {}
        return self.grad_check()

    def pop_grad_check(self):
        """grad_check() of a check that has not been read yet, else None: what the launcher asks after a check step"""
        return self.grad_check() if self._gk_pending is not None else None

    def student_check(self):
        """_summary_of --student_check_iters' counters (seg_helper.student_check_summary)"""
        return self._summary_of(self.student_check_state, seg_helper.student_check_summary)

    @torch.no_grad()
    def _teacher_check(self, wimg, img_denorm, img_box, cls_label, cams, masks, thresholds, tgt):
        """One check, eagerly on the current stream after the teacher's pass has been joined: the teacher's weights of
        THIS step (the EMA update comes later) into model_CK, its pass over the same images, the same cam2mask call on the threshold
        VALUES this step used (the queues and trackers of --usegmm are the run's: not touched), the cam-loss targets, and the reduction.
        cams = (cam, cam_aux) as cam2mask read them, masks = (main, aux | None), thresholds = ((high, low), (aux high, aux low)).
        No host sync, no RNG, and nothing the training path reads is written: model_CK's weights, shadows, operand and CAM buffers are
        its own, the library workspaces it needs are slots of their own (_C.workspace_scope)."""
        args, ck = self.args, self._checks["teacher_check"]
        ck.load(self._ema_pairs[0])
        with ck.run() as net:
            (cam_b, aux_b), (mask_b, mask_aux_b), tgt_b = teacher_products(
                net, args, wimg, img_denorm, img_box, cls_label, thresholds, self.fused_losses,
                tgt.shape[-2:] if tgt is not None else None, ck.buffers, self.refine_model)
        seg_helper.teacher_check((cams[0], cam_b), (cams[1], aux_b), (tgt, tgt_b) if tgt is not None else None, (masks[0], mask_b),
                                 (masks[1], mask_aux_b) if masks[1] is not None else None, None if args.use_cammix else cls_label, img_box,
                                 self.teacher_check_state, ignore_index=args.ignore_index, bar=seg_helper.TEACHER_CHECK_BAR)

    def teacher_check(self):
        """_summary_of --teacher_check_iters' counters (seg_helper.teacher_check_summary)"""
        return self._summary_of(self.teacher_check_state, seg_helper.teacher_check_summary)

    @torch.no_grad()
    def _act_stats(self, wimg, cls_label):
        """One pass of the --act_stats_iters monitor, eagerly on the current stream after the teacher's pass has been
        joined: the teacher's weights of THIS step (the EMA update comes later) into model_AK, the teacher's multi-scale pass over the same
        weak images in mode "fp32" with the encoder's probe set, its outputs dropped.  The probe's launches add into `act_stats_state`, whose
        last word counts the passes.  No host sync, no RNG, and nothing the training path reads is written: model_AK's weights, operand and
        CAM buffers are its own, the library workspaces it needs are slots of their own (_C.workspace_scope)."""
        args, ck = self.args, self._checks["act_stats"]
        ck.load(self._ema_pairs[0])
        with ck.run() as net:
            seg_helper.multi_scale_camseg(net, wimg, args.pseudo_scales, _active_labels=None if args.use_cammix else cls_label,
                                          _seg_scales=self.fused_losses, _buffers=ck.buffers)
        self.act_stats_state[-1:] += 1

    def act_stats(self):
        """the summary (seg_helper.act_stats_summary) of --act_stats_iters' counters since they were last zeroed (synchronises: for tests
        and the log interval); None when the monitor is off"""
        return None if self.act_stats_state is None else seg_helper.act_stats_summary(self.act_stats_state, *self.act_stats_shape)

    def _join_teacher(self):
        if self._teacher_pending:
            torch.cuda.current_stream().wait_stream(self._side)
            self._teacher_pending = False

    def _adaptive_thresholds(self, cams, cls_label, queue, ema_low, ema_high, filter_thre):
        """main.py:138-151: per-cell maxima of the validated CAMs at 1/gmmscale resolution -> queue -> rungmm -> EMA trackers.
        cam_validation (x labels) commutes exactly with the bilinear resize for {0,1} labels, so it is applied to the small map."""
        red = seg_helper.cell_bilinear(cams, self.args.crop_size // self.args.gmmscale) * cls_label[:, :, None, None]
        queue.update(red.amax(dim=1))
        fit = seg_helper.rungmm_device(queue.getqueue(), 3, filter_thre)
        # status word (include/cosa_hip.h): any bit set -- empty component, too few samples, expired grid barrier -- means the fit's
        # numbers may be finite but wrong; the trackers then keep their value (EMAtracker skips non-finite updates)
        bad = torch.full((), float("nan"), device=fit.device, dtype=fit.dtype)
        ema_low.update(torch.where(fit[3] == 0, fit[0], bad))
        ema_high.update(torch.where(fit[3] == 0, fit[1], bad))
        return ema_low.get(), ema_high.get()

    # main.py:114-252 -------------------------------------------------------------------------------
    def forward_losses(self, wimg, simg, cls_label, img_box, n_iter, gt=None):
        """gt: the ground-truth crops uint8 [b,S,S] of --gt_stats (required with the flag on, ignored with it off): read by the monitor's
        reduction only, nothing the losses are made of sees it"""
        args = self.args
        if self.gt_stats_state is not None and gt is None:
            raise ValueError("gt_stats: the trainer was built with gt_stats=True and the step got no ground-truth crops (gt=None)")
        img_denorm = torch_helper.denormalize_img(simg) if self.refine_model is not None else simg
        fused = self.fused_losses
        if fused and self._lattice is not None:
            self._lattice.start(simg, args.num_classes)
        if self._ddp_pending:
            self.prepare_ddp(wimg, cls_label)
        cam_ps, cam_aux_ps, seg_ps = self._teacher(wimg, cls_label)
        cls_final, cls_aux, _feat, seg_pred, cam_pred, cam_aux_pred = self.model_ON(simg, cam_only=False, detach=args.detach)
        self._join_teacher()
        cls_loss = seg_helper.multilabel_soft_margin(cls_final, cls_label)          # main.py:127-128, one kernel each
        cls_loss_aux = seg_helper.multilabel_soft_margin(cls_aux, cls_label)
        seg_lr = seg_pred                                                          # (the low-res logits: --student_check scores them)
        with torch.no_grad():
            if args.use_cammix:
                cam_ps = (cam_ps + cam_aux_ps) / 2
            threlow, threhigh = args.low_thre, args.high_thre
            auxthrelow, auxthrehigh = args.low_thre_aux, args.high_thre_aux
            if args.usegmm:
                # main.py:138-151,174-184: thresholds = EMA of a 3-component mixture fitted to the queue every iteration.
                # Fit, trackers and the thresholds cam2mask reads all stay on the device (the reference syncs and runs sklearn).
                threlow, threhigh = self._adaptive_thresholds(cam_ps, cls_label, self.cam_queue, self.ema_lowthre,
                                                              self.ema_highthre, args.gmmfilter_thre)
                if args.aux_cam2seg:
                    auxthrelow, auxthrehigh = self._adaptive_thresholds(cam_aux_ps, cls_label, self.camaux_queue, self.ema_auxlowthre,
                                                                        self.ema_auxhighthre, 0.05)   # main.py:181: default filter
            if args.aux_cam2seg:
                # main and auxiliary CAMs of the same images: one pass (shared bookkeeping / refine-model affinities)
                refine_mask_label, refine_mask_label_aux = seg_helper.cam2mask_multi(
                    img_denorm, img_box, [cam_ps, cam_aux_ps], cls_label, [threhigh, auxthrehigh], [threlow, auxthrelow],
                    refine_model=self.refine_model, downscale=args.par_downscale, _fold_validation=True)
            else:
                refine_mask_label_aux = None
                refine_mask_label = seg_helper.cam2mask(img_denorm, img_box, cam_ps, cls_label, threhigh, threlow,
                                                        refine_model=self.refine_model, downscale=args.par_downscale,
                                                        _fold_validation=True)
            rel_main = rel_aux = None
            if self._seg_rel[0]:
                # --seg_reliability: one weight map per label map from the CAMs, thresholds and labels cam2mask just
                # read and wrote -- one launch for both sets, thresholds still on the device under --usegmm
                aux_on = bool(args.aux_cam2seg)
                rels = (seg_helper.label_reliability if fused else seg_helper._label_reliability_torch)(
                    [cam_ps, cam_aux_ps] if aux_on else [cam_ps], cls_label,
                    [refine_mask_label, refine_mask_label_aux] if aux_on else [refine_mask_label],
                    [threhigh, auxthrehigh] if aux_on else [threhigh], [threlow, auxthrelow] if aux_on else [threlow],
                    beta=self._seg_rel[1], floor=self._seg_rel[2], stats=self.seg_rel_state)
                rel_main, rel_aux = rels[0], (rels[1] if aux_on else None)
            if self.label_stats_state is not None:
                self.update_label_stats(refine_mask_label, refine_mask_label_aux, seg_pred, cls_label, img_box,
                                        cam_ps, cam_aux_ps if args.aux_cam2seg else None)
            if self.gt_stats_state is not None:
                self.update_gt_stats(gt, refine_mask_label, refine_mask_label_aux, seg_pred, cls_label, img_box)
        if fused:
            # one forward + one backward kernel instead of ~10 full-resolution passes (same maths, main.py:167-212)
            seg_loss, reg_loss = seg_helper.fused_seg_and_energy_loss(seg_pred, refine_mask_label, refine_mask_label_aux, simg,
                                                                      img_box, self.reg_layer, prepared=self._lattice,
                                                                      fg_alpha=args.segfg_alpha, aux_alpha=args.aux_cam2seg_alpha,
                                                                      **self._rel_kw(rel_main, rel_aux))
        else:
            seg_pred = F.interpolate(seg_pred, size=refine_mask_label.shape[1:], mode='bilinear', align_corners=False)
            seg_loss = self._seg_loss_torch(seg_pred, (refine_mask_label, refine_mask_label_aux), (rel_main, rel_aux))
            reg_loss = seg_helper.get_energy_loss(img=simg, logit=seg_pred, label=refine_mask_label, img_box=img_box,
                                                  loss_layer=self.reg_layer)
        tgt, check_tgt = self._cam_target(seg_ps, cls_label, wimg.shape[-1], cam_pred.shape[-2:])
        cam_loss = self._cam_loss(tgt, cam_pred, cam_aux_pred)
        if self.model_CK is not None and self._is_check_step(n_iter):
            self._teacher_check(wimg, img_denorm, img_box, cls_label, (cam_ps, cam_aux_ps), (refine_mask_label, refine_mask_label_aux),
                                ((threhigh, threlow), (auxthrehigh, auxthrelow)), check_tgt)
        if self.model_AK is not None and self._is_check_step(n_iter, "act_stats"):
            self._act_stats(wimg, cls_label)
        tok_on, soft_on = self._tokcon[0] > 0, self._seg_soft[0] > 0
        if tok_on:
            tok_loss = self._token_contrast(_feat, refine_mask_label)
        if soft_on:
            soft_loss = self._seg_soft_loss(seg_pred, seg_ps, cls_label, img_box, wimg.shape[-1])
        # main.py:230-236: the weighted sum of the five losses (warm-up: classification losses only) as one dot product
        wkey = n_iter <= args.warmup_iters
        wl = [1.0, 1.0, 0.0, 0.0, 0.0] if wkey else [1.0, 1.0, args.seg_weight, args.cam_weight, args.reg_weight]
        if tok_on:                          # the sixth element: the token contrast term, 0 during warm-up like seg / cam / reg
            wl.append(0.0 if wkey else self._tokcon[0])
        if soft_on:                         # the soft-label seg term, after the token contrast element when both are on; 0 during warm-up too
            wl.append(0.0 if wkey else self._seg_soft[0])
        wvec = self._loss_weights.get(wkey)
        if wvec is None:
            wvec = self._loss_weights[wkey] = torch.tensor(wl, device=cls_loss.device, dtype=torch.float32)
        student_due = self.model_SK is not None and self._is_check_step(n_iter, "student")
        grad_due = self.model_GK is not None and self._is_check_step(n_iter, "grad")
        if student_due or grad_due:
            # what the checks after this step's backward (_student_check, _grad_check) read: detached references, nothing is copied or
            # computed here
            self._step_ctx = ctx = dict(simg=simg, cls_label=cls_label, img_box=img_box, masks=(refine_mask_label, refine_mask_label_aux),
                                        tgt=tgt, rel=(rel_main, rel_aux))
            if student_due:
                ctx.update(outputs=dict(seg=seg_lr.detach(), cam=cam_pred.detach(), cam_aux=cam_aux_pred.detach(),
                                        cls=cls_final.detach(), cls_aux=cls_aux.detach()),
                           losses=tuple(t.detach() for t in (cls_loss, cls_loss_aux, seg_loss, cam_loss)))
            if grad_due:                    # (the loss weights as the dot product below rounds them: fp32)
                ctx.update(weights=[float(np.float32(v)) for v in wl])
        terms = [cls_loss.reshape(()), cls_loss_aux.reshape(()), seg_loss.reshape(()).float(), cam_loss.reshape(()).float(), reg_loss.reshape(()).float()]
        if tok_on:
            terms.append(tok_loss.reshape(()).float())
        if soft_on:
            terms.append(soft_loss.reshape(()).float())
        loss = torch.dot(torch.stack(terms), wvec)
        overall = loss.detach()
        if self.label_stats_state is not None and self._skip_nonfinite:
            # teacher refusal: step_scale is 1.0f (an exact product: the bits of the step without it) or, when this step's CAMs held a
            # non-finite element, NaN -- every gradient is then NaN and the gradient guard refuses the step (under DDP on every rank)
            loss = loss * self._step_scale.reshape(())
        logs = dict(overall_loss=overall, cls_loss=cls_loss.detach(), cls_aux_loss=cls_loss_aux.detach(),
                    seg_loss=seg_loss.detach(), cam_loss=cam_loss.detach(), reg_loss=reg_loss.detach(),
                    mask=refine_mask_label, cls_logits=cls_final.detach(), cls_aux_logits=cls_aux.detach())
        if tok_on:
            logs["tok_loss"] = tok_loss.detach()
        if soft_on:
            logs["soft_loss"] = soft_loss.detach()
        return loss, logs

    @staticmethod
    def _rel_kw(rel_main, rel_aux):
        """the weight maps as the fused seg loss's keywords; none with --seg_reliability off: the call is then the one it has always been"""
        return {} if rel_main is None else dict(rel_main=rel_main, rel_aux=rel_aux)

    def _seg_loss_torch(self, up, masks, rels):
        """the torch path's seg loss on the up-sampled logits: per label map (main, auxiliary | None) seg_loss, or seg_weightloss under its
        weight map (--seg_reliability), blended by --aux_cam2seg_alpha; the step and both checks share it"""
        def one(mask, rel):
            if rel is None:
                return seg_helper.seg_loss(up, mask, fg_alpha=self.args.segfg_alpha)
            return seg_helper.seg_weightloss(up, mask, rel, fg_alpha=self.args.segfg_alpha)
        loss = one(masks[0], rels[0])
        if masks[1] is not None:
            loss = (1 - self.args.aux_cam2seg_alpha) * loss + self.args.aux_cam2seg_alpha * one(masks[1], rels[1])
        return loss

    def seg_reliability(self):
        """the mean weights (seg_helper.reliability_summary: one dict per CAM set, main then auxiliary) of --seg_reliability since the last
        call, and the counters zeroed; None when the switch is off.  Synchronises: call it where a sync already happens (an evaluation).
        The counters are not part of a state file: what they held since the last call is lost on --resume."""
        if self.seg_rel_state is None:
            return None
        summary = seg_helper.reliability_summary(self.seg_rel_state)
        self.seg_rel_state.zero_()
        return summary

    def _token_contrast(self, feat, mask):
        """the token contrast term of the step: the returned feature map [B,768,h,w] taken back to its tokens
        [B,n,768] as a view, labelled from the step's main pseudo-label map, on the HIP kernels (fused_losses) or the torch composition"""
        _, temp, purity = self._tokcon
        if getattr(self.student.encoder, "residual_stream", "fp32") == "bf16":
            raise ValueError('tokcon_weight > 0 with encoder.residual_stream = "bf16": the feature map then has no fanout view of its own, and '
                             "its gradient would meet the decoder's in bf16; leave the stream fp32 or set tokcon_weight 0")
        B, D, h, w = feat.shape
        tokens = feat.permute(0, 2, 3, 1).reshape(B, h * w, D)
        with torch.no_grad():
            labels = seg_helper.token_labels(mask, mask.shape[-1] // h, purity)
        fn = seg_helper.token_contrast_loss if self.fused_losses else seg_helper._token_contrast_torch
        return fn(tokens, labels, temp)

    def _seg_soft_loss(self, seg_pred, seg_ps, cls_label, img_box, S):
        """the soft-label seg term of the step, made here, outside the captured teacher pass: the student's low-res
        logits against the teacher's per-scale low-res segs on the HIP kernels (fused_losses), or its up-sampled logits (the torch path has
        up-sampled `seg_pred` by now) against the teacher's summed full-resolution seg on the torch composition"""
        _, temp, conf = self._seg_soft
        if self.fused_losses:
            return seg_helper.seg_soft_loss(seg_pred, seg_ps, cls_label, img_box, S, temp=temp, conf=conf, fg_alpha=self.args.segfg_alpha)
        return seg_helper.seg_soft_loss_torch(seg_pred, seg_ps, cls_label, img_box, temp, conf, self.args.segfg_alpha,
                                              n_scales=len(self.args.pseudo_scales))

    @torch.no_grad()
    def _cam_target(self, seg_ps, cls_label, S, out_hw):
        """what --camloss_version's cam loss (main.py:216-224) is taken against, from the teacher's segs (fused path: the list of per-scale
        low-res ones) -> (the target _cam_loss and the student check read, the teacher check's targets | None).  v1 / v2: targets at the
        CAM's size `out_hw` on the fused path, the refined teacher probabilities on the torch one; v3: the label map, kept as
        `cam_label_last`.  Made here, outside the captured teacher pass: the graph is the same for every version."""
        args, v3 = self.args, self.camloss_version == "v3"
        if self.fused_losses:
            if v3:
                tgt = seg_helper.cam_label_from_scales(seg_ps, cls_label, S, args.seg_softmaxtemp, args.segconf_thre,
                                                       after_softmax=args.after_softmax)
            else:
                tgt = seg_helper.cam_loss_targets(seg_ps, cls_label, S, out_hw, args.seg_softmaxtemp, after_softmax=args.after_softmax)
        else:
            tgt = seg_helper.seg_refine_by_label(seg_ps, cls_label, softmaxtemp=args.seg_softmaxtemp, after_softmax=args.after_softmax)
            if v3:
                tgt = seg_helper._cam_label_torch(tgt, args.segconf_thre)
        if v3:
            self.cam_label_last = tgt
        return tgt, (tgt if self.fused_losses and not v3 else None)

    def _cam_loss_fn(self, tgt):
        """cam -> the selected --camloss_version against `tgt` (_cam_target's), by the path this trainer takes"""
        fused = self.fused_losses
        if self.camloss_version == "v1":
            return lambda c: (seg_helper.cam_loss_from_targets if fused else seg_helper.cam_loss)(c, tgt)
        if self.camloss_version == "v3":
            return lambda c: (seg_helper.cam_lossv3 if fused else seg_helper._cam_lossv3_torch)(c, tgt)
        if fused:
            return lambda c: seg_helper.cam_lossv2_from_targets(c, tgt)
        return lambda c: seg_helper._cam_lossv2_torch(c, F.interpolate(tgt[:, 1:], size=list(c.shape[-2:]), mode='bilinear', align_corners=False))

    def _cam_loss(self, tgt, cam, cam_aux):
        """the cam loss of a forward against `tgt`, the auxiliary CAM's blended in under --aux_seg2cam; the step and both checks share it"""
        fn = self._cam_loss_fn(tgt)
        loss = fn(cam)
        if self.args.aux_seg2cam:
            loss = (1 - self.args.aux_seg2cam_alpha) * loss + self.args.aux_seg2cam_alpha * fn(cam_aux)
        return loss

    def prepare_ddp(self, wimg, cls_label):
        """first step under data parallelism on the GPU: warm up and CAPTURE the teacher pass, then wrap the student (see __init__)"""
        if self.use_graph:
            with torch.no_grad():
                while self._graph is None and self.use_graph:
                    self._teacher(wimg, cls_label)
                    self._join_teacher()
            torch.cuda.synchronize()
        self.model_ON = wrap_ddp(self.student, self.device)
        if self._student_shadows is not None:
            self._student_shadows.refresh(force=True)    # the wrap broadcast rank 0's masters: the copies were made from this rank's own
        self._ddp_pending = False

    def _gt_kw(self, gt):
        """forward_losses' keyword of --gt_stats: with the flag off the call is what it was (a gt is ignored)"""
        return {} if self.gt_stats_state is None else {"gt": gt}

    def step(self, wimg, simg, cls_label, img_box, n_iter, gt=None):
        if self._accum_steps > 1:
            return self._micro_step(wimg, simg, cls_label, img_box, n_iter, gt)
        logs = self._forward_backward(wimg, simg, cls_label, img_box, n_iter, gt)
        if "outputs" in self._step_ctx:                  # (--student_check_iters: after the backward, before the weights move)
            self._student_check()
        if "weights" in self._step_ctx:                  # (--grad_check_iters: likewise)
            self._grad_check()
        return self._apply_gradients(logs)

    def _forward_backward(self, wimg, simg, cls_label, img_box, n_iter, gt):
        """forward_losses and the backward of one batch -> logs; the gradients are left in .grad"""
        loss, logs = self.forward_losses(wimg, simg, cls_label, img_box, n_iter, **self._gt_kw(gt))
        self.optimizer.zero_grad(set_to_none=True)
        if self.device.type == "cuda" and self._student_shadows is not None:
            nn_ops.wgrad_arena_begin(self.device)        # one clear for all weight gradients of this batch (they are consumed by the caller)
        loss.backward()
        return logs

    def _apply_gradients(self, logs):
        """the optimizer's share of a step, on the gradients of one batch or on the mean left by the closing micro-step"""
        self._step_ctx = {}                              # (the checks, if any were due, have run)
        if self._tensor_stats and self._fused_step is None:
            self._tensor_stats_torch_step()
        if self._fused_step is not None:
            self._fused_step.step()
        elif self.guard_state is not None:
            torch_helper.guarded_torch_step(self.optimizer, self._ema_pairs[0], self._ema_pairs[1], self.args.momentum, self._max_norm,
                                            self._skip_nonfinite, self.guard_state)
        else:
            self.optimizer.step()
            torch_helper.ema_update(self._ema_pairs[0], self._ema_pairs[1], self.args.momentum)
        if self._student_shadows is not None:
            self._student_shadows.refresh()              # W^T, and the 16-bit copies unless the fused kernel has just written them
        if self.guard_state is not None:
            logs["grad_norm"] = torch_helper.guard_norm(self.guard_state).clone()     # a device scalar: no sync
        return logs

    def _micro_step(self, wimg, simg, cls_label, img_box, n_iter, gt=None):
        """--accum_steps N > 1: one micro-batch of the optimizer step `n_iter`.  Forward, losses and backward are
        a step's own (so the teacher, the warm-up weights and the LR are those of `n_iter` for all N calls; the label counters add up;
        with --usegmm the queues and trackers move on every call); the gradients go into the accumulator, and only the N-th call applies
        their mean -- optimizer, EMA, shadows, guard, the armed --tensor_stats sample.  Under DDP every call's backward all-reduces and the
        accumulator takes reduced gradients (correct by linearity; skipping the first N - 1 reductions is not built)."""
        k, n = self._micro_k, self._accum_steps
        logs = self._forward_backward(wimg, simg, cls_label, img_box, n_iter, gt)
        if "weights" in self._step_ctx:                  # (--grad_check_iters: the closing micro-batch's own gradient against its own loss, before it is folded)
            self._grad_check()
        if self._fused_step is not None:
            self._fused_step.accumulate(k)
        else:
            self._accum = torch_helper.accumulate_grads_torch(self._accum, [p.grad for p in self._ema_pairs[1]], k, n,
                                                              [nm for nm, _ in self.student.named_parameters()])
        self._micro_k = (k + 1) % n
        if self._micro_k != 0:
            return logs
        if self._fused_step is None:                     # the torch path reads p.grad: leave the mean there
            with torch.no_grad():
                for p, a in zip(self._ema_pairs[1], self._accum):
                    if a is not None:
                        p.grad.copy_(a)
            self._accum = None
        if "outputs" in self._step_ctx:                  # (--student_check_iters: the closing micro-batch, before the weights move)
            self._student_check()
        return self._apply_gradients(logs)

    def guard_counters(self):
        """{applied, skipped, clipped} of the gradient guard over the run so far (synchronises: for tests and the log interval); None
        when the guard is off"""
        return torch_helper.guard_counters(self.guard_state) if self.guard_state is not None else None

    # -- per-tensor diagnostics --
    def request_tensor_stats(self):
        """arm the next step's sample: that step fills the table from its gradients and its pre-step weights (no sync)"""
        if not self._tensor_stats:
            raise RuntimeError("request_tensor_stats: the trainer was built with tensor_stats=False")
        if self._fused_step is not None:
            self._fused_step.arm()
        else:
            self._tensor_stats_armed = True

    @torch.no_grad()
    def _tensor_stats_torch_step(self):
        """the torch path's share of a step (fused_optimizer=False, host trainers): the armed sample and, behind a guard, the blame"""
        grads = [p.grad if gi >= 0 else None for p, gi in zip(self._ema_pairs[1], self._tensor_groups)]
        if self._tensor_stats_armed:
            self._tensor_stats_armed = False
            self.tensor_stats_table.copy_(torch_helper.tensor_stats_torch(self._ema_pairs[1], self._ema_pairs[0], grads))
        if self.tensor_stats_state is not None:
            torch_helper.grad_blame_torch(grads, self.tensor_stats_state)

    def tensor_stats(self, values=None):
        """the summary (torch_helper.tensor_stats_summary) of the last sample and of the run's blame counters (synchronises: for tests);
        None when --tensor_stats is off.  values: (table values, blame counts or None) already on the host -- what the launcher's
        read_interval's host["tensor_stats"] -- are summarised instead, without a sync."""
        if not self._tensor_stats:
            return None
        table, blame = (self.tensor_stats_table, self.tensor_stats_state) if values is None else values
        return torch_helper.tensor_stats_summary(table, blame, self._tensor_names, self._tensor_groups, self._tensor_sizes)

    # -- pseudo-label statistics --
    @torch.no_grad()
    def update_label_stats(self, mask_main, mask_aux, seg_logits, cls_label, img_box, cam, cam_aux):
        """accumulate one step into the counters (the HIP reduction on the GPU, its torch restatement on a host trainer) and write
        `_step_scale`; no sync"""
        fn = seg_helper.label_stats if self.device.type == "cuda" else seg_helper.label_stats_torch
        return fn(mask_main, mask_aux, seg_logits, cls_label, img_box, cam, cam_aux, self.label_stats_state,
                  ignore_index=self.args.ignore_index, step_scale=self._step_scale)

    def label_stats(self):
        """_summary_of --label_stats' counters (seg_helper.label_stats_summary)"""
        return self._summary_of(self.label_stats_state, seg_helper.label_stats_summary)

    # -- pseudo labels against ground truth --
    @torch.no_grad()
    def update_gt_stats(self, gt, mask_main, mask_aux, seg_logits, cls_label, img_box):
        """accumulate one step into the counters (the HIP reduction on the GPU, its torch restatement on a host trainer); no sync"""
        fn = seg_helper.gt_stats if self.device.type == "cuda" else seg_helper.gt_stats_torch
        fn(gt, mask_main, mask_aux, seg_logits, cls_label, img_box, self.gt_stats_state, ignore_index=self.args.ignore_index)

    def gt_stats(self):
        """_summary_of --gt_stats' counters (seg_helper.gt_stats_summary)"""
        return self._summary_of(self.gt_stats_state, seg_helper.gt_stats_summary)

    # -- full-state checkpoints (cosa_amd/checkpoint.py) --
    def train_state(self):
        """the TrainState of the networks and moments (in a world of one: of everything)"""
        from . import checkpoint
        return checkpoint.trainer_state(self)

    def save_state(self, path, **extra):
        """Write everything that defines the future of this run to `path` (one snapshot launch now; copy and file write run behind the
        loop).  `extra`: the launcher's own bookkeeping, returned by load_state; tensors the launcher keeps on the device travel through
        `self.extra_state` {name: tensor} (set before the first save or load).  Under a process group rank 0 writes `path`, every rank
        `path.rank<r>`.  Older complete state files next to `path` are pruned to args.keep_states (default 2)."""
        from . import checkpoint
        assert self._micro_k == 0, f"save_state inside an optimizer step (micro-step {self._micro_k} of {self._accum_steps} is next)"
        return checkpoint.save_trainer(self, path, extra, keep=int(getattr(self.args, "keep_states", 2)))

    def wait_state(self):
        """until every state file asked for is written"""
        from . import checkpoint
        checkpoint.wait_trainer(self, keep=int(getattr(self.args, "keep_states", 2)))

    def load_state(self, path):
        """Restore a file written by save_state (verified before anything is overwritten), rebuild everything derived from the masters,
        drop the captured teacher graph; -> extra (plus `rng_at_save`, the RNG states this call has just restored)."""
        from . import checkpoint
        extra = checkpoint.load_trainer(self, path)
        self._micro_k, self._accum = 0, None             # a state file is written between optimizer steps: the accumulator is dead there
        if self._fused_step is not None:
            self._fused_step._acc_next = 0
        return extra


# ---- synthetic batches --------------------------------------------------------------------
def synthetic_batch(b, S, C, device, seed=1234, dataset="VOC12"):
    """(wimg, simg, cls_label, img_box) with the loader's contract (dataloaders/voc.py:295-305):
    smooth sinusoid images + sigma=2 noise, uint8-quantised then ImageNet-normalised; VOC-empirical label counts;
    half the boxes full, half cropped."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(S, dtype=torch.float32), torch.arange(S, dtype=torch.float32), indexing="ij")
    base = torch.zeros(b, 3, S, S)
    for _ in range(6):
        per = 64 + (400 - 64) * torch.rand(b, 3, 2, generator=g)
        ph = 2 * math.pi * torch.rand(b, 3, 2, generator=g)
        base += torch.sin(2 * math.pi * xx[None, None] / per[..., 0, None, None] + ph[..., 0, None, None]) * \
            torch.cos(2 * math.pi * yy[None, None] / per[..., 1, None, None] + ph[..., 1, None, None])
    mn, mx = base.amin(dim=(2, 3), keepdim=True), base.amax(dim=(2, 3), keepdim=True)
    img = (base - mn) / (mx - mn) * 255.0 + 2.0 * torch.randn(b, 3, S, S, generator=g)
    img = img.clamp(0, 255).floor()
    mean = torch.tensor(IMAGENET_MEAN)[None, :, None, None]
    std = torch.tensor(IMAGENET_STD)[None, :, None, None]
    wimg = (img - mean) / std
    contrast = 0.5 + torch.rand(b, 1, 1, 1, generator=g)
    simg = (((img - 127.5) * contrast + 127.5).clamp(0, 255).floor() - mean) / std
    labels = torch.zeros(b, C)
    for i in range(b):
        if dataset == "COCO":
            n_fg = int(min(7, 1 + torch.poisson(torch.tensor(1.9), generator=g).item()))
        else:
            n_fg = int(torch.multinomial(torch.tensor([0.60, 0.29, 0.09, 0.02]), 1, generator=g).item()) + 1
        labels[i, torch.randperm(C, generator=g)[:n_fg]] = 1
    boxes = torch.zeros(b, 4, dtype=torch.int16)
    for i in range(b):
        if i % 2 == 0:
            boxes[i] = torch.tensor([0, S, 0, S])
        else:
            r = torch.randint(0, S // 8 + 1, (4,), generator=g)
            boxes[i] = torch.tensor([int(r[0]), S - int(r[1]), int(r[2]), S - int(r[3])])
    return wimg.to(device), simg.to(device), labels.to(device), boxes


def smoke():
    """one tiny forward+backward of the flagship step on cuda:0 (reduced crop, same code path)."""
    dev = torch.device("cuda", 0)
    args = default_args("VOC12", crop_size=128)
    tr = CoSATrainer(args, dev)
    wimg, simg, lab, box = synthetic_batch(2, 128, 20, dev, seed=1)
    for _ in range(5):          # (the third call captures the teacher's hipGraph, the following ones replay it: the benchmarked configuration)
        logs = tr.step(wimg, simg, lab, box, n_iter=args.warmup_iters + 1)
    torch.cuda.synchronize()
    vals = {k: float(v) for k, v in logs.items() if torch.is_tensor(v) and v.numel() == 1}
    assert all(math.isfinite(v) for v in vals.values()), vals
    assert tr._graph is not None and all(bool(torch.isfinite(t).all()) for t in tr._s_out[:2]), "the replayed teacher pass must give finite CAMs"
    assert int(((logs["mask"] > 0) & (logs["mask"] < 255)).sum()) > 0, "a replayed step produced a label map without foreground"
    print("train_step smoke:", {k: round(v, 5) for k, v in vals.items()})
