"""Score two operand modes of the no-grad passes against each other on a CHECKPOINT, without training: the
stand-alone form of --teacher_check_iters, for the day released weights are at hand.

    python tools/teacher_check.py --checkpoint best_seg.pth [--mode fp16x3] [--check_mode fp16c8-x2 | fp32 | fp64] [--batches 8] [--criterion] \
        (--synthetic | --dataset VOC12 --voc12_root ... | --dataset COCO --coco_root ...) [--crop_size 448] [--batch_size 16] [--qk_gain G] \
        [launcher flags]

The checkpoint (best_seg.pth / best_cam.pth layout, read as cosa_amd.predict reads it: the restricted unpickler, --trust_checkpoint for the
full one) goes into two networks, one per mode; every batch runs what a training step derives from a teacher pass -- multi-scale CAMs,
cam2mask with the flags' thresholds, the cam-loss targets -- on both, and cosa_teacher_check accumulates the comparison.  Without
--checkpoint the networks keep the seed's random initialisation (a smoke run, not evidence).  Prints the summary
(seg_helper.teacher_check_summary) plus both mode names as ONE JSON line.  The criterion is the literal bar only.

--criterion evaluates the FULL criterion (DESIGN.md sections 3 and 20): every batch goes through three passes -- --mode, fp32 and fp64 -- and
cosa_conformance_planes applies the literal bar and the float64-bounded exemption to every active plane of cam and cam_aux.  Per batch and
set one line in the accuracy record's format (`planes N literal-ok L exempt E fail F [img i cls c: cond .. lit .. own .. fp64 .. bound ..
ok|FAIL]`); at the end ONE JSON object: the summary above (mode A against fp32) plus `criterion_planes` with the pooled counts, and `conforms` = no
failed plane, label agreement and pooled mask mIoU at the project's bars.

--qk_gain G (default 1: nothing changes) multiplies the q and k rows of every block's qkv projection by sqrt(G) before the networks are made,
so every attention logit is G times larger: the comparison, or with --criterion the criterion, then runs on sharp attention instead of a
random initialisation's near-uniform one.  tools/act_stats.py --qk_gain G says what |s| and row entropy that reached."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scale_qk(model, gain):
    """--qk_gain: cosa_amd.models.vit.qk_gain_ on the network the others are copied from"""
    from cosa_amd.models.vit import qk_gain_
    return qk_gain_(model, gain)


def get_parser():
    from cosa_amd import args as cosa_args
    p = cosa_args.get_parser()
    p.prog = "python tools/teacher_check.py"
    p.description = "Compare two operand modes of the teacher's no-grad passes on a checkpoint"
    p.add_argument("--checkpoint", type=str, default=None, help="best_seg.pth / best_cam.pth of a run (reference key names)")
    p.add_argument("--mode", type=str, default="fp16x3", help="operand mode A (any --teacher_precision value)")
    p.add_argument("--check_mode", type=str, default="auto", help="operand mode B; auto: bf16x3 against fp16x3, fp16x3 against anything else; fp32: the reference's arithmetic on the device "
                   "(the figure is then the criterion's own: DESIGN.md section 16)")
    p.add_argument("--criterion", action="store_true",
                   help="the full criterion per plane: a third pass in float64 (mode fp64) and the literal bar + exemption on the device; --check_mode is then fp32")
    p.add_argument("--batches", type=int, default=4)
    p.add_argument("--synthetic", action="store_true", help="synthetic batches (train_step.synthetic_batch) instead of a dataset")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the full unpickler for a checkpoint that torch.load(weights_only=True) refuses (runs code from the file)")
    p.add_argument("--qk_gain", type=float, default=1.0,
                   help="multiply every attention logit by G (the q and k rows of every qkv projection by sqrt(G)); 1: the weights as they are")
    return p


def main(argv=None):
    from cosa_amd import args as cosa_args
    parser = get_parser()
    argv = list(sys.argv[1:] if argv is None else argv)
    args, _ = cosa_args.handle_defaults(parser.parse_args(["teacher_check"] + argv))      # (the launcher's positional run name: of no use here)
    if args.batches < 1:
        parser.error("--batches must be >= 1")
    if args.usegmm:
        parser.error("--usegmm true: the adaptive thresholds are state of a training run; this tool compares at the fixed --high_thre / --low_thre")
    if args.criterion and args.check_mode not in ("auto", "fp32"):
        parser.error("--criterion scores --mode against fp32 and float64: --check_mode must be fp32 (or left at auto)")
    if not 0 < args.qk_gain < float("inf"):
        parser.error("--qk_gain must be a positive finite factor")
    if args.criterion and args.use_cammix:
        parser.error("--criterion: the criterion speaks of cam and cam_aux as multi_scale_camseg returns them, not of their --use_cammix mean")
    import torch
    from cosa_amd import _C
    from cosa_amd.main import _trainer_args, check_supported
    from cosa_amd.models import build_model
    from cosa_amd.models.PAR import PAR
    from cosa_amd.predict import load_checkpoint
    from cosa_amd.train_step import resolve_teacher_check_mode, resolve_teacher_precision, synthetic_batch, teacher_products
    from cosa_amd.utils import seg_helper, torch_helper
    check_supported(args)
    args.pretrained = False                         # (the checkpoint is the weights; without one, the seed's initialisation)
    args.mode = resolve_teacher_precision(args.mode, args.crop_size, bool(args.usepar))
    check_mode = "fp32" if args.criterion else resolve_teacher_check_mode(args.check_mode, args.mode)
    targs = _trainer_args(args)
    device = torch.device("cuda", 0)
    torch_helper.setup_seed(args.seed)
    first = build_model(targs)
    if args.checkpoint:
        load_checkpoint(first, args.checkpoint, trust=args.trust_checkpoint)
    scale_qk(first, args.qk_gain)
    models = []
    for mode in (args.mode, check_mode) + (("fp64",) if args.criterion else ()):      # networks of their own: shadows and buffers are keyed by parameter
        m = build_model(targs) if models else first
        if models:
            m.load_state_dict(first.state_dict())
        m.check_nograd_precision(mode)
        m = m.to(device).eval()
        for p_ in m.parameters():
            p_.requires_grad = False
        models.append(m.set_nograd_precision(mode))
    refine = PAR(num_iter=10, dilations=[1, 2, 4, 8, 12, 24]) if args.usepar else None
    K, S, b = args.num_classes, args.crop_size, args.batch_size
    if args.synthetic:
        batches = (synthetic_batch(b, S, K - 1, device, seed=args.seed + 1 + i, dataset=args.dataset) for i in range(args.batches))
    else:
        from cosa_amd.dataloaders import build_train_loader
        batches = (bt[1:] for bt in build_train_loader(args, device=device, num_workers=args.num_workers))
    counters = seg_helper.new_teacher_check(K, device)
    thresholds = ((args.high_thre, args.low_thre), (args.high_thre_aux, args.low_thre_aux))
    tgt_hw = (S // models[0].encoder.patch_size,) * 2
    buffers = ({}, {})
    n = 0
    pooled = {name: {"planes": 0, "literal_ok": 0, "exempt": 0, "failed": 0, "worst": {}, "over": []} for name in ("cam", "cam_aux")}
    for wimg, simg, cls_label, img_box in batches:
        if n == args.batches:
            break
        cls_label = cls_label.to(device)
        img_denorm = torch_helper.denormalize_img(simg) if refine is not None else simg
        out = []
        for i, m in enumerate(models[:2]):
            with _C.workspace_scope("mode%d" % i):
                out.append(teacher_products(m, targs, wimg, img_denorm, img_box, cls_label, thresholds, True, tgt_hw, buffers[i], refine))
        (cams_a, masks_a, tgt_a), (cams_b, masks_b, tgt_b) = out
        seg_helper.teacher_check((cams_a[0], cams_b[0]), (cams_a[1], cams_b[1]), (tgt_a, tgt_b), (masks_a[0], masks_b[0]),
                                 (masks_a[1], masks_b[1]) if masks_a[1] is not None else None, None if args.use_cammix else cls_label, img_box,
                                 counters, ignore_index=args.ignore_index)
        if args.criterion:
            with _C.workspace_scope("mode2"):
                c64, a64, _, sc_cam, sc_aux = seg_helper.multi_scale_camseg(models[2], wimg, targs.pseudo_scales, _active_labels=cls_label,
                                                                            _seg_scales=True, _return_scale=True)
            summ = seg_helper.conformance_summary({"cam": seg_helper.conformance_planes(cams_a[0], cams_b[0], c64, cls_label, *sc_cam),
                                                   "cam_aux": seg_helper.conformance_planes(cams_a[1], cams_b[1], a64, cls_label, *sc_aux)})
            for name, s in summ.items():
                print(f"criterion {args.mode:8s} S={S} b={b} batch={n:<2d} {name:8s}: {seg_helper.conformance_line(s)}", flush=True)
                pl = pooled[name]
                for k in ("planes", "literal_ok", "exempt", "failed"):
                    pl[k] += s[k]
                pl["worst"] = {k: max(v, pl["worst"].get(k, 0.0)) for k, v in s["worst"].items()}
                pl["over"] += [dict(r, batch=n) for r in s["over"]]
        n += 1
    res = dict(seg_helper.teacher_check_summary(counters, K), mode=args.mode, check_mode=check_mode, batches=n, crop_size=S, batch_size=b,
               checkpoint=os.path.abspath(args.checkpoint) if args.checkpoint else None, synthetic=bool(args.synthetic),
               **({"qk_gain": args.qk_gain} if args.qk_gain != 1.0 else {}))
    if args.criterion:
        failed = sum(pl["failed"] for pl in pooled.values())
        pairs = [res[p] for p in seg_helper.TEACHER_CHECK_PAIRS if res[p]["pix"]]
        res.update(criterion_planes=dict(pooled, planes_failed=failed, cam_bar=seg_helper.CAM_BAR, cond_max=seg_helper.COND_MAX,
                                         fp64_factor=seg_helper.FP64_FACTOR, scale_figures="peak / rawmax of the float64 pass"),
                   criterion="full: per active plane of cam / cam_aux the literal bar, or for conditioning > cond_max own-scale err <= bar and |A - "
                             "float64| <= bar + fp64_factor x |fp32 - float64| (criterion_planes); label agreement and mask mIoU of A against fp32",
                   exemption_evaluated=True,
                   conforms=bool(failed == 0 and all(p["agree"] >= seg_helper.AGREE_BAR and p["miou"] >= seg_helper.MIOU_BAR for p in pairs)))
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
