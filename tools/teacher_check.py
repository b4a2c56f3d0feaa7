"""Score two operand modes of the no-grad passes against each other on a CHECKPOINT, without training: the
stand-alone form of --teacher_check_iters, for the day released weights are at hand.

    python tools/teacher_check.py --checkpoint best_seg.pth [--mode fp16x3] [--check_mode fp16c8-x2 | fp32] [--batches 8] \
        (--synthetic | --dataset VOC12 --voc12_root ... | --dataset COCO --coco_root ...) [--crop_size 448] [--batch_size 16] [launcher flags]

The checkpoint (best_seg.pth / best_cam.pth layout, read as cosa_amd.predict reads it: the restricted unpickler, --trust_checkpoint for the
full one) goes into two networks, one per mode; every batch runs what a training step derives from a teacher pass -- multi-scale CAMs,
cam2mask with the flags' thresholds, the cam-loss targets -- on both, and cosa_teacher_check accumulates the comparison.  Without
--checkpoint the networks keep the seed's random initialisation (a smoke run, not evidence).  Prints the summary
(seg_helper.teacher_check_summary) plus both mode names as ONE JSON line.  The criterion is the literal bar only."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def get_parser():
    from cosa_amd import args as cosa_args
    p = cosa_args.get_parser()
    p.prog = "python tools/teacher_check.py"
    p.description = "Compare two operand modes of the teacher's no-grad passes on a checkpoint"
    p.add_argument("--checkpoint", type=str, default=None, help="best_seg.pth / best_cam.pth of a run (reference key names)")
    p.add_argument("--mode", type=str, default="fp16x3", help="operand mode A (any --teacher_precision value)")
    p.add_argument("--check_mode", type=str, default="auto", help="operand mode B; auto: bf16x3 against fp16x3, fp16x3 against anything else; fp32: the reference's arithmetic on the device "
                   "(the figure is then the criterion's own: DESIGN.md section 16)")
    p.add_argument("--batches", type=int, default=4)
    p.add_argument("--synthetic", action="store_true", help="synthetic batches (train_step.synthetic_batch) instead of a dataset")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the full unpickler for a checkpoint that torch.load(weights_only=True) refuses (runs code from the file)")
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
    check_mode = resolve_teacher_check_mode(args.check_mode, args.mode)
    targs = _trainer_args(args)
    device = torch.device("cuda", 0)
    torch_helper.setup_seed(args.seed)
    first = build_model(targs)
    if args.checkpoint:
        load_checkpoint(first, args.checkpoint, trust=args.trust_checkpoint)
    models = []
    for mode in (args.mode, check_mode):            # two networks of their own: shadows and buffers are keyed by parameter
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
    for wimg, simg, cls_label, img_box in batches:
        if n == args.batches:
            break
        cls_label = cls_label.to(device)
        img_denorm = torch_helper.denormalize_img(simg) if refine is not None else simg
        out = []
        for i, m in enumerate(models):
            with _C.workspace_scope("mode%d" % i):
                out.append(teacher_products(m, targs, wimg, img_denorm, img_box, cls_label, thresholds, True, tgt_hw, buffers[i], refine))
        (cams_a, masks_a, tgt_a), (cams_b, masks_b, tgt_b) = out
        seg_helper.teacher_check((cams_a[0], cams_b[0]), (cams_a[1], cams_b[1]), (tgt_a, tgt_b), (masks_a[0], masks_b[0]),
                                 (masks_a[1], masks_b[1]) if masks_a[1] is not None else None, None if args.use_cammix else cls_label, img_box,
                                 counters, ignore_index=args.ignore_index)
        n += 1
    res = dict(seg_helper.teacher_check_summary(counters, K), mode=args.mode, check_mode=check_mode, batches=n, crop_size=S, batch_size=b,
               checkpoint=os.path.abspath(args.checkpoint) if args.checkpoint else None, synthetic=bool(args.synthetic))
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
