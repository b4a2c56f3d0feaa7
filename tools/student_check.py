"""Score the student's TRAINING forward (bf16 operands over an fp32 residual stream) against a no-grad forward of the same weights on
another operand mode, on a CHECKPOINT, without training: the stand-alone form of --student_check_iters.

    python tools/student_check.py --checkpoint best_seg.pth [--check_mode fp32 | fp64 | bf16 | ...] [--batches 1] \
        (--synthetic | --dataset VOC12 --voc12_root ... | --dataset COCO --coco_root ...) [--crop_size 448] [--batch_size 16] [launcher flags]

The checkpoint (best_seg.pth / best_cam.pth layout, read as cosa_amd.predict reads it: the restricted unpickler, --trust_checkpoint for the
full one) goes into the student AND the teacher of a trainer; every batch runs one training forward with its losses (CoSATrainer.forward_losses:
no backward, no optimizer step, so the weights never move) and one check (CoSATrainer._student_check).  Without --checkpoint the networks keep the
seed's random initialisation (a smoke run, not evidence).  Prints the summary (seg_helper.student_check_summary) plus the mode names as ONE
JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def get_parser():
    from cosa_amd import args as cosa_args
    p = cosa_args.get_parser()
    p.prog = "python tools/student_check.py"
    p.description = "Compare the student's training forward with a no-grad forward of the same weights on a checkpoint"
    p.add_argument("--checkpoint", type=str, default=None, help="best_seg.pth / best_cam.pth of a run (reference key names)")
    p.add_argument("--check_mode", type=str, default="fp32", help="operand mode of the check pass (any --student_check_mode value; fp64: a float64 pass, DESIGN.md section 20)")
    p.add_argument("--batches", type=int, default=1)
    p.add_argument("--synthetic", action="store_true", help="synthetic batches (train_step.synthetic_batch) instead of a dataset")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the full unpickler for a checkpoint that torch.load(weights_only=True) refuses (runs code from the file)")
    return p


def main(argv=None):
    from cosa_amd import args as cosa_args
    parser = get_parser()
    argv = list(sys.argv[1:] if argv is None else argv)
    args, _ = cosa_args.handle_defaults(parser.parse_args(["student_check"] + argv))      # (the launcher's positional run name: of no use here)
    if args.batches < 1:
        parser.error("--batches must be >= 1")
    if args.usegmm:
        parser.error("--usegmm true: the adaptive thresholds are state of a training run; this tool runs at the fixed --high_thre / --low_thre")
    import torch
    from cosa_amd.main import _trainer_args, check_supported
    from cosa_amd.predict import load_checkpoint
    from cosa_amd.train_step import CoSATrainer, synthetic_batch
    from cosa_amd.utils import seg_helper
    check_supported(args)
    args.pretrained = False                         # (the checkpoint is the weights; without one, the seed's initialisation)
    args.student_check_iters, args.student_check_mode = 1, args.check_mode
    args.teacher_graph = False                      # (a handful of forwards: nothing to capture)
    targs = _trainer_args(args)
    device = torch.device("cuda", 0)
    tr = CoSATrainer(targs, device, seed=args.seed)
    if args.checkpoint:
        load_checkpoint(tr.student, args.checkpoint, trust=args.trust_checkpoint)
        tr.model_AN.load_state_dict(tr.student.state_dict())
        for sh in (tr._student_shadows, tr._teacher_shadows):       # the masters were written behind the shadows' back
            if sh is not None:
                sh.refresh(force=True)
    K, S, b = args.num_classes, args.crop_size, args.batch_size
    if args.synthetic:
        batches = (synthetic_batch(b, S, K - 1, device, seed=args.seed + 1 + i, dataset=args.dataset) for i in range(args.batches))
    else:
        from cosa_amd.dataloaders import build_train_loader
        batches = (bt[1:] for bt in build_train_loader(args, device=device, num_workers=args.num_workers))
    n = 0
    for wimg, simg, cls_label, img_box in batches:
        if n == args.batches:
            break
        cls_label = cls_label.to(device)
        tr.forward_losses(wimg, simg, cls_label, img_box, targs.warmup_iters + 1)      # (past warm-up: of no consequence, the weights never move)
        tr._student_check()
        n += 1
    res = dict(tr.student_check(), mode="bf16", check_mode=args.check_mode, batches=n, crop_size=S, batch_size=b,
               checkpoint=os.path.abspath(args.checkpoint) if args.checkpoint else None, synthetic=bool(args.synthetic))
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
