"""Check the training step's GRADIENT against central differences of its loss, on a CHECKPOINT, without training: the
stand-alone form of --grad_check_iters.

    python tools/grad_check.py [--checkpoint best_seg.pth] (--synthetic | --dataset VOC12 --voc12_root ... | --dataset COCO --coco_root ...) \
        --batches N [--dirs all | sites] [--mode fp64 | fp32] [--rho R] [--crop_size 448] [--batch_size 16] [launcher flags]

The checkpoint (best_seg.pth / best_cam.pth layout, read as cosa_amd.predict reads it) goes into the student AND the teacher of a trainer;
every batch runs one training forward with its losses, one backward and one check (CoSATrainer.grad_check_batch: no optimizer step, so the
weights never move).  Without --checkpoint the networks keep the seed's random initialisation.  Prints a table per batch -- r_star = <grad L,
g> / <g, g> per direction, 1 for an exact gradient -- and the batches' summaries as ONE JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def get_parser():
    from cosa_amd import args as cosa_args
    p = cosa_args.get_parser()
    p.prog = "python tools/grad_check.py"
    p.description = "Check the step's gradient against float64 / fp32 central differences of its loss on a checkpoint"
    p.add_argument("--checkpoint", type=str, default=None, help="best_seg.pth / best_cam.pth of a run (reference key names)")
    p.add_argument("--mode", type=str, default="fp64", help="arithmetic of the differenced forward: fp64 | fp32")
    p.add_argument("--dirs", type=str, default="all", help="all | sites (plus embed, block<i>, norm, decoder, heads)")
    p.add_argument("--rho", type=float, default=None, help="relative step of the difference (default: --grad_check_rho's)")
    p.add_argument("--batches", type=int, default=1)
    p.add_argument("--warmup_step", action="store_true", help="check the warm-up objective (classification losses only)")
    p.add_argument("--synthetic", action="store_true", help="synthetic batches (train_step.synthetic_batch) instead of a dataset")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the full unpickler for a checkpoint that torch.load(weights_only=True) refuses (runs code from the file)")
    return p


def main(argv=None):
    from cosa_amd import args as cosa_args
    parser = get_parser()
    argv = list(sys.argv[1:] if argv is None else argv)
    args, _ = cosa_args.handle_defaults(parser.parse_args(["grad_check"] + argv))         # (the launcher's positional run name: of no use here)
    if args.batches < 1:
        parser.error("--batches must be >= 1")
    if args.usegmm:
        parser.error("--usegmm true: the adaptive thresholds are state of a training run; this tool runs at the fixed --high_thre / --low_thre")
    import torch
    from cosa_amd.main import _trainer_args, check_supported
    from cosa_amd.predict import load_checkpoint
    from cosa_amd.train_step import CoSATrainer, synthetic_batch
    from cosa_amd.utils import grad_check as gcheck
    args.grad_check_iters, args.grad_check_mode, args.grad_check_dirs = 1, args.mode, args.dirs
    if args.rho is not None:
        args.grad_check_rho = args.rho
    args.accum_steps = 1
    check_supported(args)
    args.pretrained = False                         # (the checkpoint is the weights; without one, the seed's initialisation)
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
        batches = (bt[1:5] for bt in build_train_loader(args, device=device, num_workers=args.num_workers))
    n_iter = 0 if args.warmup_step else targs.warmup_iters + 1
    out = []
    for wimg, simg, cls_label, img_box in batches:
        if len(out) == args.batches:
            break
        summary = tr.grad_check_batch(wimg, simg, cls_label.to(device), img_box, n_iter)
        print(f"batch {len(out)}:\n" + gcheck.table_text(summary), flush=True)
        out.append(summary)
    res = gcheck.jsonable(dict(mode=targs.grad_check_mode, rho=targs.grad_check_rho, dirs=targs.grad_check_dirs, batches=out, crop_size=S,
                               batch_size=b, checkpoint=os.path.abspath(args.checkpoint) if args.checkpoint else None,
                               synthetic=bool(args.synthetic)))
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
