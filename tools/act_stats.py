"""Activation range and attention sharpness of a CHECKPOINT, without training: the stand-alone form of
--act_stats_iters.

    python tools/act_stats.py [--checkpoint best_seg.pth] (--synthetic | --dataset VOC12 --voc12_root ... | --dataset COCO --coco_root ...) \
        [--batches 4] [--qk_gain G] [--json] [--crop_size 448] [--batch_size 16] [launcher flags]

The checkpoint (best_seg.pth / best_cam.pth layout, read as cosa_amd.predict reads it; without --checkpoint the seed's random
initialisation) goes into one network in mode "fp32" whose encoder carries an ActProbe; every batch runs the teacher's multi-scale pass
(--pseudo_scales, images and mirror images) and the probe's two reductions accumulate per block: the range of q / k / v / o / h / x against
fp16's 65504 and 2^-14, per head the largest attention logit, the mean normalised row entropy, the mean top-1 probability and the share of
peaked rows.  Prints one line per block and then ONE JSON line with the full summary (seg_helper.act_stats_summary); --json prints the
JSON line alone.

--qk_gain G (default 1: nothing changes) multiplies the q and k rows of every block's qkv projection by sqrt(G) first, so every attention
logit is G times larger: what tools/teacher_check.py --qk_gain G then compares on."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scale_qk(model, gain):
    """--qk_gain: cosa_amd.models.vit.qk_gain_ on the network the pass runs on"""
    from cosa_amd.models.vit import qk_gain_
    return qk_gain_(model, gain)


def get_parser():
    from cosa_amd import args as cosa_args
    p = cosa_args.get_parser()
    p.prog = "python tools/act_stats.py"
    p.description = "Activation range and attention sharpness of the teacher's fp32 pass on a checkpoint"
    p.add_argument("--checkpoint", type=str, default=None, help="best_seg.pth / best_cam.pth of a run (reference key names); none: the seeded initialisation")
    p.add_argument("--batches", type=int, default=4)
    p.add_argument("--synthetic", action="store_true", help="synthetic batches (train_step.synthetic_batch) instead of a dataset")
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the full unpickler for a checkpoint that torch.load(weights_only=True) refuses (runs code from the file)")
    p.add_argument("--qk_gain", type=float, default=1.0,
                   help="multiply every attention logit by G (the q and k rows of every qkv projection by sqrt(G)); 1: the weights as they are")
    p.add_argument("--json", action="store_true", help="print the JSON summary alone")
    return p


def layer_lines(summary):
    """one line per block: the largest |x| per site, then over its heads the largest logit, the mean entropy and top-1, the peaked share"""
    lines = []
    for i, layer in enumerate(summary["layers"]):
        sites = " ".join("%s %9.3e" % (name, e["absmax"]) for name, e in layer["sites"].items())
        heads = [h for h in layer["heads"] if h["rows"]]
        rows = sum(h["rows"] for h in heads)
        if rows:
            mean = lambda k: sum(h[k] * h["rows"] for h in heads) / rows
            att = "max|s| %7.2f  ent %.3f (min %.3f)  top1 %.3f  peaked %.3f" % (
                max(h["smax"] for h in heads), mean("ent"), min(h["ent"] for h in heads), mean("top1"), mean("peaked"))
        else:
            att = "no rows"
        bad = sum(e["over"] + e["nonfinite"] for e in layer["sites"].values()) + sum(h["nonfinite_rows"] for h in layer["heads"])
        lines.append("L%-2d %s | %s%s" % (i, sites, att, "  over/nonfinite %d" % bad if bad else ""))
    return lines


def main(argv=None):
    from cosa_amd import args as cosa_args
    parser = get_parser()
    argv = list(sys.argv[1:] if argv is None else argv)
    args, _ = cosa_args.handle_defaults(parser.parse_args(["act_stats"] + argv))      # (the launcher's positional run name: of no use here)
    if args.batches < 1:
        parser.error("--batches must be >= 1")
    if not 0 < args.qk_gain < float("inf"):
        parser.error("--qk_gain must be a positive finite factor")
    import torch
    from cosa_amd import _C
    from cosa_amd.main import _trainer_args, check_supported
    from cosa_amd.models import build_model
    from cosa_amd.models.vit import ActProbe
    from cosa_amd.predict import load_checkpoint
    from cosa_amd.train_step import synthetic_batch
    from cosa_amd.utils import seg_helper, torch_helper
    check_supported(args)
    args.pretrained = False                         # (the checkpoint is the weights; without one, the seed's initialisation)
    targs = _trainer_args(args)
    device = torch.device("cuda", 0)
    torch_helper.setup_seed(args.seed)
    model = build_model(targs)
    if args.checkpoint:
        load_checkpoint(model, args.checkpoint, trust=args.trust_checkpoint)
    scale_qk(model, args.qk_gain)
    model.check_nograd_precision("fp32")
    model = model.to(device).eval()
    for p_ in model.parameters():
        p_.requires_grad = False
    model.set_nograd_precision("fp32")
    depth, heads = len(model.encoder.blocks), model.encoder.num_heads
    counters = seg_helper.new_act_stats(depth, heads, device)
    model.encoder.act_probe = ActProbe(depth, heads, table=seg_helper.act_stats_table(counters, depth, heads))
    K, S, b = args.num_classes, args.crop_size, args.batch_size
    if args.synthetic:
        batches = (synthetic_batch(b, S, K - 1, device, seed=args.seed + 1 + i, dataset=args.dataset) for i in range(args.batches))
    else:
        from cosa_amd.dataloaders import build_train_loader
        batches = (bt[1:] for bt in build_train_loader(args, device=device, num_workers=args.num_workers))
    n = 0
    for wimg, _simg, cls_label, _img_box in batches:
        if n == args.batches:
            break
        with _C.workspace_scope("act_stats"):
            seg_helper.multi_scale_camseg(model, wimg, targs.pseudo_scales, _active_labels=cls_label.to(device), _seg_scales=True)
        counters[-1:] += 1
        n += 1
    summary = seg_helper.act_stats_summary(counters, depth, heads)
    res = dict(summary, mode="fp32", batches=n, crop_size=S, batch_size=b, qk_gain=args.qk_gain,
               checkpoint=os.path.abspath(args.checkpoint) if args.checkpoint else None, synthetic=bool(args.synthetic))
    if not args.json:
        for line in layer_lines(summary):
            print(line, flush=True)
        print(seg_helper.act_stats_line(summary).strip(), flush=True)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
