"""Command-line surface of the reference launcher (args.py:82-165 / args_coco.py, `handle_defaults` :168-180) as ONE table.

Every flag of the reference is accepted with the same name, type and default (VOC12 column; the COCO column lists the seven defaults
args_coco.py changes); flags left unset on the command line take the table's default and the ones that were set are reported as
"changed", as the reference does.  `--usepar`, inert in the reference (args.py:67 is never read by main.py), is live here: it selects
`refine_model=PAR(num_iter=10, dilations=[1,2,4,8,12,24])` for both cam2mask calls."""
import argparse


def str2bool(v):
    if isinstance(v, bool):
        return v
    if v.lower() in ('yes', 'true', 't', 'y', '1'):
        return True
    if v.lower() in ('no', 'false', 'f', 'n', '0'):
        return False
    raise argparse.ArgumentTypeError('Boolean value expected.')


_LISTF = ("floats", )          # marker: nargs='+' of float
# (flag, type, VOC12 default)            type None = store_true flag
FLAGS = [
    # model
    ("model", str, 'vit'), ("backbone", str, 'vit_base_patch16_224'), ("decoder", str, 'LargeFOV'), ("pretrained", str2bool, True),
    ("freeze_norm", None, False), ("aux_layer", int, -3), ("isgap", str2bool, False),
    # misc
    ("finalval", str2bool, True), ("seed", int, 0), ("random_seed", None, False), ("work_dir", str, ''), ("output_dir", str, None),
    ("device", str, 'cuda'), ("save_per_eval", int, 10), ("eval_iters", int, 2000), ("turnon_rawcam", None, False), ("fasteval", None, False),
    ("valfull", None, False), ("eval_threshold_filters", _LISTF, None),
    # data
    ("dataset", str, 'VOC12'), ("coco_root", str, ''), ("voc12_root", str, ''), ("crop_size", int, 448), ("scales", tuple, (0.5, 2)),
    ("ignore_index", int, 255), ("num_classes", int, 21), ("batch_size", int, 2), ("num_workers", int, 4),
    # train
    ("max_iters", int, 40000), ("warmup_iters", int, 6000), ("lr", float, 6e-5), ("lrscale", float, 10.), ("min_mult", float, 0.),
    ("wt_dec", float, 1e-2), ("wt_dec_mult", float, 1.), ("cam_weight", float, 0.05), ("camloss_version", str, 'v1'),
    ("seg_weight", float, 0.1), ("segfg_alpha", float, 0.5), ("reg_weight", float, 0.05), ("momentum", float, 0.9994),
    ("pseudo_scales", _LISTF, [1.0, 0.5, 1.5]), ("high_thre", float, 0.7), ("high_thre_aux", float, 0.7), ("bkg_thre", float, 0.5),
    ("low_thre", float, 0.25), ("low_thre_aux", float, 0.25), ("usegmm", str2bool, False), ("usegmmaux", str2bool, False),
    ("gmmscale", int, 16), ("gmmfilter_thre", float, 0.05), ("gmmemadecay", float, 0.99), ("queue_update_ratio", int, 100),
    ("camweight_beta", float, 1.0), ("par_downscale", int, 2), ("usepar", str2bool, False), ("aux_cam2seg", str2bool, True),
    ("aux_cam2seg_traditional", str2bool, True), ("aux_cam2seg_alpha", float, 0.5), ("aux_seg2cam", str2bool, False),
    ("aux_seg2cam_alpha", float, 0.5), ("seg_softmaxtemp", float, 0.01), ("segconf_thre", float, 0.25), ("after_softmax", str2bool, False),
    ("detach", str, 'none'), ("use_cammix", str2bool, False), ("oracle_camloss_version", str, 'v1'),
    ("oracle_camloss_detach", str2bool, False), ("oracle_camloss_bgmax", str2bool, True), ("find_unused", str2bool, True),
]
COCO_DEFAULTS = dict(eval_iters=6000, dataset='COCO', num_classes=81, batch_size=4, max_iters=60000, warmup_iters=10000, high_thre=0.65)
# what this build adds (none of them changes the reference's defaults)
EXTRA = [
    ("pretrained_path", str, None),          # local timm ViT-B/16 checkpoint for --pretrained true (no network here)
    ("name_list_dir", str, None),            # split lists / cls_labels_onehot.npy (default: ./dataloaders/<dataset>/ as the reference)
    ("teacher_precision", str, "auto"), # auto (fp16x3: train_step.resolve_teacher_precision) | bf16 | fp16 | bf16x3 | fp16x3 | fp16c8[-n[mk]|-xn[mk]] | fp16c4[...] | fp32 (fp32 operands on the f32-input MFMA: the reference's arithmetic, several times the default's teacher time): operand precision of the teacher's no-grad passes;
                                             # the default meets the 1e-3 / IoU 0.999 tolerance against the fp32 reference, bf16 (faster) does not
    ("log_iters", int, 20),
    # full-state checkpoints (cosa_amd/checkpoint.py): bit-exact resumption
    ("save_iters", int, 0),                  # write <output_dir>/state_<iteration>.cosa every N iterations; 0: never (nothing changes)
    ("keep_states", int, 2),                 # complete state files kept; older ones go once a newer one is in place
    ("resume", str, None),                   # a state file, or "auto": the newest complete state_*.cosa of the output directory, if any
    # the gradient guard, decided on the device by the optimizer's own kernels; both off: nothing changes
    ("clip_grad_norm", float, 0.0),          # clip the gradients by their global L2 norm to this bound (clip_grad_norm_'s formula); 0: off
    ("skip_nonfinite", str2bool, False),     # refuse a step whose gradients hold an inf / NaN: weights, moments and the EMA teacher stay
    # per-step pseudo-label statistics and the teacher finite check; off: nothing changes
    ("label_stats", str2bool, False),        # count ignore / bg / fg, main-aux agreement, the student's IoU and non-finite CAMs on the device;
                                             # logged and written to <output_dir>/label_stats.jsonl every log_iters; with --skip_nonfinite a
                                             # step whose teacher CAMs hold an inf / NaN is refused
    # per-tensor diagnostics; off: nothing changes
    ("tensor_stats", str2bool, False),       # per-tensor gradient / weight norms and the EMA gap, sampled on the step that closes each log_iters
                                             # interval, and -- behind the gradient guard -- which tensor held the inf / NaN of a refused step;
                                             # logged and written to <output_dir>/tensor_stats.jsonl
    # gradient accumulation; 1: nothing changes
    ("accum_steps", int, 1),                 # micro-batches of --batch_size per optimizer step: their mean gradient is applied once, so the
                                             # effective batch is batch_size x accum_steps x world; all *_iters flags stay in optimizer steps
    # the teacher-precision monitor; 0: nothing changes
    ("teacher_check_iters", int, 0),         # every N-th optimizer step runs the teacher's pass a second time on --teacher_check_mode operands and
                                             # scores the two passes against each other on the device (literal 1e-3 bar, label agreement, mask
                                             # mIoU); logged and written to <output_dir>/teacher_check.jsonl every log_iters; training is untouched
    ("teacher_check_mode", str, "auto"),     # any --teacher_precision value; auto: bf16x3 against an fp16x3 teacher (the same kernels with fp32's
                                             # exponent range: an fp16 overflow shows), fp16x3 against every other teacher mode; fp32: the teacher's mode against
                                             # the reference's arithmetic -- the figure is then the conformance criterion's own;
                                             # fp64: against a float64 pass on the f64 MFMA (section 20; a check mode only: --teacher_precision fp64 is refused)
    # the student-forward monitor; 0: nothing changes
    ("student_check_iters", int, 0),         # every N-th optimizer step runs the student's weights of that step through a second, no-grad forward on
                                             # --student_check_mode operands over the batch it trained on and scores the training forward against it on the
                                             # device (per-tensor rel-L2, seg argmax agreement, loss terms); logged and written to
                                             # <output_dir>/student_check.jsonl every log_iters; training is untouched
    ("student_check_mode", str, "fp32"),     # any --teacher_precision value but auto; fp32: the reference's arithmetic on the fp32 masters; bf16: the no-grad
                                             # path evaluate(s_or_t='s') runs
    # pseudo labels against ground truth; off: nothing changes, no PNG is read
    ("gt_stats", str2bool, False),           # decode each training image's ground-truth map, crop it on the device with the image's own draws and count
                                             # the main / auxiliary pseudo labels and the student's prediction against it (confusion matrices, mIoU);
                                             # logged and written to <output_dir>/gt_stats.jsonl every log_iters; training is untouched
    ("gt_dir", str, None),                   # where --gt_stats finds <name>.png (default: the dataset root's SegmentationClassAug for VOC12,
                                             # SegmentationClass/train2014 for COCO: what the Seg datasets read)
    # activation range and attention sharpness; 0: nothing changes
    ("act_stats_iters", int, 0),             # every N-th optimizer step runs the teacher's weights of that step through an fp32 pass of its own over the
                                             # weak images and reduces, per block, the range of q / k / v / o / h / x (bits of headroom under fp16's 65504)
                                             # and per head the attention logits' magnitude and row entropy; logged and written to
                                             # <output_dir>/act_stats.jsonl every log_iters; training is untouched
    # the gradient check; 0: nothing changes
    ("grad_check_iters", int, 0),            # every N-th optimizer step differences the step's objective along the step's own raw gradient on a
                                             # no-grad network of its own (four perturbed weight sets per direction, written on the device) and reports
                                             # r = <grad L, g> / <g, g>: 1 for an exact gradient; logged with the next log line and written to
                                             # <output_dir>/grad_check.jsonl; training is untouched; a world of one only
    ("grad_check_mode", str, "fp64"),        # fp64 | fp32: the arithmetic of the differenced forward (a 16-bit one is rounding noise: refused)
    ("grad_check_dirs", str, "all"),         # all: one direction, every tensor with a gradient; sites: plus embed, block<i>, norm, decoder, heads
    ("grad_check_rho", float, 1e-5),         # the relative step |s g| / |w| of the difference (utils/grad_check.py: DEFAULT_RHO)
    # per-image evaluation scores; off: nothing changes
    ("image_scores", str2bool, False),       # every evaluate() of the run also counts each image's label maps against its ground truth on the
                                             # device and writes <output_dir>/<iteration>/image_scores_<s|t>.jsonl and iou_dic_<s|t>.pth (the
                                             # reference's iou_dic.pth); read them with tools/image_scores.py
    # per-image Boundary IoU counters; off: nothing changes
    ("boundary_scores", str2bool, False),    # every evaluate() of the run also counts the same maps over the pixels within d of each map's own
                                             # contours and writes <output_dir>/<iteration>/boundary_scores_<s|t>.jsonl (the same format)
    ("boundary_ratio", float, 0.02),         # d = max(1, round(ratio * the image's diagonal)), in (0, 1)
    ("boundary_d", int, 0),                  # a fixed d in pixels, 1..64; 0: use the ratio
    # the supervised-contrastive token loss: this build's own objective, beyond the reference; 0: nothing changes
    ("tokcon_weight", float, 0.0),           # weight of the term on the student's final patch tokens, labelled from the step's main pseudo-label
                                             # map (0 during warm-up, like seg / cam / reg); > 0 adds `tok_loss` to the log line
    ("tokcon_temp", float, 0.5),             # its temperature, in [0.01, 10]
    ("tokcon_purity", float, 1.0),           # the share of a token's pixels one class must hold for the token to take its label, in (0.5, 1]
    # the reliability-weighted seg loss: the reference's seg_weightloss under this build's own weight; off: nothing changes
    ("seg_reliability", str2bool, False),    # weigh each pseudo-labelled pixel's seg loss by how far its CAM lies from the threshold it passed,
                                             # raised to the reference's --camweight_beta (in [0, 8]; read with this switch on only); the mean
                                             # weights are logged and written to <output_dir>/seg_reliability.jsonl at each evaluation
    ("seg_reliability_floor", float, 0.0),   # the weight of a pixel the CAM does not support (w = floor + (1 - floor) r^beta), in [0, 1)
    # the soft-label seg loss: the reference's seg_softloss against the teacher's own segmentation; 0: nothing changes
    ("seg_soft_weight", float, 0.0),         # weight of the student's seg logits' cross-entropy against softmax(mean of the teacher's seg passes / T)
                                             # over the background and the image's classes, class-balanced by --segfg_alpha (0 during warm-up, like
                                             # seg / cam / reg); > 0 adds `soft_loss` to the log line
    ("seg_soft_temp", float, 1.0),           # its temperature T, in [0.05, 20]
    ("seg_soft_conf", float, 0.0),           # a pixel whose largest target probability is not above this takes no part, in [0, 1); 0: no gate
]


def get_parser():
    p = argparse.ArgumentParser('End to end weakly supervised segmentation model (cosa_amd launcher)', add_help=True)
    p.add_argument('name', type=str)
    for flag, typ, _default in FLAGS + EXTRA:
        if typ is None:
            p.add_argument('--' + flag, action='store_true', default=None)
        elif typ is _LISTF:
            p.add_argument('--' + flag, type=float, metavar='N', nargs='+', default=None)
        elif typ is tuple:
            p.add_argument('--' + flag, type=float, metavar='N', nargs=2, default=None)
        else:
            p.add_argument('--' + flag, type=typ, default=None)
    return p


def handle_defaults(args):
    """args.py:168-180: unset flags take their default (COCO's when --dataset COCO); returns (args, {flag: value given on the command line})"""
    table = {f: d for f, _t, d in FLAGS + EXTRA}
    dataset = args.dataset if args.dataset is not None else table["dataset"]
    if dataset == 'COCO':
        table.update(COCO_DEFAULTS)
    elif dataset != 'VOC12':
        raise NotImplementedError(dataset)
    changed = {}
    for k, v in table.items():
        cur = getattr(args, k)
        if cur is None:
            setattr(args, k, v)
        else:
            if k == "scales":
                cur = tuple(cur)
                setattr(args, k, cur)
            changed[k] = cur
    return args, changed


def parse(argv=None):
    return handle_defaults(get_parser().parse_args(argv))
