"""Launcher of the MI355X-native trainer -- the reference's `main.py` (set-up :24-104, loop :106-252, logging :254-311, evaluation cadence
:313-383, finaleval :401-433) on cosa_amd's own loop:

    torchrun --master_port $PORT --nproc_per_node=8 -m cosa_amd.main EXP_VOC --work_dir $DIR --dataset VOC12 \
        --voc12_root $HOME/data/VOCdevkit/VOC2012 --max_iters 32000 --aux_layer -4            (run_voc.sh:7-11)

Same flags and defaults (cosa_amd/args.py), same artefacts in <work_dir>/<name>/ (best_seg.pth, best_cam.pth, log_val.txt,
loss_dataframe.pt).  What differs is where the work runs: one process per GPU over RCCL (`backend="nccl"` is RCCL on ROCm), the device
input pipeline, the fused training step (CoSATrainer.step: no per-iteration host sync -- the losses and the classification AP of an
iteration stay on the device and are read back once per `log_iters`), device-resident evaluation.  `--usepar true` is live."""
import datetime
import os
import random
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist

from . import args as cosa_args
from . import checkpoint
from . import monitors
from .dataloaders import build_test_loader, build_train_loader, build_val_loader
from .evaluation_engine import evaluate
from .models import build_model
from .models.backbones import get_backbone
from .train_step import CoSATrainer, check_iters, default_args, refuse_fp64_teacher, reliability_settings, seg_soft_settings, tokcon_settings
from .utils import evaluation
from .utils import grad_check as gcheck
from .utils import torch_helper


def init_distributed_mode(args):
    """utils/misc.py:405-445: env:// rendezvous from torchrun's RANK / WORLD_SIZE / LOCAL_RANK (or SLURM_PROCID); one process per GPU.
    A plain `python -m cosa_amd.main` runs as a world of one (the reference raises NotImplementedError there)."""
    if 'RANK' in os.environ and 'WORLD_SIZE' in os.environ:
        args.rank, args.world_size, args.gpu = int(os.environ["RANK"]), int(os.environ['WORLD_SIZE']), int(os.environ['LOCAL_RANK'])
    elif 'SLURM_PROCID' in os.environ:
        args.rank = int(os.environ['SLURM_PROCID'])
        args.world_size = int(os.environ.get('SLURM_NTASKS', '1'))
        args.gpu = args.rank % max(torch.cuda.device_count(), 1)
    else:
        args.rank, args.world_size, args.gpu, args.distributed = 0, 1, 0, False
        torch.cuda.set_device(0)
        return
    args.distributed = True
    args.gpu = args.gpu % max(torch.cuda.device_count(), 1)          # (single-card rehearsals put several ranks on one card)
    torch.cuda.set_device(args.gpu)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    backend = os.environ.get("COSA_DIST_BACKEND", "nccl")             # "nccl" == RCCL; gloo only for single-card rehearsals
    print(f'| distributed init (rank {args.rank}): env://, backend {backend}', flush=True)
    dist.init_process_group(backend, **({"device_id": torch.device("cuda", args.gpu)} if backend == "nccl" else {}))
    dist.barrier()


def _trainer_args(args):
    """the parsed flags + the build's own switches (compute dtype, fused paths) in the form CoSATrainer reads"""
    return default_args(args.dataset, **{k: v for k, v in vars(args).items() if k != "dataset"})


def check_supported(args):
    """Flags this build parses but does not honour must not be accepted silently (the reference dispatches on them, main.py:216-224,338):
    a run that asks for another objective or for dumps fails here instead of training / evaluating something else."""
    if args.camloss_version != 'v1':
        raise NotImplementedError(f"--camloss_version {args.camloss_version}: only cam_loss v1 is built (the reference dispatches "
                                  f"cam_lossv2 / cam_lossv3_wrap with --segconf_thre, main.py:216-224)")
    if args.turnon_rawcam:
        raise NotImplementedError("--turnon_rawcam: raw-CAM dumps (evaluate(save_rawcam=True)) are not part of the device evaluation path")
    if args.model != 'vit' or args.decoder != 'LargeFOV':
        raise NotImplementedError("only --model vit --decoder LargeFOV (the run scripts' configuration) is built")
    get_backbone(args.backbone)                                   # NotImplementedError listing the built encoders
    if getattr(args, "accum_steps", 1) < 1:
        raise ValueError(f"--accum_steps {args.accum_steps}: a positive number of micro-batches per optimizer step")
    for which in ("teacher", "student", "act_stats", "grad"):
        check_iters(args, which, flag="--")
    if check_iters(args, "grad") > 0:
        gcheck.check_mode(getattr(args, "grad_check_mode", "fp64"))
        gcheck.check_dirs(getattr(args, "grad_check_dirs", "all"))
        gcheck.check_rho(getattr(args, "grad_check_rho", gcheck.DEFAULT_RHO))
    refuse_fp64_teacher(getattr(args, "teacher_precision", "auto"), flag="--")
    tokcon_settings(args, flag="--")                              # the token contrast term: ranges, and not together with --grad_check_iters
    rel_on, rel_beta, _ = reliability_settings(args, flag="--")       # the reliability-weighted seg loss: ranges
    seg_soft_settings(args, flag="--")                            # the soft-label seg term: ranges, and not together with --grad_check_iters
    notes = []
    if not rel_on and rel_beta != 1.0:
        notes.append("--camweight_beta: only read with --seg_reliability true")
    if not args.find_unused:
        notes.append("--find_unused false: no effect (DDP runs without find_unused_parameters; the unused ImageNet head is frozen)")
    if args.segconf_thre != 0.25:
        notes.append("--segconf_thre: only read by cam_loss v3, which is not built")
    if getattr(args, "gt_stats", False) and not (getattr(args, "gt_dir", None) or
                                                 (args.voc12_root if args.dataset == 'VOC12' else args.coco_root)):
        raise ValueError("--gt_stats true needs the ground-truth maps of the training images: give the dataset root (--voc12_root / "
                         "--coco_root: its SegmentationClassAug / SegmentationClass/train2014) or --gt_dir")
    evaluation.check_boundary_settings(getattr(args, "boundary_ratio", 0.02), getattr(args, "boundary_d", 0))      # or a ValueError
    for n in notes:
        print("note:", n, flush=True)


BASE_KEYS = ('overall_loss', 'cls_loss', 'cls_acc', 'cls_aux_loss', 'cls_aux_acc', 'seg_loss', 'cam_loss', 'reg_loss')


def interval_keys(tokcon_on, soft_on=False):
    """the keys of the interval's running sums `acc`, of the log line and of loss_dataframe.pt: the reference's eight, `tok_loss` after
    `reg_loss` with the token contrast term on (--tokcon_weight > 0), and `soft_loss` after that with the soft-label seg term on
    (--seg_soft_weight > 0)"""
    return BASE_KEYS + (('tok_loss',) if tokcon_on else ()) + (('soft_loss',) if soft_on else ())


def interval_terms(logs, cls_acc, cls_aux_acc, tokcon_on, soft_on=False):
    """one step's contribution to `acc`, in interval_keys' order"""
    terms = [logs['overall_loss'], logs['cls_loss'], cls_acc, logs['cls_aux_loss'], cls_aux_acc, logs['seg_loss'], logs['cam_loss'], logs['reg_loss']]
    if tokcon_on:
        terms.append(logs['tok_loss'])
    if soft_on:
        terms.append(logs['soft_loss'])
    return torch.stack([t.reshape(()).double() for t in terms])


def interval_line(head, vals, tokcon_on, soft_on=False):
    """the log line's loss part from interval_keys' values"""
    line = (" overall_loss: %.4f, cls_loss: %.4f, cls_acc: %.3f,  cls_aux_loss: %.4f, cls_aux_acc: %.3f, seg_loss: %.4f, cam_loss: %.4f, "
            "reg_loss: %.4f" % tuple(vals[:8]))
    if tokcon_on:
        line += ", tok_loss: %.4f" % vals[8]
    if soft_on:
        line += ", soft_loss: %.4f" % vals[9 if tokcon_on else 8]
    return head + line + " ..."


EXTRA_KEYS_STATE = "launcher.extra_keys"      # a state file's tensor aux.<this>, written with the soft-label seg term on only


def extra_keys_word(tokcon_on, soft_on, device):
    """the set of keys beyond the reference's eight as one int64 word (bit 0: tok_loss, bit 1: soft_loss).  It travels in a state file only
    with the soft-label seg term on: the length of `launcher.acc` cannot tell `tok_loss` alone from `soft_loss` alone, the presence of this
    tensor can -- and files written with the term off keep the tensors they always had."""
    return torch.tensor([int(tokcon_on) | 2 * int(soft_on)], device=device, dtype=torch.int64)


def load_state_checked(trainer, path, tokcon_on, soft_on=False):
    """trainer.load_state(path); a refusal over the launcher's own tensors names the flag instead of a tensor or a shape.  A file written
    under the other on / off setting of the soft-label seg term has or lacks `aux.launcher.extra_keys`; one written under the other setting
    of the token contrast term differs in the length of `launcher.acc`."""
    try:
        return trainer.load_state(path)
    except ValueError as e:
        if EXTRA_KEYS_STATE in str(e):
            raise ValueError(f"{path}: written with --seg_soft_weight {'0 (the term off)' if soft_on else '> 0 (the term on)'}, this run has "
                             f"--seg_soft_weight {'> 0' if soft_on else '0'}: resume with the setting the file was written under "
                             f"(its interval sums {'lack' if soft_on else 'carry'} the key soft_loss) [{e}]") from e
        if "launcher.acc" in str(e) and "differs" in str(e):
            raise ValueError(f"{path}: written with --tokcon_weight {'0 (the term off)' if tokcon_on else '> 0 (the term on)'}, this run has "
                             f"--tokcon_weight {'> 0' if tokcon_on else '0'}: resume with the setting the file was written under "
                             f"(its interval sums carry {'eight' if tokcon_on else 'nine'} keys) [{e}]") from e
        raise


def read_interval(acc, log_iters, monitors):
    """The log interval's ONE host sync: -> (means of the running sums `acc`, {monitor name: its host values}).  monitors: [(Monitor, its
    tensors)] of the ones that are on (monitors.active).  What each packs rides along in the same transfer, in the list's order, and each
    unpacks its own slice front to back (`acc` keeps its length); then `acc` and what a monitor holds per interval are zeroed on the device,
    what is the run's stays (cosa_amd/monitors.py)."""
    packed = [[v.reshape(-1) for v in m.pack(t)] for m, t in monitors]
    parts = [acc / log_iters] + [v for p in packed for v in p]
    vals = (torch.cat(parts) if len(parts) > 1 else parts[0]).tolist()
    host, at = {}, acc.numel()
    acc.zero_()
    for (m, t), p in zip(monitors, packed):
        n = sum(v.numel() for v in p)
        host[m.name] = m.unpack(t, vals[at:at + n])
        m.zero(t)
        at += n
    return vals[:acc.numel()], host


def grad_check_record(summary, n_iter, targs):
    """one line of <output_dir>/grad_check.jsonl: the iteration, mode and rho of a check and its directions (utils.grad_check.summarize)"""
    import json
    return json.dumps(gcheck.jsonable(dict(iters=int(n_iter), mode=targs.grad_check_mode, rho=float(targs.grad_check_rho), dirs=summary)))


def append_grad_check(output_dir, summary, n_iter, targs):
    with (Path(output_dir) / "grad_check.jsonl").open("a") as f:
        f.write(grad_check_record(summary, n_iter, targs) + "\n")


SEG_REL_SETS = ("main", "aux")


def seg_rel_line(summary):
    """the evaluation's fragment of --seg_reliability (trainer.seg_reliability(): one dict per CAM set): ' seg_rel: main bg 0.612 fg 0.371,
    aux bg ... fg ...'; a group without a pixel prints '-'"""
    f = lambda v: "-" if v is None else "%.3f" % v
    return " seg_rel: " + ", ".join("%s bg %s fg %s" % (n, f(s["bg"]), f(s["fg"])) for n, s in zip(SEG_REL_SETS, summary))


def append_seg_reliability(output_dir, summary, n_iter, targs):
    """one line of <output_dir>/seg_reliability.jsonl: the iteration, the weight's settings and the mean weights since the last evaluation"""
    import json
    rec = dict(iters=int(n_iter), beta=float(targs.camweight_beta), floor=float(targs.seg_reliability_floor),
               **{n: s for n, s in zip(SEG_REL_SETS, summary)})
    with (Path(output_dir) / "seg_reliability.jsonl").open("a") as f:
        f.write(json.dumps(rec) + "\n")


def next_batch(it, new_iter, pos):
    """-> (iterator, batch): the next batch, from a new iterator (new_iter() resets `pos`) when this one is exhausted.  pos["consumed"]
    counts BATCHES drawn from the current iterator -- with --accum_steps N an optimizer step draws N -- so --resume skips the right number."""
    try:
        batch = next(it)
    except StopIteration:
        it = new_iter()
        batch = next(it)
    pos["consumed"] += 1
    return it, batch


def main(args):
    check_supported(args)
    output_dir = Path(args.output_dir) if args.output_dir else Path(args.work_dir) / args.name
    output_dir.mkdir(parents=True, exist_ok=True)
    args.output_dir = output_dir
    init_distributed_mode(args)
    device = torch.device("cuda", args.gpu)
    if args.random_seed:
        args.seed = random.randint(1, 10000)
    is_main = args.rank == 0
    log = (lambda *a, **k: print(*a, **k, flush=True)) if is_main else (lambda *a, **k: None)
    log("{}".format(args).replace(', ', ',\n'))

    targs = _trainer_args(args)
    trainer = CoSATrainer(targs, device, ddp=args.distributed, seed=args.seed)       # seeds, both networks, DDP, PolyWarmupAdamW, EMA, PAR hook
    train_loader = build_train_loader(args, device=device, num_workers=args.num_workers)
    val_loader = build_val_loader(args)
    log(f"train items: {len(train_loader.dataset)}, val items: {len(val_loader.dataset)}")
    n_parameters = sum(p.numel() for p in trainer.student.parameters() if p.requires_grad)
    log('Number of trainable params for Network: {}M'.format(n_parameters // 1000000))

    # the loader position (cosa_amd/checkpoint.py): the RNG states just before the current new_iter(), the sampler epoch it drew and the
    # number of batches taken since -- enough to make a new process draw batch k+1 exactly as this one would have
    saving = args.save_iters > 0
    pos = {"rng": None, "epoch": None, "consumed": 0}

    def new_iter(skip=0):
        if saving:
            pos["rng"] = checkpoint.pack_rng(device)
        pos["epoch"], pos["consumed"] = None, skip
        if getattr(train_loader, "sampler", None) is not None and hasattr(train_loader.sampler, "set_epoch"):
            pos["epoch"] = int(np.random.randint(args.max_iters))                    # main.py:74,111
            train_loader.sampler.set_epoch(pos["epoch"])
        return train_loader.iter_from(skip) if skip else iter(train_loader)

    tokcon_on = float(getattr(args, "tokcon_weight", 0.0) or 0.0) > 0           # (off: keys, line and `acc` as ever)
    soft_on = float(getattr(args, "seg_soft_weight", 0.0) or 0.0) > 0          # (likewise)
    keys = interval_keys(tokcon_on, soft_on)
    acc = torch.zeros(len(keys), device=device, dtype=torch.float64)           # running sums of the interval, on the device
    # ... and part of a state file: saved and restored in place, no sync (next to what the trainer keeps there: --label_stats' counters)
    trainer._add_extra_state("launcher.acc", acc)
    if soft_on:
        trainer._add_extra_state(EXTRA_KEYS_STATE, extra_keys_word(tokcon_on, soft_on, device))
    resume = args.resume
    if resume == "auto":
        resume = checkpoint.newest_state(output_dir)                                # none: a fresh start
    resumed = None
    if resume:
        resumed = load_state_checked(trainer, resume, tokcon_on, soft_on)
        checkpoint.unpack_rng(resumed["loader"]["rng"], device)                     # 1. the states the interrupted run built its iterator from
        it = new_iter(skip=int(resumed["loader"]["consumed"]))                      # 2./3. same sampler epoch, the consumed batches drawn and dropped
        assert pos["epoch"] == resumed["loader"]["epoch"], "the sampler epoch of the resumed iterator differs from the saved one"
        checkpoint.unpack_rng(resumed["rng_at_save"], device)                       # 4. the states of the save point
        log(f"Resumed from {resume}: continuing at iteration {int(resumed['n_iter']) + 1}")
    else:
        it = new_iter()
    log("Start training")
    start_time, time0, tick = time.time(), datetime.datetime.now().replace(microsecond=0), time.time()
    loss_df = {k: [] for k in keys + ('iters',)}
    best_seg = best_cam = -1
    df = None
    first_iter = 0
    if resumed is not None:
        first_iter = int(resumed["n_iter"]) + 1
        best_seg, best_cam, df = resumed["best_seg"], resumed["best_cam"], resumed["df"]
        loss_df = {k: list(resumed["loss_df"][k]) for k in loss_df}
    tstats_on = bool(getattr(args, "tensor_stats", False))                        # per-tensor diagnostics
    n_micro = int(getattr(args, "accum_steps", 1))                                # micro-batches per optimizer step
    gcheck_on, gcheck_line = check_iters(args, "grad") > 0, ""                    # the gradient check
    for n_iter in range(first_iter, args.max_iters):
        if tstats_on and (n_iter + 1) % args.log_iters == 0:
            trainer.request_tensor_stats()                                         # this step closes the interval: it samples the table
        for _micro in range(n_micro):                                             # the last call applies the mean gradient; `acc` sums over all
            it, (img_name, wimg, simg, cls_label, img_box, *gt) = next_batch(it, new_iter, pos)      # (gt: the sixth element of --gt_stats)
            cls_label = cls_label.to(device, non_blocking=True)
            logs = trainer.step(wimg, simg, cls_label, img_box, n_iter, *gt)
            with torch.no_grad():                                                 # main.py:257-268, without the per-iteration .item() syncs
                ap, ok = torch_helper.average_precision(cls_label, torch.sigmoid(logs["cls_logits"].float()))
                apa, oka = torch_helper.average_precision(cls_label, torch.sigmoid(logs["cls_aux_logits"].float()))
                acc += interval_terms(logs, (ap * ok).sum() / ok.sum().clamp_min(1), (apa * oka).sum() / oka.sum().clamp_min(1), tokcon_on, soft_on)
        if gcheck_on and (n_iter + 1) % args.grad_check_iters == 0:              # a check step: its record is read here (the check's one sync)
            gsum = trainer.pop_grad_check()
            if gsum is not None and is_main:
                append_grad_check(output_dir, gsum, n_iter + 1, targs)
                gcheck_line = gcheck.line(gsum, targs.grad_check_mode)
        if (n_iter + 1) % args.log_iters == 0:
            vals, host = read_interval(acc, args.log_iters * n_micro, monitors.active(trainer))   # the one host sync of the interval
            now = time.time()
            itertime, tick = (now - tick) / args.log_iters, now
            delta = datetime.datetime.now().replace(microsecond=0) - time0
            eta = delta * (args.max_iters - n_iter - 1) / (n_iter + 1)
            if is_main:
                for k, v in zip(keys, vals):
                    loss_df[k].append(v)
                loss_df['iters'].append(n_iter + 1)
                head = "Iter: %d; Elasped: %s; ETA: %s; Itertime: %.3f; LR: %.3e; \n" % (
                    n_iter + 1, delta, str(eta).split('.')[0], itertime, trainer.optimizer.param_groups[0]['lr'])
                line = interval_line(head, vals, tokcon_on, soft_on)
                for m in monitors.MONITORS:                                                # (a monitor that is off: the line as ever)
                    if m.name in host:
                        summary = host[m.name] if m.summary is None else m.summary(trainer, args, host[m.name])
                        if m.gate(summary):
                            line += m.line(summary, targs)
                            if m.record_extra is not None:
                                monitors.append_monitor(output_dir, m, summary, n_iter + 1, targs)
                line, gcheck_line = line + gcheck_line, ""                                 # (the last check since the previous line, if any)
                log(line)
        if (n_iter + 1) % args.eval_iters == 0:                                   # main.py:313-383
            score_kw = {"image_scores": True} if args.image_scores else {}           # (off: the calls as ever)
            if getattr(args, "boundary_scores", False):
                score_kw["boundary_scores"] = True
            rel_summary = trainer.seg_reliability()                                 # (--seg_reliability; None with the switch off: nothing printed)
            if rel_summary is not None and is_main:
                log(seg_rel_line(rel_summary))
                append_seg_reliability(output_dir, rel_summary, n_iter + 1, targs)
            res_o = evaluate(trainer.student, val_loader, args, df=df, epoch=n_iter + 1, s_or_t='s', get_camiou=True,
                             threshold_filters=args.eval_threshold_filters, **score_kw)
            if is_main:
                tab, segvd, camiou, df, aps = res_o
                log(f'ON Model Classification: cls:{aps[0]}, clsaux: {aps[1]}')
                log(tab)
            res_a = evaluate(trainer.model_AN, val_loader, args, df=df, epoch=n_iter + 1, s_or_t='t', get_camiou=True,
                             threshold_filters=args.eval_threshold_filters, **score_kw)
            if is_main:
                tab_a, segvd_a, camiou_a, df, aps_a = res_a
                log(f'AN: cls:{aps_a[0]}, clsaux: {aps_a[1]}')
                log(tab_a)
                for kind, cands, best in (("seg", [round(segvd, 2), round(segvd_a, 2)], best_seg), ("cam", [round(camiou, 2), round(camiou_a, 2)], best_cam)):
                    cmp_list = cands + [best]
                    idx = max(range(3), key=cmp_list.__getitem__)
                    if idx != 2:
                        torch_helper.save_best(output_dir, trainer.student if idx == 0 else trainer.model_AN, finish_epoch=n_iter + 1,
                                               result=max(cmp_list), args=args, s_or_t='s' if idx == 0 else 't', comment=kind)
                    if kind == "seg":
                        best_seg = max(cmp_list)
                    else:
                        best_cam = max(cmp_list)
                with (output_dir / "log_val.txt").open("a") as f:
                    f.write(f'iters:{n_iter}\n')
                    f.write(f'ON model: cls:{aps[0]}, clsaux: {aps[1]}\n{tab}\n')
                    f.write(f'AN model: cls:{aps_a[0]}, clsaux: {aps_a[1]}\n{tab_a}\n')
        if saving and (n_iter + 1) % args.save_iters == 0:                        # after this iteration's evaluation and save_best bookkeeping
            trainer.save_state(checkpoint.state_path(output_dir, n_iter + 1), n_iter=n_iter, best_seg=best_seg, best_cam=best_cam,
                               loss_df=loss_df, df=df, loader=dict(pos))
    trainer.wait_state()
    torch.cuda.synchronize()
    if is_main:
        total = str(datetime.timedelta(seconds=int(time.time() - start_time)))
        log('Training time {}'.format(total), 'Best val Seg mIoU: %.2f' % best_seg, 'Best val CAM mIoU: %.2f' % best_cam)
        torch.save(loss_df, output_dir / 'loss_dataframe.pt')                    # (a plain dict of lists: the reference wraps it in a DataFrame)
    if args.distributed:
        dist.barrier()
    if args.finalval and (output_dir / 'best_seg.pth').exists():
        args.bestseg_path = output_dir / 'best_seg.pth'
        log('Perform final validation on best model')
        finaleval(args)
    if args.distributed:
        dist.destroy_process_group()


@torch.no_grad()
def finaleval(args):
    """main.py:401-433: reload best_seg.pth (strict) into a fresh network and evaluate it on the test split with dense-CRF post-processing
    (getcrf=True: rows Seg_vd and Seg_crf; the CRF is seg_helper.DenseCRF on the device lattice kernels)."""
    output_dir = Path(args.output_dir) if args.output_dir else Path(args.work_dir) / args.name
    device = torch.device("cuda", getattr(args, "gpu", 0))
    model = build_model(_trainer_args(args))
    torch_helper.load_best(model, args.bestseg_path, strict=True)
    model = model.to(device)
    res = evaluate(model, build_test_loader(args), args, df=None, epoch='best1', isfinal=True, getcrf=True,   # main.py:414-425
                   threshold_filters=None, **({"image_scores": output_dir / "best1"} if getattr(args, "image_scores", False) else {}),
                   **({"boundary_scores": output_dir / "best1"} if getattr(args, "boundary_scores", False) else {}))
    if getattr(args, "rank", 0) == 0:
        print('Final Model Result:\n' + res[0], flush=True)
        with (output_dir / "log_val.txt").open("a") as f:
            f.write('------------' * 3 + "\nFinal Model Result:\n" + '------------' * 3 + "\n" + res[0] + "\n")
    return res


if __name__ == "__main__":
    parsed, changed = cosa_args.parse()
    print(f'runnning on {parsed.dataset}')
    print("Changed arguments:")
    print(changed)
    main(parsed)
