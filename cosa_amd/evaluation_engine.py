"""evaluation_engine -- the validation pass of the reference (evaluation_engine.py:11-297), device-resident.

Same call surface and return values as the reference's `evaluate`.  What changes is where the work happens:

* per image: five scales x two flips through the network (`seg_helper.multi_scale_camsegv3`), then ONE kernel turns the (S,S) CAMs and
  logits into the three uint8 label maps at the ground truth's resolution (`seg_helper.eval_label_maps` = F.interpolate x3 +
  cam_to_label x2 + seg_validation + argmax x2 of the reference) -- nothing of size [1,C,H,W] is materialised;
* the maps never leave the GPU: four confusion matrices are accumulated on the device (`evaluation.ConfusionMeter`) and summed over
  ranks with one all-reduce, instead of storing every map in host lists and shipping them to rank 0 through temp files (:203-216);
* per-image average precision is computed on the device and accumulated without a host sync.

`threshold_filters` (evaluation_engine.py:43-50,132-152,252-262): for every threshold t the pseudo-label maps cam2mask(valid CAM,
high = 1 - t, low = t) of the main and the auxiliary CAMs at the ground truth's resolution, scored with `pseudo_scores` (pixels labelled
255 are dropped) into rows `cam_<t>` / `camaux_<t>` of the table.

`getcrf` (evaluation_engine.py:204-211,247-250; `finaleval` passes it): per image the validated logits at the ground truth's resolution ->
softmax -> one mean-field step of the dense CRF (`seg_helper.crf_inference_infv2`: two permutohedral-lattice filters on the device) ->
argmax, scored as the row `Seg_crf`.  Parity of that row with pydensecrf is unpinned (see seg_helper.DenseCRF).

`evaluate` writes no image files (`save_result`, `save_rawcam` raise NotImplementedError) -- only, with `image_scores=...`, the per-image score
files of DESIGN.md section 22 (off by default: nothing changes); `export_predictions` below does: the same forward, one packed record per
image at the image's own size, one asynchronous copy to pinned memory, a pool of writer threads (command line:
`python -m cosa_amd.predict`).  The two share `_eval_pass` (model state and the captured pass), `_seg_crf_map` and `evaluation.ScoreLog`
(a score table from the first image to its file); the export's host logic is `check_export_request` (every refusal before the device is
touched) and `_RecordPlan` (every byte offset of an image's record, computed once).
"""
import contextlib
import functools
import math
import os
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist
import torch.nn.functional as F

from .utils import evaluation, export_io, seg_helper, torch_helper
from .utils.export_io import export_shard                         # noqa: F401  (the sharding rule, part of this module's surface)

EVAL_SCALES = [1.0, 0.5, 1.5, 0.75, 1.25]          # evaluation_engine.py:84


class _GraphedCamSeg:
    """multi_scale_camsegv3 at a fixed input shape (evaluation resizes every image to crop_size x crop_size, batch 1) as one hipGraph:
    ten encoder passes at batch 1 are ~1000 small launches, i.e. launch-bound when issued one by one.  Two eager calls first (library
    kernel selection), then capture; any other input shape falls back to eager."""

    def __init__(self, model, scales, enabled=True):
        self.model, self.scales, self.enabled = model, scales, enabled
        self.calls, self.graph, self.static_in, self.outs = 0, None, None, None

    def __call__(self, inputs):
        eager = lambda x: seg_helper.multi_scale_camsegv3(self.model, x, self.scales, getcls=True, _per_image_cls=True)
        if not self.enabled or (self.static_in is not None and inputs.shape != self.static_in.shape):
            return eager(inputs)
        if self.graph is None:
            self.calls += 1
            if self.calls <= 2:
                return eager(inputs)
            self.static_in = inputs.clone()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self.outs = eager(self.static_in)
            self.graph = g
        self.static_in.copy_(inputs)
        self.graph.replay()
        return self.outs


@contextlib.contextmanager
def _eval_pass(model, use_graph):
    """The state both passes below run in: eval mode, no grad, and the heads and the decoder batch-invariant (the narrow heads on their own
    kernel), so that grouped items reproduce the one-at-a-time bits.  Yields the multi-scale pass; flags and mode come back on every path."""
    was_training = model.training
    net = model.module if hasattr(model, "module") else model
    heads_before = getattr(net, "batch_invariant_heads", None)
    model.eval()
    if heads_before is not None:
        net.batch_invariant_heads = True
        net.decoder.batch_invariant = True
    try:
        with torch.no_grad():
            yield _GraphedCamSeg(model, EVAL_SCALES, enabled=use_graph and getattr(model, "can_forward_multi", None) is not None)
    finally:
        if heads_before is not None:
            net.batch_invariant_heads = heads_before
            net.decoder.batch_invariant = heads_before
        if was_training:
            model.train()


def _seg_crf_map(seg_logits, cls_row, img_org, size):
    """The Seg_crf label map of one image (evaluation_engine.py:204-211): softmax of the validated logits [1,C+1,S,S] at the ground truth's
    size, the de-normalised uint8 image, one mean-field step, argmax -> uint8 [1,H,W].  `img_org` is de-normalised IN PLACE: whatever reads
    the normalised image comes before this."""
    rs = F.interpolate(seg_logits, size=size, mode='bilinear', align_corners=False)
    vd = seg_helper.seg_validation(rs, cls_row).softmax(dim=1)[0]
    ori = torch_helper.denormalize_img_(img_org)[0].permute(1, 2, 0)
    q = seg_helper.crf_inference_infv2(ori, vd.contiguous())
    return q.argmax(dim=0, keepdim=True).to(torch.uint8)


def _write_iou_dic(path, records, num_classes, map_index):
    """the reference's iou_dic.pth (evaluation_engine.py:160-168,282-283) of one map of the score records; means as Python floats"""
    iou_dic = {}
    for rec in records:
        cl = [1 if c + 1 in rec["present"] else 0 for c in range(num_classes - 1)]
        a = evaluation.assist_from_row(rec["row"], num_classes, map_index, cl)
        iou_dic[rec["name"]] = {k: (float(v) if k in ("miou", "wmiou") else v) for k, v in a.items()}
    torch.save(iou_dic, path)


def evaluate(model, data_loader, args, df=None, save_result=False, save_rawcam=False, epoch=None, threshold_filters=None, getcrf=False,
             s_or_t='t', get_camiou=False, isfinal=False, class_list=None, use_graph=True, eval_group=4, image_scores=None,
             boundary_scores=None):
    """`image_scores`: None (default) adds nothing.  A directory, or True for args.output_dir/<epoch, five digits>/, scores every label map
    this call produces against the ground truth per image on the device (evaluation.ImageScores: one launch per image, one copy at the
    end) and has rank 0 write image_scores_<s_or_t>.jsonl and iou_dic_<s_or_t>.pth there.
    `boundary_scores`: None or False (default) adds nothing.  A directory or True, as above: the same maps, counted over the pixels within
    d of each map's own contours (evaluation.BoundaryScores: Boundary IoU; d from args.boundary_ratio, default 0.02 of the image's diagonal,
    or a fixed args.boundary_d > 0), into boundary_scores_<s_or_t>.jsonl.  Independent of `image_scores`."""
    if save_result or save_rawcam:
        raise NotImplementedError("evaluate: save_result / save_rawcam (image dumps) are not part of the device path of evaluate(); "
                                  "files are written by evaluation_engine.export_predictions / python -m cosa_amd.predict")
    threshold_filters = list(threshold_filters) if threshold_filters else []
    assert s_or_t in ['s', 't']
    distributed = dist.is_available() and dist.is_initialized()
    rank = dist.get_rank() if distributed else 0
    device = next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("evaluate runs on the GPU (HIP kernels); no CPU path")
    nc = args.num_classes
    meters = {k: evaluation.ConfusionMeter(nc, device) for k in ("cam", "cam_aux", "seg_ps", "seg_vd")}
    if getcrf:
        meters["seg_crf"] = evaluation.ConfusionMeter(nc, device)
    for thre in threshold_filters:                    # pseudo_scores' relabelling: a prediction of 255 drops the pixel (utils/evaluation.py:43-46)
        meters[f"cam_{thre}"] = evaluation.ConfusionMeter(nc, device, pseudo=True)
        meters[f"camaux_{thre}"] = evaluation.ConfusionMeter(nc, device, pseudo=True)
    world = dist.get_world_size() if distributed else 1
    logs = {}                                         # per-image counters of the same maps, in the meters' order (off: nothing is built)
    for kind, where, band in (("image", image_scores, None),
                              ("boundary", boundary_scores, (getattr(args, "boundary_ratio", 0.02), getattr(args, "boundary_d", 0)))):
        if where is not None and where is not False:  # the loader is this rank's share already
            logs[kind] = (where, evaluation.ScoreLog(nc, list(meters), [m.pseudo for m in meters.values()], data_loader, 1, device, band))
    ap_sum = torch.zeros(2, device=device, dtype=torch.float64)          # sums of per-batch mean AP (cls, cls_aux) ...
    ap_cnt = 0                                                           # ... over the batches (AverageMeter semantics, :86-92)
    # Every image is resized to crop_size x crop_size before the network (:82), so `eval_group` loader items share one multi-scale pass
    # (GEMMs with several times the rows instead of ten batch-1 encoder passes per image: 137 -> 242 img/s at 4); label maps, histograms
    # and AP stay per image.  Every kernel on the CAM / seg path (patch projection, encoder, convs, narrow heads, CAM tail) gives a token
    # the same bits whatever else is in the batch, so the score table and the AP are those of the one-image-at-a-time loop exactly
    # (tested).  eval_group=1 is the reference's loop literally.
    def flush(group):
        if not group:
            return
        nonlocal ap_cnt
        inputs = torch.cat([g[0] for g in group], dim=0)
        cams, cams_aux, seg_ps, cls_final, cls_aux = camseg(inputs)
        for i, (_, labels, cls_label, img_org, meta) in enumerate(group):
            # classification AP of this item (:86-92; cls_* are sums over scales and flips, compared with every label row)
            for j, logit in enumerate((cls_final[i:i + 1], cls_aux[i:i + 1])):
                ap, valid = torch_helper.average_precision(cls_label, torch.sigmoid(logit.float()).expand_as(cls_label))
                ap_sum[j] += (ap * valid).sum() / valid.sum().clamp_min(1)
            ap_cnt += 1
            size = labels.shape[1:]
            cam_label, pred_ps, pred_vd = seg_helper.eval_label_maps(cams[i:i + 1], seg_ps[i:i + 1], cls_label, size, args.bkg_thre)
            cam_aux_label, _, _ = seg_helper.eval_label_maps(cams_aux[i:i + 1], None, cls_label, size, args.bkg_thre)
            gt = labels.to(torch.uint8)
            maps = {"cam": cam_label, "cam_aux": cam_aux_label, "seg_ps": pred_ps, "seg_vd": pred_vd}
            if getcrf:
                maps["seg_crf"] = _seg_crf_map(seg_ps[i:i + 1], cls_label, img_org, size)
            if threshold_filters:
                # evaluation_engine.py:132-152: the CAMs resized to the ground truth's size, validated, then cam2mask with the box
                # [0, -1, 0, -1] (Python slice semantics: the last row and column stay `ignore`, as in the reference) and no refine model
                shape_only = torch.zeros(1, device=device).expand(1, 3, *size)
                for thre in threshold_filters:
                    for key, c in ((f"cam_{thre}", cams), (f"camaux_{thre}", cams_aux)):
                        rc = F.interpolate(c[i:i + 1], size=size, mode='bilinear', align_corners=False)
                        m = seg_helper.cam2mask(images=shape_only, img_boxes=[[0, -1, 0, -1]], cams=seg_helper.cam_validation(rc, cls_label),
                                                cls_labels=cls_label, threshold_high=1 - thre, threshold_low=thre)
                        maps[key] = m.to(torch.uint8)
            for key, meter in meters.items():         # every map of this image exists: into its confusion matrix ...
                meter.update(gt, maps[key])
            for _, log in logs.values():              # ... and into the per-image tables: one launch (per eight maps), no host wait
                log.add(*meta, size[0], size[1], gt, [maps[k] for k in meters])

    with _eval_pass(model, use_graph) as camseg:
        group = []
        for data in data_loader:
            name, img_org, labels, cls_label = data
            names = [name] if isinstance(name, str) else list(name)
            cls_host = cls_label                          # the loader's tensor: the score file's `present` is read from it after the loop
            labels = labels.to(device, non_blocking=True)
            cls_label = cls_label.to(device, non_blocking=True).float()
            img_org = img_org.to(device, non_blocking=True)
            inputs = F.interpolate(img_org, size=[args.crop_size, args.crop_size], mode='bilinear', align_corners=False)
            if inputs.shape[0] != 1:                      # a loader with its own batching: one pass per item, as before
                flush(group)
                group = []
                for i in range(inputs.shape[0]):
                    flush([(inputs[i:i + 1], labels[i:i + 1], cls_label[i:i + 1], img_org[i:i + 1], (str(names[i]), cls_host[i]))])
                continue
            group.append((inputs, labels, cls_label, img_org if getcrf else None, (str(names[0]), cls_host[0])))
            if len(group) >= max(1, int(eval_group)):
                flush(group)
                group = []
        flush(group)
    for m in meters.values():
        m.all_reduce()
    for kind, (where, log) in logs.items():           # every rank gathers, rank 0 writes (DESIGN.md sections 22 and 26)
        out_dir = Path(args.output_dir) / str(epoch).zfill(5) if where is True else Path(where)
        records = log.write(out_dir / f"{kind}_scores_{s_or_t}.jsonl",
                            {"epoch": epoch, "s_or_t": s_or_t, "checkpoint": getattr(args, "checkpoint", None)}, rank, world)
        if rank == 0 and kind == "image":
            _write_iou_dic(out_dir / f"iou_dic_{s_or_t}.pth", records, nc, list(meters).index("seg_vd"))
    if rank != 0:
        return (None,) * (5 if get_camiou else 4)

    cam_score, cam_aux_score, seg_vd_score = meters["cam"].scores(), meters["cam_aux"].scores(), meters["seg_vd"].scores()
    metrics, names = [cam_score, cam_aux_score, seg_vd_score], ["CAM", "aux_CAM", "Seg_vd"]
    if isfinal:
        metrics, names = [seg_vd_score], ["Seg_vd"]
    if getcrf:                                           # evaluation_engine.py:247-250
        metrics, names = metrics + [meters["seg_crf"].scores()], names + ["Seg_crf"]
    if threshold_filters:                                # evaluation_engine.py:252-262: inserted after the first three rows
        tk = [f"cam_{t}" for t in threshold_filters] + [f"camaux_{t}" for t in threshold_filters]
        metrics = metrics[:3] + [meters[k].scores() for k in tk] + metrics[3:]
        names = names[:3] + tk + names[3:]
    cls_aps = [float(v) / max(ap_cnt, 1) for v in ap_sum.tolist()]
    if class_list is None:
        class_list = [str(i) for i in range(nc)]
    tab_results, _, mioulist = torch_helper.format_tabs(scores=metrics, name_list=names, cat_list=class_list)
    if not df:
        df = {'Iterations': [], 'mIoU': [], 'Metrics': [], 'ST': []}
    df['Iterations'].extend([epoch] * len(names))
    df['mIoU'].extend(mioulist)
    df['Metrics'].extend(names)
    df['ST'].extend([s_or_t] * len(names))
    # evaluation_engine.py:287-290 of the reference: the "seg" score handed back is the LAST row of the table (second to last with the CRF row).
    # With `threshold_filters` that row is a pseudo-label sweep row (camaux_<t>), not Seg_vd -- the reference's behaviour, kept so that
    # best-checkpoint selection in main.py follows the reference run for run (README: "--eval_threshold_filters").
    seg_vd_miou, cam_miou = (mioulist[-1] if not getcrf else mioulist[-2]), mioulist[0]
    if get_camiou:
        return tab_results, seg_vd_miou, cam_miou, df, cls_aps
    return tab_results, seg_vd_miou, df, cls_aps


# ---------------------------------------------------------------------------------------------------------------------------------
# export: segmentation / pseudo-label PNGs and raw-CAM dictionaries
# ---------------------------------------------------------------------------------------------------------------------------------
EXPORT_PRODUCTS = tuple(seg_helper.EXPORT_BITS)                   # seg, pseudo, pseudo_aux, rawcam, rawcam_aux, pseudo_par, pseudo_aux_par
CAM_PRODUCTS = tuple(p for p in EXPORT_PRODUCTS if p != "seg")    # these need the image-level label row
PICTURE_PRODUCTS = ("camheat", "camheat_aux", "panel")             # one RGB picture per present class, behind the record's slots (section 27)
SCORED_PRODUCTS = ("seg", "pseudo", "pseudo_aux", "pseudo_par", "pseudo_aux_par", "seg_crf")      # the uint8 label maps: scores=True


class _ExportSlot:
    """one record in flight: the device record `cosa_export_maps` / `cosa_export_refine` write, its pinned host copy, the event that says the copy is done
    and the writer job that still reads the host copy"""

    def __init__(self, device):
        self.device = device
        self.dev = self.host = None
        self.event = torch.cuda.Event()
        self.job = None

    def reserve(self, nbytes):
        if self.job is not None:                   # the host copy is still being encoded: the only place the loop waits for a writer
            job, self.job = self.job, None
            job.result()
        if self.dev is None or self.dev.numel() < nbytes:
            size = max(int(nbytes), 1 << 20)
            self.dev = torch.empty(size, device=self.device, dtype=torch.uint8)
            self.host = torch.empty(size, dtype=torch.uint8).pin_memory()


_EXPORT_SLOTS = {}                                  # str(device) -> [slots], grow-only: a second call reuses the records


def _export_slots(device, n):
    slots = _EXPORT_SLOTS.setdefault(str(device), [])
    while len(slots) < n:
        slots.append(_ExportSlot(device))
    return slots[:n]


def _sharded(data_loader, rank, world):
    """every item exactly once over the ranks: index % world == rank (export_shard), not DistributedSampler(drop_last=True)"""
    if world == 1:
        return data_loader
    ds = getattr(data_loader, "dataset", None)
    if ds is not None and isinstance(data_loader, torch.utils.data.DataLoader):
        return torch.utils.data.DataLoader(dataset=ds, batch_size=1, shuffle=False, sampler=export_shard(len(ds), rank, world),
                                           num_workers=data_loader.num_workers, pin_memory=False, drop_last=False)
    items = list(data_loader)
    return [items[i] for i in export_shard(len(items), rank, world)]


_BITS = seg_helper.EXPORT_BITS
_MAPS_OF_CAM = _BITS["pseudo"] | _BITS["rawcam"]                  # cosa_export_maps reads the main CAMs for these ...
_MAPS_OF_CAM_AUX = _BITS["pseudo_aux"] | _BITS["rawcam_aux"]      # ... and the auxiliary ones for these
_HEAT_SOURCE = {"camheat": "rawcam", "camheat_aux": "rawcam_aux"}  # the slot whose planes a heat picture shows


def check_export_request(what, classes, cls_thre, cls_min, overlay_alpha, scores, boundary, getcrf, writers, args):
    """Everything export_predictions refuses before it touches the device (host logic only), and the request read once: -> a namespace of
    `what`, `products` (what + seg_crf), `mask` (the record's COSA_EXPORT_* slots), `par_mask`, `par_downscale`, `overlay`, `pictures`,
    `predicted`, `writers` and `scored` (the label-map products that scores=True / boundary=True count)."""
    what = tuple(what)
    for extra in ("overlay",) + PICTURE_PRODUCTS:
        if what.count(extra) > 1:
            raise ValueError(f"export_predictions: `{extra}` named twice in {list(what)}")
    overlay = "overlay" in what
    pictures = tuple(p for p in PICTURE_PRODUCTS if p in what)
    slot_names = tuple(w for w in what if w != "overlay" and w not in PICTURE_PRODUCTS)
    mask = seg_helper.export_what_mask(slot_names) if slot_names or not what else 0
    for p in pictures:                              # a picture shows the numbers of its slots: computed even where no .npy / .png is asked for
        mask |= _BITS["rawcam"] | _BITS["seg"] if p == "panel" else _BITS[_HEAT_SOURCE[p]]
    if overlay:                                     # the overlay shows the seg map: its slot is computed even where no seg file is asked for
        mask |= _BITS["seg"]
        seg_helper.overlay_alpha256(overlay_alpha)  # [0, 1], or a ValueError before anything runs
    if classes not in (None, "given", "predicted", "none"):
        raise ValueError(f"export_predictions: classes must be None, 'given', 'predicted' or 'none' (got {classes!r})")
    if classes == "none" and (mask & ~_BITS["seg"]):
        raise ValueError(f"export_predictions: classes='none' leaves only 'seg' (and its overlay) to export (asked for {list(what)})")
    if classes == "predicted":
        seg_helper.cls_threshold_logit(cls_thre)    # (0, 1), or a ValueError before anything runs
        if not 0 <= int(cls_min) <= args.num_classes - 1:
            raise ValueError(f"export_predictions: cls_min must be in 0..{args.num_classes - 1} (got {cls_min})")
    writers = export_io.check_writers(writers)
    if getattr(args, "usepar", False):
        raise NotImplementedError("export_predictions: `usepar` does not select an export product; the PAR-refined labels are the products "
                                  "pseudo_par / pseudo_aux_par (--what pseudo_par)")
    par_mask = mask & seg_helper.EXPORT_PAR_MASK
    par_downscale = int(getattr(args, "par_downscale", 2) or 0)
    if par_mask and par_downscale not in (0, 2):
        raise ValueError(f"export_predictions: pseudo_par / pseudo_aux_par are built for par_downscale 2 and 0 (got {par_downscale})")
    products = what + (("seg_crf",) if getcrf else ())
    scored = [p for p in products if p in SCORED_PRODUCTS]
    for flag, on in (("scores", scores), ("boundary", boundary)):
        if on and not scored:
            raise ValueError(f"export_predictions: {flag}=True needs a label-map product (one of {list(SCORED_PRODUCTS)}), got {list(products)}")
    return SimpleNamespace(what=what, products=products, mask=mask, par_mask=par_mask, par_downscale=par_downscale, overlay=overlay,
                           pictures=pictures, predicted=classes == "predicted", writers=writers, scored=scored)


class _RecordPlan:
    """Where everything of ONE image lies in its packed record, computed once: `offsets` (slot -> byte offset) are cosa_export_record_layout's
    and behind them, each on the next 16-byte boundary, seg_crf | overlay | camheat | camheat_aux | panel (one picture per present class: none
    without one); `copy_bytes` go to the host; `heat_at`: where each heat plane is rendered -- its own slot, or for a panel without camheat
    files a scratch plane behind the copied bytes; `reserve_bytes`: what the record must hold.  `view` is the only reader of the offsets."""

    def __init__(self, C, H, W, k_live, item_mask, getcrf=False, overlay=False, pictures=(), panel_cols=3):
        self.mask, self.k_live = item_mask, k_live
        self.offsets, end = seg_helper.export_record_layout(C, H, W, k_live, item_mask)
        self.shapes = {p: (k_live,) if p.endswith("_idx") else (k_live, H, W) if p.startswith("rawcam") else (H, W) for p in self.offsets}
        extra = [("seg_crf", (H, W))] * bool(getcrf) + [("overlay", (H, W, 3))] * bool(overlay)      # bytes, like every slot but rawcam*
        if k_live:
            extra += [(p, (k_live, H, W, 3)) for p in _HEAT_SOURCE if p in pictures]
            extra += [("panel", (k_live, H, panel_cols * W, 3))] * ("panel" in pictures)
        for p, shape in extra:
            self.offsets[p], self.shapes[p], end = end, shape, end + ((math.prod(shape) + 15) & ~15)
        self.copy_bytes = end
        self.heat_at = {p: self.offsets[p] for p in _HEAT_SOURCE if p in self.offsets}
        if "panel" in self.offsets:
            self.heat_at.setdefault("camheat", end)
        self.heat_bytes = 3 * k_live * H * W
        self.reserve_bytes = max([end] + [o + self.heat_bytes for o in self.heat_at.values()])

    def view(self, record, slot):
        """the slot inside `record` (the device record or the host copy's numpy array: uint8, flat): label maps uint8 [H,W], rawcam* float32
        [k_live,H,W], rawcam*_idx int32 [k_live], overlay uint8 [H,W,3], the pictures uint8 [k_live,H,cols W,3]"""
        o, shape = self.offsets[slot], self.shapes[slot]
        if not slot.startswith("rawcam"):
            return record[o:o + math.prod(shape)].reshape(shape)
        lib = torch if torch.is_tensor(record) else np       # rawcam*, rawcam*_idx: 4-byte words
        return record[o:o + 4 * math.prod(shape)].view(lib.int32 if slot.endswith("_idx") else lib.float32).reshape(shape)


class _PredictedRows:
    """classes="predicted" (DESIGN.md section 23): one group's [rows | logits | k_live | nonfinite] in 4-byte words, on the device and
    pinned; per group one `seg_helper.predict_classes` launch, one small copy and the one host wait of the predicted path."""

    def __init__(self, gmax, C, device, cls_thre, cls_min):
        self.C, self.cls_thre, self.cls_min, self.wait_seconds = C, cls_thre, cls_min, 0.0
        self.dev = torch.empty(gmax * (2 * C + 2), device=device, dtype=torch.float32)
        self.host = torch.empty(gmax * (2 * C + 2), dtype=torch.float32).pin_memory()
        self.event = torch.cuda.Event()

    def __call__(self, cls_final, G):
        """-> (rows on the device [G,C], host rows, k_live, nonfinite, logits)"""
        C = self.C
        if cls_final.shape != (G, C):
            raise RuntimeError(f"export_predictions: the pass returned logits {tuple(cls_final.shape)} for {G} images of {C} classes")
        rows, logits = self.dev[:G * C].view(G, C), self.dev[G * C:2 * G * C].view(G, C)
        ints = self.dev[2 * G * C:2 * G * C + 2 * G].view(torch.int32)
        logits.copy_(cls_final)
        seg_helper.predict_classes(logits, self.cls_thre, self.cls_min, out=(rows, ints[:G], ints[G:]))
        n = G * (2 * C + 2)
        self.host[:n].copy_(self.dev[:n], non_blocking=True)
        self.event.record()
        t = time.perf_counter()
        self.event.synchronize()                    # the only host wait of the predicted path: once per group
        self.wait_seconds += time.perf_counter() - t
        h = self.host[:n].numpy().copy()
        hi = h[2 * G * C:].view(np.int32)
        return rows, h[:G * C].reshape(G, C), hi[:G], hi[G:], h[G * C:2 * G * C].reshape(G, C)


def _fill_record(plan, record, cam, cam_aux, seg_logits, cls_row, img_org, gt, req, thresholds, overlay_alpha):
    """Every slot of one image's `record` on the device, nothing waited for.  cam / cam_aux [C,S,S] and seg_logits [1,C+1,S,S] are the pass's,
    `img_org` [1,3,H,W] the normalised image, `gt` the ground truth of its size or None (the panel's third column), `thresholds` export_maps'.
    The order matters: the overlay and the pictures read the slots just written and the image, which the CRF lines then rescale in place."""
    H, W = img_org.shape[-2:]
    maps_mask = plan.mask & seg_helper.EXPORT_MAPS_MASK
    if maps_mask:
        seg_helper.export_maps(cam if maps_mask & _MAPS_OF_CAM else None, cam_aux if maps_mask & _MAPS_OF_CAM_AUX else None, seg_logits[0],
                               cls_row, (H, W), maps_mask, out=record, k_live=plan.k_live, **thresholds)
    if plan.mask & seg_helper.EXPORT_PAR_MASK:      # the PAR slots lie behind the others: the same record, the same one copy
        seg_helper.export_refine(torch_helper.denormalize_img(img_org), cam if plan.mask & _BITS["pseudo_par"] else None,
                                 cam_aux if plan.mask & _BITS["pseudo_aux_par"] else None, cls_row, plan.mask, downscale=req.par_downscale,
                                 out=record, k_live=plan.k_live, **thresholds)
    if req.overlay:
        seg_helper.export_overlay(img_org, plan.view(record, "seg"), overlay_alpha, out=plan.view(record, "overlay"))
    heat = {p: seg_helper.export_camheat(plan.view(record, _HEAT_SOURCE[p]), img_org, out=record[o:o + plan.heat_bytes]) for p, o in plan.heat_at.items()}
    if "panel" in plan.offsets:
        seg_helper.export_panel(heat["camheat"], plan.view(record, "seg"), plan.view(record, "rawcam_idx"), img_org, gt=gt,
                                out=plan.view(record, "panel"))
    if "seg_crf" in plan.offsets:
        plan.view(record, "seg_crf").copy_(_seg_crf_map(seg_logits, cls_row, img_org, (H, W))[0])


def _host_products(plan, slot, products, picture_names):
    """In a writer thread: wait for the record's copy (the loop itself never does), then the products asked for as views of the host copy,
    in the shapes PredictionWriter.submit takes"""
    slot.event.synchronize()
    rec = slot.host.numpy()
    out = {}
    for p in (p for p in products if p in plan.offsets):      # not there: no label row (seg only), or no present class to picture
        if p in PICTURE_PRODUCTS:                    # one picture per present class, named by the class
            out[p] = (plan.view(rec, p), [picture_names[c] for c in plan.view(rec, _HEAT_SOURCE.get(p, "rawcam") + "_idx")])
        elif p in _HEAT_SOURCE.values():
            out[p] = (plan.view(rec, p), plan.view(rec, p + "_idx"))
        else:
            out[p] = plan.view(rec, p)
    return out


def export_predictions(model, data_loader, args, out_dir, what=("seg",), getcrf=False, high_thre=None, low_thre=None, eval_group=4,
                       use_graph=True, writers=4, settings=None, scores=False, classes=None, cls_thre=0.5, cls_min=1, overlay_alpha=0.5,
                       boundary=False, boundary_ratio=0.02, boundary_d=None):
    """Write the predictions of `model` over `data_loader` (items `(name, image [1,3,H,W], labels, cls_label [1,C])` as the evaluation
    loaders give them; an item without a label row -- `cls_label` None or not 2-D, the `test` stage -- can only give `seg`) into
    `out_dir` (layout: utils/export_io.py).  The forward is evaluate()'s: resize to crop_size, the captured multi-scale pass, groups of
    `eval_group` items, batch-invariant heads -- what is written is what evaluate() scores.  `what`: out of EXPORT_PRODUCTS;
    `getcrf` adds `seg_crf` (the lines of evaluate()'s Seg_crf row).  Thresholds default to args.high_thre / args.low_thre.
    `pseudo_par` / `pseudo_aux_par` are the labels CoSA trains on: cam2mask with PAR(num_iter=10, dilations=[1,2,4,8,12,24]) at
    `args.par_downscale` (2 or 0) on the image's own size (seg_helper.export_refine), into the same record as the other products.
    `scores=True` (items must carry their ground-truth map as third element): every uint8 product of an image -- seg, pseudo*, pseudo*_par,
    seg_crf -- is scored against it straight from the device record (evaluation.ImageScores; pseudo* maps with pseudo=1), rank 0 writes
    `scores.jsonl` and the result gains "scores": {product: {"miou", "labelled"}}; off: nothing changes.
    `boundary=True` (independent of `scores`, the same demands on the items): the same maps counted over the pixels within d of each map's
    own contours (evaluation.BoundaryScores; `boundary_ratio` of the image's diagonal or a fixed `boundary_d`), rank 0 writes
    `boundary_scores.jsonl`, the result gains "boundary": {product: {"miou"}} and the manifest the settings.
    `classes`: where an image's class row comes from.  None (default): what the items carry -- their row, or none
    (`seg` only).  "given": the same, but an item without a row is an error.  "none": no row even where the items carry one.  "predicted":
    the model's own head -- per group one `seg_helper.predict_classes` launch on the pass's `cls_final` logits (`cls_thre`, `cls_min`) and
    one small copy that the loop waits for (k_live sizes the records); every product is then made as with a given row, rank 0 writes
    `classes.jsonl`, and where the items carry rows too the result gains "classes": predicted against given, from integer counts.
    `what` may also name `overlay`: the written `seg` map over the image (`overlay_alpha`), RGB bytes behind the record's other slots.
    `camheat` / `camheat_aux` / `panel` (they need a class row): per present class the `rawcam` / `rawcam_aux` plane
    as a heat map over the image, and the panel heat map | seg == class | ground truth == class | image (the ground-truth column where
    the item carries a map of the image's size).  Their slots (`rawcam`, `rawcam_aux`; `seg` and `rawcam` for the panel) are computed even
    where no file of them is asked for; the pictures lie behind the overlay's bytes and ride in the same copy.
    Returns {"images", "seconds", "img_per_s", "bytes_written"} of this process."""
    req = check_export_request(what, classes, cls_thre, cls_min, overlay_alpha, scores, boundary, getcrf, writers, args)
    thresholds = {"high_thre": float(args.high_thre if high_thre is None else high_thre),
                  "low_thre": float(args.low_thre if low_thre is None else low_thre), "ignore_index": int(getattr(args, "ignore_index", 255))}
    distributed = dist.is_available() and dist.is_initialized()
    rank, world = (dist.get_rank(), dist.get_world_size()) if distributed else (0, 1)
    device = next(model.parameters()).device
    if device.type != "cuda":
        raise RuntimeError("export_predictions runs on the GPU (HIP kernels); no CPU path")
    nc, C = args.num_classes, args.num_classes - 1
    settings = settings or {}
    writer = export_io.PredictionWriter(out_dir, req.products, req.writers)
    slots = _export_slots(device, req.writers + 1)
    logs = {}                                       # scores / boundary -> the table of the label-map products (off: nothing is built)
    for flag, on, band in (("scores", scores, None), ("boundary", boundary, (boundary_ratio, boundary_d))):
        if on:
            logs[flag] = evaluation.ScoreLog(nc, req.scored, [p.startswith("pseudo") for p in req.scored], data_loader, world, device, band)
    class_names = export_io.class_names(settings.get("dataset", getattr(args, "dataset", None)), C)
    predict_rows = _PredictedRows(max(1, int(eval_group)), C, device, cls_thre, cls_min) if req.predicted else None
    class_records, count = [], 0                    # classes="predicted": (dataset position, record) per image

    def flush(group):
        nonlocal count
        if not group:
            return
        cams, cams_aux, seg_ps, cls_final, _ = camseg(torch.cat([g[1] for g in group], dim=0))
        if req.predicted:
            rows_dev, rows_h, k_h, nf_h, logits_h = predict_rows(cls_final, len(group))
        for i, (name, _, cls_dev, k_live, img_org, gt, cls_host) in enumerate(group):
            H, W = int(img_org.shape[-2]), int(img_org.shape[-1])
            if req.predicted:
                cls_dev, k_live = rows_dev[i:i + 1], int(k_h[i])
                rec = export_io.class_record(name, logits_h[i], rows_h[i], k_live, nf_h[i])
                rec["given"] = None if cls_host is None else (cls_host.reshape(-1) != 0).numpy()
                class_records.append((rank + count * world, rec))
                if cls_host is None:                # the score files' `present`: the given row where there is one
                    cls_host = torch.from_numpy(rows_h[i])
            if gt is not None and gt.numel() != H * W:
                gt = None
            item_mask = req.mask if cls_dev is not None else _BITS["seg"]
            plan = _RecordPlan(C, H, W, k_live, item_mask, getcrf, req.overlay, req.pictures, 4 if gt is not None else 3)
            slot = slots[count % len(slots)]
            slot.reserve(plan.reserve_bytes)
            _fill_record(plan, slot.dev, cams[i], cams_aux[i], seg_ps[i:i + 1], cls_dev, img_org, gt, req, thresholds, overlay_alpha)
            for flag, log in logs.items():          # scored where they lie, before the copy: one launch each, no host wait
                if item_mask != req.mask or gt is None:
                    raise ValueError(f"export_predictions: {flag}=True needs the label row and a ground-truth map of the image's size ({name!r})")
                log.add(name, cls_host, H, W, gt, [plan.view(slot.dev, p) for p in req.scored])
            slot.host[:plan.copy_bytes].copy_(slot.dev[:plan.copy_bytes], non_blocking=True)      # the one device-to-host copy of the image
            slot.event.record()
            slot.job = writer.submit(name, H, W, functools.partial(_host_products, plan, slot, req.products, class_names))
            count += 1

    t0 = time.perf_counter()
    try:
        with _eval_pass(model, use_graph) as camseg:
            group = []
            for data in _sharded(data_loader, rank, world):
                names, img_org, labels, cls_label = data
                names = [names] if isinstance(names, str) else list(names)
                has_cls = torch.is_tensor(cls_label) and cls_label.dim() == 2
                if not has_cls and ((req.mask & ~_BITS["seg"]) or classes == "given") and not req.predicted:
                    raise ValueError(f"export_predictions: item {names[0]!r} has no image-level label row; only 'seg' can be exported "
                                     f"for it (asked for {list(req.what)})")
                use_cls = has_cls and classes in (None, "given")                # predicted rows come per group, in flush
                k_lives = (cls_label != 0).sum(dim=1).tolist() if use_cls else [0] * len(names)      # the loader's host tensor: no device wait
                cls_dev = cls_label.to(device, non_blocking=True).float() if use_cls else None
                img_org = img_org.to(device, non_blocking=True)
                inputs = F.interpolate(img_org, size=[args.crop_size, args.crop_size], mode='bilinear', align_corners=False)
                gts = labels.to(device, non_blocking=True).to(torch.uint8) if (logs or "panel" in req.pictures) and torch.is_tensor(labels) else None
                for i in range(inputs.shape[0]):
                    group.append((str(names[i]), inputs[i:i + 1], cls_dev[i:i + 1] if use_cls else None, int(k_lives[i]),
                                  img_org[i:i + 1], gts[i] if gts is not None and gts.dim() == 3 else None, cls_label[i] if has_cls else None))
                    if len(group) >= max(1, int(eval_group)):
                        flush(group)
                        group = []
            flush(group)
        writer.drain()
    finally:
        for s in slots:
            s.job = None
        if writer.futures:                          # an error on the way: let the threads finish before it propagates
            try:
                writer.drain()
            except BaseException:                   # noqa: B902  (the first error is the one being raised)
                pass
        writer.pool.shutdown(wait=True)
    seconds = time.perf_counter() - t0
    images = writer.images
    if distributed:
        gathered = [None] * world
        dist.all_gather_object(gathered, images)
        images = sorted(x for part in gathered for x in part)
        dist.barrier()                              # every rank's files are on disk
    summaries = {}                                  # scores / boundary -> {product: dataset figures} on rank 0
    for flag, log in logs.items():
        records = log.write(os.path.join(out_dir, "scores.jsonl" if flag == "scores" else "boundary_scores.jsonl"),
                            {"epoch": None, "s_or_t": settings.get("s_or_t"), "checkpoint": settings.get("checkpoint")}, rank, world)
        if rank == 0:
            ds = evaluation.dataset_scores(np.stack([r["row"] for r in records]), nc) if records else []
            summaries[flag] = {p: {k: evaluation.nan_to_none(d[k]) for k in (("miou", "labelled") if flag == "scores" else ("miou",))}
                               for p, d in zip(req.scored, ds)}
    class_summary = None
    if req.predicted:                               # gathered as the score records are: dataset order, rank 0 writes
        records = evaluation.gather_records(class_records)
        if rank == 0:
            os.makedirs(out_dir, exist_ok=True)
            export_io.write_classes_file(os.path.join(out_dir, "classes.jsonl"), records, class_names)
            if records and all(r["given"] is not None for r in records):
                class_summary = export_io.classification_figures([r["row"] for r in records], [r["given"] for r in records])
    if rank == 0:
        info = {"split": getattr(data_loader.dataset, "split", None) if hasattr(data_loader, "dataset") else None,
                "products": list(req.products), "high_thre": thresholds["high_thre"], "low_thre": thresholds["low_thre"],
                "ignore_index": thresholds["ignore_index"], "crop_size": args.crop_size, "scales": EVAL_SCALES,
                "backbone": getattr(args, "backbone", None), "num_classes": nc, "world_size": world}
        if req.par_mask:
            info["par"] = {"num_iter": seg_helper.PAR_NUM_ITER, "dilations": list(seg_helper.PAR_DILATIONS), "downscale": req.par_downscale}
        if classes is not None:                     # (unset: the manifest keeps today's keys)
            info["classes"] = classes
        if req.predicted:
            info.update({"cls_thre": float(cls_thre), "cls_min": int(cls_min)})
            if class_summary is not None:
                info["classes_vs_given"] = class_summary
        if req.overlay:
            info["overlay_alpha"] = float(overlay_alpha)
        if "boundary" in logs:
            info["boundary"] = logs["boundary"].table.settings()
        if req.pictures:
            info["camheat"] = {"ramp": "jet-int", "panel_colour": list(seg_helper.PANEL_COLOUR)}
        info.update(settings)
        export_io.write_manifest_file(out_dir, info, images)
    res = {"images": len(writer.images), "seconds": seconds, "img_per_s": len(writer.images) / seconds if seconds > 0 else 0.0,
           "bytes_written": writer.bytes_written}
    for flag in logs:
        res[flag] = summaries.get(flag)             # None on the other ranks
    if req.predicted:
        res["class_wait_seconds"] = predict_rows.wait_seconds
        if class_summary is not None:
            res["classes"] = class_summary
    return res
