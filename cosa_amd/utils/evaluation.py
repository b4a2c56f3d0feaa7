"""utils.evaluation -- segmentation scores from a confusion matrix (reference: utils/evaluation.py).

`scores` / `pseudo_scores` keep the reference's call surface (lists of label maps in, dict of pAcc / mAcc / miou / iou out) but count
on the GPU: the maps go through `cosa_confusion_hist` (LDS-privatised counters) into one [nc, nc] int64 matrix.  `ConfusionMeter`
is the streaming form the evaluation engine uses: device-resident accumulation over the whole validation set, one all-reduce across
ranks at the end (the reference gathers every prediction map on rank 0 through temp files, evaluation_engine.py:203-216).
"""
import json
import math
import os
import warnings

import numpy as np
import torch

from .. import _C


def _as_u8_cuda(x, device):
    if not torch.is_tensor(x):
        x = torch.from_numpy(np.ascontiguousarray(x))
    if x.dtype != torch.uint8:
        x = x.to(torch.uint8)                       # the reference stores every map as uint8 (evaluation_engine.py:198-200)
    return x.to(device, non_blocking=True).contiguous()


class ConfusionMeter:
    """hist[t, p] over all pixels with truth t < num_classes (255 = ignore).  pseudo=True applies pseudo_scores' relabelling
    (utils/evaluation.py:43-46): pixels whose PREDICTION is 255 are dropped."""

    def __init__(self, num_classes, device=None, pseudo=False):
        device = torch.device(device if device is not None else "cuda")
        if device.type != "cuda":
            raise RuntimeError("ConfusionMeter counts on the GPU (cosa_confusion_hist); no CPU path")
        self.num_classes, self.pseudo = int(num_classes), bool(pseudo)
        self.hist = torch.zeros((self.num_classes, self.num_classes), device=device, dtype=torch.int64)

    def update(self, label_true, label_pred):
        gt, pr = _as_u8_cuda(label_true, self.hist.device), _as_u8_cuda(label_pred, self.hist.device)
        if gt.numel() != pr.numel():
            raise ValueError("ConfusionMeter.update: truth and prediction differ in size")
        _C.check(_C.lib().cosa_confusion_hist(_C.ptr(gt), _C.ptr(pr), gt.numel(), self.num_classes, int(self.pseudo), _C.ptr(self.hist),
                                              _C.stream_ptr()), "cosa_confusion_hist")

    def all_reduce(self):
        """sum over ranks (replaces the temp-file gather of evaluation_engine.py:203-216)"""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.hist)
        return self

    def scores(self):
        return scores_from_hist(self.hist.cpu().numpy())


def scores_from_hist(hist):
    """utils/evaluation.py:21-35 on an accumulated confusion matrix (row = truth)."""
    hist = np.asarray(hist, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = np.diag(hist).sum() / hist.sum()
        acc_cls = np.nanmean(np.diag(hist) / hist.sum(axis=1))
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
    valid = hist.sum(axis=1) > 0
    return {"pAcc": acc, "mAcc": acc_cls, "miou": np.nanmean(iu[valid]), "iou": dict(zip(range(hist.shape[0]), iu))}


def _scores(label_trues, label_preds, num_classes, pseudo):
    meter = ConfusionMeter(num_classes, pseudo=pseudo)
    for lt, lp in zip(label_trues, label_preds):
        meter.update(lt, lp)
    return meter.scores()


def scores(label_trues, label_preds, num_classes):
    """utils/evaluation.py:17-35"""
    return _scores(label_trues, label_preds, num_classes, False)


def pseudo_scores(label_trues, label_preds, num_classes):
    """utils/evaluation.py:37-70 (the inputs are NOT modified in place, unlike the reference's `lt[lp==255] = 255`)"""
    return _scores(label_trues, label_preds, num_classes, True)


# ---------------------------------------------------------------------------------------------------------------------------------
# per-image scores: the counters of cosa_image_scores, the reference's assist_seg from them, the score files
# ---------------------------------------------------------------------------------------------------------------------------------
MAX_MAPS = _C.constant("COSA_IMAGE_SCORES_MAX_MAPS")     # maps per launch


def row_words(num_classes, n_maps):
    """words of one row: [n, n_valid, then per map and class I, P, G, A]"""
    return 2 + int(n_maps) * int(num_classes) * 4


class ImageScores:
    """Device table [capacity, words] int64 of per-image counters: row `index` = [n, n_valid, then for map m, class c: I, P, G, A]
    (cosa_image_scores; include/cosa_hip.h).  `add` launches and returns -- no host wait; `rows()` is the one device-to-host copy.
    More than eight maps go in chunks of eight, each launch re-reading the ground truth; a chunk's launch writes its own [n, n_valid]
    in front of its maps, so the table keeps one such pair per chunk and `rows()` drops all but the first."""

    _entry = "cosa_image_scores"                  # the C entry that fills a chunk's words; `<entry>_words` sizes them

    def __init__(self, num_classes, map_names, pseudo_flags, capacity, device=None):
        who = type(self).__name__
        device = torch.device(device if device is not None else "cuda")
        if device.type != "cuda":
            raise RuntimeError(f"{who} counts on the GPU ({self._entry}); no CPU path")
        self.num_classes, self.map_names = int(num_classes), [str(m) for m in map_names]
        self.pseudo_flags = [int(bool(p)) for p in pseudo_flags]
        if len(self.pseudo_flags) != len(self.map_names) or not self.map_names or len(set(self.map_names)) != len(self.map_names):
            raise ValueError(f"{who}: one pseudo flag per map, at least one map, every name once")
        self._chunks, off = [], 0                 # (first map, maps, word offset in the table's row)
        for first in range(0, len(self.map_names), MAX_MAPS):
            k = min(MAX_MAPS, len(self.map_names) - first)
            words = getattr(_C.lib(), self._entry + "_words")(self.num_classes, k)
            if not words:
                _C.check(1, self._entry + "_words")
            self._chunks.append((first, k, off))
            off += words
        self.table = torch.zeros((max(int(capacity), 1), off), device=device, dtype=torch.int64)

    def _launch(self, gt, ptrs, first, k, row, stream):
        """one chunk of maps of one image into the words at `row`"""
        return _C.lib().cosa_image_scores(_C.ptr(gt), ptrs, _C.int_array(self.pseudo_flags[first:first + k]), k, gt.numel(), self.num_classes,
                                          row, stream)

    def add(self, index, gt, preds):
        """score the uint8 device maps `preds` (one per map name) of one image against its uint8 ground truth into row `index`"""
        who = type(self).__name__
        index = int(index)
        if len(preds) != len(self.map_names):
            raise ValueError(f"{who}.add: {len(self.map_names)} maps expected, got {len(preds)}")
        if index < 0:
            raise IndexError(index)
        if index >= self.table.shape[0]:             # a loader that did not tell its length: grow on the device, no host wait
            grown = torch.zeros((max(2 * self.table.shape[0], index + 1), self.table.shape[1]), device=self.table.device, dtype=torch.int64)
            grown[:self.table.shape[0]] = self.table
            self.table = grown
        _C.require_cuda(gt, *preds)
        n = gt.numel()
        maps = []
        for p in preds:
            if p.dtype != torch.uint8 or gt.dtype != torch.uint8 or p.numel() != n:
                raise ValueError(f"{who}.add: uint8 maps of the ground truth's size")
            maps.append(p.contiguous())
        gt = gt.contiguous()
        st = _C.stream_ptr()
        for first, k, off in self._chunks:
            ptrs = (_C.c_void_p * k)(*[m.data_ptr() for m in maps[first:first + k]])
            row = _C.c_void_p(self.table.data_ptr() + 8 * (index * self.table.shape[1] + off))
            _C.check(self._launch(gt, ptrs, first, k, row, st), self._entry)

    def rows(self, count=None):
        """-> numpy [count or capacity, 2 + maps * num_classes * 4] int64: the single device-to-host copy"""
        t = self.table.cpu().numpy()
        if count is not None:
            t = t[:count]
        parts = [t[:, :2]]
        for _, k, off in self._chunks:
            parts.append(t[:, off + 2:off + 2 + k * self.num_classes * 4])
        return np.ascontiguousarray(np.concatenate(parts, axis=1))


MAX_BOUNDARY_D = 64                               # cosa_boundary_scores' envelope: 2 % of a 3200-pixel diagonal


def boundary_width(h, w, ratio=0.02, d=None):
    """the band's width in pixels for an h x w image: a fixed `d`, or `ratio` of the diagonal (Boundary IoU: 0.02), at least 1"""
    if d:
        return int(d)
    return max(1, int(round(ratio * math.sqrt(h * h + w * w))))


def check_boundary_settings(ratio, d):
    """-> (ratio, fixed d or None) or a ValueError: a ratio in (0, 1), a fixed d in 1..64 (0 / None: use the ratio)"""
    ratio, d = float(ratio), int(d or 0)
    if not 0.0 < ratio < 1.0:
        raise ValueError(f"boundary scores: the ratio must be in (0, 1) (got {ratio})")
    if not 0 <= d <= MAX_BOUNDARY_D:
        raise ValueError(f"boundary scores: a fixed d must be in 0..{MAX_BOUNDARY_D}, 0 for the ratio (got {d})")
    return ratio, (d or None)


class BoundaryScores(ImageScores):
    """ImageScores' table over BAND pixels (cosa_boundary_scores): row `index` = [n, n_valid, then for map m, class
    c: I, P, G, A] counted over the pixels within `d` of each map's own contours; Boundary IoU of a class is I / (P + G - I), the dataset
    figure `dataset_scores` of the rows.  `add` takes 2-D maps, forms d = boundary_width(H, W, ratio, d) on the host from the shape alone
    and launches; `widths` keeps each row's d for the files.  `pseudo_flags` are recorded for the files only."""
    _entry = "cosa_boundary_scores"

    def __init__(self, num_classes, map_names, pseudo_flags, capacity, device=None, ratio=0.02, d=None):
        self.ratio, self.d = check_boundary_settings(ratio, d)
        self.widths = {}                          # row index -> the d its maps were scored with
        super().__init__(num_classes, map_names, pseudo_flags, capacity, device)

    def _launch(self, gt, ptrs, first, k, row, stream):
        return _C.lib().cosa_boundary_scores(_C.ptr(gt), ptrs, k, self._shape[0], self._shape[1], self._width, self.num_classes, row, stream)

    def add(self, index, gt, preds):
        if gt.dim() != 2 or any(p.dim() != 2 or p.shape != gt.shape for p in preds):
            raise ValueError("BoundaryScores.add: 2-D uint8 maps [H, W] of one size")
        self._shape = (int(gt.shape[0]), int(gt.shape[1]))
        width = boundary_width(*self._shape, ratio=self.ratio, d=self.d)
        self._width = min(width, max(self._shape))                       # no pixel is interior from max(H, W) on: the same row
        if self._width > MAX_BOUNDARY_D:
            raise ValueError(f"BoundaryScores.add: d = {width} for a {self._shape[0]} x {self._shape[1]} image is beyond the kernel's {MAX_BOUNDARY_D}")
        super().add(index, gt, preds)
        self.widths[int(index)] = width

    def settings(self):
        """the `boundary` entry of a score file's settings line"""
        return {"ratio": self.ratio, "d": self.d}


def split_row(row, num_classes):
    """one row -> (n, n_valid, counts [maps, num_classes, 4] in the order I, P, G, A)"""
    row = np.asarray(row, dtype=np.int64)
    return int(row[0]), int(row[1]), row[2:].reshape(-1, int(num_classes), 4)


def assist_from_counts(I, A, G_all, n, cls_label):
    """The reference's assist_seg (evaluation_engine.py:311-329) from integer counts: per class id c (1-based: entry c - 1 of cls_label is
    set) I = #{seg == c and gt == c}, A = #{seg == c}, G_all = #{gt == c}, all over the n pixels of the image; arrays indexed by class
    id.  -> {c: (iou, gt_ratio), 'miou', 'wmiou'} in the reference's arithmetic: sums of bool tensors are integers and their quotient is a
    float32 division of the two integers cast to float32 (0 / 0 is NaN and stays one in `miou`), the union is A + G_all - I, the means are
    numpy's over Python floats."""
    ious = {}
    for c, j in enumerate(np.asarray(cls_label).reshape(-1)):
        if j > 0:
            k = c + 1
            with np.errstate(divide="ignore", invalid="ignore"):
                iou = np.float32(int(I[k])) / np.float32(int(A[k]) + int(G_all[k]) - int(I[k]))
                ratio = np.float32(int(G_all[k])) / np.float32(int(n))
            ious[k] = (float(iou), float(ratio))
    with np.errstate(divide="ignore", invalid="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # an image without a present class: the mean of nothing, NaN as the reference
        mean_iou = np.mean([ious[i][0] for i in ious])
        wmean = np.sum([ious[i][0] * ious[i][1] for i in ious]) / np.sum([ious[i][1] for i in ious])
    ious['miou'] = mean_iou
    ious['wmiou'] = wmean
    return ious


def assist_from_row(row, num_classes, map_index, cls_label):
    """assist_from_counts of one map of a row.  G_all is the map's own G: the ground-truth area over the pixels the map labels with a
    class -- for a map that labels every pixel (seg_vd, seg_crf, cam, ...: all but the pseudo maps) that is #{gt == c} of the whole image,
    the reference's gt_area."""
    n, _, cnt = split_row(row, num_classes)
    c = cnt[map_index]
    return assist_from_counts(c[:, 0], c[:, 3], c[:, 2], n, cls_label)


def dataset_scores(rows, num_classes):
    """rows [images, words] -> per map {"iou": [num_classes], "miou"} from the summed I, P, G: scores_from_hist's formula and `valid` rule on
    the matrix's diagonal, column sums and row sums."""
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, np.shape(rows)[-1])
    cnt = rows[:, 2:].sum(axis=0).reshape(-1, int(num_classes), 4).astype(np.float64)
    out = []
    for c in cnt:
        I, P, G = c[:, 0], c[:, 1], c[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            iu = I / (G + P - I)
        valid = G > 0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            out.append({"iou": iu, "miou": np.nanmean(iu[valid]) if valid.any() else float("nan"),
                        "labelled": float(P.sum() / rows[:, 1].sum()) if rows[:, 1].sum() else float("nan")})
    return out


def nan_to_none(x):
    x = float(x)
    return None if x != x else x                 # NaN is written as null


def score_record(name, h, w, present, row, d=None):
    """one image of a score file (host data only): `present` = the class ids of cls_label (1-based), `row` its counters; `d`: the band's
    width where the row is a boundary row (BoundaryScores), else the record has no such key"""
    rec = {"name": str(name), "h": int(h), "w": int(w), "present": [int(c) for c in present], "row": np.asarray(row, dtype=np.int64)}
    if d is not None:
        rec["d"] = int(d)
    return rec


def merge_records(shards):
    """shards: per rank the list of (dataset position, record).  -> records in dataset order; a name met twice keeps its first row"""
    seen, out = set(), []
    for _, rec in sorted((pr for shard in shards for pr in shard), key=lambda pr: pr[0]):
        if rec["name"] not in seen:
            seen.add(rec["name"])
            out.append(rec)
    return out


def write_score_file(path, settings, records):
    """settings line, then one line per image: name, h, w, n, n_valid, present, and per map the non-zero classes with their integer
    I, P, G, A and assist_seg's miou / wmiou"""
    nc, maps = int(settings["num_classes"]), list(settings["maps"])
    lines = [json.dumps(dict(settings, image_scores=1), sort_keys=True)]
    for rec in records:
        n, n_valid, cnt = split_row(rec["row"], nc)
        cls_label = np.zeros(max(nc - 1, 0), np.int64)
        cls_label[[c - 1 for c in rec["present"]]] = 1
        per_map = {}
        for m, name in enumerate(maps):
            a = assist_from_counts(cnt[m][:, 0], cnt[m][:, 3], cnt[m][:, 2], n, cls_label)
            per_map[name] = {"classes": {str(c): [int(v) for v in cnt[m][c]] for c in range(nc) if cnt[m][c].any()},
                             "miou": nan_to_none(a["miou"]), "wmiou": nan_to_none(a["wmiou"])}
        lines.append(json.dumps(dict({"name": rec["name"], "h": rec["h"], "w": rec["w"], "n": n, "n_valid": n_valid, "present": rec["present"],
                                      "maps": per_map}, **({"d": rec["d"]} if "d" in rec else {}))))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def read_score_file(path):
    """-> (settings, records) with every record's `row` rebuilt"""
    with open(path) as f:
        lines = [json.loads(ln) for ln in f if ln.strip()]
    settings = lines[0]
    nc, maps = int(settings["num_classes"]), list(settings["maps"])
    records = []
    for d in lines[1:]:
        row = np.zeros(row_words(nc, len(maps)), np.int64)
        row[0], row[1] = d["n"], d["n_valid"]
        cnt = row[2:].reshape(len(maps), nc, 4)
        for m, name in enumerate(maps):
            for c, v in d["maps"][name]["classes"].items():
                cnt[m, int(c)] = v
        records.append(score_record(d["name"], d["h"], d["w"], d["present"], row, d.get("d")))
    return settings, records


def gather_records(local):
    """`local`: this rank's [(dataset position, record)].  -> on rank 0 the merged records in dataset order, elsewhere None"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        shards = [None] * dist.get_world_size()
        dist.all_gather_object(shards, local)
        return merge_records(shards) if dist.get_rank() == 0 else None
    return merge_records([local])


def local_score_records(meta, rows, rank, world, widths=None):
    """This rank's [(dataset position, score_record)] from host data alone.  `meta`: per scored image, in the order it was scored,
    (name, class row, h, w); `rows`: its counters.  A loader that deals the items round-robin (DistributedSampler(shuffle=False),
    export_shard) hands rank r the dataset positions r, r + world, ...: the k-th item of this rank is r + k world.  `present` is the class
    row's non-zero entries as 1-based class ids; `widths` (row index -> d) is given for boundary rows and only then the records carry `d`."""
    return [(rank + k * world, score_record(name, h, w, (torch.nonzero(torch.as_tensor(cl).reshape(-1)).reshape(-1) + 1).tolist(), rows[k],
                                            None if widths is None else widths[k])) for k, (name, cl, h, w) in enumerate(meta)]


class ScoreLog:
    """One per-image score table -- ImageScores, or BoundaryScores where `boundary` = (ratio, fixed d) is given -- with the host facts of
    its rows (name, class row, size), from the first image to the score file.  `add` launches and returns; `write` is the table's one
    device-to-host copy, the gather over the ranks and rank 0's file."""

    def __init__(self, num_classes, map_names, pseudo_flags, loader, shards, device, boundary=None):
        try:                                          # a guess, the table grows: this rank's share of the loader's items (shards = 1
            capacity = len(loader) // max(int(shards), 1) + 1      # where the loader is the rank's own share already)
        except TypeError:
            capacity = 64
        kind, kw = (ImageScores, {}) if boundary is None else (BoundaryScores, {"ratio": boundary[0], "d": boundary[1]})
        self.table, self.meta = kind(num_classes, map_names, pseudo_flags, capacity, device, **kw), []

    def add(self, name, class_row, H, W, gt, maps):
        """the uint8 device maps of one image (H W elements each) against its ground truth, no host wait; `class_row`: a HOST tensor"""
        self.table.add(len(self.meta), gt.reshape(H, W), [m.reshape(H, W) for m in maps])
        self.meta.append((name, class_row, int(H), int(W)))

    def write(self, path, settings, rank=0, world=1):
        """-> on rank 0 the records of every rank in dataset order, written to `path` under `settings` plus what the table knows (maps,
        pseudo, num_classes, world_size, and boundary for a band table); elsewhere None"""
        widths = getattr(self.table, "widths", None)                    # a band table's d per row
        records = gather_records(local_score_records(self.meta, self.table.rows(len(self.meta)), rank, world, widths))
        if rank == 0:
            settings = dict(settings, maps=self.table.map_names, pseudo=self.table.pseudo_flags, num_classes=self.table.num_classes,
                            world_size=world, **({} if widths is None else {"boundary": self.table.settings()}))
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            write_score_file(path, settings, records)
        return records
