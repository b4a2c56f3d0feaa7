"""Write a trained model's predictions as files:

    python -m cosa_amd.predict NAME --checkpoint best_seg.pth --dataset VOC12 --voc12_root $VOC --split val|test|train|train_aug \
        --out DIR --what seg[,pseudo,pseudo_aux,pseudo_par,pseudo_aux_par,rawcam,rawcam_aux] [--crf] [--high_thre H --low_thre L] [--writers N] \
        [--scores] [--boundary [--boundary_ratio R | --boundary_d N]]

Segmentation PNGs of `val` / `test` (what the VOC evaluation server takes), pseudo-label PNGs of `train_aug` / `train` for a second-stage
network (`pseudo`: thresholds only; `pseudo_par`: refined by PAR(num_iter=10, dilations=[1,2,4,8,12,24]) at `--par_downscale` 2 or 0, the
labels CoSA itself trains on), raw CAMs as `.npy` dictionaries.  Every flag of the training launcher is accepted (cosa_amd/args.py: `--backbone`,
`--crop_size`, `--num_classes`, `--name_list_dir`, ...); the thresholds default to the run's `--high_thre` / `--low_thre`.  The
checkpoint is loaded strictly, as `finaleval` loads it.  `--split test` has no ground truth and no image-level labels: `seg` only.
Under `torchrun` the images are sharded over the ranks (`index % world == rank`), each written exactly once; rank 0 writes
`manifest.json` last.  Prints the engine's result as one JSON line.  `--scores` (splits with ground-truth maps on disk: val, train,
train_aug) also reads each image's mask, scores every exported label map against it on the device and writes `scores.jsonl` (per-image
integer counters; read it with tools/image_scores.py); the result line gains the products' mIoU and labelled share.
`--boundary` (the same splits, with or without `--scores`) counts the same maps over the pixels within d of each map's own contours --
Boundary IoU, d = `--boundary_ratio` (0.02) of the image's diagonal or a fixed `--boundary_d` -- into `boundary_scores.jsonl` (the same
format); the result line gains the products' boundary mIoU and the manifest the settings.

Any folder of pictures:

    python -m cosa_amd.predict NAME --checkpoint best_seg.pth --num_classes 21 --images DIR|LIST.txt --out DIR \
        --what seg,pseudo,rawcam,overlay [--classes predicted|none] [--cls_thre 0.5] [--cls_min 1] [--overlay_alpha 0.5]

`--images` takes a directory (its *.jpg / *.jpeg / *.png, not its sub-directories) or a text file of image paths instead of a data set:
no data root, no name list, no label file.  An item is named by its file's stem.  `--classes` says where an image's class row comes
from: `given` (the data set's `cls_labels_onehot.npy`), `none` (`seg` only, the plain argmax) or `predicted` -- the model's own
classification head: class c is present iff its `cls_final` logit of the multi-scale pass reaches log(t / (1 - t)) for `--cls_thre` t,
and the largest remaining logits are added until `--cls_min` classes are present.  Unset, it is `given` where the split has rows, `none`
for `test`, and `predicted` with `--images`.  Predicted rows go through the same kernels as given ones: every product can be made for
unlabelled images, `test` keeps the class validation of `Seg_vd`, and `classes.jsonl` lists each image's classes, logits and
probabilities.  On a labelled split `--classes predicted` may be combined with `--scores`; the result line then also compares the
predicted rows with the given ones (exact-match share, micro precision / recall / F1).  `--what overlay` writes `overlay/<name>.png`:
the `seg` map as written, in the VOC colours, blended over the image with weight `--overlay_alpha`.

The CAM pictures (they need a class row, given or predicted): `--what camheat` writes `cam/<name>_<class>.png`
for every present class -- the class's `rawcam` plane as a jet heat map over the image, in exact integers -- `camheat_aux` the same for
the auxiliary CAM into `camaux/`, and `panel` writes `merged/<name>_<class>.png`: heat map | the `seg` map's pixels of the class | the
ground truth's (on `val` / `train`, where the masks are on disk; left out elsewhere) | the image.  `<class>` is the data set's class name
with spaces as `_`, or the 1-based index where the head has another number of classes."""
import json
import os
import sys

from . import args as cosa_args
from .utils.export_io import MAX_WRITERS

PRODUCTS = ("seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux", "pseudo_par", "pseudo_aux_par", "overlay", "camheat", "camheat_aux", "panel")
CLASS_SOURCES = ("given", "predicted", "none")
SPLITS = ("val", "test", "train", "train_aug")


def get_parser():
    p = cosa_args.get_parser()
    p.prog = "python -m cosa_amd.predict"
    p.description = "Export segmentation / pseudo-label PNGs and raw CAMs of a trained CoSA model"
    p.add_argument("--checkpoint", type=str, required=True, help="best_seg.pth / best_cam.pth of a run (reference key names)")
    p.add_argument("--split", type=str, default=None, choices=SPLITS, help="the data set's split (default val); not with --images")
    p.add_argument("--images", type=str, default=None, help="a directory of *.jpg / *.jpeg / *.png, or a text file of image paths, instead of a split")
    p.add_argument("--classes", type=str, default=None, choices=CLASS_SOURCES,
                   help="the image-level class row: the data set's (given), the model's own head (predicted), or none (seg only); "
                        "default: given where the split has rows, none for test, predicted with --images")
    p.add_argument("--cls_thre", type=float, default=0.5, help="--classes predicted: a class is present from this sigmoid probability on, in (0, 1)")
    p.add_argument("--cls_min", type=int, default=1, help="--classes predicted: at least this many classes per image (0..C), the largest logits first")
    p.add_argument("--overlay_alpha", type=float, default=0.5, help="--what overlay: the weight of the class colour, in [0, 1]")
    p.add_argument("--out", type=str, required=True, help="output directory")
    p.add_argument("--what", type=str, default="seg", help="comma-separated products out of " + ", ".join(PRODUCTS))
    p.add_argument("--crf", action="store_true", help="also write seg_crf/ (dense-CRF post-processing, as finaleval scores it)")
    p.add_argument("--scores", action="store_true", help="score every exported label map against the ground-truth mask: scores.jsonl")
    p.add_argument("--boundary", action="store_true",
                   help="Boundary IoU counters of every exported label map against the ground-truth mask: boundary_scores.jsonl "
                        "(--boundary_ratio of the diagonal, or a fixed --boundary_d)")
    p.add_argument("--writers", type=int, default=4, help=f"PNG / npy writer threads (1..{MAX_WRITERS})")
    p.add_argument("--eval_group", type=int, default=4)
    p.add_argument("--trust_checkpoint", action="store_true",
                   help="allow the full unpickler for a checkpoint that torch.load(weights_only=True) refuses (runs code from the file)")
    return p


def parse(argv=None):
    """-> (args, products); every argument error is raised here (parser.error: exit status 2), before the GPU is touched"""
    parser = get_parser()
    args, _ = cosa_args.handle_defaults(parser.parse_args(argv))
    what = tuple(w.strip() for w in args.what.split(",") if w.strip())
    bad = [w for w in what if w not in PRODUCTS]
    if bad or not what or len(set(what)) != len(what):
        parser.error(f"--what: products are {', '.join(PRODUCTS)} (each once); got {args.what!r}")
    args.image_items = None
    if args.images is not None:
        if args.split is not None:
            parser.error("--images replaces the data set's split: give one of --images and --split")
        if args.scores:
            parser.error("--scores needs ground-truth maps: --images has none")
        if args.boundary:
            parser.error("--boundary needs ground-truth maps: --images has none")
        if args.classes == "given":
            parser.error("--classes given: --images has no image-level label rows (use predicted or none)")
        try:
            from .utils.export_io import list_images
            args.image_items = list_images(args.images)
        except ValueError as e:
            parser.error(f"--images: {e}")
    elif args.split is None:
        args.split = "val"
    if args.classes == "given" and args.split == "test":
        parser.error("--classes given: --split test has no image-level label rows (use predicted or none)")
    args.class_source = args.classes or ("predicted" if args.images is not None else "none" if args.split == "test" else "given")
    if not 0.0 < args.cls_thre < 1.0:
        parser.error(f"--cls_thre must lie in (0, 1) (got {args.cls_thre})")
    if not 0 <= args.cls_min <= args.num_classes - 1:
        parser.error(f"--cls_min must be in 0..{args.num_classes - 1}, the number of classes (got {args.cls_min})")
    if not 0.0 <= args.overlay_alpha <= 1.0:
        parser.error(f"--overlay_alpha must lie in [0, 1] (got {args.overlay_alpha})")
    if args.class_source == "none" and any(w not in ("seg", "overlay") for w in what):
        where = "--split test has" if args.split == "test" and args.classes is None else "--classes none leaves"
        parser.error(f"{where} no image-level labels: only `seg` (and `overlay`) can be exported (got --what {args.what}); "
                     f"--classes predicted takes them from the model's own head")
    if args.scores and args.split == "test":
        parser.error("--scores needs ground-truth maps: --split test has none")
    if args.scores and not (args.crf or any(w in ("seg",) or w.startswith("pseudo") for w in what)):
        parser.error(f"--scores needs a label-map product (seg, pseudo*, --crf), got --what {args.what}")
    if args.boundary and args.split == "test":
        parser.error("--boundary needs ground-truth maps: --split test has none")
    if args.boundary and not (args.crf or any(w in ("seg",) or w.startswith("pseudo") for w in what)):
        parser.error(f"--boundary needs a label-map product (seg, pseudo*, --crf), got --what {args.what}")
    if args.boundary:
        from .utils import evaluation
        try:
            evaluation.check_boundary_settings(args.boundary_ratio, args.boundary_d)
        except ValueError as e:
            parser.error(str(e))
    if not 1 <= args.writers <= MAX_WRITERS:
        parser.error(f"--writers must be in 1..{MAX_WRITERS} (got {args.writers})")
    if args.usepar:
        parser.error("--usepar true does not select an export product: ask for the PAR-refined labels with --what pseudo_par[,pseudo_aux_par]")
    if any(w.endswith("_par") for w in what) and args.par_downscale not in (0, 2):
        parser.error(f"--par_downscale must be 2 or 0 for --what pseudo_par / pseudo_aux_par (got {args.par_downscale})")
    if args.eval_group < 1:
        parser.error("--eval_group must be >= 1")
    if args.dataset == "COCO" and args.split in ("test", "train_aug"):
        parser.error(f"--dataset COCO has no {args.split} split")
    return args, what


def load_checkpoint(model, path, trust=False):
    """`ckpt["model"]` into the network, strictly (as finaleval: torch_helper.load_best), read with the restricted unpickler: tensors,
    plain containers and the `args` namespace the trainer stores.  Anything else in the file needs --trust_checkpoint."""
    import argparse
    import pathlib
    import pickle
    import torch
    from .utils import torch_helper
    try:
        with torch.serialization.safe_globals([argparse.Namespace, pathlib.PosixPath, pathlib.Path]):
            ckpt = torch.load(path, map_location="cpu", weights_only=True)
    except pickle.UnpicklingError as e:
        if not trust:
            raise RuntimeError(f"{path}: not loadable with weights_only=True ({str(e).splitlines()[0]}); pass --trust_checkpoint to "
                               f"unpickle it in full") from e
        return torch_helper.load_best(model, path, strict=True)
    getattr(model, "module", model).load_state_dict(ckpt["model"], strict=True)
    return ckpt


def build_dataset(args):
    from .dataloaders.train_loader import COCOSegDataset, VOC12SegDataset
    stage = "test" if args.split == "test" else "val"
    if args.dataset == "VOC12":
        return VOC12SegDataset(root_dir=args.voc12_root, name_list_dir=args.name_list_dir or './dataloaders/voc/', split=args.split, stage=stage)
    return COCOSegDataset(root_dir=args.coco_root, name_list_dir=args.name_list_dir or './dataloaders/coco/', split=args.split, stage=stage)


class _ImageFiles:
    """`--images`: items `(name, image, 0, 0)` as _ImagesOnly gives them for `test`, read from any files"""
    split = "images"

    def __init__(self, items):
        self.items = list(items)

    def __len__(self):
        return len(self.items)

    def __getitem__(self, idx):
        import numpy as np
        from PIL import Image
        from .dataloaders.train_loader import normalize_img
        name, path = self.items[idx]
        image = np.asarray(Image.open(path).convert('RGB'))
        return name, np.transpose(normalize_img(image), (2, 0, 1)), 0, 0


class _ImagesOnly:
    """the dataset without its ground-truth masks: export reads none, and `train_aug` / `train` items need not have one on disk"""

    def __init__(self, ds):
        self.ds, self.split = ds, ds.split

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, idx):
        import numpy as np
        from PIL import Image
        from .dataloaders.train_loader import normalize_img
        ds = self.ds
        name = str(ds.name_list[idx])
        image = np.asarray(Image.open(os.path.join(ds.img_dir, name + '.jpg')).convert('RGB'))
        cls_label = 0 if ds.stage == "test" else ds.label_list[name]
        return name, np.transpose(normalize_img(image), (2, 0, 1)), 0, cls_label


def main(argv=None):
    args, what = parse(argv)
    import torch
    import torch.distributed as dist
    from torch.utils.data import DataLoader
    from .evaluation_engine import export_predictions
    from .main import _trainer_args, check_supported, init_distributed_mode
    from .models import build_model
    check_supported(args)
    init_distributed_mode(args)
    device = torch.device("cuda", args.gpu)
    model = build_model(_trainer_args(args))
    ckpt = load_checkpoint(model, args.checkpoint, trust=args.trust_checkpoint)
    model = model.to(device).eval()
    if args.image_items is not None:
        dataset = _ImageFiles(args.image_items)
    else:
        dataset = build_dataset(args)             # (its items read the ground-truth mask: only --scores / --boundary / panel want it)
        wants_gt = args.scores or args.boundary or ("panel" in what and args.split in ("val", "train"))    # the panel's ground-truth column
        dataset = dataset if wants_gt else _ImagesOnly(dataset)
    loader = DataLoader(dataset=dataset, batch_size=1, shuffle=False, num_workers=args.num_workers, pin_memory=False)
    settings = {"checkpoint": os.path.abspath(args.checkpoint), "checkpoint_epoch": ckpt.get("epoch"), "s_or_t": ckpt.get("s_or_t"),
                "dataset": args.dataset, "split": args.split, "crf": bool(args.crf)}
    extra = {"scores": True} if args.scores else {}
    if args.boundary:
        extra.update({"boundary": True, "boundary_ratio": args.boundary_ratio, "boundary_d": args.boundary_d})
    if args.images is not None:
        settings.update({"split": None, "images": os.path.abspath(args.images)})
    if args.classes is not None or args.images is not None:           # unset on a split: the engine's defaults, nothing new in the manifest
        extra.update({"classes": args.class_source, "cls_thre": args.cls_thre, "cls_min": args.cls_min})
    if "overlay" in what:
        extra["overlay_alpha"] = args.overlay_alpha
    res = export_predictions(model, loader, args, args.out, what=what, getcrf=args.crf, eval_group=args.eval_group, writers=args.writers,
                             settings=settings, **extra)
    print(json.dumps(res), flush=True)
    if args.distributed:
        dist.destroy_process_group()
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
