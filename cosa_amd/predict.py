"""Write a trained model's predictions as files:

    python -m cosa_amd.predict NAME --checkpoint best_seg.pth --dataset VOC12 --voc12_root $VOC --split val|test|train|train_aug \
        --out DIR --what seg[,pseudo,pseudo_aux,pseudo_par,pseudo_aux_par,rawcam,rawcam_aux] [--crf] [--high_thre H --low_thre L] [--writers N] \
        [--scores]

Segmentation PNGs of `val` / `test` (what the VOC evaluation server takes), pseudo-label PNGs of `train_aug` / `train` for a second-stage
network (`pseudo`: thresholds only; `pseudo_par`: refined by PAR(num_iter=10, dilations=[1,2,4,8,12,24]) at `--par_downscale` 2 or 0, the
labels CoSA itself trains on), raw CAMs as `.npy` dictionaries.  Every flag of the training launcher is accepted (cosa_amd/args.py: `--backbone`,
`--crop_size`, `--num_classes`, `--name_list_dir`, ...); the thresholds default to the run's `--high_thre` / `--low_thre`.  The
checkpoint is loaded strictly, as `finaleval` loads it.  `--split test` has no ground truth and no image-level labels: `seg` only.
Under `torchrun` the images are sharded over the ranks (`index % world == rank`), each written exactly once; rank 0 writes
`manifest.json` last.  Prints the engine's result as one JSON line.  `--scores` (splits with ground-truth maps on disk: val, train,
train_aug) also reads each image's mask, scores every exported label map against it on the device and writes `scores.jsonl` (per-image
integer counters; read it with tools/image_scores.py); the result line gains the products' mIoU and labelled share."""
import json
import os
import sys

from . import args as cosa_args
from .utils.export_io import MAX_WRITERS

PRODUCTS = ("seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux", "pseudo_par", "pseudo_aux_par")
SPLITS = ("val", "test", "train", "train_aug")


def get_parser():
    p = cosa_args.get_parser()
    p.prog = "python -m cosa_amd.predict"
    p.description = "Export segmentation / pseudo-label PNGs and raw CAMs of a trained CoSA model"
    p.add_argument("--checkpoint", type=str, required=True, help="best_seg.pth / best_cam.pth of a run (reference key names)")
    p.add_argument("--split", type=str, default="val", choices=SPLITS)
    p.add_argument("--out", type=str, required=True, help="output directory")
    p.add_argument("--what", type=str, default="seg", help="comma-separated products out of " + ", ".join(PRODUCTS))
    p.add_argument("--crf", action="store_true", help="also write seg_crf/ (dense-CRF post-processing, as finaleval scores it)")
    p.add_argument("--scores", action="store_true", help="score every exported label map against the ground-truth mask: scores.jsonl")
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
    if args.split == "test" and any(w != "seg" for w in what):
        parser.error(f"--split test has no image-level labels: only `seg` can be exported (got --what {args.what})")
    if args.scores and args.split == "test":
        parser.error("--scores needs ground-truth maps: --split test has none")
    if args.scores and not (args.crf or any(w in ("seg",) or w.startswith("pseudo") for w in what)):
        parser.error(f"--scores needs a label-map product (seg, pseudo*, --crf), got --what {args.what}")
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
    dataset = build_dataset(args)                 # (its items read the ground-truth mask: only --scores wants it)
    loader = DataLoader(dataset=dataset if args.scores else _ImagesOnly(dataset), batch_size=1, shuffle=False, num_workers=args.num_workers, pin_memory=False)
    settings = {"checkpoint": os.path.abspath(args.checkpoint), "checkpoint_epoch": ckpt.get("epoch"), "s_or_t": ckpt.get("s_or_t"),
                "dataset": args.dataset, "split": args.split, "crf": bool(args.crf)}
    res = export_predictions(model, loader, args, args.out, what=what, getcrf=args.crf, eval_group=args.eval_group, writers=args.writers,
                             settings=settings, **({"scores": True} if args.scores else {}))
    print(json.dumps(res), flush=True)
    if args.distributed:
        dist.destroy_process_group()
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
