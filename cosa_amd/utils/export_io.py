"""utils.export_io -- the host half of prediction export: file formats, the writer pool, the sharding rule.

Pure numpy / PIL: nothing here touches the GPU.  `evaluation_engine.export_predictions` hands finished host records to a
`PredictionWriter`; its threads encode and write

    <out_dir>/seg|seg_crf|pseudo|pseudo_aux|pseudo_par|pseudo_aux_par/<name>.png
                                                            palette PNGs (mode P) with the PASCAL VOC colour map
    <out_dir>/overlay/<name>.png                            RGB PNGs: the written `seg` map painted over the image (cosa_export_overlay)
    <out_dir>/cam|camaux/<name>_<class>.png                 RGB PNGs, one per present class: the main / auxiliary CAM plane as a heat map over
                                                            the image (products camheat / camheat_aux; cosa_export_camheat)
    <out_dir>/merged/<name>_<class>.png                     RGB PNGs, one per present class: heat map | seg == class | ground truth == class
                                                            (where the item has one) | image (product panel; cosa_export_panel)
    <out_dir>/camraw|camraw_aux/<name>.npy                  a pickled dict {0-based class index: float32 [H,W]} (np.load(...,
                                                            allow_pickle=True).item()), as the reference's save_cam_npv2 writes it;
                                                            an image without any present class gets no file
    <out_dir>/classes.jsonl                                 with classes="predicted": one line per image, the class row the model's own
                                                            head gave it and the logits behind it (write_classes_file)
    <out_dir>/manifest.json                                 settings + (name, H, W) per image, written LAST: a directory that has a
                                                            manifest is complete
"""
import json
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image

MAX_WRITERS = 8                      # a GPU job has 16 CPUs: loader workers and the main thread need the rest
PNG_PRODUCTS = ("seg", "seg_crf", "pseudo", "pseudo_aux", "pseudo_par", "pseudo_aux_par")
RGB_PRODUCTS = ("overlay",)
NPY_DIRS = {"rawcam": "camraw", "rawcam_aux": "camraw_aux"}
CLASS_RGB_DIRS = {"camheat": "cam", "camheat_aux": "camaux", "panel": "merged"}      # one RGB PNG per present class; the reference's directory names
IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png")
VOC_CLASSES = ("aeroplane", "bicycle", "bird", "boat", "bottle", "bus", "car", "cat", "chair", "cow", "diningtable", "dog", "horse", "motorbike",
               "person", "pottedplant", "sheep", "sofa", "train", "tvmonitor")
COCO_CLASSES = ("person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light", "fire hydrant", "stop sign",
                "parking meter", "bench", "bird", "cat", "dog", "horse", "sheep", "cow", "elephant", "bear", "zebra", "giraffe", "backpack",
                "umbrella", "handbag", "tie", "suitcase", "frisbee", "skis", "snowboard", "sports ball", "kite", "baseball bat", "baseball glove",
                "skateboard", "surfboard", "tennis racket", "bottle", "wine glass", "cup", "fork", "knife", "spoon", "bowl", "banana", "apple",
                "sandwich", "orange", "broccoli", "carrot", "hot dog", "pizza", "donut", "cake", "chair", "couch", "potted plant", "bed",
                "dining table", "toilet", "tv", "laptop", "mouse", "remote", "keyboard", "cell phone", "microwave", "oven", "toaster", "sink",
                "refrigerator", "book", "clock", "vase", "scissors", "teddy bear", "hair drier", "toothbrush")


def class_names(dataset, C):
    """the names of classes 1..C: the data set's own list when it has exactly C entries, else the 1-based indices as strings"""
    names = {"VOC12": VOC_CLASSES, "COCO": COCO_CLASSES}.get(dataset, ())
    return list(names) if len(names) == int(C) else [str(c + 1) for c in range(int(C))]


def class_file_name(name, class_name):
    """<name>_<class>: the file stem of a per-class picture; the class name with every space replaced by `_`"""
    return f"{name}_{str(class_name).replace(' ', '_')}"


def list_images(source):
    """`--images`: a directory (its *.jpg / *.jpeg / *.png files, any letter case, not its sub-directories) or a text file with one image
    path per line (relative paths from the file's own directory).  -> [(name, path)] sorted by file name, name = the stem.  An empty
    source and two items with one stem are ValueErrors."""
    source = str(source)
    if os.path.isdir(source):
        paths = [os.path.join(source, f) for f in sorted(os.listdir(source))
                 if f.lower().endswith(IMAGE_SUFFIXES) and os.path.isfile(os.path.join(source, f))]
    elif os.path.isfile(source):
        with open(source) as f:
            lines = [ln.strip() for ln in f]
        paths = [ln if os.path.isabs(ln) else os.path.join(os.path.dirname(os.path.abspath(source)), ln) for ln in lines if ln]
    else:
        raise ValueError(f"{source}: neither a directory nor a text file")
    items = [(os.path.splitext(os.path.basename(p))[0], p) for p in paths]
    if not items:
        raise ValueError(f"{source}: no images (*.jpg, *.jpeg, *.png)")
    seen = {}
    for name, p in items:
        if name in seen:
            raise ValueError(f"{source}: two images are named {name!r} ({seen[name]}, {p}): their files would overwrite each other")
        seen[name] = p
    return items


def voc_colormap(n=256):
    """The PASCAL VOC colour map by its bit-interleaving rule: the bits of the index, three at a time from the lowest, go to the top
    bits of R, G and B downwards.  Index 0 is black, 1 (128,0,0), ..., 255 (`ignore`) the usual off-white (224,224,192)."""
    cmap = np.zeros((n, 3), np.uint8)
    for i in range(n):
        c = i
        for j in range(8):
            for ch in range(3):
                cmap[i, ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
    return cmap


_PALETTE = voc_colormap().reshape(-1).tolist()


def export_shard(n, rank, world):
    """the indices of `range(n)` that rank `rank` of `world` writes: index % world == rank.  Every index belongs to exactly one rank
    (no padding, nothing dropped -- unlike DistributedSampler)."""
    if not (world >= 1 and 0 <= rank < world and n >= 0):
        raise ValueError(f"export_shard: bad arguments n={n} rank={rank} world={world}")
    return list(range(rank, n, world))


def check_writers(writers):
    writers = int(writers)
    if not 1 <= writers <= MAX_WRITERS:
        raise ValueError(f"writers must be in 1..{MAX_WRITERS} (got {writers})")
    return writers


def write_png(path, label_map):
    a = np.ascontiguousarray(label_map)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise ValueError(f"write_png: uint8 [H,W] expected, got {a.dtype} {a.shape}")
    im = Image.fromarray(a)                       # mode L ...
    im.putpalette(_PALETTE)                       # ... becomes P: the bytes are the class indices
    im.save(path, format="PNG")
    return os.path.getsize(path)


def write_png_rgb(path, rgb):
    a = np.ascontiguousarray(rgb)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"write_png_rgb: uint8 [H,W,3] expected, got {a.dtype} {a.shape}")
    Image.fromarray(a, mode="RGB").save(path, format="PNG")
    return os.path.getsize(path)


def class_record(name, logits, row, k_live, nonfinite):
    """one image of classes.jsonl (host data only): float32 logits [C], its {0, 1} row, and the kernel's two counts"""
    return {"name": str(name), "logits": np.asarray(logits, dtype=np.float32).copy(), "row": np.asarray(row).astype(bool).copy(),
            "k_live": int(k_live), "nonfinite": int(nonfinite)}


def write_classes_file(path, records, names):
    """one line per image: name, classes (1-based, as scores.jsonl's `present`), class_names, logits (every float32 by its repr: the
    shortest decimal that reads back as the same float32; NaN / Infinity as Python's json writes them), prob (the float64 sigmoid),
    k_live, nonfinite"""
    lines = []
    for rec in records:
        x = rec["logits"]
        with np.errstate(over="ignore"):
            prob = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
        idx = np.nonzero(rec["row"])[0]
        head = json.dumps({"name": rec["name"], "classes": [int(c) + 1 for c in idx], "class_names": [names[c] for c in idx]})
        logits = "[" + ", ".join(_float_repr(np.float32(v)) for v in x) + "]"
        tail = json.dumps({"prob": [float(v) for v in prob], "k_live": rec["k_live"], "nonfinite": rec["nonfinite"]})
        lines.append(head[:-1] + ', "logits": ' + logits + ", " + tail[1:])
    with open(path, "w") as f:
        f.write("".join(ln + "\n" for ln in lines))


def _float_repr(v):
    if v != v:
        return "NaN"
    if np.isinf(v):
        return "Infinity" if v > 0 else "-Infinity"
    return repr(float(str(v)))                    # str(np.float32) is the float32's shortest repr; through float() it becomes a JSON number


def classification_figures(predicted, given):
    """predicted / given: {0, 1} rows [N, C].  -> integer counts and, from them, the exact-match share and micro precision / recall / F1
    (None where a denominator is zero)"""
    p, g = np.asarray(predicted).astype(bool).reshape(len(predicted), -1), np.asarray(given).astype(bool).reshape(len(given), -1)
    if p.shape != g.shape:
        raise ValueError(f"classification_figures: {p.shape} against {g.shape}")
    tp, fp, fn = int((p & g).sum()), int((p & ~g).sum()), int((~p & g).sum())
    exact, n = int((p == g).all(axis=1).sum()), int(p.shape[0])
    div = lambda a, b: a / b if b else None
    return {"images": n, "exact": exact, "tp": tp, "fp": fp, "fn": fn, "exact_match": div(exact, n), "precision": div(tp, tp + fp),
            "recall": div(tp, tp + fn), "f1": div(2 * tp, 2 * tp + fp + fn)}


def write_cam_npy(path, planes, class_idx):
    """planes float32 [K,H,W], class_idx int [K] -> {class index: [H,W]}; K == 0 writes nothing (returns 0)"""
    if len(class_idx) == 0:
        return 0
    d = {int(c): np.array(planes[k], dtype=np.float32, copy=True) for k, c in enumerate(class_idx)}
    with open(path, "wb") as f:
        np.save(f, d, allow_pickle=True)
    return os.path.getsize(path)


class PredictionWriter:
    """A pool of `writers` threads that encode and write one image's products per job.  A job that raises is re-raised in the caller:
    by the next `submit`, by waiting on the job's future, or at the latest by `close` -- which writes the manifest only if every job
    succeeded."""

    def __init__(self, out_dir, products, writers=4):
        self.out_dir = str(out_dir)
        self.writers = check_writers(writers)
        unknown = [p for p in products if p not in PNG_PRODUCTS and p not in NPY_DIRS and p not in RGB_PRODUCTS and p not in CLASS_RGB_DIRS]
        if unknown:
            raise ValueError(f"unknown export products {unknown}")
        self.products = tuple(products)
        for p in self.products:
            os.makedirs(os.path.join(self.out_dir, NPY_DIRS.get(p, CLASS_RGB_DIRS.get(p, p))), exist_ok=True)
        self.pool = ThreadPoolExecutor(max_workers=self.writers, thread_name_prefix="cosa-export")
        self.lock = threading.Lock()
        self.bytes_written = 0
        self.images = []                          # (name, H, W) in submission order
        self.futures = []
        self.closed = False

    def _job(self, name, get_products, release):
        try:
            n = 0
            for key, val in get_products().items():
                if key in NPY_DIRS:
                    planes, idx = val
                    n += write_cam_npy(os.path.join(self.out_dir, NPY_DIRS[key], name + ".npy"), planes, idx)
                elif key in PNG_PRODUCTS:
                    n += write_png(os.path.join(self.out_dir, key, name + ".png"), val)
                elif key in RGB_PRODUCTS:
                    n += write_png_rgb(os.path.join(self.out_dir, key, name + ".png"), val)
                elif key in CLASS_RGB_DIRS:
                    pictures, names = val
                    for picture, cls in zip(pictures, names):
                        n += write_png_rgb(os.path.join(self.out_dir, CLASS_RGB_DIRS[key], class_file_name(name, cls) + ".png"), picture)
                else:
                    raise ValueError(f"unknown export product {key!r}")
            with self.lock:
                self.bytes_written += n
            return n
        finally:
            if release is not None:
                release()

    def _raise_finished(self):
        keep = []
        for f in self.futures:
            if f.done():
                f.result()                        # re-raises the job's exception here
            else:
                keep.append(f)
        self.futures = keep

    def submit(self, name, H, W, products, release=None):
        """products: {product: uint8 [H,W]} / {"rawcam"|"rawcam_aux": (float32 [K,H,W], int [K])} /
        {"camheat"|"camheat_aux"|"panel": (uint8 [k,H,cols*W,3], class names [k])} (cols: 1 for the heat maps, 3 or 4 for the panel; one
        file per class), or a callable returning that dict (run inside the job: the engine waits there for the record's copy).  The
        arrays must stay valid until the job is done; `release` is called then, whether the job succeeded or not.  Returns the job's
        future."""
        if self.closed:
            raise RuntimeError("PredictionWriter is closed")
        self._raise_finished()
        name = str(name)
        if not name or os.sep in name or name in (".", ".."):
            raise ValueError(f"bad image name {name!r}")
        self.images.append((name, int(H), int(W)))
        get = products if callable(products) else (lambda: products)
        f = self.pool.submit(self._job, name, get, release)
        self.futures.append(f)
        return f

    def drain(self):
        """wait for every job; the first failure is raised"""
        futures, self.futures = self.futures, []
        err = None
        for f in futures:
            try:
                f.result()
            except BaseException as e:            # noqa: B902  (keep waiting for the others: no thread may outlive the writer)
                err = err or e
        if err is not None:
            raise err

    def close(self, settings=None, images=None, write_manifest=True):
        """Wait for every file, then write manifest.json (`images`: the full list when several processes wrote into the directory;
        default: this writer's own).  Nothing is written if a job failed."""
        self.closed = True
        try:
            self.drain()
        finally:
            self.pool.shutdown(wait=True)
        if write_manifest:
            write_manifest_file(self.out_dir, settings or {}, self.images if images is None else images)
        return self.bytes_written


def write_manifest_file(out_dir, settings, images):
    tmp = os.path.join(str(out_dir), "manifest.json.tmp")
    with open(tmp, "w") as f:
        f.write(json.dumps({"settings": settings, "images": [{"name": n, "H": int(h), "W": int(w)} for n, h, w in images]}) + "\n")
    os.replace(tmp, os.path.join(str(out_dir), "manifest.json"))
