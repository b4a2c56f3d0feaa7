"""utils.export_io -- the host half of prediction export: file formats, the writer pool, the sharding rule.

Pure numpy / PIL: nothing here touches the GPU.  `evaluation_engine.export_predictions` hands finished host records to a
`PredictionWriter`; its threads encode and write

    <out_dir>/seg|seg_crf|pseudo|pseudo_aux|pseudo_par|pseudo_aux_par/<name>.png
                                                            palette PNGs (mode P) with the PASCAL VOC colour map
    <out_dir>/camraw|camraw_aux/<name>.npy                  a pickled dict {0-based class index: float32 [H,W]} (np.load(...,
                                                            allow_pickle=True).item()), as the reference's save_cam_npv2 writes it;
                                                            an image without any present class gets no file
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
NPY_DIRS = {"rawcam": "camraw", "rawcam_aux": "camraw_aux"}


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
        unknown = [p for p in products if p not in PNG_PRODUCTS and p not in NPY_DIRS]
        if unknown:
            raise ValueError(f"unknown export products {unknown}")
        self.products = tuple(products)
        for p in self.products:
            os.makedirs(os.path.join(self.out_dir, NPY_DIRS.get(p, p)), exist_ok=True)
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
        """products: {product: uint8 [H,W]} / {"rawcam"|"rawcam_aux": (float32 [K,H,W], int [K])}, or a callable returning that dict (run
        inside the job: the engine waits there for the record's copy).  The arrays must stay valid until the job is done; `release` is
        called then, whether the job succeeded or not.  Returns the job's future."""
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
