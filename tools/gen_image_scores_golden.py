"""Write tests/golden/image_scores_assist.npz: (seg, gt, cls_label) triples and what the REFERENCE's own `assist_seg`
(evaluation_engine.py:311-329) returns for them (authoring container only: needs the reference tree, located as oracle.ref_loader
locates it).  Data only.

    python tools/gen_image_scores_golden.py [seed]

The reference's evaluation_engine module cannot be imported here (its imports pull packages this image lacks), so the one function is
taken out of the file's syntax tree and executed with numpy and torch in scope -- at generation time only; nothing of it is stored.
Six cases at 21 classes on 24 x 31 maps (int64 tensors, as evaluate() hands them over):
  0 ordinary                         1 gt with 255 regions the prediction labels (A != P)      2 a present class predicted nowhere (IoU 0)
  3 a present class in neither map (NaN miou)            4 a single present class              5 all 20 classes present
Per case k: seg_k, gt_k [24,31] uint8, cls_k [20] int64, ids_k [present] int64, iou_k / ratio_k [present] float64, means_k [miou, wmiou].
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader                                # noqa: E402

H, W, NC = 24, 31, 21


def reference_assist_seg():
    path = os.path.join(ref_loader.REF, "evaluation_engine.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "assist_seg"]
    assert len(fn) == 1, "assist_seg not found in the reference"
    scope = {"np": np, "torch": torch}
    exec(compile(ast.Module(body=fn, type_ignores=[]), path, "exec"), scope)
    return scope["assist_seg"]


def blocks(rng, classes, noise):
    """a map of rectangular regions of `classes` with `noise` share of pixels redrawn"""
    m = np.zeros((H, W), np.uint8)
    for c in classes:
        y, x = rng.integers(0, H - 6), rng.integers(0, W - 6)
        m[y:y + rng.integers(4, 12), x:x + rng.integers(4, 12)] = c
    flip = rng.random((H, W)) < noise
    m[flip] = rng.choice([0] + list(classes), size=int(flip.sum()))
    return m


def cases(rng):
    out = []
    gt = blocks(rng, [3, 8, 15], 0.0)                                        # 0: ordinary
    seg = np.where(rng.random((H, W)) < 0.8, gt, blocks(rng, [3, 8, 15], 0.3))
    out.append((seg, gt, [3, 8, 15]))
    gt = blocks(rng, [2, 12], 0.0)                                           # 1: ignore regions that the prediction labels
    seg = np.where(rng.random((H, W)) < 0.85, gt, blocks(rng, [2, 12], 0.2))
    gt = gt.copy()
    gt[:4] = 255
    gt[10:14, 5:20] = 255
    seg[:4, :10] = 2
    seg[10:14, 5:20] = 12
    out.append((seg, gt, [2, 12]))
    gt = blocks(rng, [5, 9], 0.0)                                            # 2: class 9 present, predicted nowhere
    gt[20:, 25:] = 9
    seg = np.where(gt == 9, 0, gt)
    out.append((seg, gt, [5, 9]))
    gt = blocks(rng, [7], 0.0)                                               # 3: class 19 present in the label row, in neither map
    gt[gt == 19] = 0
    seg = np.where(rng.random((H, W)) < 0.9, gt, 0).astype(np.uint8)
    out.append((seg, gt, [7, 19]))
    gt = blocks(rng, [20], 0.0)                                              # 4: one present class
    gt[2:8, 2:9] = 20
    seg = np.roll(gt, 2, axis=1)
    out.append((seg, gt, [20]))
    ids = list(range(1, 21))                                                 # 5: all 20 present
    gt = rng.integers(0, 21, (H, W)).astype(np.uint8)
    gt[:, :2] = np.arange(H)[:, None] % 20 + 1
    seg = np.where(rng.random((H, W)) < 0.6, gt, rng.integers(0, 21, (H, W))).astype(np.uint8)
    gt[-2:] = 255
    out.append((seg, gt, ids))
    return out


def main(seed):
    assert os.path.isfile(os.path.join(ref_loader.REF, "evaluation_engine.py")), "reference tree not present"
    assist_seg = reference_assist_seg()
    rng = np.random.default_rng(seed)
    out = {"seed": np.int64(seed), "num_classes": np.int64(NC)}
    for k, (seg, gt, present) in enumerate(cases(rng)):
        cls = np.zeros(NC - 1, np.int64)
        cls[[c - 1 for c in present]] = 1
        with np.errstate(all="ignore"):
            d = assist_seg(torch.from_numpy(seg.astype(np.int64)), torch.from_numpy(gt.astype(np.int64)), torch.from_numpy(cls))
        ids = [i for i in d if i not in ("miou", "wmiou")]
        assert ids == sorted(present)
        out[f"seg_{k}"], out[f"gt_{k}"], out[f"cls_{k}"] = seg.astype(np.uint8), gt.astype(np.uint8), cls
        out[f"ids_{k}"] = np.array(ids, np.int64)
        out[f"iou_{k}"] = np.array([d[i][0] for i in ids], np.float64)
        out[f"ratio_{k}"] = np.array([d[i][1] for i in ids], np.float64)
        out[f"means_{k}"] = np.array([d["miou"], d["wmiou"]], np.float64)
    path = os.path.join(ROOT, "tests", "golden", "image_scores_assist.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    for k in range(6):
        print(k, out[f"ids_{k}"].tolist(), out[f"iou_{k}"].round(3).tolist(), out[f"means_{k}"].tolist())


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 0)
