"""Read per-image score files: `image_scores_<s|t>.jsonl` of `--image_scores true` / evaluate(image_scores=...) and
`scores.jsonl` of `python -m cosa_amd.predict --scores`; and the boundary files in the same format:
`boundary_scores_<s|t>.jsonl` of `--boundary_scores true` and `boundary_scores.jsonl` of `predict --boundary`, whose counters are taken
over the pixels within d of each map's own contours, so that every IoU below is then a Boundary IoU.  numpy only, no GPU.

    python tools/image_scores.py summary FILE [--json]
    python tools/image_scores.py worst FILE --map seg_vd [-n 20] [--json]
    python tools/image_scores.py compare A B --map seg_vd [--resamples 2000 --seed 0] [--json]

summary  per map the dataset IoU per class and the mIoU, recomputed from the summed integer counters I, P, G of the rows with the
         confusion-matrix formula I / (G + P - I) over the classes with G > 0: the table evaluate() printed.
worst    the images with the lowest per-image mIoU (assist_seg's `miou` of the file; images whose mIoU is NaN come last).
compare  two files joined by image name: the per-image mIoU deltas (B - A) sorted, the dataset mIoU of A and of B over the joined images,
         their difference, and a paired bootstrap 95 % interval of it: images are resampled with replacement, the same resample for both
         files, and the mIoU recomputed from the resample's summed counters (weights @ counts).  The same seed gives the same bytes.
"""
import argparse
import json
import sys

import numpy as np


def read(path):
    """-> (settings, names, counts [images, maps, num_classes, 4] int64 in the order I, P, G, A, per-image lines)"""
    with open(path) as f:
        lines = [json.loads(ln) for ln in f if ln.strip()]
    if not lines or "maps" not in lines[0] or "num_classes" not in lines[0]:
        raise SystemExit(f"{path}: not a score file (no settings line)")
    settings, images = lines[0], lines[1:]
    maps, nc = list(settings["maps"]), int(settings["num_classes"])
    counts = np.zeros((len(images), len(maps), nc, 4), np.int64)
    for i, d in enumerate(images):
        for m, name in enumerate(maps):
            for c, v in d["maps"][name]["classes"].items():
                counts[i, m, int(c)] = v
    return settings, [d["name"] for d in images], counts, images


def iou_from_counts(cnt):
    """cnt [..., num_classes, 4] summed counters -> (iou [..., num_classes], miou [...]): I / (G + P - I), mean over the classes with G > 0"""
    cnt = np.asarray(cnt, dtype=np.float64)
    I, P, G = cnt[..., 0], cnt[..., 1], cnt[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        iu = I / (G + P - I)
        valid = G > 0
        kept = np.where(valid & ~np.isnan(iu), iu, 0.0).sum(axis=-1)
        num = (valid & ~np.isnan(iu)).sum(axis=-1)
        miou = kept / num
    return iu, miou


def _map_index(settings, name, path):
    maps = list(settings["maps"])
    if name not in maps:
        raise SystemExit(f"{path}: no map {name!r} (it holds {', '.join(maps)})")
    return maps.index(name)


def summary(path):
    settings, names, counts, lines = read(path)
    total = counts.sum(axis=0)
    iu, _ = iou_from_counts(total)
    out = {"file": path, "images": len(names), "num_classes": int(settings["num_classes"]), "maps": {}}
    for m, name in enumerate(settings["maps"]):
        valid = total[m, :, 2] > 0                       # the mean exactly as the confusion-matrix scores take it: nanmean over G > 0
        miou = float(np.nanmean(iu[m][valid])) if valid.any() else float("nan")
        out["maps"][name] = {"iou": [None if v != v else float(v) for v in iu[m]], "miou": None if miou != miou else miou}
    if "boundary" in settings:                           # a boundary file: the band's settings and the widths the images were scored with
        ds = sorted({int(d["d"]) for d in lines if "d" in d})
        out["boundary"] = dict(settings["boundary"], d_min=ds[0] if ds else None, d_max=ds[-1] if ds else None)
    return out


def worst(path, map_name, n):
    settings, names, _, images = read(path)
    _map_index(settings, map_name, path)
    scored = [(d["maps"][map_name]["miou"], d["name"]) for d in images]
    scored.sort(key=lambda t: (t[0] is None, t[0] if t[0] is not None else 0.0, t[1]))
    return {"file": path, "map": map_name, "worst": [{"name": nm, "miou": v} for v, nm in scored[:n]]}


def compare(path_a, path_b, map_name, resamples=2000, seed=0):
    sa, names_a, ca, ia = read(path_a)
    sb, names_b, cb, ib = read(path_b)
    ma, mb = _map_index(sa, map_name, path_a), _map_index(sb, map_name, path_b)
    if int(sa["num_classes"]) != int(sb["num_classes"]):
        raise SystemExit("the two files differ in num_classes")
    pos_b = {}
    for i, nm in enumerate(names_b):
        pos_b.setdefault(nm, i)
    join = [(i, pos_b[nm]) for i, nm in enumerate(names_a) if nm in pos_b]
    if not join:
        raise SystemExit("the two files share no image name")
    A = ca[[i for i, _ in join], ma][..., :3].astype(np.float64)          # [images, classes, 3]
    B = cb[[j for _, j in join], mb][..., :3].astype(np.float64)
    miou_a, miou_b = float(iou_from_counts(A.sum(axis=0))[1]), float(iou_from_counts(B.sum(axis=0))[1])
    deltas = []
    for i, j in join:
        va, vb = ia[i]["maps"][map_name]["miou"], ib[j]["maps"][map_name]["miou"]
        deltas.append({"name": names_a[i], "a": va, "b": vb, "delta": None if va is None or vb is None else vb - va})
    deltas.sort(key=lambda d: (d["delta"] is None, d["delta"] if d["delta"] is not None else 0.0, d["name"]))
    # paired bootstrap: one multinomial draw of image weights per resample, used for both files
    rng = np.random.default_rng(seed)
    n = len(join)
    diffs = np.empty(resamples, np.float64)
    flat_a, flat_b = A.reshape(n, -1), B.reshape(n, -1)
    for lo in range(0, resamples, 256):
        k = min(256, resamples - lo)
        w = rng.multinomial(n, np.full(n, 1.0 / n), size=k).astype(np.float64)          # [k, images]
        ra = iou_from_counts((w @ flat_a).reshape(k, -1, 3))[1]
        rb = iou_from_counts((w @ flat_b).reshape(k, -1, 3))[1]
        diffs[lo:lo + k] = rb - ra
    lo95, hi95 = (float(v) for v in np.percentile(diffs, [2.5, 97.5])) if resamples else (float("nan"), float("nan"))
    return {"a": path_a, "b": path_b, "map": map_name, "images": n, "only_a": len(names_a) - n, "only_b": len(set(names_b)) - n,
            "miou_a": miou_a, "miou_b": miou_b, "diff": miou_b - miou_a, "ci95": [lo95, hi95], "resamples": resamples, "seed": seed,
            "deltas": deltas}


def _pct(v):
    return "  nan" if v is None or v != v else f"{100 * v:6.2f}"


def main(argv=None):
    p = argparse.ArgumentParser(prog="python tools/image_scores.py", description="per-image score files: summary, worst images, paired comparison")
    sub = p.add_subparsers(dest="cmd", required=True)
    q = sub.add_parser("summary")
    q.add_argument("file")
    q = sub.add_parser("worst")
    q.add_argument("file")
    q.add_argument("--map", required=True)
    q.add_argument("-n", type=int, default=20)
    q = sub.add_parser("compare")
    q.add_argument("a")
    q.add_argument("b")
    q.add_argument("--map", required=True)
    q.add_argument("--resamples", type=int, default=2000)
    q.add_argument("--seed", type=int, default=0)
    for q in sub.choices.values():
        q.add_argument("--json", action="store_true", help="one JSON document instead of the table")
    a = p.parse_args(argv)
    if a.cmd == "summary":
        res = summary(a.file)
        text = [f"{a.file}: {res['images']} images"]
        if "boundary" in res:
            b = res["boundary"]
            text[0] += (f", Boundary IoU: band of d = {b['d']} pixels" if b["d"] else f", Boundary IoU: band of {b['ratio']} of the diagonal") + \
                f" (d {b['d_min']}..{b['d_max']})"
        for name, d in res["maps"].items():
            text.append(f"{name:>14s}  mIoU {_pct(d['miou'])}  | " + " ".join(_pct(v).strip() for v in d["iou"]))
    elif a.cmd == "worst":
        res = worst(a.file, a.map, a.n)
        text = [f"{_pct(d['miou'])}  {d['name']}" for d in res["worst"]]
    else:
        if a.resamples < 0:
            p.error("--resamples must be >= 0")
        res = compare(a.a, a.b, a.map, a.resamples, a.seed)
        text = [f"{res['images']} images in both files ({res['only_a']} only in A, {res['only_b']} only in B), map {a.map}",
                f"dataset mIoU  A {_pct(res['miou_a'])}  B {_pct(res['miou_b'])}  B - A {100 * res['diff']:+.3f}  "
                f"95 % interval [{100 * res['ci95'][0]:+.3f}, {100 * res['ci95'][1]:+.3f}] ({res['resamples']} paired resamples, seed {res['seed']})"]
        moved = [d for d in res["deltas"] if d["delta"]]
        for d in moved[:10] + ([{"name": "...", "delta": None}] if len(moved) > 20 else []) + moved[10:][-10:]:
            text.append(f"{'' if d['delta'] is None else format(100 * d['delta'], '+8.2f')}  {d['name']}")
    sys.stdout.write(json.dumps(res, sort_keys=True) + "\n" if a.json else "\n".join(text) + "\n")
    return res


if __name__ == "__main__":
    main()
