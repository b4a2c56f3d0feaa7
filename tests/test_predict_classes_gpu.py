"""Label-free export on the GPU: `cosa_predict_classes` and `cosa_export_overlay` against their numpy restatements
(tests/predict_ref.py), exactly; `python -m cosa_amd.predict --images` end to end -- the predicted path adds nothing but the row; the
defaults write today's bytes; `--classes predicted --scores` on a labelled split."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import image_scores_ref as SR
import predict_ref as R

pytestmark = pytest.mark.gpu
EINVAL = 1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random_logits(rng, G, C):
    """one decimal: plenty of equal logits, some exactly 0 = L at t 0.5; NaN and +-inf sprinkled in where there is room"""
    x = np.round(rng.standard_normal((G, C)) * 2, 1).astype(np.float32)
    if C >= 20:
        for g in range(G):
            x[g, rng.choice(C, 3, replace=False)] = [np.nan, np.inf, -np.inf]
    x[0, : max(1, C // 3)] = -1.5 - np.arange(max(1, C // 3), dtype=np.float32) % 2          # a stretch below every threshold, with ties
    return x


def _run(x, t, cls_min):
    from cosa_amd.utils import seg_helper
    rows, k_live, bad = seg_helper.predict_classes(dev(x), t, cls_min)
    assert rows.dtype == torch.float32 and k_live.dtype == torch.int32 and bad.dtype == torch.int32
    return rows.cpu().numpy(), k_live.cpu().numpy(), bad.cpu().numpy()


@pytest.mark.parametrize("G", [1, 5])
@pytest.mark.parametrize("C", [1, 20, 63, 64, 65, 80, 256])
def test_predict_classes_equals_the_restatement(C, G):
    rng = np.random.default_rng(1000 * C + G)
    x = _random_logits(rng, G, C)
    low = np.full((G, C), -7.0, np.float32) - (np.arange(C, dtype=np.float32) % 5)          # nothing present anywhere: the fill does all the work
    for cls_min in sorted({0, 1, min(3, C), C}):
        for t in (0.5, 0.3, 0.9):
            for src in (x, low):
                got, want = _run(src, t, cls_min), R.predict_classes_ref(src, t, cls_min)
                for a, b, what in zip(got, want, ("rows", "k_live", "nonfinite")):
                    assert a.shape == b.shape and np.array_equal(a, b), (what, C, G, cls_min, t)
    rows, k_live, _ = _run(low, 0.5, C)
    assert rows.min() == 1 and k_live.tolist() == [C] * G


@pytest.mark.parametrize("C", [R.CRAFTED_C, 64 + R.CRAFTED_C])
def test_predict_classes_on_the_crafted_rows(C):
    """the hand-written cases of the CPU test at G = 5: on their own (the answers written out there must come back) and in the second
    register's lanes behind 64 very low logits"""
    rng = np.random.default_rng(7)
    for k, ((logits, t, cls_min), (present, nonfinite)) in enumerate(R.CRAFTED):
        x = _random_logits(rng, 5, C)
        g = k % 5
        x[g, :C - R.CRAFTED_C] = -100.0 - np.arange(C - R.CRAFTED_C, dtype=np.float32)
        x[g, C - R.CRAFTED_C:] = logits
        got, want = _run(x, t, cls_min), R.predict_classes_ref(x, t, cls_min)
        for a, b in zip(got, want):
            assert np.array_equal(a, b), (k, C)
        if C == R.CRAFTED_C:
            assert np.nonzero(got[0][g])[0].tolist() == present and got[1][g] == len(present) and got[2][g] == nonfinite, k


def test_predict_classes_refuses_outside_the_envelope():
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    L = _C.lib()
    x = torch.zeros(4, 8, device="cuda")
    rows = torch.full((4, 8), 7.0, device="cuda")
    k_live, bad = torch.full((4,), -3, device="cuda", dtype=torch.int32), torch.full((4,), -5, device="cuda", dtype=torch.int32)
    p, null, s = _C.ptr, ctypes.c_void_p(0), _C.stream_ptr()
    for G, C, thr, cls_min, ptrs in ((4, 0, 0.0, 0, None), (4, 257, 0.0, 1, None), (0, 8, 0.0, 1, None), (65536, 8, 0.0, 1, None),
                                     (4, 8, 0.0, -1, None), (4, 8, 0.0, 9, None), (4, 8, float("nan"), 1, None),
                                     (4, 8, 0.0, 1, (null, p(rows), p(k_live), p(bad))), (4, 8, 0.0, 1, (p(x), null, p(k_live), p(bad))),
                                     (4, 8, 0.0, 1, (p(x), p(rows), null, p(bad))), (4, 8, 0.0, 1, (p(x), p(rows), p(k_live), null))):
        a = ptrs or (p(x), p(rows), p(k_live), p(bad))
        assert L.cosa_predict_classes(a[0], G, C, thr, cls_min, a[1], a[2], a[3], s) == EINVAL, (G, C, thr, cls_min)
    torch.cuda.synchronize()
    assert bool((rows == 7).all()) and bool((k_live == -3).all()) and bool((bad == -5).all())          # the poison is still there
    with pytest.raises(_C.CosaError, match="cls_min"):
        seg_helper.predict_classes(x, 0.5, 9)
    with pytest.raises(ValueError):
        seg_helper.predict_classes(x, 1.0, 1)
    with pytest.raises(_C.CosaError):
        seg_helper.predict_classes(x.cpu(), 0.5, 1)
    assert L.cosa_predict_classes(p(x), 4, 8, 0.0, 1, p(rows), p(k_live), p(bad), s) == 0
    assert k_live.tolist() == [8] * 4 and bool((rows == 1).all()) and bad.tolist() == [0] * 4


def _normalised(u8):
    from cosa_amd.dataloaders.train_loader import normalize_img
    return dev(np.transpose(normalize_img(u8), (2, 0, 1)))


@pytest.mark.parametrize("alpha", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("size", [(1, 1), (3, 5), (17, 33), (64, 64)])
def test_export_overlay_equals_the_restatement(size, alpha):
    from cosa_amd.utils import export_io, seg_helper
    H, W = size
    pal = export_io.voc_colormap()
    rng = np.random.default_rng(100 * H + W)
    for rep in range(2):
        u8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        u8.reshape(-1)[:2] = [0, 255]
        seg = rng.choice(np.array([0, 0, 1, 2, 7, 20, 21, 254, 255], np.uint8), (H, W))
        seg.reshape(-1)[0] = 255 if rep else 0                                             # both labels also at one pixel
        seg.reshape(-1)[-1] = 0 if rep else 255
        want = R.overlay_ref(u8, seg, pal, alpha)
        x = _normalised(u8)
        got = seg_helper.export_overlay(x, dev(seg), alpha)
        assert got.dtype == torch.uint8 and got.shape == (H, W, 3) and np.array_equal(got.cpu().numpy(), want)
        # into a record: the seg slot in front, the RGB bytes behind it at a 16-byte offset, the poison after them untouched
        off = (H * W + 15) & ~15
        rec = torch.full((off + 3 * H * W + 32,), 0xA5, device="cuda", dtype=torch.uint8)
        rec[:H * W] = dev(seg).reshape(-1)
        seg_helper.export_overlay(x, rec[:H * W], alpha, out=rec[off:off + 3 * H * W])
        back = rec.cpu().numpy()
        assert np.array_equal(back[off:off + 3 * H * W].reshape(H, W, 3), want) and (back[off + 3 * H * W:] == 0xA5).all()
        assert (back[H * W:off] == 0xA5).all()
        # buffers off their natural boundaries: the one-pixel path for every pixel, the same bytes
        buf = torch.zeros(H * W + 1, device="cuda", dtype=torch.uint8)
        buf[1:] = dev(seg).reshape(-1)
        out = torch.full((3 * H * W + 3,), 0x5A, device="cuda", dtype=torch.uint8)
        seg_helper.export_overlay(x, buf[1:], alpha, out=out[1:1 + 3 * H * W])
        back = out.cpu().numpy()
        assert np.array_equal(back[1:1 + 3 * H * W].reshape(H, W, 3), want) and back[0] == 0x5A and (back[-2:] == 0x5A).all()


def test_export_overlay_refuses_outside_the_envelope():
    from cosa_amd import _C
    from cosa_amd.utils import export_io, seg_helper
    L = _C.lib()
    x, seg = torch.zeros(3, 4, 4, device="cuda"), torch.ones(16, device="cuda", dtype=torch.uint8)
    pal, out = dev(export_io.voc_colormap()), torch.full((48,), 9, device="cuda", dtype=torch.uint8)
    p, null, s = _C.ptr, ctypes.c_void_p(0), _C.stream_ptr()
    for H, W, a, ptrs in ((0, 4, 128, None), (4, 0, 128, None), (-1, 4, 128, None), (1 << 15, 1 << 14, 128, None), (4, 4, -1, None),
                          (4, 4, 257, None), (4, 4, 128, (null, p(seg), p(pal), p(out))), (4, 4, 128, (p(x), null, p(pal), p(out))),
                          (4, 4, 128, (p(x), p(seg), null, p(out))), (4, 4, 128, (p(x), p(seg), p(pal), null))):
        q = ptrs or (p(x), p(seg), p(pal), p(out))
        assert L.cosa_export_overlay(q[0], q[1], q[2], H, W, a, q[3], s) == EINVAL, (H, W, a)
    torch.cuda.synchronize()
    assert bool((out == 9).all())
    with pytest.raises(ValueError):
        seg_helper.export_overlay(x, seg, 1.5)
    with pytest.raises(ValueError):
        seg_helper.export_overlay(x, seg[:15], 0.5)
    with pytest.raises(ValueError):
        seg_helper.export_overlay(x, seg, 0.5, out=out[:47])
    with pytest.raises(_C.CosaError):
        seg_helper.export_overlay(x.cpu(), seg.cpu(), 0.5)


# ---------------------------------------------------------------------------------------------------------------------------------
# the engine and the command line: a seeded tiny model, crop 64, C = 4
# ---------------------------------------------------------------------------------------------------------------------------------
C4 = 4
COMMON = ["--pretrained", "false", "--crop_size", "64", "--num_classes", str(C4 + 1), "--num_workers", "0"]


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """the trainer's own file for the seeded tiny network, and the parsed arguments that go with it"""
    from cosa_amd import predict
    from cosa_amd.main import _trainer_args
    from cosa_amd.models import build_model
    from cosa_amd.utils import torch_helper
    d = tmp_path_factory.mktemp("ckpt")
    args, _ = predict.parse(["run", "--checkpoint", "x", "--out", "x"] + COMMON)
    torch.manual_seed(0)
    return torch_helper.save_best(d, build_model(_trainer_args(args)), 1, 0.0, args, 't', comment='seg'), args


def _load_model(checkpoint):
    from cosa_amd import predict
    from cosa_amd.main import _trainer_args
    from cosa_amd.models import build_model
    path, args = checkpoint
    model = build_model(_trainer_args(args))
    predict.load_checkpoint(model, path)
    return model.cuda().eval()


def _model_and_loader(n=5, seed=0):
    """as tests/test_export_gpu.py builds them: items with a ground-truth map and a two-class row"""
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    torch.manual_seed(seed)
    args = default_args("VOC12", crop_size=64, batch_size=1)
    args.num_classes, args.bkg_thre = C4 + 1, 0.5
    model = build_model(args).cuda().eval()
    rng = np.random.default_rng(3)
    loader = []
    for k, (H, W) in enumerate([(50, 70), (64, 64), (81, 47), (33, 90), (37, 41)][:n]):
        img = torch.from_numpy(rng.standard_normal((1, 3, H, W)).astype(np.float32))
        lab = torch.from_numpy(rng.integers(0, C4 + 1, (1, H, W)).astype(np.int64))
        lab[0, :3] = 255
        cls = torch.zeros(1, C4)
        cls[0, rng.choice(C4, 2, replace=False)] = 1
        loader.append((f"img_{k:02d}", img, lab, cls))
    return args, model, loader


def test_images_folder_end_to_end(checkpoint, tmp_path, capsys):
    from cosa_amd import evaluation_engine as ee
    from cosa_amd import predict
    from cosa_amd.utils import export_io
    path, args = checkpoint
    rng = np.random.default_rng(5)
    pics = tmp_path / "pics"
    pics.mkdir()
    files = [("e.jpg", (40, 60)), ("a.jpg", (64, 48)), ("c.png", (33, 35)), ("b.JPG", (57, 64)), ("d.jpeg", (48, 81))]
    for f, (H, W) in files:
        small = rng.integers(0, 256, (H // 8 + 2, W // 8 + 2, 3), dtype=np.uint8)
        Image.fromarray(small).resize((W, H), Image.BICUBIC).save(pics / f, format="PNG" if f.endswith("png") else "JPEG")
    names = ["a", "b", "c", "d", "e"]
    sizes = dict((os.path.splitext(f)[0], s) for f, s in files)
    out = tmp_path / "out"
    res = predict.main(["run", "--checkpoint", path, "--out", str(out), "--images", str(pics), "--what", "seg,pseudo,rawcam,overlay"] + COMMON)
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["images"] == 5 and printed["images"] == 5 and "classes" not in res and res["class_wait_seconds"] >= 0
    assert sorted(os.listdir(out)) == ["camraw", "classes.jsonl", "manifest.json", "overlay", "pseudo", "seg"]
    man = json.loads((out / "manifest.json").read_text())
    assert man["images"] == [{"name": n, "H": sizes[n][0], "W": sizes[n][1]} for n in names]
    st = man["settings"]
    assert (st["classes"], st["cls_thre"], st["cls_min"], st["overlay_alpha"]) == ("predicted", 0.5, 1, 0.5) and st["images"] == str(pics)
    lines = [json.loads(ln) for ln in open(out / "classes.jsonl")]
    assert [ln["name"] for ln in lines] == names
    # a separate pass over the same inputs, grouped as the run grouped them
    model = _load_model(checkpoint)
    model.batch_invariant_heads = model.decoder.batch_invariant = True
    ds = predict._ImageFiles(export_io.list_images(pics))
    imgs = [torch.from_numpy(ds[k][1])[None] for k in range(5)]
    camseg = ee._GraphedCamSeg(model, ee.EVAL_SCALES, enabled=model.can_forward_multi is not None)
    logits = []
    with torch.no_grad():
        for group in (imgs[:4], imgs[4:]):
            x = torch.cat([torch.nn.functional.interpolate(i.cuda(), size=[64, 64], mode="bilinear", align_corners=False) for i in group], dim=0)
            logits.append(camseg(x)[3].float().cpu().numpy().copy())
    model.batch_invariant_heads = model.decoder.batch_invariant = False
    logits = np.concatenate(logits, axis=0)
    rows, k_live, bad = R.predict_classes_ref(logits, 0.5, 1)
    given = []
    for k, ln in enumerate(lines):
        row = np.zeros(C4, np.float32)
        row[[c - 1 for c in ln["classes"]]] = 1
        assert np.array_equal(row, rows[k]) and ln["k_live"] == k_live[k] >= 1 and ln["nonfinite"] == bad[k] == 0, ln["name"]
        assert ln["class_names"] == [str(c) for c in ln["classes"]] and len(ln["logits"]) == len(ln["prob"]) == C4
        assert np.array_equal(np.array(ln["prob"]), 1.0 / (1.0 + np.exp(-np.array(ln["logits"], np.float32).astype(np.float64))))
        given.append((ln["name"], imgs[k], 0, torch.from_numpy(row)[None]))
    # the same rows handed in as GIVEN labels: the same bytes in every file
    ee.export_predictions(model, given, args, tmp_path / "given", what=("seg", "pseudo", "rawcam"), classes="given")
    a, b = _tree(out), _tree(tmp_path / "given")
    for d, ext in (("seg", ".png"), ("pseudo", ".png"), ("camraw", ".npy")):
        for n in names:
            key = os.path.join(d, n + ext)
            assert a[key] == b[key], key
    assert not (tmp_path / "given" / "classes.jsonl").exists()
    pal = export_io.voc_colormap()
    for (n, p) in export_io.list_images(pics):
        H, W = sizes[n]
        seg = Image.open(out / "seg" / (n + ".png"))
        assert seg.mode == "P" and seg.size == (W, H) and Image.open(out / "pseudo" / (n + ".png")).size == (W, H)
        cam = np.load(out / "camraw" / (n + ".npy"), allow_pickle=True).item()
        assert sorted(cam) == [c - 1 for c in lines[names.index(n)]["classes"]] and all(v.shape == (H, W) for v in cam.values())
        ov = Image.open(out / "overlay" / (n + ".png"))
        assert ov.mode == "RGB"
        src = np.asarray(Image.open(p).convert("RGB"))
        assert np.array_equal(np.asarray(ov), R.overlay_ref(src, np.asarray(seg), pal, 0.5)), n


def test_unset_classes_write_todays_bytes(tmp_path):
    from cosa_amd import evaluation_engine as ee
    args, model, loader = _model_and_loader(n=3)
    what = ("seg", "pseudo", "rawcam_aux")
    ee.export_predictions(model, loader, args, tmp_path / "unset", what=what)
    ee.export_predictions(model, loader, args, tmp_path / "given", what=what, classes="given")
    free = [(n, img, 0, torch.tensor([0])) for n, img, _, _ in loader]                      # the test stage's items
    ee.export_predictions(model, free, args, tmp_path / "free_unset", what=("seg",))
    ee.export_predictions(model, free, args, tmp_path / "free_none", what=("seg",), classes="none")
    ee.export_predictions(model, loader, args, tmp_path / "rows_none", what=("seg",), classes="none")      # rows there, not used
    for x, y in (("unset", "given"), ("free_unset", "free_none"), ("free_unset", "rows_none")):
        a, b = _tree(tmp_path / x), _tree(tmp_path / y)
        assert sorted(a) == sorted(b) and "classes.jsonl" not in a and len(a) > 1
        assert all(a[k] == b[k] for k in a if k != "manifest.json"), (x, y)
    unset = json.loads((tmp_path / "unset" / "manifest.json").read_text())["settings"]
    given = json.loads((tmp_path / "given" / "manifest.json").read_text())["settings"]
    assert "classes" not in unset and "cls_thre" not in unset and given.pop("classes") == "given" and given == unset
    with pytest.raises(ValueError, match="label row"):
        ee.export_predictions(model, free, args, tmp_path / "bad", what=("seg",), classes="given")
    with pytest.raises(ValueError):
        ee.export_predictions(model, loader, args, tmp_path / "bad2", what=("seg", "pseudo"), classes="none")
    with pytest.raises(ValueError):
        ee.export_predictions(model, loader, args, tmp_path / "bad3", what=("seg",), classes="predicted", cls_min=C4 + 1)
    # an empty predicted row (cls_min 0 under a threshold nothing reaches) gives the bytes of a given all-zero row
    zero = [(n, img, lab, torch.zeros(1, C4)) for n, img, lab, _ in loader]
    ee.export_predictions(model, zero, args, tmp_path / "zero_given", what=("seg", "pseudo", "rawcam"))
    res = ee.export_predictions(model, free, args, tmp_path / "zero_pred", what=("seg", "pseudo", "rawcam", "overlay"), classes="predicted",
                                cls_thre=1 - 1e-15, cls_min=0)
    a, b = _tree(tmp_path / "zero_given"), _tree(tmp_path / "zero_pred")
    assert all(a[k] == b[k] for k in a if k != "manifest.json") and not any(k.startswith("camraw") for k in b) and "classes" not in res
    for n, img, _, _ in loader:
        assert not np.asarray(Image.open(tmp_path / "zero_pred" / "seg" / (n + ".png"))).any()
    assert [json.loads(ln)["classes"] for ln in open(tmp_path / "zero_pred" / "classes.jsonl")] == [[], [], []]


def test_predicted_rows_with_scores_on_a_labelled_split(checkpoint, tmp_path, capsys):
    from cosa_amd import predict
    from cosa_amd.utils import evaluation as ev
    from cosa_amd.utils import export_io
    path, _ = checkpoint
    rng = np.random.default_rng(0)
    root, lists = tmp_path / "voc", tmp_path / "lists"
    names, sizes = ["2007_000001", "2007_000002", "2007_000003"], [(40, 60), (64, 48), (33, 35)]
    os.makedirs(root / "JPEGImages")
    os.makedirs(root / "SegmentationClassAug")
    masks = {}
    for n, (H, W) in zip(names, sizes):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(root / "JPEGImages" / (n + ".jpg"))
        masks[n] = rng.integers(0, C4 + 1, (H, W)).astype(np.uint8)
        masks[n][:2] = 255
        Image.fromarray(masks[n]).save(root / "SegmentationClassAug" / (n + ".png"))
    os.makedirs(lists)
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    onehot = {n: np.eye(C4, dtype=np.float32)[k] + np.eye(C4, dtype=np.float32)[3] * (k < 3) for k, n in enumerate(names)}
    np.save(lists / "cls_labels_onehot.npy", onehot, allow_pickle=True)
    common = COMMON + ["--voc12_root", str(root), "--name_list_dir", str(lists)]
    out = tmp_path / "val"
    res = predict.main(["run", "--checkpoint", path, "--out", str(out), "--split", "val", "--what", "seg,pseudo", "--classes", "predicted",
                        "--cls_min", "2", "--scores"] + common)
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["images"] == 3 and printed["scores"] == res["scores"] and printed["classes"] == res["classes"]
    settings, recs = ev.read_score_file(out / "scores.jsonl")
    assert settings["maps"] == ["seg", "pseudo"] and [r["name"] for r in recs] == names
    nc = C4 + 1
    cnt = np.stack([r["row"] for r in recs])[:, 2:].sum(axis=0).reshape(2, nc, 4)
    for m, (prod, pseudo) in enumerate((("seg", False), ("pseudo", True))):
        conf = sum(SR.confusion(masks[n], np.asarray(Image.open(out / prod / (n + ".png"))), nc, pseudo) for n in names)
        assert np.array_equal(cnt[m][:, 0], np.diag(conf)) and np.array_equal(cnt[m][:, 1], conf.sum(axis=0))
        assert np.array_equal(cnt[m][:, 2], conf.sum(axis=1)), prod
    for r, n in zip(recs, names):                                                          # `present` stays the truth's
        assert r["present"] == (np.nonzero(onehot[n])[0] + 1).tolist()
    lines = [json.loads(ln) for ln in open(out / "classes.jsonl")]
    pred = np.zeros((3, C4))
    for k, ln in enumerate(lines):
        assert ln["name"] == names[k] and ln["k_live"] == len(ln["classes"]) >= 2
        pred[k, [c - 1 for c in ln["classes"]]] = 1
        seen = set(np.unique(np.asarray(Image.open(out / "seg" / (names[k] + ".png")))).tolist())
        assert seen <= {0} | set(ln["classes"])                                            # the maps were validated by the predicted row
    exact, tp, fp, fn = R.classification_ref(pred, np.stack([onehot[n] for n in names]))
    c = res["classes"]
    assert (c["exact"], c["tp"], c["fp"], c["fn"], c["images"]) == (exact, tp, fp, fn, 3) and tp + fp >= 6
    assert c["precision"] == tp / (tp + fp) and c["recall"] == tp / (tp + fn) and c["exact_match"] == exact / 3
    assert c["f1"] == 2 * tp / (2 * tp + fp + fn)
    assert json.loads((out / "manifest.json").read_text())["settings"]["classes_vs_given"] == c
    assert c == export_io.classification_figures(pred, np.stack([onehot[n] for n in names]))
