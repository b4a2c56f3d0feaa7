"""Label-free export without a GPU: the command line's argument errors, the `--images` source, the resolution of
an unset `--classes`, the numpy restatement of the class rule on cases whose answers are written out, the overlay restatement, the
classification figures and the host writers."""
import json

import numpy as np
import pytest
from PIL import Image

import predict_ref as R

BASE = ["run", "--checkpoint", "best_seg.pth", "--out", "out"]


def _pictures(d, names=("b.jpg", "a.PNG", "c.JPEG")):
    d.mkdir(parents=True, exist_ok=True)
    for k, n in enumerate(names):
        Image.fromarray(np.full((4 + k, 5, 3), 40 * k, np.uint8)).save(d / n, format="PNG" if n.lower().endswith("png") else "JPEG")
    return d


def test_argument_errors_exit_with_status_2(tmp_path, capsys):
    from cosa_amd import predict
    pics = _pictures(tmp_path / "pics")
    empty = tmp_path / "empty"
    empty.mkdir()
    (empty / "notes.txt").write_text("no picture\n")
    twice = _pictures(tmp_path / "twice", ("x.jpg", "x.png"))
    lst = tmp_path / "twice.txt"
    lst.write_text(f"{pics / 'a.PNG'}\n{twice / 'x.jpg'}\n{twice / 'x.png'}\n")
    none = tmp_path / "none.txt"
    none.write_text("\n\n")
    for extra, needle in (
            (["--images", str(twice)], "two images"),                                               # two items with one stem
            (["--images", str(lst)], "two images"),
            (["--images", str(empty)], "no images"),                                       # an empty source
            (["--images", str(none)], "no images"),
            (["--images", str(tmp_path / "missing")], "--images"),
            (["--images", str(pics), "--split", "val"], "--split"),                        # with an explicit split
            (["--images", str(pics), "--scores"], "--scores"),                             # no masks
            (["--images", str(pics), "--classes", "given"], "given"),                      # a source without class rows
            (["--split", "test", "--classes", "given"], "given"),
            (["--classes", "sometimes"], "--classes"),
            (["--classes", "none", "--what", "seg,pseudo"], "label"),
            (["--classes", "predicted", "--cls_thre", "0"], "--cls_thre"),
            (["--classes", "predicted", "--cls_thre", "1.0"], "--cls_thre"),
            (["--classes", "predicted", "--cls_min", "-1"], "--cls_min"),
            (["--classes", "predicted", "--cls_min", "21"], "--cls_min"),
            (["--what", "overlay", "--overlay_alpha", "1.5"], "--overlay_alpha"),
            (["--what", "overlay,overlay"], "--what"),
            (["--what", "overlay", "--scores"], "--scores")):
        with pytest.raises(SystemExit) as e:
            predict.parse(BASE + extra)
        assert e.value.code == 2 and needle in capsys.readouterr().err, extra


def test_images_source_lists_sorted_stems(tmp_path):
    from cosa_amd import predict
    from cosa_amd.utils import export_io
    pics = _pictures(tmp_path / "pics")
    (pics / "readme.txt").write_text("not a picture")
    _pictures(pics / "sub", ("deep.jpg",))                                                 # not searched
    items = export_io.list_images(pics)
    assert [n for n, _ in items] == ["a", "b", "c"] and [p for _, p in items] == [str(pics / f) for f in ("a.PNG", "b.jpg", "c.JPEG")]
    lst = tmp_path / "list.txt"
    lst.write_text(f"pics/c.JPEG\n\n{pics / 'a.PNG'}\n")                                   # relative to the list, in the list's order
    assert [n for n, _ in export_io.list_images(lst)] == ["c", "a"]
    with pytest.raises(ValueError, match="x"):
        export_io.list_images(_pictures(tmp_path / "twice", ("x.jpg", "x.png")))
    args, what = predict.parse(BASE + ["--images", str(pics), "--what", "seg,pseudo,rawcam,overlay", "--num_classes", "5"])
    assert what == ("seg", "pseudo", "rawcam", "overlay") and args.class_source == "predicted" and args.split is None
    assert [n for n, _ in args.image_items] == ["a", "b", "c"] and (args.cls_thre, args.cls_min, args.overlay_alpha) == (0.5, 1, 0.5)
    ds = predict._ImageFiles(args.image_items)
    name, img, lab, cls = ds[1]
    assert len(ds) == 3 and name == "b" and img.shape == (3, 4, 5) and img.dtype == np.float32 and (lab, cls) == (0, 0)
    assert predict.parse(BASE + ["--images", str(pics), "--classes", "none"])[0].class_source == "none"


def test_unset_classes_resolve_to_todays_behaviour():
    from cosa_amd import predict
    for split, source in (("val", "given"), ("train", "given"), ("train_aug", "given"), ("test", "none")):
        args, _ = predict.parse(BASE + ["--split", split])
        assert args.classes is None and args.class_source == source and args.split == split
    args, _ = predict.parse(BASE)
    assert args.split == "val" and args.class_source == "given" and args.image_items is None
    args, what = predict.parse(BASE + ["--split", "test", "--classes", "predicted", "--what", "seg,pseudo", "--cls_thre", "0.3", "--cls_min", "0"])
    assert args.class_source == "predicted" and what == ("seg", "pseudo") and (args.cls_thre, args.cls_min) == (0.3, 0)
    assert predict.parse(BASE + ["--classes", "predicted", "--scores"])[0].scores is True                 # a labelled split: legal together


def test_threshold_logit_is_float32_of_the_float64_logit():
    from cosa_amd.utils import seg_helper
    assert R.threshold_logit(0.5) == 0 and seg_helper.cls_threshold_logit(0.5) == 0.0
    assert R.threshold_logit(0.3) == np.float32(-0.84729785) and R.threshold_logit(0.9) == np.float32(2.1972246)
    for t in (0.3, 0.5, 0.9, 0.01, 0.999):
        assert np.float32(seg_helper.cls_threshold_logit(t)) == R.threshold_logit(t)
    assert np.nextafter(np.float32(2.1972246), np.float32(0)) == np.float32(2.1972244)                    # the crafted "one below L"
    for bad in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            seg_helper.cls_threshold_logit(bad)


@pytest.mark.parametrize("k", range(len(R.CRAFTED)))
def test_restatement_on_hand_written_cases(k):
    (logits, t, cls_min), (present, nonfinite) = R.CRAFTED[k]
    rows, k_live, bad = R.predict_classes_ref(np.array(logits, np.float32), t, cls_min)
    want = np.zeros(R.CRAFTED_C, np.float32)
    want[present] = 1
    assert rows.dtype == np.float32 and rows.shape == (1, R.CRAFTED_C) and np.array_equal(rows[0], want)
    assert k_live.dtype == np.int32 and k_live.tolist() == [len(present)] and bad.tolist() == [nonfinite]


def test_overlay_restatement_on_hand_written_pixels():
    from cosa_amd.utils import export_io
    pal = export_io.voc_colormap()
    img = np.array([[[10, 20, 30], [200, 100, 0], [255, 255, 255], [1, 2, 3]]], np.uint8)
    seg = np.array([[0, 1, 255, 2]], np.uint8)                                            # colours (128,0,0), (224,224,192), (0,128,0)
    assert np.array_equal(R.overlay_ref(img, seg, pal, 0.0), img)
    assert np.array_equal(R.overlay_ref(img, seg, pal, 1.0)[0], [[10, 20, 30], [128, 0, 0], [224, 224, 192], [0, 128, 0]])
    # alpha 0.5: (128 p + 128 i + 128) >> 8
    assert np.array_equal(R.overlay_ref(img, seg, pal, 0.5)[0], [[10, 20, 30], [164, 50, 0], [240, 240, 224], [1, 65, 2]])
    assert R.alpha256(0.5) == 128 and R.alpha256(1.0) == 256 and R.alpha256(0.3) == 77


def test_classification_figures_on_three_images():
    from cosa_amd.utils import export_io
    given = np.array([[1, 0, 1, 0], [0, 1, 0, 0], [1, 1, 0, 0]])
    pred = np.array([[1, 0, 1, 0], [0, 1, 1, 0], [0, 1, 0, 1]])
    # image 0 exact; image 1: tp 1, fp 1; image 2: tp 1, fp 1, fn 1
    f = export_io.classification_figures(pred, given)
    assert (f["exact"], f["tp"], f["fp"], f["fn"], f["images"]) == (1, 4, 2, 1, 3) == R.classification_ref(pred, given) + (3,)
    assert f["exact_match"] == 1 / 3 and f["precision"] == 4 / 6 and f["recall"] == 4 / 5 and f["f1"] == 8 / 11
    none = export_io.classification_figures(np.zeros((2, 3)), np.zeros((2, 3)))
    assert none["exact_match"] == 1.0 and none["precision"] is None and none["recall"] is None and none["f1"] is None


def test_classes_file_and_rgb_writer(tmp_path):
    from cosa_amd.utils import export_io
    logits = np.array([0.1, -2.5, np.nan, np.inf, 1e-30], np.float32)
    rows, k_live, bad = R.predict_classes_ref(logits, 0.5, 1)
    rec = export_io.class_record("pic", logits, rows[0], k_live[0], bad[0])
    export_io.write_classes_file(tmp_path / "classes.jsonl", [rec], export_io.class_names("VOC12", 5))
    line = (tmp_path / "classes.jsonl").read_text().splitlines()
    assert len(line) == 1 and '"logits": [0.1, -2.5, NaN, Infinity, 1e-30]' in line[0]                    # float32 by its own repr
    d = json.loads(line[0])
    assert d["name"] == "pic" and d["classes"] == [1, 4, 5] and d["class_names"] == ["1", "4", "5"] and d["k_live"] == 3 and d["nonfinite"] == 2
    back = np.array(d["logits"], np.float32)
    assert np.array_equal(back, logits, equal_nan=True)
    assert d["prob"][0] == 1.0 / (1.0 + np.exp(-np.float64(np.float32(0.1)))) and d["prob"][3] == 1.0
    assert export_io.class_names("VOC12", 20)[14] == "person" and len(export_io.class_names("COCO", 80)) == 80
    rgb = np.arange(2 * 3 * 3, dtype=np.uint8).reshape(2, 3, 3)
    n = export_io.write_png_rgb(tmp_path / "o.png", rgb)
    im = Image.open(tmp_path / "o.png")
    assert n > 0 and im.mode == "RGB" and np.array_equal(np.asarray(im), rgb)
    with pytest.raises(ValueError):
        export_io.write_png_rgb(tmp_path / "bad.png", rgb[:, :, 0])
    w = export_io.PredictionWriter(tmp_path / "w", ("seg", "overlay"), writers=1)
    w.submit("p", 2, 3, {"seg": np.zeros((2, 3), np.uint8), "overlay": rgb})
    w.close()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "w" / "overlay" / "p.png")), rgb)
