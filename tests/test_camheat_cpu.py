"""The CAM pictures of prediction export, host side: the colour ramp's shape, `predict`'s parser, the per-class file
names, and the record layout, which the pictures leave as it was."""
import json
import os

import numpy as np
import pytest
from PIL import Image

import camheat_ref as R

BASE = ["run", "--checkpoint", "best_seg.pth", "--out", "out"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "export_record_layout.json")


def test_the_ramp_is_the_classic_jet_in_integers():
    jet = R.jet_table()
    assert jet.shape == (256, 3) and jet.min() == 0 and jet.max() == 255
    assert tuple(jet[0]) == (0, 0, 128) and tuple(jet[255]) == (128, 0, 0)
    assert jet[128, 1] == 255
    for c in range(3):                                  # one rise and one fall, plateaus between: the steps change sign at most once
        d = np.diff(jet[:, c])
        steps = d[d != 0]
        flips = np.count_nonzero(np.diff(np.sign(steps)))
        assert flips <= 1 and np.abs(d).max() <= 4, (c, flips)
        top = np.nonzero(jet[:, c] == 255)[0]
        assert len(top) > 1 and np.array_equal(top, np.arange(top[0], top[-1] + 1))       # the top is one stretch
    assert np.array_equal(np.argmax(jet, axis=0)[::-1], sorted(np.argmax(jet, axis=0)))     # blue peaks first, then green, then red
    assert (jet[:, 2] >= 128).sum() > 0 and jet[:, 2][0] == 128                             # every picture's maximum is >= 128 ...
    assert (jet.max(axis=1) >= 128).all()                                                    # ... whatever the index


def test_index_truncates_and_clamps():
    f = np.float32
    below_one = np.nextafter(f(1.0), f(0.0))
    x = np.array([0.0, 1.0, below_one, 1.5, -0.25, np.nan, np.inf, -np.inf, 0.5, 1.0 / 255.0], np.float32)
    assert R.heat_index(x).tolist() == [0, 255, 254, 255, 0, 0, 255, 0, 127, int(np.trunc(f(255.0) * f(1.0 / 255.0)))]
    assert R.image_bytes(np.zeros((3, 1, 1), np.float32))[0, 0].tolist() == [124, 116, 104]      # rint of the means


def test_restatement_on_a_hand_case():
    """one pixel: m = 0.5 -> idx 127 -> jet (126, 255, 130); image byte (10, 20, 30): s = (136, 275, 160), M = 275"""
    heat = R.camheat_ref(np.full((1, 1, 1), 0.5, np.float32), np.array([[[10, 20, 30]]], np.uint8))
    assert tuple(R.jet_table()[127]) == (126, 255, 130)
    assert heat[0, 0, 0].tolist() == [255 * 136 // 275, 255, 255 * 160 // 275]
    seg, gt = np.array([[2]], np.uint8), np.array([[255]], np.uint8)
    p = R.panel_ref(np.concatenate([heat, heat]), seg, [1, 254], np.array([[[10, 20, 30]]], np.uint8), gt=gt)
    assert p.shape == (2, 1, 4, 3)
    assert p[0, 0].tolist() == [heat[0, 0, 0].tolist(), [10, 186, 181], [0, 0, 0], [10, 20, 30]]
    assert p[1, 0, 1].tolist() == [0, 0, 0] and p[1, 0, 2].tolist() == [0, 0, 0]              # class 255 against a gt of 255: no match
    assert R.panel_ref(heat, seg, [1], np.array([[[10, 20, 30]]], np.uint8)).shape == (1, 1, 3, 3)


def test_predict_parser_takes_the_picture_products(capsys):
    from cosa_amd import predict
    args, what = predict.parse(BASE + ["--what", "camheat,camheat_aux,panel"])
    assert what == ("camheat", "camheat_aux", "panel") and args.class_source == "given"
    _, what = predict.parse(BASE + ["--what", "seg,panel", "--classes", "predicted"])
    assert what == ("seg", "panel")
    for extra in (["--classes", "none"], ["--split", "test"]):
        for w in ("camheat", "camheat_aux", "panel", "camheat,camheat_aux,panel"):
            with pytest.raises(SystemExit) as e:
                predict.parse(BASE + ["--what", w] + extra)
            assert e.value.code == 2 and "label" in capsys.readouterr().err
    assert {"camheat", "camheat_aux", "panel"} <= set(predict.PRODUCTS) and "heatmap" not in predict.PRODUCTS


def test_file_names_replace_the_spaces_of_a_class_name(tmp_path):
    from cosa_amd.utils import export_io
    names = export_io.class_names("COCO", 80)
    assert names[9] == "traffic light" and export_io.class_file_name("000000000139", names[9]) == "000000000139_traffic_light"
    assert export_io.class_file_name("a", "person") == "a_person" and export_io.class_file_name("a", "3") == "a_3"
    assert export_io.CLASS_RGB_DIRS == {"camheat": "cam", "camheat_aux": "camaux", "panel": "merged"}
    rng = np.random.default_rng(0)
    heat = rng.integers(0, 256, (2, 4, 6, 3), dtype=np.uint8)
    wide = rng.integers(0, 256, (2, 4, 24, 3), dtype=np.uint8)
    w = export_io.PredictionWriter(tmp_path, ("camheat", "camheat_aux", "panel"), writers=2)
    w.submit("img", 4, 6, {"camheat": (heat, [names[9], names[0]]), "camheat_aux": (heat[::-1], [names[9], names[0]]),
                           "panel": (wide, [names[9], names[0]])})
    w.submit("none", 4, 6, {"camheat": (heat[:0], [])})                             # no present class: no file
    n = w.close(settings={})
    assert sorted(os.listdir(tmp_path)) == ["cam", "camaux", "manifest.json", "merged"]
    for d in ("cam", "camaux", "merged"):
        assert sorted(os.listdir(tmp_path / d)) == ["img_person.png", "img_traffic_light.png"]
    assert n == sum(os.path.getsize(tmp_path / d / f) for d in ("cam", "camaux", "merged") for f in os.listdir(tmp_path / d))
    for d, a in (("cam", heat), ("camaux", heat[::-1]), ("merged", wide)):
        im = Image.open(tmp_path / d / "img_traffic_light.png")
        assert im.mode == "RGB" and np.array_equal(np.asarray(im), a[0])
        assert np.array_equal(np.asarray(Image.open(tmp_path / d / "img_person.png")), a[1])
    with pytest.raises(ValueError, match="unknown"):
        export_io.PredictionWriter(tmp_path / "x", ("heatmap",), writers=1)


def test_record_layout_is_the_one_before_the_pictures():
    """every mask of the existing slots at two shapes, against the table recorded from the commit before the pictures (and two rows of it
    worked out by hand): the pictures lie behind the record, the layout does not know them"""
    from cosa_amd.utils import seg_helper
    table = json.load(open(GOLDEN))
    assert table["slots"] == list(seg_helper._EXPORT_SLOTS) and seg_helper.EXPORT_BITS == {
        "seg": 1, "pseudo": 2, "pseudo_aux": 4, "rawcam": 8, "rawcam_aux": 16, "pseudo_par": 32, "pseudo_aux_par": 64}
    by_hand = {(20, 5, 7, 2): [848, 0, 48, 96, 144, 432, 720, 736, 752, 800],       # 35 -> 48 per map, 2 * 35 * 4 = 280 -> 288 per stack, 8 -> 16 per index row
               (80, 33, 31, 3): [29728, 0, 1024, 2048, 3072, 15360, 27648, 27664, 27680, 28704]}        # 1023 -> 1024, 3 * 1023 * 4 = 12276 -> 12288, 12 -> 16
    for shape, full in by_hand.items():
        rows = table["shapes"][",".join(map(str, shape))]
        assert len(rows) == 127 and rows[126] == full
        for mask in range(1, 128):
            offs, n = seg_helper.export_record_layout(*shape, mask)
            assert [n] + [offs.get(s, -1) for s in seg_helper._EXPORT_SLOTS] == rows[mask - 1], (shape, mask)
    for name in ("camheat", "camheat_aux", "panel", "heatmap"):
        with pytest.raises(ValueError):
            seg_helper.export_what_mask((name,))
