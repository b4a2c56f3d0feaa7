"""Per-image evaluation scores, host side: the reference's assist_seg from integer counters, the dataset table from
summed rows, the score file, the rank merge, tools/image_scores.py and the flags.  No GPU."""
import importlib.util
import json
import os

import numpy as np
import pytest

import image_scores_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = 21


def _tool():
    spec = importlib.util.spec_from_file_location("image_scores_tool", os.path.join(ROOT, "tools", "image_scores.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("k", range(6))
def test_assist_from_counts_has_the_reference_bits(golden, k):
    from cosa_amd.utils import evaluation as ev
    g = golden("image_scores_assist")
    seg, gt, cls = g[f"seg_{k}"], g[f"gt_{k}"], g[f"cls_{k}"]
    d = ev.assist_from_counts(*R.ref_counts(seg, gt, NC), cls)
    ids = [i for i in d if i not in ("miou", "wmiou")]
    assert ids == g[f"ids_{k}"].tolist()
    for name, got in (("iou", [d[i][0] for i in ids]), ("ratio", [d[i][1] for i in ids]), ("means", [d["miou"], d["wmiou"]])):
        got, want = np.array(got, np.float64), g[f"{name}_{k}"]
        assert got.tobytes() == want.tobytes() or (np.array_equal(np.isnan(got), np.isnan(want))
                                                   and got[~np.isnan(got)].tobytes() == want[~np.isnan(want)].tobytes()), (name, got, want)
    # the same through a row: a map that labels every pixel with a class has G == G_all on the valid pixels ... but assist_seg's
    # gt_area ignores nothing, so the row route is exact only where gt holds no 255 (cases 0, 2, 3, 4)
    if not (gt == 255).any():
        row = R.ref_row(gt, [seg], [0], NC)
        d2 = ev.assist_from_row(row, NC, 0, cls)
        assert repr(d2) == repr(d)


def test_golden_covers_the_cases_the_row_distinguishes(golden):
    g = golden("image_scores_assist")
    row = R.ref_row(g["gt_1"], [g["seg_1"]], [0], NC)
    cnt = row[2:].reshape(1, NC, 4)[0]
    assert (cnt[:, 3] > cnt[:, 1]).any()                                  # A != P: the prediction labels ignored ground truth
    assert 0.0 in g["iou_2"] and np.isnan(g["means_3"][0]) and len(g["ids_4"]) == 1 and len(g["ids_5"]) == 20


def _random_maps(rng, n_img, nc):
    out = []
    for _ in range(n_img):
        n = int(rng.integers(50, 400))
        gt = rng.integers(0, nc, n).astype(np.uint8)
        gt[rng.random(n) < 0.1] = 255
        plain = np.where(rng.random(n) < 0.6, gt, rng.integers(0, nc, n)).astype(np.uint8)
        plain[plain == 255] = 0
        pseudo = plain.copy()
        pseudo[rng.random(n) < 0.2] = 255
        out.append((gt, plain, pseudo))
    return out


@pytest.mark.parametrize("nc", [2, 21, 81])
def test_dataset_scores_equal_scores_from_hist(nc):
    from cosa_amd.utils import evaluation as ev
    rng = np.random.default_rng(nc)
    maps = _random_maps(rng, 9, nc)
    rows = np.stack([R.ref_row(gt, [a, b], [0, 1], nc) for gt, a, b in maps])
    got = ev.dataset_scores(rows, nc)
    for m, pseudo in ((0, False), (1, True)):
        hist = sum(R.confusion(t[0], t[1 + m], nc, pseudo) for t in maps)
        want = ev.scores_from_hist(hist)
        cnt = rows[:, 2:].sum(axis=0).reshape(2, nc, 4)[m]
        assert np.array_equal(cnt[:, 0], np.diag(hist)) and np.array_equal(cnt[:, 1], hist.sum(axis=0)) and np.array_equal(cnt[:, 2], hist.sum(axis=1))
        assert np.array_equal(got[m]["iou"], np.array(list(want["iou"].values())), equal_nan=True)
        assert got[m]["miou"] == want["miou"]
    assert got[0]["labelled"] == 1.0 and 0.7 < got[1]["labelled"] < 0.9


def _records(rng, names, nc=NC, better=()):
    from cosa_amd.utils import evaluation as ev
    recs = []
    for nm in names:
        n = 24 * 31
        gt = np.zeros(n, np.uint8)
        present = sorted(rng.choice(np.arange(1, nc), 2, replace=False).tolist())
        gt[100:300], gt[400:600] = present
        gt[:20] = 255
        err = 0.1 if nm in better else 0.4
        vd = np.where(rng.random(n) < err, rng.choice([0] + present, n), gt).astype(np.uint8)
        vd[gt == 255] = present[0]
        ps = vd.copy()
        ps[rng.random(n) < 0.3] = 255
        recs.append(ev.score_record(nm, 24, 31, present, R.ref_row(gt, [vd, ps], [0, 1], nc)))
    return recs


SETTINGS = {"maps": ["seg_vd", "cam_0.3"], "pseudo": [0, 1], "num_classes": NC, "epoch": 7, "s_or_t": "t", "world_size": 1, "checkpoint": None}


def test_score_file_round_trip(tmp_path):
    from cosa_amd.utils import evaluation as ev
    recs = _records(np.random.default_rng(0), [f"im{i}" for i in range(5)])
    recs.append(ev.score_record("empty", 3, 4, [], R.ref_row(np.full(12, 255, np.uint8), [np.zeros(12, np.uint8)] * 2, [0, 1], NC)))
    ev.write_score_file(tmp_path / "a.jsonl", SETTINGS, recs)
    lines = [json.loads(ln) for ln in open(tmp_path / "a.jsonl")]                   # plain JSON: NaN is null
    assert lines[0]["maps"] == SETTINGS["maps"] and lines[0]["pseudo"] == [0, 1] and lines[0]["epoch"] == 7
    assert set(lines[1]) == {"name", "h", "w", "n", "n_valid", "present", "maps"} and lines[1]["n"] == 744 and lines[1]["n_valid"] == 724
    assert lines[-1]["maps"]["seg_vd"]["miou"] is None and "NaN" not in open(tmp_path / "a.jsonl").read()
    first = recs[0]
    n, _, cnt = ev.split_row(first["row"], NC)
    cls = np.zeros(NC - 1, np.int64)
    cls[[c - 1 for c in first["present"]]] = 1
    want = ev.assist_from_counts(cnt[0][:, 0], cnt[0][:, 3], cnt[0][:, 2], n, cls)
    assert lines[1]["maps"]["seg_vd"]["miou"] == want["miou"] and lines[1]["maps"]["seg_vd"]["wmiou"] == want["wmiou"]
    assert all(any(v) for v in lines[1]["maps"]["seg_vd"]["classes"].values())      # non-zero classes only
    settings, back = ev.read_score_file(tmp_path / "a.jsonl")
    assert settings["num_classes"] == NC and len(back) == len(recs)
    for a, b in zip(recs, back):
        assert a["name"] == b["name"] and (a["h"], a["w"], a["present"]) == (b["h"], b["w"], b["present"]) and np.array_equal(a["row"], b["row"])
    ev.write_score_file(tmp_path / "b.jsonl", settings, back)
    assert open(tmp_path / "a.jsonl", "rb").read() == open(tmp_path / "b.jsonl", "rb").read()


def test_rank_merge_gives_dataset_order_and_first_of_a_duplicate():
    from cosa_amd.utils import evaluation as ev
    recs = _records(np.random.default_rng(1), ["a", "b", "c", "d", "a"])      # positions 0..4 over two ranks; the sampler's padding repeats "a"
    shard0 = [(0, recs[0]), (2, recs[2]), (4, recs[4])]
    shard1 = [(1, recs[1]), (3, recs[3])]
    merged = ev.merge_records([shard1, shard0])
    assert [r["name"] for r in merged] == ["a", "b", "c", "d"] and merged[0] is recs[0]
    assert [r["name"] for r in ev.gather_records(shard0)] == ["a", "c"]      # no process group: this rank's own, merged


def test_compare_tool(tmp_path, capsys):
    from cosa_amd.utils import evaluation as ev
    T = _tool()
    names = [f"im{i:03d}" for i in range(60)]
    ev.write_score_file(tmp_path / "a.jsonl", SETTINGS, _records(np.random.default_rng(2), names))
    ev.write_score_file(tmp_path / "b.jsonl", SETTINGS, _records(np.random.default_rng(2), names, better=set(names[::10])))      # 10 % improved
    same = T.compare(str(tmp_path / "a.jsonl"), str(tmp_path / "a.jsonl"), "seg_vd", 200, 0)
    assert same["diff"] == 0.0 and same["ci95"] == [0.0, 0.0] and same["images"] == 60 and all(d["delta"] == 0 for d in same["deltas"])
    res = T.compare(str(tmp_path / "a.jsonl"), str(tmp_path / "b.jsonl"), "seg_vd", 500, 0)
    assert res["diff"] > 0 and res["ci95"][0] > 0 and res["ci95"][0] <= res["diff"] <= res["ci95"][1]
    assert [d["delta"] for d in res["deltas"]] == sorted(d["delta"] for d in res["deltas"])
    # the data-set figures are those of the library's dataset_scores
    _, ra = ev.read_score_file(tmp_path / "a.jsonl")
    assert res["miou_a"] == ev.dataset_scores(np.stack([r["row"] for r in ra]), NC)[0]["miou"]
    outs = []
    for _ in range(2):
        T.main(["compare", str(tmp_path / "a.jsonl"), str(tmp_path / "b.jsonl"), "--map", "seg_vd", "--resamples", "300", "--seed", "5", "--json"])
        outs.append(capsys.readouterr().out)
    assert outs[0] == outs[1] and json.loads(outs[0])["seed"] == 5
    T.main(["compare", str(tmp_path / "a.jsonl"), str(tmp_path / "b.jsonl"), "--map", "seg_vd", "--resamples", "300", "--seed", "6", "--json"])
    assert json.loads(capsys.readouterr().out)["ci95"] != json.loads(outs[0])["ci95"]
    with pytest.raises(SystemExit):
        T.compare(str(tmp_path / "a.jsonl"), str(tmp_path / "b.jsonl"), "nope")


def test_summary_and_worst_tool(tmp_path, capsys):
    from cosa_amd.utils import evaluation as ev
    T = _tool()
    recs = _records(np.random.default_rng(3), [f"im{i}" for i in range(12)])
    ev.write_score_file(tmp_path / "a.jsonl", SETTINGS, recs)
    s = T.summary(str(tmp_path / "a.jsonl"))
    want = ev.dataset_scores(np.stack([r["row"] for r in recs]), NC)
    for m, name in enumerate(SETTINGS["maps"]):
        assert s["maps"][name]["miou"] == want[m]["miou"]
        assert np.array_equal(np.array([np.nan if v is None else v for v in s["maps"][name]["iou"]]), want[m]["iou"], equal_nan=True)
    w = T.worst(str(tmp_path / "a.jsonl"), "seg_vd", 3)["worst"]
    per = sorted(json.loads(ln)["maps"]["seg_vd"]["miou"] for ln in list(open(tmp_path / "a.jsonl"))[1:])
    assert [d["miou"] for d in w] == per[:3]
    T.main(["summary", str(tmp_path / "a.jsonl")])
    T.main(["worst", str(tmp_path / "a.jsonl"), "--map", "seg_vd", "-n", "2"])
    assert "mIoU" in capsys.readouterr().out


def test_flags(capsys):
    from cosa_amd import args as cosa_args
    from cosa_amd import predict
    assert cosa_args.parse(["run"])[0].image_scores is False
    a, changed = cosa_args.parse(["run", "--image_scores", "true"])
    assert a.image_scores is True and changed["image_scores"] is True
    base = ["run", "--checkpoint", "x.pth", "--out", "o"]
    assert predict.parse(base)[0].scores is False and predict.parse(base + ["--scores", "--split", "train_aug", "--what", "pseudo_par"])[0].scores is True
    with pytest.raises(SystemExit) as e:
        predict.parse(base + ["--scores", "--split", "test"])
    assert e.value.code == 2 and "ground-truth" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        predict.parse(base + ["--scores", "--what", "rawcam"])
    assert e.value.code == 2
