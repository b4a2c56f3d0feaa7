"""Boundary IoU counters without a GPU: the two routes of the numpy restatement against each other, the band's width,
the row's properties, the score file and the tools on it, the flags and their refusals."""
import importlib.util
import json
import os

import numpy as np
import pytest

import boundary_scores_ref as B
import image_scores_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = 6


def _tool():
    spec = importlib.util.spec_from_file_location("image_scores_tool", os.path.join(ROOT, "tools", "image_scores.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _maps(seed, H, W, n_maps=3):
    rng = np.random.default_rng(seed)
    vals = list(range(NC)) + [255, NC + 3]
    gt = B.run_map(rng, H, W, vals)
    if H > 8 and W > 8:                                                  # an object in its one-pixel ring of 255
        gt[2:7, 2:8] = 255
        gt[3:6, 3:7] = 2
    return gt, [B.run_map(rng, H, W, vals) for _ in range(n_maps - 1)] + [gt.copy()]


@pytest.mark.parametrize("shape", [(1, 1), (1, 17), (13, 1), (7, 9), (24, 31)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_window_definition_equals_d_erosions(shape):
    H, W = shape
    for d in (1, 2, 3, 5, max(H, W)):
        gt, preds = _maps(H * 100 + W + d, H, W)
        for L in [gt] + preds:
            assert np.array_equal(B.band(L, d, NC), B.band_by_erosion(L, d, NC)), d
        assert np.array_equal(B.row(gt, preds, d, NC), B.row(gt, preds, d, NC, band_fn=B.band_by_erosion))


def test_band_of_a_block_is_its_frame():
    L = np.full((20, 30), 255, np.uint8)
    L[4:15, 5:25] = 1                                                    # 11 x 20 of class 1
    for d, inner in ((1, 9 * 18), (2, 7 * 16), (5, 1 * 10), (6, 0)):
        b = B.band(L, d, NC)
        assert b.sum() == 11 * 20 - inner and not b[L == 255].any()
    assert not B.band(np.full((9, 9), 0, np.uint8), 4, NC)[4, 4] and B.band(np.full((9, 9), 0, np.uint8), 4, NC).sum() == 80
    assert not B.band(np.full((9, 9), NC, np.uint8), 1, NC).any()        # a value that is no class is in no band


def test_boundary_width():
    """d = max(1, int(round(ratio * sqrt(H*H + W*W)))) in Python arithmetic, exactly this expression.  375 x 500 is itself a tie of round():
    its diagonal is 625 exactly, 0.02 * 625.0 == 12.5 in binary64, and Python rounds a tie to the even neighbour: 12, which is also what the
    Boundary IoU paper's code (the same expression) gives.  The feature request quotes 13 for this size next to the expression; the two
    cannot both hold, and the expression is the definition the kernel's callers, the reference and the files share, so 12 it is.
    376 x 500 (12.51) is the nearest size that gives 13."""
    from cosa_amd.utils.evaluation import boundary_width
    assert 0.02 * np.sqrt(375 * 375 + 500 * 500) == 12.5
    assert boundary_width(375, 500) == 12 == max(1, int(round(0.02 * np.sqrt(375 * 375 + 500 * 500))))
    assert boundary_width(376, 500) == 13 and boundary_width(500, 376) == 13
    assert boundary_width(1, 1) == 1 and boundary_width(10, 10) == 1
    # ties of round(): 0.02 * 125 = 2.5 and 0.02 * 175 = 3.5 exactly (75-100-125 and 105-140-175 triangles) go to the even neighbour
    assert 0.02 * 125 == 2.5 and boundary_width(75, 100) == 2 == int(round(2.5))
    assert 0.5 * 5.0 == 2.5 and boundary_width(3, 4, ratio=0.5) == 2 and boundary_width(9, 12, ratio=0.5) == 8   # 7.5 -> 8
    for h, w, r in ((333, 500, 0.02), (500, 281, 0.02), (64, 64, 0.1), (2000, 2500, 0.02)):
        assert boundary_width(h, w, r) == max(1, int(round(r * (h * h + w * w) ** 0.5)))
    assert boundary_width(375, 500, d=5) == 5 and boundary_width(375, 500, ratio=0.5, d=1) == 1      # a fixed d wins
    assert boundary_width(375, 500, d=0) == 12 and boundary_width(375, 500, d=None) == 12          # 0 / None: the ratio


@pytest.mark.parametrize("shape", [(1, 9), (7, 9), (16, 12)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_no_interior_gives_the_region_counts(shape):
    H, W = shape
    gt, preds = _maps(H + W, H, W)
    for d in (max(H, W), max(H, W) + 3):
        assert np.array_equal(B.row(gt, preds, d, NC), R.ref_row(gt, preds, [0] * len(preds), NC))


def test_a_map_equal_to_the_ground_truth():
    gt, preds = _maps(5, 24, 31)
    for d in (1, 2, 4):
        cnt = B.row(gt, preds, d, NC)[2:].reshape(len(preds), NC, 4)
        assert np.array_equal(cnt[-1, :, 0], cnt[-1, :, 1]) and np.array_equal(cnt[-1, :, 0], cnt[-1, :, 2]) and cnt[-1, :, 0].sum() > 0
        assert np.array_equal(cnt[-1, :, 3], cnt[-1, :, 0])              # gt's band pixels are class pixels: A adds nothing
        assert (cnt[:-1, :, 0] <= np.minimum(cnt[:-1, :, 1], cnt[:-1, :, 2])).all()


def _records(seed, names, d=None):
    from cosa_amd.utils import evaluation as ev
    recs = []
    for k, name in enumerate(names):
        H, W = 20 + k, 30 - k
        gt, preds = _maps(seed + k, H, W)
        w = ev.boundary_width(H, W, d=d)
        recs.append(ev.score_record(name, H, W, [1, 3], B.row(gt, preds, w, NC), w))
    return recs


def test_score_file_round_trip_and_tools(tmp_path, capsys):
    from cosa_amd.utils import evaluation as ev
    T = _tool()
    names = [f"img_{k}" for k in range(5)]
    settings = {"maps": ["a", "b", "gt"], "pseudo": [0, 1, 0], "num_classes": NC, "epoch": 3, "s_or_t": "t", "world_size": 1, "checkpoint": None,
                "boundary": {"ratio": 0.02, "d": 2}}
    recs = _records(0, names, d=2)
    path = tmp_path / "boundary_scores_t.jsonl"
    ev.write_score_file(path, settings, recs)
    got_settings, got = ev.read_score_file(path)
    assert got_settings["boundary"] == {"ratio": 0.02, "d": 2} and got_settings["maps"] == settings["maps"]
    assert len(got) == len(recs)
    for a, b in zip(recs, got):
        assert a["name"] == b["name"] and a["d"] == b["d"] == 2 and np.array_equal(a["row"], b["row"]) and a["present"] == b["present"]
    ev.write_score_file(tmp_path / "again.jsonl", got_settings, got)
    assert open(path, "rb").read() == open(tmp_path / "again.jsonl", "rb").read()
    # a record without a width writes the line it always wrote
    plain = [ev.score_record(r["name"], r["h"], r["w"], r["present"], r["row"]) for r in recs]
    ev.write_score_file(tmp_path / "plain.jsonl", {k: v for k, v in settings.items() if k != "boundary"}, plain)
    assert all("d" not in json.loads(ln) and "boundary" not in json.loads(ln) for ln in open(tmp_path / "plain.jsonl"))
    # the tools read the file as it is
    s = T.summary(str(path))
    want = ev.dataset_scores(np.stack([r["row"] for r in recs]), NC)
    for m, name in enumerate(settings["maps"]):
        assert np.array_equal(np.array([np.nan if v is None else v for v in s["maps"][name]["iou"]]), want[m]["iou"], equal_nan=True)
        assert s["maps"][name]["miou"] == want[m]["miou"]
    assert s["maps"]["gt"]["miou"] == 1.0 and s["boundary"] == {"ratio": 0.02, "d": 2, "d_min": 2, "d_max": 2}
    assert "boundary" not in T.summary(str(tmp_path / "plain.jsonl"))
    T.main(["summary", str(path)])
    assert "Boundary IoU: band of d = 2 pixels" in capsys.readouterr().out
    res = T.main(["compare", str(path), str(path), "--map", "a", "--resamples", "100", "--json"])
    capsys.readouterr()
    assert res["images"] == 5 and res["diff"] == 0.0 and res["ci95"] == [0.0, 0.0] and all(not d["delta"] for d in res["deltas"])
    res = T.main(["worst", str(path), "--map", "b", "-n", "2"])
    assert len(res["worst"]) == 2


def test_flags_and_refusals():
    from cosa_amd import args as cosa_args, main as launcher
    from cosa_amd.utils import evaluation as ev
    a, changed = cosa_args.parse(["exp"])
    assert (a.boundary_scores, a.boundary_ratio, a.boundary_d) == (False, 0.02, 0) and not changed
    launcher.check_supported(a)
    a, changed = cosa_args.parse(["exp", "--boundary_scores", "true", "--boundary_ratio", "0.01", "--boundary_d", "64"])
    assert (a.boundary_scores, a.boundary_ratio, a.boundary_d) == (True, 0.01, 64) and set(changed) == {"boundary_scores", "boundary_ratio", "boundary_d"}
    launcher.check_supported(a)
    for extra in (["--boundary_ratio", "0"], ["--boundary_ratio", "1"], ["--boundary_ratio", "-0.5"], ["--boundary_ratio", "1.5"],
                  ["--boundary_d", "65"], ["--boundary_d", "-1"]):
        bad, _ = cosa_args.parse(["exp"] + extra)
        with pytest.raises(ValueError):
            launcher.check_supported(bad)
    assert ev.check_boundary_settings(0.02, 0) == (0.02, None) and ev.check_boundary_settings(0.5, 7) == (0.5, 7)


def test_predict_flags(capsys):
    from cosa_amd import predict
    base = ["run", "--checkpoint", "x", "--out", "x"]
    a, _ = predict.parse(base + ["--boundary"])
    assert a.boundary and not a.scores and (a.boundary_ratio, a.boundary_d) == (0.02, 0)
    a, _ = predict.parse(base + ["--boundary", "--boundary_d", "5", "--scores", "--what", "seg,pseudo"])
    assert a.boundary and a.scores and a.boundary_d == 5
    assert not predict.parse(base)[0].boundary
    for extra in (["--split", "test", "--boundary"], ["--images", str(ROOT), "--boundary"], ["--boundary", "--boundary_d", "65"],
                  ["--boundary", "--boundary_ratio", "1"], ["--boundary", "--what", "rawcam"]):
        with pytest.raises(SystemExit) as e:
            predict.parse(base + extra)
        assert e.value.code == 2
    capsys.readouterr()


def test_the_table_has_no_cpu_path():
    from cosa_amd.utils import evaluation as ev
    with pytest.raises(RuntimeError):
        ev.BoundaryScores(NC, ["a"], [0], 1, "cpu")
    with pytest.raises(ValueError):
        ev.BoundaryScores(NC, ["a"], [0], 1, "cpu", d=65)
    assert issubclass(ev.BoundaryScores, ev.ImageScores)
