"""--gt_stats without a GPU: the source tables against this machine's Pillow, the draws with and without a gt_dir,
the counter layout, the summary, the torch partner against the numpy yardstick (tests/gt_stats_ref.py), the flags and a host trainer."""
import json
import random

import numpy as np
import pytest
import torch
from PIL import Image

import gt_stats_ref as R
import test_student_check_cpu as SC


def _t(d):
    return {k: torch.from_numpy(v) for k, v in d.items()}


def test_tables_equal_the_pillow_pipeline_bit_for_bit():
    from cosa_amd.dataloaders.augment import draw_params, label_tables
    random.seed(5)
    np.random.seed(5)
    rng = np.random.default_rng(5)
    sizes = ((375, 500), (500, 333), (112, 150), (60, 97))
    maps = {hw: R.random_map(rng, *hw) for hw in sizes}
    assert all(set(np.unique(m)) <= set(range(21)) | {255} and (m == 255).any() for m in maps.values())
    seen = dict(up=0, down=0, flip=0, noflip=0, pad_top=0, pad_bottom=0, pad_left=0, pad_right=0, smaller=0, draws=0)
    for S in (64, 448):
        for i in range(30):
            for h, w in sizes:
                p = draw_params(h, w, crop_size=S)
                src_y, src_x = label_tables(p, S)
                assert src_y.dtype == src_x.dtype == np.int32 and src_y.shape == src_x.shape == (S,)
                assert src_y.max() < h and src_x.max() < w and src_y.min() >= -1 and src_x.min() >= -1
                want = R.pillow_crop(maps[h, w], p, S)
                got = R.gather(maps[h, w], src_y, src_x)
                assert np.array_equal(got, want), (S, h, w, p)
                b0, b1, b2, b3 = (int(v) for v in p["img_box"])                          # -1 exactly outside img_box
                assert np.array_equal(src_y >= 0, (np.arange(S) >= b0) & (np.arange(S) < b1))
                assert np.array_equal(src_x >= 0, (np.arange(S) >= b2) & (np.arange(S) < b3))
                seen["draws"] += 1
                seen["up"] += p["new_h"] > h
                seen["down"] += p["new_h"] < h
                seen["flip" if p["flip"] else "noflip"] += 1
                seen["pad_top"] += b0 > 0
                seen["pad_bottom"] += b1 < S
                seen["pad_left"] += b2 > 0
                seen["pad_right"] += b3 < S
                seen["smaller"] += p["new_h"] < S and p["new_w"] < S
    assert seen["draws"] >= 200 and all(v > 0 for v in seen.values()), seen


def _tree_with_gt(make_voc_tree, tmp_path, n=4):
    root, lists, names, labels = make_voc_tree(tmp_path, n=n)
    gt_dir = tmp_path / "gt"
    gt_dir.mkdir()
    rng = np.random.default_rng(3)
    for name in names:
        w, h = Image.open(f"{root}/JPEGImages/{name}.jpg").size
        Image.fromarray(R.random_map(rng, h, w)).save(gt_dir / (name + ".png"))
    return root, lists, names, str(gt_dir)


def test_draws_and_generator_states_do_not_depend_on_gt_dir(make_voc_tree, tmp_path):
    from cosa_amd.dataloaders.train_loader import VOC12ClsDatasetNew
    root, lists, names, gt_dir = _tree_with_gt(make_voc_tree, tmp_path)
    runs = []
    for gd in (None, gt_dir):
        ds = VOC12ClsDatasetNew(root, name_list_dir=lists, crop_size=64, gt_dir=gd)
        random.seed(11)
        np.random.seed(11)
        items = [ds[i] for i in range(len(ds))]
        runs.append((items, random.getstate(), np.random.get_state()))
    (plain, py_a, np_a), (with_gt, py_b, np_b) = runs
    assert py_a == py_b and all(np.array_equal(x, y) for x, y in zip(np_a, np_b))
    for a, b in zip(plain, with_gt):
        assert len(a) == 4 and len(b) == 5 and a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3])
        assert a[2].keys() == b[2].keys() and all(np.array_equal(a[2][k], b[2][k]) for k in a[2])
        gt, src_y, src_x = b[4]
        assert gt.dtype == np.uint8 and gt.shape == a[1].shape[:2]
        assert np.array_equal(R.gather(gt, src_y, src_x), R.pillow_crop(gt, b[2], 64))
    # a missing map and a map of another size are errors that name the file
    ds = VOC12ClsDatasetNew(root, name_list_dir=lists, crop_size=64, gt_dir=gt_dir)
    path = f"{gt_dir}/{names[1]}.png"
    Image.fromarray(np.zeros((7, 9), np.uint8)).save(path)
    with pytest.raises(ValueError, match=names[1]):
        ds[1]
    import os
    os.remove(path)
    with pytest.raises(FileNotFoundError, match=names[1]):
        ds[1]


def test_collate_and_dataset_builder(make_voc_tree, tmp_path):
    from types import SimpleNamespace
    from cosa_amd.dataloaders import train_loader
    root, lists, names, gt_dir = _tree_with_gt(make_voc_tree, tmp_path)
    base = dict(dataset="VOC12", voc12_root=root, coco_root="/c", name_list_dir=lists, scales=(0.5, 2), crop_size=64, ignore_index=255, num_classes=21)
    assert train_loader.build_train_datasetv2(SimpleNamespace(**base)).gt_dir is None
    assert train_loader.build_train_datasetv2(SimpleNamespace(**base, gt_stats=False, gt_dir=gt_dir)).gt_dir is None
    assert train_loader.build_train_datasetv2(SimpleNamespace(**base, gt_stats=True, gt_dir=None)).gt_dir == f"{root}/SegmentationClassAug"
    assert train_loader.train_gt_dir(SimpleNamespace(**dict(base, dataset="COCO"), gt_stats=True)) == "/c/SegmentationClass/train2014"
    ds = train_loader.build_train_datasetv2(SimpleNamespace(**base, gt_stats=True, gt_dir=gt_dir))
    assert ds.gt_dir == gt_dir
    out = train_loader._collate([ds[0], ds[1]])
    assert len(out) == 5 and len(out[4]) == 2 and out[4][0][0].dtype == np.uint8
    ds.gt_dir = None
    assert len(train_loader._collate([ds[0], ds[1]])) == 4


def test_layout_offsets_and_size():
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    for K in (2, 21, 81, 128):
        off, n = seg_helper.gt_stats_layout(K)
        want, want_n = R.layout(K)
        assert off == want and n == want_n == 4 + 2 * K * (K + 1) + K * K and list(off) == list(seg_helper.GT_STATS_SLOTS)
        assert (off["steps"], off["pix"], off["valid"], off["gt_other"], off["main"]) == (0, 1, 2, 3, 4)
        assert off["aux"] == 4 + K * (K + 1) and off["student"] == 4 + 2 * K * (K + 1)
        assert seg_helper.new_gt_stats(K, "cpu").shape == (n,)
    for bad in (1, 129, 0, -3):
        with pytest.raises(ValueError):
            seg_helper.gt_stats_layout(bad)
        assert _C.lib().cosa_gt_stats_uses_lds(bad) == -1
    assert _C.lib().cosa_gt_stats_uses_lds(21) == 1 and _C.lib().cosa_gt_stats_uses_lds(2) == 1      # VOC's K counts in LDS
    assert _C.lib().cosa_gt_stats_uses_lds(81) == 0 and _C.lib().cosa_gt_stats_uses_lds(128) == 0


def test_summary_on_hand_made_counters():
    from cosa_amd.utils import seg_helper
    K = 3
    off, n = R.layout(K)
    c = np.zeros(n, np.int64)
    c[off["steps"]], c[off["pix"]], c[off["valid"]], c[off["gt_other"]] = 4, 200, 100, 3
    main = np.array([[30, 10, 0, 10],        # gt 0: 30 right, 10 called class 1, 10 ignored
                     [5, 25, 0, 20],         # gt 1
                     [0, 0, 0, 0]])          # gt 2: never seen, never labelled -> empty union
    aux = np.array([[20, 0, 0, 30], [0, 10, 0, 40], [0, 0, 0, 0]])
    student = np.array([[40, 10, 0], [20, 30, 0], [0, 0, 0]])
    c[off["main"]:off["aux"]], c[off["aux"]:off["student"]], c[off["student"]:] = main.reshape(-1), aux.reshape(-1), student.reshape(-1)
    for counters in (c, c.tolist(), torch.from_numpy(c)):
        s = seg_helper.gt_stats_summary(counters, K)
        assert (s["steps"], s["pix"], s["valid_frac"], s["gt_other"]) == (4, 200, 0.5, 3)
        assert s["main"]["labelled"] == 0.7 and s["aux"]["labelled"] == 0.3
        assert s["main"]["iou"] == [30 / 45, 25 / 40, None] and s["main"]["miou"] == (30 / 45 + 25 / 40) / 2
        assert s["main"]["iou_strict"] == [30 / 55, 25 / 60, None] and s["main"]["miou_strict"] == (30 / 55 + 25 / 60) / 2
        assert s["aux"]["iou"] == [1.0, 1.0, None] and s["aux"]["iou_strict"] == [20 / 50, 10 / 50, None]
        assert s["student"]["iou"] == [40 / 70, 30 / 60, None] and s["student"]["miou"] == (40 / 70 + 30 / 60) / 2
        json.dumps(s)
    z = seg_helper.gt_stats_summary(np.zeros(n, np.int64), K)
    assert z["steps"] == z["pix"] == z["gt_other"] == 0 and z["valid_frac"] == 0.0
    assert z["main"]["miou"] == z["main"]["miou_strict"] == z["main"]["labelled"] == z["aux"]["miou"] == z["student"]["miou"] == 0.0
    assert z["main"]["iou"] == z["student"]["iou"] == [None] * K
    json.dumps(z)
    with pytest.raises(ValueError):
        seg_helper.gt_stats_summary(np.zeros(n + 1, np.int64), K)


# h / S is a power of two in both: on integer logits every bilinear weight and product is exact, in F.interpolate as in spec R, so the
# ties are ties in both and only the first-maximum rule decides
CASES = {"K6int": dict(B=2, K=6, S=64, h=4, seed=31, box_kinds=("full", "interior"), label_kinds=("some", "all"), integer_logits=True,
                       gt_kinds=("mixed", "mixed")),
         "K21": dict(B=3, K=21, S=96, h=6, seed=32, box_kinds=("interior", "empty", "row"), label_kinds=("some", "some", "none"), margin=1e-4,
                     gt_kinds=("mixed", "mixed", "all255"))}


@pytest.mark.parametrize("case", list(CASES))
def test_torch_partner_equals_the_numpy_reference(case, oracle_c):
    import label_stats_ref as LR
    from cosa_amd.utils import seg_helper
    d = R.draw(oracle_c, **CASES[case])
    K, S = CASES[case]["K"], CASES[case]["S"]
    off, n = R.layout(K)
    if CASES[case].get("integer_logits"):
        assert LR.top_two_margin(LR.resized_logits(oracle_c, d["seg"], d["cls"], S)) == 0.0          # the ties are there
    want = R.reference(oracle_c, d["gt"], d["mask_main"], d["mask_aux"], d["seg"], d["cls"], d["boxes"])
    assert want[off["valid"]] > 0 and want[off["pix"]] > want[off["valid"]] and want[off["gt_other"]] > 0
    assert want[off["main"]:off["aux"]].reshape(K, K + 1)[:, K].sum() > 0 and want[off["student"]:].sum() == want[off["valid"]]
    t = _t(d)
    counters = seg_helper.new_gt_stats(K, "cpu")
    seg_helper.gt_stats_torch(t["gt"], t["mask_main"], t["mask_aux"], t["seg"], t["cls"], t["boxes"], counters)
    assert np.array_equal(counters.numpy(), want), np.nonzero(counters.numpy() != want)[0]
    # a second call accumulates; without the auxiliary map its block stays as it is; a mask value that is no label is in valid only
    mm = d["mask_main"].copy()
    y, x = np.argwhere(LR.inside_boxes(d["boxes"], S)[0] & (d["gt"][0] < K))[0]
    mm[0, y, x] = 1.5
    want2 = R.reference(oracle_c, d["gt"], mm, None, d["seg"], d["cls"], d["boxes"])
    assert want2[off["main"]:off["aux"]].sum() == want2[off["valid"]] - 1 and not want2[off["aux"]:off["student"]].any()
    seg_helper.gt_stats_torch(t["gt"], torch.from_numpy(mm), None, t["seg"], t["cls"], t["boxes"], counters)
    assert np.array_equal(counters.numpy(), want + want2) and counters[off["steps"]] == 2


def test_flags_parse_default_off_and_the_launcher_refuses_a_run_without_maps():
    from cosa_amd import args as cosa_args
    from cosa_amd import main as launcher
    from cosa_amd.train_step import default_args
    a, changed = cosa_args.parse(["EXP"])
    assert a.gt_stats is False and a.gt_dir is None and "gt_stats" not in changed and "gt_dir" not in changed
    launcher.check_supported(a)
    a, changed = cosa_args.parse(["EXP", "--gt_stats", "true"])
    assert a.gt_stats is True and changed["gt_stats"] is True
    assert default_args("VOC12").gt_stats is False
    assert default_args("VOC12", **{k: v for k, v in vars(a).items() if k != "dataset"}).gt_stats is True
    with pytest.raises(ValueError, match="gt_dir"):
        launcher.check_supported(a)                                                   # neither a dataset root nor --gt_dir
    launcher.check_supported(cosa_args.parse(["EXP", "--gt_stats", "true", "--gt_dir", "/maps"])[0])
    launcher.check_supported(cosa_args.parse(["EXP", "--gt_stats", "true", "--voc12_root", "/voc"])[0])
    with pytest.raises(ValueError, match="gt_dir"):
        launcher.check_supported(cosa_args.parse(["EXP", "--gt_stats", "true", "--dataset", "COCO", "--voc12_root", "/voc"])[0])


def test_host_trainer_counts_registers_its_state_and_needs_gt(tmp_path, monkeypatch, capsys, oracle_c):
    from cosa_amd import monitors
    d = R.draw(oracle_c, **dict(CASES["K6int"], B=3, box_kinds=("full", "interior", "row"), label_kinds=("some", "all", "none"),
                                gt_kinds=("mixed",) * 3))
    want = R.reference(oracle_c, d["gt"], d["mask_main"], d["mask_aux"], d["seg"], d["cls"], d["boxes"])
    off_tr = SC._host_trainer(monkeypatch, seed=1)
    assert off_tr.gt_stats_state is None and off_tr.gt_stats() is None and not hasattr(off_tr, "extra_state")
    assert [m.name for m, _ in monitors.active(off_tr)] == []
    a = SC._host_trainer(monkeypatch, seed=1, gt_stats=True)
    assert a.extra_state["gt_stats.counters"] is a.gt_stats_state and int(a.gt_stats_state.abs().sum()) == 0
    assert [m.name for m, _ in monitors.active(a)] == ["gt_stats"] and monitors.BY_NAME["gt_stats"].state_name in a.train_state().names
    t = _t(d)
    for k in range(2):
        a.update_gt_stats(t["gt"], t["mask_main"], t["mask_aux"], t["seg"], t["cls"], t["boxes"])
    assert a.gt_stats()["steps"] == 2 and np.array_equal(a.gt_stats_state.numpy(), 2 * want)
    z = torch.zeros(3, 3, 48, 48)
    with pytest.raises(ValueError, match="gt"):                                          # the flag on and no ground truth: before anything runs
        a.step(z, z, torch.zeros(3, 5), torch.zeros(3, 4, dtype=torch.int16), 0)
    # the state file: carried, and reconciled with a note in both directions
    with_gt, without = str(tmp_path / "state_00000003.cosa"), str(tmp_path / "state_00000000.cosa")
    a.save_state(with_gt, n_iter=2)
    a.wait_state()
    off_tr.save_state(without, n_iter=-1)
    off_tr.wait_state()
    b = SC._host_trainer(monkeypatch, seed=9, gt_stats=True)
    capsys.readouterr()
    assert b.load_state(with_gt)["n_iter"] == 2 and "note:" not in capsys.readouterr().out
    assert np.array_equal(b.gt_stats_state.numpy(), 2 * want)
    notes = monitors.BY_NAME["gt_stats"].notes
    b.load_state(without)
    assert notes[1] in capsys.readouterr().out and int(b.gt_stats_state.abs().sum()) == 0
    c = SC._host_trainer(monkeypatch, seed=5)
    c.load_state(with_gt)
    assert notes[0] in capsys.readouterr().out and c.gt_stats_state is None
    for p, q in zip(a.student.parameters(), c.student.parameters()):
        assert torch.equal(p, q)


def test_launcher_line_record_and_interval_read(tmp_path):
    from types import SimpleNamespace
    from cosa_amd import main as launcher
    from cosa_amd import monitors
    from cosa_amd.utils import seg_helper
    K = 3
    m = monitors.BY_NAME["gt_stats"]
    assert monitors.MONITORS[5] is m and m.state_name == "aux.gt_stats.counters"
    off, n = R.layout(K)
    c = torch.zeros(n, dtype=torch.int64)
    c[off["steps"]], c[off["pix"]], c[off["valid"]] = 2, 50, 40
    c[off["main"]:off["main"] + K + 1] = torch.tensor([20, 0, 0, 20])                    # gt 0: half labelled, all of it right
    c[off["student"]:off["student"] + K] = torch.tensor([10, 30, 0])
    acc = torch.arange(8, dtype=torch.float64) * 2
    vals, host = launcher.read_interval(acc, 2, [(m, c)])
    assert vals == [float(i) for i in range(8)] and host["gt_stats"][off["valid"]] == 40 and not c.any()      # an interval's: zeroed
    s = m.summary(None, SimpleNamespace(num_classes=K), host["gt_stats"])
    assert m.gate(s) and m.line(s, None) == " gt: main 1.000 (lab 0.500), aux -, student 0.125"
    monitors.append_monitor(tmp_path, m, s, 2, None)
    rec = json.loads(open(tmp_path / "gt_stats.jsonl").read())
    assert rec["iters"] == 2 and rec["main"]["miou"] == 1.0 and rec["main"]["miou_strict"] == 0.5 and rec["student"]["iou"] == [0.25, 0.0, None]
    s["aux"]["pixels"], s["aux"]["miou"] = 5, 0.125
    assert " aux 0.125," in m.line(s, None)
