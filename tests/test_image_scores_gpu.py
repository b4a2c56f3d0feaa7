"""Per-image evaluation scores on the device: cosa_image_scores against the numpy restatement of its row, word for
word; the rows against ConfusionMeter; evaluate(image_scores=...) and export_predictions(scores=True) end to end."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import image_scores_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5
EINVAL = 1


def _tool():
    spec = importlib.util.spec_from_file_location("image_scores_tool", os.path.join(ROOT, "tools", "image_scores.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _maps(rng, n, nc, n_maps):
    """gt with 255 runs, predictions in runs (label maps are made of runs) with noise, stray values in [nc, 254] and 255s"""
    run = max(1, n // 7)
    gt = np.repeat(rng.integers(0, nc, n // run + 1), run)[:n].astype(np.uint8)
    gt[rng.random(n) < 0.08] = 255
    if nc < 255:
        gt[rng.random(n) < 0.02] = nc                                  # a truth that is neither a class nor 255 is no class either
    preds = []
    for _ in range(n_maps):
        p = np.where(rng.random(n) < 0.7, gt, rng.integers(0, nc, n)).astype(np.uint8)
        p[p >= nc] = rng.integers(0, nc)
        if nc < 255:
            stray = rng.random(n) < 0.05
            p[stray] = rng.integers(nc, 255, int(stray.sum()))         # [nc, 254]
        p[rng.random(n) < 0.1] = 255
        preds.append(p)
    return gt, preds


def _place(arrays, offsets):
    """each array into its own device buffer at the given byte offset from a 16-byte boundary -> (views, owners)"""
    views = []
    for a, off in zip(arrays, offsets):
        buf = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + a.size]
        v.copy_(torch.from_numpy(a))
        views.append(v)
    return views


def _call(gt, preds, pseudo, nc, table, word, n=None, n_maps=None, null_map=None, row_ptr=None):
    from cosa_amd import _C
    k = len(preds) if n_maps is None else n_maps
    ptrs = (ctypes.c_void_p * max(len(preds), 1))(*[None if i == null_map else p.data_ptr() for i, p in enumerate(preds)])
    row = ctypes.c_void_p(table.data_ptr() + 8 * word if row_ptr is None else row_ptr)
    return _C.lib().cosa_image_scores(_C.ptr(gt), ptrs, _C.int_array(pseudo), k, gt.numel() if n is None else n, nc, row, _C.stream_ptr())


def _table(words):
    return torch.full((words + 8,), SENTINEL, dtype=torch.int64, device="cuda")


def _check(table, words, want):
    got = table.cpu().numpy()
    assert (got[:4] == SENTINEL).all() and (got[4 + words:] == SENTINEL).all()        # the words around the row survive
    bad = np.nonzero(got[4:4 + words] != want)[0]
    assert bad.size == 0, (bad[:8], got[4:4 + words][bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 37 * 53, 375 * 500])
def test_kernel_equals_the_restatement_word_for_word(n):
    from cosa_amd import _C
    rng = np.random.default_rng(n)
    for nc in (2, 21, 81, 255):
        for n_maps in (1, 3, 8):
            if n == 375 * 500 and (nc, n_maps) not in ((21, 8), (255, 3), (2, 1), (81, 8)):
                continue                                               # the large map: the corners of the table
            gt, preds = _maps(rng, n, nc, n_maps)
            pseudo = [(m + nc) % 2 for m in range(n_maps)]               # mixed flags
            offs = [int(o) for o in rng.integers(0, 4, n_maps + 1)]
            offs[0] = (nc + n_maps) % 4                                  # gt at 0..3 bytes off, the maps at their own 0..3
            if n_maps >= 3:
                offs[1:4] = [1, 2, 3]
            dev = _place([gt] + preds, offs)
            words = _C.lib().cosa_image_scores_words(nc, n_maps)
            assert words == 2 + n_maps * nc * 4
            table = _table(words)
            table[4:4 + words] = 0
            assert _call(dev[0], dev[1:], pseudo, nc, table, 4) == 0
            want = R.ref_row(gt, preds, pseudo, nc)
            _check(table, words, want)
            if n_maps == 3:                                              # a second call into the same row accumulates
                assert _call(dev[0], dev[1:], pseudo, nc, table, 4) == 0
                _check(table, words, 2 * want)


def test_ground_truth_entirely_ignored():
    rng = np.random.default_rng(0)
    n, nc = 1000, 21
    gt = np.full(n, 255, np.uint8)
    preds = [rng.integers(0, nc, n).astype(np.uint8), np.full(n, 255, np.uint8)]
    dev = _place([gt] + preds, [3, 0, 5])
    table = _table(2 + 2 * nc * 4)
    table[4:-4] = 0
    assert _call(dev[0], dev[1:], [0, 1], nc, table, 4) == 0
    want = R.ref_row(gt, preds, [0, 1], nc)
    assert want[1] == 0 and want[2:].reshape(2, nc, 4)[..., :3].sum() == 0 and want[2:].reshape(2, nc, 4)[0, :, 3].sum() == n
    _check(table, 2 + 2 * nc * 4, want)


def test_refused_arguments_leave_the_row_untouched():
    from cosa_amd import _C
    L = _C.lib()
    gt, p = _place([np.zeros(100, np.uint8), np.ones(100, np.uint8)], [0, 0])
    table = _table(2 + 9 * 21 * 4)
    before = table.clone()
    ok = dict(gt=gt, preds=[p], pseudo=[0], nc=21)
    bad = [dict(ok, nc=0), dict(ok, nc=256), dict(ok, nc=-3), dict(ok, preds=[p] * 9, pseudo=[0] * 9), dict(ok, n_maps=0), dict(ok, n=0),
           dict(ok, null_map=0), dict(ok, preds=[p, p], pseudo=[0, 0], null_map=1), dict(ok, row_ptr=0), dict(ok, row_ptr=table.data_ptr() + 4)]
    for kw in bad:
        assert _call(kw.pop("gt"), kw.pop("preds"), kw.pop("pseudo"), kw.pop("nc"), table, 4, **kw) == EINVAL, kw
        assert L.cosa_last_error()
    assert L.cosa_image_scores(None, (ctypes.c_void_p * 1)(p.data_ptr()), _C.int_array([0]), 1, 100, 21, _C.ptr(table), _C.stream_ptr()) == EINVAL
    assert L.cosa_image_scores(_C.ptr(gt), None, _C.int_array([0]), 1, 100, 21, _C.ptr(table), _C.stream_ptr()) == EINVAL
    assert L.cosa_image_scores(_C.ptr(gt), (ctypes.c_void_p * 1)(p.data_ptr()), None, 1, 100, 21, _C.ptr(table), _C.stream_ptr()) == EINVAL
    for nc, k in ((0, 1), (256, 1), (21, 0), (21, 9)):
        assert L.cosa_image_scores_words(nc, k) == 0
    assert torch.equal(table, before)
    assert _call(gt, [p], [0], 21, table, 4) == 0                            # and the accepted call still runs after them


@pytest.mark.parametrize("nc", [5, 21, 81])
def test_summed_rows_are_the_confusion_matrix_margins(nc):
    from cosa_amd.utils import evaluation as ev
    rng = np.random.default_rng(nc)
    names = [f"m{i}" for i in range(11)]                                     # 11 maps: two launches per image (8 + 3)
    flags = [i % 3 == 0 for i in range(11)]
    meters = [ev.ConfusionMeter(nc, "cuda", pseudo=f) for f in flags]
    table = ev.ImageScores(nc, names, flags, 2, "cuda")                      # capacity 2: the third image makes it grow
    want = []
    for i, n in enumerate((37 * 53, 4099, 640)):
        gt, preds = _maps(rng, n, nc, 11)
        g = torch.from_numpy(gt).cuda()
        ps = [torch.from_numpy(p).cuda() for p in preds]
        for m, p in zip(meters, ps):
            m.update(g, p)
        table.add(i, g, ps)
        want.append(R.ref_row(gt, preds, flags, nc))
    rows = table.rows(3)
    assert rows.shape == (3, ev.row_words(nc, 11)) and np.array_equal(rows, np.stack(want))
    cnt = rows[:, 2:].sum(axis=0).reshape(11, nc, 4)
    for m, meter in enumerate(meters):
        hist = meter.hist.cpu().numpy()
        assert np.array_equal(cnt[m, :, 0], np.diag(hist)) and np.array_equal(cnt[m, :, 1], hist.sum(axis=0))
        assert np.array_equal(cnt[m, :, 2], hist.sum(axis=1))
    got = ev.dataset_scores(rows, nc)
    assert all(got[m]["miou"] == meters[m].scores()["miou"] for m in range(11))
    with pytest.raises(ValueError):
        table.add(0, g, ps[:3])
    with pytest.raises(ValueError):
        table.add(0, g, [p.float() for p in ps])


def _model_and_loader(C=4, S=64, n=6, seed=0):
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    torch.manual_seed(seed)
    args = default_args("VOC12", crop_size=S, batch_size=1)
    args.num_classes, args.bkg_thre = C + 1, 0.5
    model = build_model(args).cuda().eval()
    rng = np.random.default_rng(3)
    loader = []
    for k, (H, W) in enumerate([(50, 70), (64, 64), (81, 47), (33, 90), (64, 64), (70, 50)][:n]):
        img = torch.from_numpy(rng.standard_normal((1, 3, H, W)).astype(np.float32))
        lab = torch.from_numpy(rng.integers(0, C + 1, (1, H, W)).astype(np.int64))
        lab[0, :3] = 255
        cls = torch.zeros(1, C)
        cls[0, rng.choice(C, 2, replace=False)] = 1
        loader.append((f"img_{k:02d}", img, lab, cls))
    return args, model, loader


def test_evaluate_writes_per_image_scores(tmp_path):
    from cosa_amd import evaluation_engine as ee
    T = _tool()
    args, model, loader = _model_and_loader()
    args.output_dir = tmp_path / "run"
    kw = dict(epoch=7, s_or_t='t', get_camiou=True, getcrf=True, threshold_filters=[0.3])
    off = ee.evaluate(model, loader, args, **kw)
    assert not (tmp_path / "run").exists()                                   # the default adds nothing: no table, no launch, no file
    on = ee.evaluate(model, loader, args, image_scores=True, **kw)
    assert on[0] == off[0] and on[1] == off[1] and on[2] == off[2] and on[3] == off[3] and on[4] == off[4]
    d = tmp_path / "run" / "00007"
    assert sorted(os.listdir(d)) == ["image_scores_t.jsonl", "iou_dic_t.pth"]
    lines = [json.loads(ln) for ln in open(d / "image_scores_t.jsonl")]
    maps = ["cam", "cam_aux", "seg_ps", "seg_vd", "seg_crf", "cam_0.3", "camaux_0.3"]
    assert lines[0]["maps"] == maps and lines[0]["pseudo"] == [0, 0, 0, 0, 0, 1, 1] and lines[0]["epoch"] == 7 and lines[0]["s_or_t"] == "t"
    assert [ln["name"] for ln in lines[1:]] == [n for n, *_ in loader]
    for ln, (_, img, lab, cls) in zip(lines[1:], loader):
        assert (ln["h"], ln["w"]) == tuple(lab.shape[1:]) and ln["n"] == lab[0].numel() and ln["n_valid"] == int((lab != 255).sum())
        assert ln["present"] == (np.nonzero(cls[0].numpy())[0] + 1).tolist()
    # the file alone gives the table evaluate printed
    s = T.summary(str(d / "image_scores_t.jsonl"))
    df = on[3]
    assert df["Metrics"] == ["CAM", "aux_CAM", "Seg_vd", "cam_0.3", "camaux_0.3", "Seg_crf"]
    for row, name in zip(df["Metrics"], ["cam", "cam_aux", "seg_vd", "cam_0.3", "camaux_0.3", "seg_crf"]):
        iou = np.array([np.nan if v is None else v for v in s["maps"][name]["iou"]])
        assert np.round(iou * 100, 2).mean() == df["mIoU"][df["Metrics"].index(row)], (row, iou)
    # the reference's iou_dic.pth structure: {name: {class id: (iou, gt_ratio), 'miou', 'wmiou'}} of seg_vd
    dic = torch.load(d / "iou_dic_t.pth", weights_only=True)
    assert list(dic) == [n for n, *_ in loader]
    for ln in lines[1:]:
        e = dic[ln["name"]]
        assert [k for k in e if k not in ("miou", "wmiou")] == ln["present"]
        assert all(isinstance(e[c], tuple) and len(e[c]) == 2 and 0 <= e[c][0] <= 1 and 0 <= e[c][1] <= 1 for c in ln["present"])
        assert e["miou"] == ln["maps"]["seg_vd"]["miou"] == np.mean([e[c][0] for c in ln["present"]])
    # grouping changes no byte of either file
    files = {}
    for g in (1, 4):
        ee.evaluate(model, loader, args, image_scores=tmp_path / f"g{g}", eval_group=g, **kw)
        files[g] = [open(tmp_path / f"g{g}" / f, "rb").read() for f in ("image_scores_t.jsonl", "iou_dic_t.pth")]
    assert files[1] == files[4] and files[4][0] == open(d / "image_scores_t.jsonl", "rb").read()
    with pytest.raises(NotImplementedError):
        ee.evaluate(model, loader, args, epoch=1, save_result=True, image_scores=True)


def test_export_scores_are_those_of_the_files_on_disk(tmp_path):
    from cosa_amd import evaluation_engine as ee
    args, model, loader = _model_and_loader(n=3)
    nc = args.num_classes
    what = ("seg", "pseudo", "pseudo_aux_par", "rawcam")
    plain = ee.export_predictions(model, loader, args, tmp_path / "a", what=what, getcrf=True)
    res = ee.export_predictions(model, loader, args, tmp_path / "b", what=what, getcrf=True, scores=True)
    assert "scores" not in plain and not (tmp_path / "a" / "scores.jsonl").exists()
    assert open(tmp_path / "a" / "manifest.json", "rb").read() == open(tmp_path / "b" / "manifest.json", "rb").read()
    lines = [json.loads(ln) for ln in open(tmp_path / "b" / "scores.jsonl")]
    names = ["seg", "pseudo", "pseudo_aux_par", "seg_crf"]
    assert lines[0]["maps"] == names and lines[0]["pseudo"] == [0, 1, 1, 0] and len(lines) == 4
    from cosa_amd.utils import evaluation as ev
    _, recs = ev.read_score_file(tmp_path / "b" / "scores.jsonl")
    rows = []
    for rec, (name, _, lab, _) in zip(recs, loader):
        assert rec["name"] == name
        preds = [np.asarray(Image.open(tmp_path / "b" / p / (name + ".png"))) for p in names]
        rows.append(R.ref_row(lab[0].numpy().astype(np.uint8), preds, [0, 1, 1, 0], nc))
        assert np.array_equal(rec["row"], rows[-1]), name
    want = ev.dataset_scores(np.stack(rows), nc)
    assert list(res["scores"]) == names
    for p, w in zip(names, want):
        assert res["scores"][p]["miou"] == w["miou"] and res["scores"][p]["labelled"] == w["labelled"]
    assert res["scores"]["seg"]["labelled"] == 1.0 and res["scores"]["pseudo"]["labelled"] <= 1.0
    with pytest.raises(ValueError):
        ee.export_predictions(model, loader, args, tmp_path / "c", what=("rawcam",), scores=True)


def test_predict_command_line_with_scores(tmp_path, capsys):
    """python -m cosa_amd.predict --scores on a tiny VOC-shaped tree with masks: scores.jsonl holds the counters of the PNGs against the masks"""
    from cosa_amd import predict
    from cosa_amd.main import _trainer_args
    from cosa_amd.models import build_model
    from cosa_amd.utils import evaluation as ev
    from cosa_amd.utils import torch_helper
    rng = np.random.default_rng(0)
    root, lists = tmp_path / "voc", tmp_path / "lists"
    names, sizes = ["2007_000001", "2007_000002", "2007_000003"], [(40, 60), (64, 48), (33, 35)]
    os.makedirs(root / "JPEGImages")
    os.makedirs(root / "SegmentationClassAug")
    masks = {}
    for n, (H, W) in zip(names, sizes):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(root / "JPEGImages" / (n + ".jpg"))
        masks[n] = rng.integers(0, 5, (H, W)).astype(np.uint8)
        masks[n][:2] = 255
        Image.fromarray(masks[n]).save(root / "SegmentationClassAug" / (n + ".png"))
    os.makedirs(lists)
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    onehot = {n: np.eye(4, dtype=np.float32)[k] + np.eye(4, dtype=np.float32)[3] * (k < 3) for k, n in enumerate(names)}
    np.save(lists / "cls_labels_onehot.npy", onehot, allow_pickle=True)
    common = ["--pretrained", "false", "--crop_size", "64", "--num_classes", "5", "--voc12_root", str(root), "--name_list_dir", str(lists),
              "--num_workers", "0"]
    args, _ = predict.parse(["run", "--checkpoint", "x", "--out", "x"] + common)
    torch.manual_seed(0)
    ckpt = torch_helper.save_best(tmp_path, build_model(_trainer_args(args)), 1, 0.0, args, 't', comment='seg')
    res = predict.main(["run", "--checkpoint", ckpt, "--out", str(tmp_path / "val"), "--split", "val", "--what", "seg,pseudo", "--scores"] + common)
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert res["images"] == 3 and list(printed["scores"]) == ["seg", "pseudo"] and printed["scores"] == res["scores"]
    settings, recs = ev.read_score_file(tmp_path / "val" / "scores.jsonl")
    assert settings["maps"] == ["seg", "pseudo"] and settings["pseudo"] == [0, 1] and settings["checkpoint"] == os.path.abspath(ckpt)
    for rec, n in zip(recs, names):
        preds = [np.asarray(Image.open(tmp_path / "val" / p / (n + ".png"))) for p in ("seg", "pseudo")]
        assert rec["name"] == n and rec["present"] == (np.nonzero(onehot[n])[0] + 1).tolist()
        assert np.array_equal(rec["row"], R.ref_row(masks[n], preds, [0, 1], 5))
    plain = predict.main(["run", "--checkpoint", ckpt, "--out", str(tmp_path / "plain"), "--split", "val", "--what", "seg,pseudo"] + common)
    assert "scores" not in plain and sorted(os.listdir(tmp_path / "plain")) == ["manifest.json", "pseudo", "seg"]
    assert open(tmp_path / "plain" / "manifest.json", "rb").read() == open(tmp_path / "val" / "manifest.json", "rb").read()
