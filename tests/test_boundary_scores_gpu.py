"""Boundary IoU counters on the device: cosa_boundary_scores through the C ABI against the numpy restatement of its
row (tests/boundary_scores_ref.py, the window definition pixel by pixel), word for word; against cosa_image_scores where no pixel is
interior; evaluate(boundary_scores=...) and export_predictions(boundary=True) end to end.  Every comparison is integer equality."""
import ctypes
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import boundary_scores_ref as B
import image_scores_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A5A5A5A5A5A5A5
EINVAL = 1
SHAPES = [(1, 1), (1, 40), (40, 1), (7, 9), (37, 53), (64, 64), (65, 129), (130, 70), (97, 211)]
WIDTHS = [1, 2, 3, 13, 64]
# every shape at every width; 64 is `d >= both sides` for the shapes up to 64 x 64, which also take d = max(H, W) exactly (beyond 64 the
# envelope refuses the call, so a larger shape has no such case)
CASES = [(s, d) for s in SHAPES for d in WIDTHS + ([max(s)] if max(s) < 64 and max(s) not in WIDTHS else [])]


def _tool():
    spec = importlib.util.spec_from_file_location("image_scores_tool", os.path.join(ROOT, "tools", "image_scores.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _maps(seed, H, W, nc, n_maps):
    """gt: blocks of classes (one of them wider than any band of d <= 3, one ringed by a pixel of 255 as in VOC), a 255 region, values in
    [nc, 255).  Maps: the gt shifted by a pixel or two with blocks of their own, then by turns one label only, a checkerboard (every
    pixel is band), a map with 255 regions and stray values, the gt itself."""
    rng = np.random.default_rng(seed)
    vals = list(range(min(nc, 6))) + [nc - 1]
    gt = B.run_map(rng, H, W, vals)
    if H >= 12 and W >= 12:
        gt[2:H // 2, 3:W // 2] = vals[1]                               # an object ...
        gt[1, 2:W // 2 + 1] = gt[H // 2, 2:W // 2 + 1] = 255           # ... in its one-pixel ring of 255
        gt[1:H // 2 + 1, 2] = gt[1:H // 2 + 1, W // 2] = 255
    if H * W > 1:
        gt[H - 1 - H // 8:, : W // 3 + 1] = 255
    if nc < 255 and H * W > 1:
        gt[: H // 5 + 1, W - 1 - W // 6:] = nc + (seed % (255 - nc))     # neither a class nor 255: no class either
    preds = []
    for m in range(n_maps):
        kind = m % 5
        if kind == 0:
            p = np.roll(np.roll(gt, 1 + m % 2, axis=0), -2, axis=1).copy()
            p[p >= nc] = vals[2 % len(vals)]
        elif kind == 1:
            p = np.full((H, W), vals[1 % len(vals)], np.uint8)
        elif kind == 2:
            yy, xx = np.indices((H, W))
            p = np.where((yy + xx) % 2 == 0, vals[0], vals[-1]).astype(np.uint8)
        elif kind == 3:
            p = B.run_map(rng, H, W, vals + [255, 255] + ([nc, 254] if nc < 255 else []))
        else:
            p = gt.copy()
        preds.append(np.ascontiguousarray(p, dtype=np.uint8))
    return gt, preds


@functools.lru_cache(maxsize=None)
def _case(H, W, d, nc, n_maps):
    """maps and their reference row, computed once and shared (read-only)"""
    gt, preds = _maps(H * 1000 + W + nc, H, W, nc, n_maps)
    want = B.row(gt, preds, d, nc)
    for a in [gt, want] + preds:
        a.setflags(write=False)
    return gt, preds, want


def _place(arrays, offsets):
    """each [H, W] array dense into its own device buffer at the given byte offset from a 16-byte boundary"""
    views = []
    for a, off in zip(arrays, offsets):
        buf = torch.zeros(a.size + 64, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        v = buf[off:off + a.size]
        v.copy_(torch.from_numpy(np.array(a)).reshape(-1))
        views.append(v)
    return views


def _call(gt, preds, H, W, d, nc, table, word=4, n_maps=None, null_map=None, row_ptr=None):
    from cosa_amd import _C
    k = len(preds) if n_maps is None else n_maps
    ptrs = (ctypes.c_void_p * max(len(preds), 1))(*[None if i == null_map else p.data_ptr() for i, p in enumerate(preds)])
    row = ctypes.c_void_p(table.data_ptr() + 8 * word if row_ptr is None else row_ptr)
    return _C.lib().cosa_boundary_scores(_C.ptr(gt), ptrs, k, H, W, d, nc, row, _C.stream_ptr())


def _table(words):
    t = torch.full((words + 8,), SENTINEL, dtype=torch.int64, device="cuda")
    t[4:4 + words] = 0
    return t


def _check(table, words, want):
    got = table.cpu().numpy()
    assert (got[:4] == SENTINEL).all() and (got[4 + words:] == SENTINEL).all()        # the words around the row survive
    bad = np.nonzero(got[4:4 + words] != want)[0]
    assert bad.size == 0, (bad[:8], got[4:4 + words][bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("shape,d", CASES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"d{v}")
def test_kernel_equals_the_window_definition(shape, d):
    """every shape at every width, 21 classes, three maps at 1, 3 and 8 bytes off a 16-byte boundary (the ground truth at 3)"""
    from cosa_amd import _C
    H, W = shape
    gt, preds, want = _case(H, W, d, 21, 3)
    dev = _place([gt] + preds, [3, 1, 3, 8])
    words = _C.lib().cosa_boundary_scores_words(21, 3)
    assert words == 2 + 3 * 21 * 4 == _C.lib().cosa_image_scores_words(21, 3)
    table = _table(words)
    assert _call(dev[0], dev[1:], H, W, d, 21, table) == 0
    _check(table, words, want)
    if d in (2, 13):                                                     # a second call into the same row accumulates
        assert _call(dev[0], dev[1:], H, W, d, 21, table) == 0
        _check(table, words, 2 * want)


@pytest.mark.parametrize("n_maps", [1, 3, 8])
@pytest.mark.parametrize("nc", [2, 21, 81, 255])
def test_classes_and_maps(nc, n_maps):
    """the counter table's corners: on a map across tile edges at d = 3 and at d = 64, and below a tile at d = 2"""
    from cosa_amd import _C
    for H, W, d in ((65, 129, 3), (37, 53, 2), (65, 129, 64)):
        gt, preds, want = _case(H, W, d, nc, n_maps)
        dev = _place([gt] + preds, [(nc + n_maps) % 16] + [(1, 3, 8, 0, 5, 15, 2, 9)[m] for m in range(n_maps)])
        words = _C.lib().cosa_boundary_scores_words(nc, n_maps)
        table = _table(words)
        assert _call(dev[0], dev[1:], H, W, d, nc, table) == 0
        _check(table, words, want)


def test_properties_of_the_row():
    """a map equal to the ground truth has I = P = G; a one-label map of a size beyond 2d+1 has its frame of width d as band; on a
    checkerboard every pixel is band; two runs give the same bytes"""
    H, W, d, nc = 65, 129, 13, 21
    gt, preds, want = _case(H, W, d, nc, 5)
    dev = _place([gt] + preds, [0, 1, 3, 8, 0, 2])
    tables = []
    for _ in range(2):
        table = _table(2 + 5 * nc * 4)
        assert _call(dev[0], dev[1:], H, W, d, nc, table) == 0
        tables.append(table.cpu().numpy())
    assert np.array_equal(tables[0], tables[1])
    _check(torch.from_numpy(tables[0]), 2 + 5 * nc * 4, want)
    cnt = tables[0][4 + 2:-4].reshape(5, nc, 4)
    assert np.array_equal(cnt[4, :, 0], cnt[4, :, 1]) and np.array_equal(cnt[4, :, 0], cnt[4, :, 2]) and cnt[4, :, 0].sum() > 0
    assert cnt[1, :, 3].sum() == H * W - (H - 2 * d) * (W - 2 * d)       # one label: all but the interior block
    assert cnt[2, :, 3].sum() == H * W                                   # the checkerboard


@pytest.mark.parametrize("shape", [(1, 40), (7, 9), (37, 53), (64, 64)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_no_interior_gives_the_region_row_of_the_other_kernel(shape):
    """d >= max(H, W): cosa_boundary_scores' row is cosa_image_scores' own row byte for byte (one kernel against the other)"""
    from cosa_amd import _C
    H, W = shape
    nc, n_maps = 21, 3
    gt, preds, _ = _case(H, W, max(H, W), nc, n_maps)
    dev = _place([gt] + preds, [3, 1, 3, 8])
    words = 2 + n_maps * nc * 4
    region = _table(words)
    ptrs = (ctypes.c_void_p * n_maps)(*[p.data_ptr() for p in dev[1:]])
    assert _C.lib().cosa_image_scores(_C.ptr(dev[0]), ptrs, _C.int_array([0] * n_maps), n_maps, H * W, nc,
                                      ctypes.c_void_p(region.data_ptr() + 32), _C.stream_ptr()) == 0
    for d in sorted({max(H, W), 64}):                                    # (64 >= both sides of every shape here)
        table = _table(words)
        assert _call(dev[0], dev[1:], H, W, d, nc, table) == 0
        assert torch.equal(table, region), d
    _check(region, words, R.ref_row(gt, preds, [0] * n_maps, nc))


def test_refused_arguments_leave_the_row_untouched():
    from cosa_amd import _C
    L = _C.lib()
    H, W = 10, 10
    gt, p = _place([np.zeros((H, W), np.uint8), np.ones((H, W), np.uint8)], [0, 0])
    table = torch.full((2 + 9 * 21 * 4 + 8,), SENTINEL, dtype=torch.int64, device="cuda")
    before = table.clone()
    ok = dict(gt=gt, preds=[p], H=H, W=W, d=2, nc=21)
    bad = [dict(ok, nc=0), dict(ok, nc=256), dict(ok, nc=-3), dict(ok, preds=[p] * 9), dict(ok, n_maps=0), dict(ok, H=0), dict(ok, W=0),
           dict(ok, H=-1), dict(ok, H=1 << 16, W=1 << 16), dict(ok, H=(1 << 31) - 1, W=3), dict(ok, d=0), dict(ok, d=65), dict(ok, d=-1),
           dict(ok, null_map=0), dict(ok, preds=[p, p], null_map=1), dict(ok, row_ptr=0), dict(ok, row_ptr=table.data_ptr() + 4)]
    for kw in bad:
        args = [kw.pop(k) for k in ("gt", "preds", "H", "W", "d", "nc")]
        assert _call(*args, table, **kw) == EINVAL, kw
        assert L.cosa_last_error()
    one = (ctypes.c_void_p * 1)(p.data_ptr())
    assert L.cosa_boundary_scores(None, one, 1, H, W, 2, 21, _C.ptr(table), _C.stream_ptr()) == EINVAL
    assert L.cosa_boundary_scores(_C.ptr(gt), None, 1, H, W, 2, 21, _C.ptr(table), _C.stream_ptr()) == EINVAL
    for nc, k in ((0, 1), (256, 1), (21, 0), (21, 9)):
        assert L.cosa_boundary_scores_words(nc, k) == 0
    assert torch.equal(table, before)
    table[4:-4] = 0
    assert _call(gt, [p], H, W, 2, 21, table) == 0                        # and the accepted call still runs after them


def test_boundary_scores_table_in_two_chunks():
    """BoundaryScores: 11 maps are two launches per image (8 + 3); d from each image's shape on the host; a table that grows"""
    from cosa_amd.utils import evaluation as ev
    nc = 21
    names = [f"m{i}" for i in range(11)]
    table = ev.BoundaryScores(nc, names, [i % 3 == 0 for i in range(11)], 1, "cuda")          # capacity 1: the second image makes it grow
    fixed = ev.BoundaryScores(nc, names, [0] * 11, 2, "cuda", d=3)
    want, want3 = [], []
    for i, (H, W) in enumerate(((37, 53), (65, 129))):
        d = ev.boundary_width(H, W)
        assert d == (1, 3)[i]
        gt, preds, w = _case(H, W, d, nc, 11)
        g = torch.from_numpy(np.array(gt)).cuda()
        ps = [torch.from_numpy(np.array(p)).cuda() for p in preds]
        table.add(i, g, ps)
        fixed.add(i, g, ps)
        want.append(w)
        want3.append(_case(H, W, 3, nc, 11)[2])
    assert table.widths == {0: 1, 1: 3} and fixed.widths == {0: 3, 1: 3}
    rows = table.rows(2)
    assert rows.shape == (2, ev.row_words(nc, 11)) and np.array_equal(rows, np.stack(want))
    assert np.array_equal(fixed.rows(2), np.stack(want3))
    assert table.settings() == {"ratio": 0.02, "d": None} and fixed.settings() == {"ratio": 0.02, "d": 3}
    with pytest.raises(ValueError):
        table.add(0, g.reshape(-1), [p.reshape(-1) for p in ps])         # the shape is what d comes from
    with pytest.raises(ValueError):
        table.add(0, g, ps[:3])


def _model_and_loader(C=4, S=64, n=4, seed=0):
    """the tiny synthetic loader of tests/test_image_scores_gpu.py, with ground truth made of blocks"""
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
        lab = torch.from_numpy(B.run_map(rng, H, W, list(range(C + 1))).astype(np.int64))[None]
        lab[0, :3] = 255
        cls = torch.zeros(1, C)
        cls[0, rng.choice(C, 2, replace=False)] = 1
        loader.append((f"img_{k:02d}", img, lab, cls))
    return args, model, loader


def _recording(monkeypatch):
    """every BoundaryScores.add of the call, as host arrays: the maps the call produced"""
    from cosa_amd.utils import evaluation as ev
    seen = []
    plain = ev.BoundaryScores.add

    def add(self, index, gt, preds):
        seen.append((gt.cpu().numpy().copy(), [p.cpu().numpy().copy() for p in preds]))
        return plain(self, index, gt, preds)
    monkeypatch.setattr(ev.BoundaryScores, "add", add)
    return seen


def test_evaluate_writes_boundary_scores(tmp_path, monkeypatch):
    from cosa_amd import evaluation_engine as ee
    from cosa_amd.utils import evaluation as ev
    T = _tool()
    args, model, loader = _model_and_loader()
    nc = args.num_classes
    args.output_dir = tmp_path / "run"
    kw = dict(epoch=7, s_or_t='t', get_camiou=True, threshold_filters=[0.3])
    # off: what a call without the keyword gives, the image_scores file included
    before = ee.evaluate(model, loader, args, image_scores=tmp_path / "before", **kw)
    off = ee.evaluate(model, loader, args, image_scores=tmp_path / "off", boundary_scores=None, **kw)
    assert all(a == b for a, b in zip(before, off))
    assert sorted(os.listdir(tmp_path / "off")) == ["image_scores_t.jsonl", "iou_dic_t.pth"]
    for f in ("image_scores_t.jsonl", "iou_dic_t.pth"):
        assert open(tmp_path / "off" / f, "rb").read() == open(tmp_path / "before" / f, "rb").read()
    # on alone (True: args.output_dir/<epoch>), at a fixed d
    seen = _recording(monkeypatch)
    args.boundary_ratio, args.boundary_d = 0.02, 3
    on = ee.evaluate(model, loader, args, boundary_scores=True, **kw)
    assert all(a == b for a, b in zip(before, on))
    assert sorted(os.listdir(tmp_path / "run" / "00007")) == ["boundary_scores_t.jsonl"]
    settings, recs = ev.read_score_file(tmp_path / "run" / "00007" / "boundary_scores_t.jsonl")
    maps = ["cam", "cam_aux", "seg_ps", "seg_vd", "cam_0.3", "camaux_0.3"]
    assert settings["maps"] == maps and settings["boundary"] == {"ratio": 0.02, "d": 3} and settings["epoch"] == 7
    assert len(recs) == len(seen) == len(loader)
    for rec, (gt, preds), (name, _, lab, _) in zip(recs, seen, loader):
        assert rec["name"] == name and rec["d"] == 3 and np.array_equal(gt.reshape(lab.shape[1:]), lab[0].numpy().astype(np.uint8))
        assert np.array_equal(rec["row"], B.row(gt.reshape(lab.shape[1:]), [p.reshape(lab.shape[1:]) for p in preds], 3, nc)), name
    # both on, d from the ratio: both files are right
    del seen[:]
    args.boundary_d = 0
    both = ee.evaluate(model, loader, args, image_scores=tmp_path / "both", boundary_scores=tmp_path / "both", **kw)
    assert all(a == b for a, b in zip(before, both))
    assert sorted(os.listdir(tmp_path / "both")) == ["boundary_scores_t.jsonl", "image_scores_t.jsonl", "iou_dic_t.pth"]
    for f in ("image_scores_t.jsonl", "iou_dic_t.pth"):
        assert open(tmp_path / "both" / f, "rb").read() == open(tmp_path / "before" / f, "rb").read()
    settings, recs = ev.read_score_file(tmp_path / "both" / "boundary_scores_t.jsonl")
    assert settings["boundary"] == {"ratio": 0.02, "d": None}
    rows = []
    for rec, (gt, preds), (_, _, lab, _) in zip(recs, seen, loader):
        H, W = lab.shape[1:]
        d = ev.boundary_width(H, W)
        assert rec["d"] == d == max(1, int(round(0.02 * (H * H + W * W) ** 0.5)))
        rows.append(B.row(gt.reshape(H, W), [p.reshape(H, W) for p in preds], d, nc))
        assert np.array_equal(rec["row"], rows[-1])
    s = T.summary(str(tmp_path / "both" / "boundary_scores_t.jsonl"))       # the tool reads the file as it is
    want = ev.dataset_scores(np.stack(rows), nc)
    for m, name in enumerate(maps):
        iou = np.array([np.nan if v is None else v for v in s["maps"][name]["iou"]])
        assert np.array_equal(iou, want[m]["iou"], equal_nan=True)


def test_export_boundary_scores_are_those_of_the_files_on_disk(tmp_path):
    from cosa_amd import evaluation_engine as ee
    from cosa_amd.utils import evaluation as ev
    args, model, loader = _model_and_loader(n=3)
    nc = args.num_classes
    what = ("seg", "pseudo", "pseudo_aux_par", "rawcam")
    plain = ee.export_predictions(model, loader, args, tmp_path / "a", what=what, getcrf=True)
    off = ee.export_predictions(model, loader, args, tmp_path / "b", what=what, getcrf=True, boundary=False)
    res = ee.export_predictions(model, loader, args, tmp_path / "c", what=what, getcrf=True, boundary=True, boundary_d=2)
    assert "boundary" not in plain and "boundary" not in off and "scores" not in res
    assert not (tmp_path / "b" / "boundary_scores.jsonl").exists() and not (tmp_path / "c" / "scores.jsonl").exists()
    assert open(tmp_path / "a" / "manifest.json", "rb").read() == open(tmp_path / "b" / "manifest.json", "rb").read()
    manifest = json.load(open(tmp_path / "c" / "manifest.json"))
    assert manifest["settings"]["boundary"] == {"ratio": 0.02, "d": 2}
    plain_manifest = json.load(open(tmp_path / "a" / "manifest.json"))
    assert {k: v for k, v in manifest["settings"].items() if k != "boundary"} == plain_manifest["settings"] and manifest["images"] == plain_manifest["images"]
    names = ["seg", "pseudo", "pseudo_aux_par", "seg_crf"]
    settings, recs = ev.read_score_file(tmp_path / "c" / "boundary_scores.jsonl")
    assert settings["maps"] == names and settings["pseudo"] == [0, 1, 1, 0] and settings["boundary"] == {"ratio": 0.02, "d": 2} and len(recs) == 3
    rows = []
    for rec, (name, _, lab, _) in zip(recs, loader):
        assert rec["name"] == name and rec["d"] == 2
        preds = [np.asarray(Image.open(tmp_path / "c" / p / (name + ".png"))) for p in names]
        rows.append(B.row(lab[0].numpy().astype(np.uint8), preds, 2, nc))
        assert np.array_equal(rec["row"], rows[-1]), name
    want = ev.dataset_scores(np.stack(rows), nc)
    assert list(res["boundary"]) == names
    for p, w in zip(names, want):
        assert res["boundary"][p] == {"miou": ev.nan_to_none(w["miou"])}
    with pytest.raises(ValueError):
        ee.export_predictions(model, loader, args, tmp_path / "d", what=("rawcam",), boundary=True)
