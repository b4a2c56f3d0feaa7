"""The CAM pictures of prediction export on the GPU: `cosa_export_camheat` and `cosa_export_panel` against their numpy
restatements (tests/camheat_ref.py), byte for byte; the engine end to end -- every picture equals the restatement applied to the written
`.npy` plane and the image, and an export without the pictures writes the bytes it wrote before."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import camheat_ref as R

pytestmark = pytest.mark.gpu
EINVAL = 1
SIZES = [(5, 7), (33, 31), (64, 64)]              # H W % 4 = 3 under one workgroup; % 4 = 3 over several; aligned, no tail


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _normalised(u8):
    from cosa_amd.dataloaders.train_loader import normalize_img
    return dev(np.transpose(normalize_img(u8), (2, 0, 1)).astype(np.float32))


def _planes(rng, k, H, W):
    """random planes in [0, 1) with, in every plane: exact 0 and 1.0, j / 255 and the float below it for three j, a NaN, a value above 1
    and a negative one, at random places"""
    f = np.float32
    p = rng.random((k, H, W), dtype=np.float32)
    special = [f(0.0), f(1.0), f(np.nan), f(1.5), f(-0.25)]
    for j in (37, 128, 254):
        special += [f(j / 255.0), np.nextafter(f(j / 255.0), f(0.0))]
    for j in range(k):
        p[j].reshape(-1)[rng.choice(H * W, len(special), replace=False)] = special
    return p


def _images(rng, H, W):
    u8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    u8.reshape(-1)[:2] = [0, 255]
    return {"random": u8, "zeros": np.zeros((H, W, 3), np.uint8), "full": np.full((H, W, 3), 255, np.uint8)}


def _check_camheat(planes, u8, tag):
    from cosa_amd.utils import seg_helper
    k, H, W = planes.shape
    want = R.camheat_ref(planes, u8)
    x, p = _normalised(u8), dev(planes)
    assert np.array_equal(R.image_bytes(x.cpu().numpy()), u8)                               # the rule gives the bytes back
    got = seg_helper.export_camheat(p, x)
    assert got.dtype == torch.uint8 and got.shape == (k, H, W, 3)
    first = got.cpu().numpy()
    bad = np.argwhere(first != want)
    assert len(bad) == 0, (tag, len(bad), bad[:4].tolist())
    # again, into a record slice at a 16-byte offset: the same bytes, the poison around them untouched
    n = 3 * k * H * W
    rec = torch.full((16 + n + 32,), 0xA5, device="cuda", dtype=torch.uint8)
    seg_helper.export_camheat(p, x, out=rec[16:16 + n])
    back = rec.cpu().numpy()
    assert np.array_equal(back[16:16 + n].reshape(k, H, W, 3), first), tag
    assert (back[:16] == 0xA5).all() and (back[16 + n:] == 0xA5).all(), tag
    return want


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("size", SIZES)
def test_export_camheat_equals_the_restatement(size, k):
    H, W = size
    rng = np.random.default_rng(1000 * H + 10 * W + k)
    planes = _planes(rng, k, H, W)
    for tag, u8 in _images(rng, H, W).items():
        _check_camheat(planes, u8, (size, k, tag))
    assert (R.picture_max(planes, np.full((H, W, 3), 255, np.uint8)) == 510).all()          # the all-255 image reaches M = 510
    assert (R.picture_max(planes, np.zeros((H, W, 3), np.uint8)) == 255).all()
    low = np.zeros((k, H, W), np.float32)                                                   # index 0 everywhere over black: M = 128, the smallest
    assert (R.picture_max(low, np.zeros((H, W, 3), np.uint8)) == 128).all()
    want = _check_camheat(low, np.zeros((H, W, 3), np.uint8), (size, k, "M=128"))
    assert (want == np.array([0, 0, 255], np.uint8)).all()


def test_export_camheat_at_an_image_size():
    H, W = 375, 500
    rng = np.random.default_rng(5)
    _check_camheat(_planes(rng, 3, H, W), _images(rng, H, W)["random"], "375x500")


@pytest.mark.parametrize("size", [(5, 7), (33, 31)])
def test_camheat_index_is_that_of_the_written_rawcam(size):
    """export_maps, then export_camheat on its rawcam view: the picture is the restatement of the plane as read back -- idx = trunc(255 rawcam)
    -- over a black image, where the bytes are the ramp's alone, and over a random one"""
    from cosa_amd.utils import seg_helper
    H, W = size
    C, S = 6, 16
    rng = np.random.default_rng(H)
    cam = dev((rng.random((C, S, S), dtype=np.float32) * 1.2 - 0.1).astype(np.float32))
    seg = dev(rng.standard_normal((C + 1, S, S)).astype(np.float32))
    cls = np.zeros(C, np.float32)
    cls[[1, 3, 4]] = 1
    v = seg_helper.export_maps(cam, cam.flip(0).contiguous(), seg, dev(cls), (H, W), ("seg", "rawcam", "rawcam_aux"), 0.7, 0.25, k_live=3)
    assert v["rawcam_idx"].tolist() == [1, 3, 4]
    for tag, u8 in _images(rng, H, W).items():
        for slot in ("rawcam", "rawcam_aux"):
            got = seg_helper.export_camheat(v[slot], _normalised(u8)).cpu().numpy()
            raw = v[slot].cpu().numpy()
            assert np.array_equal(got, R.camheat_ref(raw, u8)), (size, tag, slot)
            if tag == "zeros":                          # M = 255 wherever an index reaches a plateau: the bytes are the ramp's own
                idx = np.trunc(np.clip(np.float32(255.0) * raw, 0, 255)).astype(np.int64)
                M = R.jet_table()[idx].reshape(3, -1).max(axis=1)
                assert np.array_equal(got.astype(np.int64), 255 * R.jet_table()[idx] // M[:, None, None, None])


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("size", [(5, 7), (33, 31)])
def test_export_panel_equals_the_restatement(size, k):
    from cosa_amd.utils import seg_helper
    H, W = size
    rng = np.random.default_rng(77 * H + k)
    u8 = _images(rng, H, W)["random"]
    x = _normalised(u8)
    heat = rng.integers(0, 256, (k, H, W, 3), dtype=np.uint8)
    seg = rng.choice(np.array([0, 1, 3, 4], np.uint8), (H, W))                             # class 2 is in no pixel of seg
    gt = rng.choice(np.array([0, 1, 2, 3, 255], np.uint8), (H, W))
    gt[0, 0], gt[-1, -1] = 255, 255
    class_idx = np.array([[1], [0, 1, 254]][k // 2], np.int32)                             # 0-based: class 2 (absent from seg); class 255 against a gt of 255
    for g in (gt, None):
        want = R.panel_ref(heat, seg, class_idx, u8, gt=g)
        cols = 4 if g is not None else 3
        assert want.shape == (k, H, cols * W, 3)
        runs = [seg_helper.export_panel(dev(heat), dev(seg), dev(class_idx), x, gt=dev(g) if g is not None else None).cpu().numpy() for _ in range(2)]
        assert runs[0].shape == want.shape and np.array_equal(runs[0], want) and np.array_equal(runs[1], want), (size, k, cols)
        j = list(class_idx).index(1)
        assert not want[j, :, W:2 * W].any()                                                # the absent class: a black column
        if g is not None and k == 3:
            assert not want[2, :, 2 * W:3 * W].any() and (g == 255).any()                   # a gt of 255 matches no class
        n = want.size
        rec = torch.full((n + 32,), 0x5A, device="cuda", dtype=torch.uint8)
        seg_helper.export_panel(dev(heat), dev(seg), dev(class_idx), x, gt=dev(g) if g is not None else None, out=rec[:n])
        back = rec.cpu().numpy()
        assert np.array_equal(back[:n].reshape(want.shape), want) and (back[n:] == 0x5A).all()


def test_pictures_refuse_outside_the_envelope():
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    L = _C.lib()
    H, W, k = 4, 4, 2
    planes, x = torch.rand(k, H, W, device="cuda"), torch.zeros(3, H, W, device="cuda")
    out = torch.full((3 * k * H * W,), 9, device="cuda", dtype=torch.uint8)
    ws = torch.full((64,), 7, device="cuda", dtype=torch.uint8)
    p, null, s = _C.ptr, ctypes.c_void_p(0), _C.stream_ptr()
    for kk, h, w, nout, nws, ptrs in ((0, H, W, 96, 64, None), (-1, H, W, 96, 64, None), (257, H, W, 1 << 20, 4096, None), (k, 0, W, 96, 64, None),
                                      (k, H, 0, 96, 64, None), (k, 1 << 15, 1 << 14, 1 << 40, 64, None), (k, H, W, 95, 64, None),
                                      (k, H, W, 96, 7, None), (k, H, W, 96, 64, (null, p(x), p(out), p(ws))),
                                      (k, H, W, 96, 64, (p(planes), null, p(out), p(ws))), (k, H, W, 96, 64, (p(planes), p(x), null, p(ws))),
                                      (k, H, W, 96, 64, (p(planes), p(x), p(out), null))):
        q = ptrs or (p(planes), p(x), p(out), p(ws))
        assert L.cosa_export_camheat(q[0], q[1], kk, h, w, q[2], nout, q[3], nws, s) == EINVAL, (kk, h, w, nout, nws)
    heat, seg = torch.zeros(k, H, W, 3, device="cuda", dtype=torch.uint8), torch.ones(H * W, device="cuda", dtype=torch.uint8)
    idx = torch.tensor([0, 1], device="cuda", dtype=torch.int32)
    pout = torch.full((3 * k * H * 4 * W,), 9, device="cuda", dtype=torch.uint8)
    for kk, h, w, nout, ptrs in ((0, H, W, 384, None), (257, H, W, 1 << 20, None), (k, 0, W, 384, None), (k, 1 << 15, 1 << 14, 1 << 40, None),
                                 (k, H, W, 383, None), (k, H, W, 384, (null, p(seg), p(idx), p(x), p(pout))),
                                 (k, H, W, 384, (p(heat), null, p(idx), p(x), p(pout))), (k, H, W, 384, (p(heat), p(seg), null, p(x), p(pout))),
                                 (k, H, W, 384, (p(heat), p(seg), p(idx), null, p(pout))), (k, H, W, 384, (p(heat), p(seg), p(idx), p(x), null))):
        q = ptrs or (p(heat), p(seg), p(idx), p(x), p(pout))
        assert L.cosa_export_panel(q[0], q[1], p(seg), q[2], q[3], kk, h, w, q[4], nout, s) == EINVAL, (kk, h, w, nout)
    assert L.cosa_export_panel(p(heat), p(seg), null, p(idx), p(x), k, H, W, p(pout), 287, s) == EINVAL          # three columns: 288 bytes
    torch.cuda.synchronize()
    assert bool((out == 9).all()) and bool((ws == 7).all()) and bool((pout == 9).all())     # nothing was launched
    with pytest.raises(ValueError):
        seg_helper.export_camheat(planes[:0], x)                                            # k = 0
    with pytest.raises(ValueError):
        seg_helper.export_camheat(planes, x, out=out[:95])
    with pytest.raises(ValueError):
        seg_helper.export_camheat(planes[:, :3], x)
    with pytest.raises(_C.CosaError):
        seg_helper.export_camheat(planes.cpu(), x.cpu())
    with pytest.raises(ValueError):
        seg_helper.export_panel(heat[:0], seg, idx[:0], x)
    with pytest.raises(ValueError):
        seg_helper.export_panel(heat, seg, idx, x, gt=seg, out=pout[:383])
    with pytest.raises(ValueError):
        seg_helper.export_panel(heat, seg[:15], idx, x)
    with pytest.raises(_C.CosaError):
        seg_helper.export_panel(heat.cpu(), seg.cpu(), idx.cpu(), x.cpu())
    assert bool((out == 9).all()) and bool((pout == 9).all())
    assert seg_helper.export_camheat(planes, x, out=out).shape == (k, H, W, 3) and not bool((out == 9).all())


def _model_and_loader(C=4, S=64, n=3):
    """the model and items of tests/test_export_gpu.py at its crop"""
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    torch.manual_seed(0)
    args = default_args("VOC12", crop_size=S, batch_size=1)
    args.num_classes, args.bkg_thre = C + 1, 0.5
    model = build_model(args).cuda().eval()
    rng = np.random.default_rng(3)
    loader = []
    for k, (H, W) in enumerate([(50, 70), (37, 41), (64, 64)][:n]):
        img = torch.from_numpy(rng.standard_normal((1, 3, H, W)).astype(np.float32))
        lab = torch.from_numpy(rng.integers(0, C + 1, (1, H, W)).astype(np.int64))
        lab[0, :3] = 255
        cls = torch.zeros(1, C)
        cls[0, rng.choice(C, 2, replace=False)] = 1
        loader.append((f"img_{k:02d}", img, lab, cls))
    return args, model, loader


def _tree(root):
    out = {}
    for d, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


def _png(path):
    im = Image.open(path)
    assert im.mode == "RGB"
    return np.asarray(im)


def test_pictures_end_to_end(tmp_path):
    from cosa_amd import evaluation_engine as ee
    args, model, loader = _model_and_loader()
    C = args.num_classes - 1
    what = ("seg", "rawcam", "camheat", "camheat_aux", "panel")
    res = ee.export_predictions(model, loader, args, tmp_path / "a", what=what)
    assert res["images"] == len(loader)
    ee.export_predictions(model, loader, args, tmp_path / "b", what=("seg", "rawcam"))
    ee.export_predictions(model, loader, args, tmp_path / "aux", what=("rawcam_aux",))     # the auxiliary planes, for the camaux pictures
    a, b = _tree(tmp_path / "a"), _tree(tmp_path / "b")
    expected = {"manifest.json"}
    for name, img, lab, cls in loader:
        H, W = img.shape[2:]
        keys = np.nonzero(cls[0].numpy())[0]
        u8 = R.image_bytes(img[0].numpy())
        expected |= {f"seg/{name}.png", f"camraw/{name}.npy"}
        expected |= {f"{d}/{name}_{c + 1}.png" for d in ("cam", "camaux", "merged") for c in keys}        # 4 classes: the names are the indices
        seg = np.asarray(Image.open(tmp_path / "a" / "seg" / (name + ".png")))
        gt = lab[0].numpy().astype(np.uint8)
        raw = np.load(tmp_path / "a" / "camraw" / (name + ".npy"), allow_pickle=True).item()
        raw_aux = np.load(tmp_path / "aux" / "camraw_aux" / (name + ".npy"), allow_pickle=True).item()
        assert sorted(raw) == keys.tolist() == sorted(raw_aux)
        for planes, d in ((raw, "cam"), (raw_aux, "camaux")):
            want = R.camheat_ref(np.stack([planes[c] for c in keys]), u8)
            for j, c in enumerate(keys):
                got = _png(tmp_path / "a" / d / f"{name}_{c + 1}.png")
                assert got.shape == (H, W, 3) and np.array_equal(got, want[j]), (name, d, c)
        heat = np.stack([_png(tmp_path / "a" / "cam" / f"{name}_{c + 1}.png") for c in keys])
        want = R.panel_ref(heat, seg, keys, u8, gt=gt)
        for j, c in enumerate(keys):
            got = _png(tmp_path / "a" / "merged" / f"{name}_{c + 1}.png")
            assert got.shape == (H, 4 * W, 3) and np.array_equal(got, want[j]), (name, c)
            assert np.array_equal(got[:, W:2 * W].any(axis=2), seg == c + 1)                # the second column is the seg PNG's region
            assert np.array_equal(got[:, 2 * W:3 * W].any(axis=2), gt == c + 1) and np.array_equal(got[:, 3 * W:], u8)
    assert set(a) == expected                                                               # every expected file and no other
    # without the pictures: the same seg and camraw bytes, today's manifest keys
    assert sorted(b) == sorted(k for k in a if k.split("/")[0] in ("seg", "camraw", "manifest.json"))
    assert all(b[k] == a[k] for k in b if k != "manifest.json")
    man_a, man_b = json.loads(a["manifest.json"])["settings"], json.loads(b["manifest.json"])["settings"]
    assert man_a["camheat"] == {"ramp": "jet-int", "panel_colour": [10, 186, 181]} and man_a["products"] == list(what)
    assert "camheat" not in man_b and set(man_a) - set(man_b) == {"camheat"}
    assert res["bytes_written"] == sum(len(v) for k, v in a.items() if k != "manifest.json")
    # rows from the model's own head, items without a ground-truth map: three columns, the pictures of the classes the head names
    free = [(n, img, 0, 0) for n, img, _, _ in loader]
    ee.export_predictions(model, free, args, tmp_path / "p", what=("rawcam", "panel"), classes="predicted")
    p = _tree(tmp_path / "p")
    rows = [json.loads(ln) for ln in p["classes.jsonl"].decode().splitlines()]
    assert [r["name"] for r in rows] == [n for n, *_ in loader] and all(len(r["classes"]) >= 1 for r in rows)
    assert not any(k.startswith(("cam/", "camaux/", "seg/")) for k in p)
    assert sorted(k for k in p if k.startswith("merged/")) == sorted(f"merged/{r['name']}_{c}.png" for r in rows for c in r["classes"])
    for (name, img, _, _), r in zip(loader, rows):
        H, W = img.shape[2:]
        raw = np.load(tmp_path / "p" / "camraw" / (name + ".npy"), allow_pickle=True).item()
        keys = [c - 1 for c in r["classes"]]
        heat = R.camheat_ref(np.stack([raw[c] for c in keys]), R.image_bytes(img[0].numpy()))
        for j, c in enumerate(keys):
            got = _png(tmp_path / "p" / "merged" / f"{name}_{c + 1}.png")
            assert got.shape == (H, 3 * W, 3) and np.array_equal(got[:, :W], heat[j]) and np.array_equal(got[:, 2 * W:], R.image_bytes(img[0].numpy()))
    # no class row, no picture: refused as a pseudo label is
    with pytest.raises(ValueError, match="classes='none'"):
        ee.export_predictions(model, loader, args, tmp_path / "n", what=("seg", "camheat"), classes="none")
    with pytest.raises(ValueError, match="label row"):
        ee.export_predictions(model, free, args, tmp_path / "n2", what=("panel",))
    assert not (tmp_path / "n").exists() or not (tmp_path / "n" / "manifest.json").exists()
