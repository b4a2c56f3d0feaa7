"""Prediction export on the GPU: the rectangular record kernel `cosa_export_maps` against `cosa_eval_labels` and the
C oracle, the raw CAMs against float64, and the engine: what `export_predictions` writes is what `evaluate` scores."""
import gc
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu
ALL = ("seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux")
SIZES = [(1, 1), (64, 64), (375, 500), (500, 333), (17, 1023)]
HI, LO = 0.7, 0.25
FP64_FACTOR = 4.0                      # the HIP error may be this many times the fp32 CPU operator's own
ERROR_FILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r08_export_rawcam_error.txt")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def threshold_rule(valid, hi, lo, ignore=255):
    """cam2mask without a refine model on already sized, validated planes [K,H,W] of the classes `keys` (0-based), whole image box:
    the threshold plane is key 0 and wins ties.  Pinned against seg_helper._cam2mask_generic in tests/test_export_cpu.py."""
    planes, keys = valid
    if len(keys) == 0:
        return np.zeros(planes.shape[1:], np.uint8)
    m, k = planes.max(axis=0), np.asarray(keys)[planes.argmax(axis=0)] + 1
    return np.where(m > np.float32(hi), k, np.where(m > np.float32(lo), ignore, 0)).astype(np.uint8)


def _label_rows(rng, C):
    rows = []
    for n in (1, 2, C):
        r = np.zeros(C, np.float32)
        r[rng.choice(C, n, replace=False)] = 1
        rows.append(r)
    return rows


_errors = {}


@pytest.mark.parametrize("S", [28, 56])
@pytest.mark.parametrize("C", [4, 20, 80])
def test_export_maps_vs_eval_labels_and_oracle(oracle_c, S, C):
    from cosa_amd.utils import seg_helper
    rng = np.random.default_rng(100 * S + C)
    cam = rng.random((C, S, S), dtype=np.float32)
    aux = rng.random((C, S, S), dtype=np.float32)
    seg = rng.standard_normal((C + 1, S, S)).astype(np.float32)
    dcam, daux, dseg = dev(cam), dev(aux), dev(seg)
    worst = _errors.setdefault((S, C), [0.0, 0.0])
    for (H, W) in SIZES:
        plain = seg_helper.export_maps(None, None, dseg, None, (H, W), ("seg",), None, None)
        assert list(plain) == ["seg"] and plain["seg"].dtype == torch.uint8 and plain["seg"].shape == (H, W)
        for cls in _label_rows(rng, C):
            keys = np.nonzero(cls)[0]
            v = seg_helper.export_maps(dcam, daux, dseg, dev(cls), (H, W), ALL, HI, LO)
            _, lab_ps, lab_vd = seg_helper.eval_label_maps(None, dseg[None], dev(cls)[None], (H, W), 0.5)
            # seg: the bits of cosa_eval_labels (and of the C oracle)
            assert torch.equal(v["seg"], lab_vd[0]) and torch.equal(plain["seg"], lab_ps[0])
            _, o_ps, o_vd = oracle_c.eval_labels(cam, seg, cls, H, W, 0.5)
            assert np.array_equal(v["seg"].cpu().numpy(), o_vd) and np.array_equal(plain["seg"].cpu().numpy(), o_ps)
            for tag, src, t in (("", cam, dcam), ("_aux", aux, daux)):
                # pseudo labels: C oracle's resize -> validation -> threshold rule over the full box, byte for byte
                valid = oracle_c.resize_bilinear(src[keys], H, W) * cls[keys][:, None, None]
                pseudo = v["pseudo" + tag].cpu().numpy()
                assert np.array_equal(pseudo, threshold_rule((valid, keys), HI, LO))
                raw = v["rawcam" + tag].cpu().numpy()
                assert raw.shape == (len(keys), H, W) and np.array_equal(v["rawcam" + tag + "_idx"].cpu().numpy(), keys)
                # (a) the dumps are self-consistent: thresholding the exported planes gives the exported labels
                assert np.array_equal(threshold_rule((raw, keys), HI, LO), pseudo)
                # (b) against F.interpolate on the CPU: the HIP error against float64 within FP64_FACTOR x the fp32 operator's own, plus one
                # ulp of the plane's maximum
                planes = torch.from_numpy(src[keys])[None]
                f32 = torch.nn.functional.interpolate(planes, size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
                f64 = torch.nn.functional.interpolate(planes.double(), size=(H, W), mode="bilinear", align_corners=False)[0].numpy()
                for k in range(len(keys)):
                    e_hip, e_cpu = np.abs(raw[k].astype(np.float64) - f64[k]).max(), np.abs(f32[k].astype(np.float64) - f64[k]).max()
                    ulp = float(np.spacing(np.float32(np.abs(f64[k]).max())))
                    worst[0], worst[1] = max(worst[0], e_hip), max(worst[1], e_cpu)
                    assert e_hip <= FP64_FACTOR * e_cpu + ulp, (S, C, H, W, int(keys[k]), e_hip, e_cpu)
    os.makedirs(os.path.dirname(ERROR_FILE), exist_ok=True)
    with open(ERROR_FILE, "w") as f:
        f.write("# exported raw CAM planes: max |x - float64 F.interpolate| per (S, C) over sizes %s and 1, 2, C present classes\n" % (SIZES,))
        f.write("# S C max|HIP - f64| max|fp32 CPU F.interpolate - f64|   (asserted per plane: HIP <= %g x CPU + 1 ulp of the plane's max)\n" % FP64_FACTOR)
        for (s, c), (a, b) in sorted(_errors.items()):
            f.write(f"{s} {c} {a:.6e} {b:.6e}\n")


def test_export_maps_refuses_outside_the_envelope():
    from cosa_amd._C import CosaError
    from cosa_amd.utils import seg_helper
    cam, seg, cls = torch.rand(4, 8, 8, device="cuda"), torch.randn(5, 8, 8, device="cuda"), torch.tensor([1.0, 0, 0, 1], device="cuda")
    with pytest.raises(CosaError, match="label row"):
        seg_helper.export_maps(cam, cam, seg, None, (5, 7), ("seg", "pseudo"), HI, LO)
    with pytest.raises(CosaError):
        seg_helper.export_maps(cam, cam, seg, cls, (0, 7), ("seg",), HI, LO)
    with pytest.raises(CosaError, match="auxiliary"):
        seg_helper.export_maps(cam, None, seg, cls, (5, 7), ("pseudo_aux",), HI, LO)
    with pytest.raises(CosaError):
        seg_helper.export_maps(cam.cpu(), None, seg.cpu(), cls.cpu(), (5, 7), ("seg",), HI, LO)             # device tensors only
    with pytest.raises(ValueError):
        seg_helper.export_maps(cam, cam, seg, cls, (5, 7), ALL, HI, LO, out=torch.empty(64, device="cuda", dtype=torch.uint8))
    big = torch.zeros(255, 2, 2, device="cuda")
    with pytest.raises(CosaError):
        seg_helper.export_maps(big, big, torch.zeros(256, 2, 2, device="cuda"), torch.ones(255, device="cuda"), (3, 3), ("seg",), HI, LO)
    out = torch.full((4096,), 7, device="cuda", dtype=torch.uint8)                                          # a caller-owned record is written in place
    v = seg_helper.export_maps(cam, cam, seg, cls, (5, 7), ("seg", "pseudo"), HI, LO, out=out, k_live=2)
    assert v["seg"].data_ptr() == out.data_ptr() and torch.equal(out[:35].reshape(5, 7), v["seg"]) and int(out[4000]) == 7


def _model_and_loader(C=4, S=64, backbone=None, n=7, seed=0):
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    torch.manual_seed(seed)
    kw = {"backbone": backbone} if backbone else {}
    args = default_args("VOC12", crop_size=S, batch_size=1, **kw)
    args.num_classes, args.bkg_thre = C + 1, 0.5
    model = build_model(args).cuda().eval()
    rng = np.random.default_rng(3)
    loader = []
    for k, (H, W) in enumerate([(50, 70), (64, 64), (81, 47), (33, 90), (64, 64), (70, 50), (37, 41)][:n]):
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
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def test_what_is_written_is_what_is_scored(oracle_c, tmp_path):
    from cosa_amd import evaluation_engine as ee
    args, model, loader = _model_and_loader()
    C = args.num_classes - 1
    what = ("seg", "pseudo", "pseudo_aux", "rawcam")
    model.train()                                                         # the flags come back as they were
    res = ee.export_predictions(model, loader, args, tmp_path / "a", what=what, getcrf=True)
    assert model.training and model.batch_invariant_heads is False and model.decoder.batch_invariant is False
    model.eval()
    assert res["images"] == 7 and res["seconds"] > 0 and res["img_per_s"] > 0
    files = _tree(tmp_path / "a")
    assert res["bytes_written"] == sum(len(b) for k, b in files.items() if k != "manifest.json")
    for d, ext in (("seg", ".png"), ("seg_crf", ".png"), ("pseudo", ".png"), ("pseudo_aux", ".png"), ("camraw", ".npy")):
        assert sorted(os.listdir(tmp_path / "a" / d)) == [n + ext for n, *_ in loader]                     # exactly one file per item and product
    assert sorted(os.listdir(tmp_path / "a")) == ["camraw", "manifest.json", "pseudo", "pseudo_aux", "seg", "seg_crf"]
    man = json.loads((tmp_path / "a" / "manifest.json").read_text())
    assert man["images"] == [{"name": n, "H": img.shape[2], "W": img.shape[3]} for n, img, _, _ in loader]
    assert man["settings"]["products"] == list(what) + ["seg_crf"] and man["settings"]["crop_size"] == 64
    # the PNGs, scored in numpy against the loader's ground truth == evaluate()'s Seg_vd and Seg_crf rows
    tab, seg_miou, df, _ = ee.evaluate(model, loader, args, epoch=1, getcrf=True, isfinal=False)
    assert df["Metrics"] == ["CAM", "aux_CAM", "Seg_vd", "Seg_crf"]
    for d, row in (("seg", "Seg_vd"), ("seg_crf", "Seg_crf")):
        hist = np.zeros((C + 1, C + 1), np.int64)
        for name, _, lab, _ in loader:
            im = Image.open(tmp_path / "a" / d / (name + ".png"))
            assert im.mode == "P"
            pred, gt = np.asarray(im), lab[0].numpy().astype(np.uint8)
            assert pred.shape == gt.shape
            keep = gt < C + 1
            hist += np.bincount((C + 1) * gt[keep].astype(np.int64) + pred[keep], minlength=(C + 1) ** 2).reshape(C + 1, C + 1)
        miou = np.round(np.array(list(oracle_c.scores_from_hist(hist)["iou"].values())) * 100, 2).mean()
        np.testing.assert_allclose(df["mIoU"][df["Metrics"].index(row)], miou, atol=1e-9)
    # the raw-CAM dictionaries: present classes only, and thresholding them gives the pseudo-label PNG
    for name, _, _, cls in loader:
        d = np.load(tmp_path / "a" / "camraw" / (name + ".npy"), allow_pickle=True).item()
        keys = np.nonzero(cls[0].numpy())[0]
        assert sorted(d) == keys.tolist()
        planes = np.stack([d[k] for k in keys])
        assert np.array_equal(threshold_rule((planes, keys), args.high_thre, args.low_thre), np.asarray(Image.open(tmp_path / "a" / "pseudo" / (name + ".png"))))
    # grouping and graph capture change no byte
    for tag, kw in (("g1", dict(eval_group=1)), ("g3", dict(eval_group=3)), ("eager", dict(use_graph=False)), ("w1", dict(writers=1))):
        ee.export_predictions(model, loader, args, tmp_path / tag, what=what, getcrf=True, **kw)
        other = _tree(tmp_path / tag)
        assert sorted(other) == sorted(files)
        assert all(other[k] == files[k] for k in files if k != "manifest.json"), tag
    with pytest.raises(ValueError):
        ee.export_predictions(model, loader, args, tmp_path / "w9", writers=9)
    args.usepar = True
    with pytest.raises(NotImplementedError, match="PAR"):
        ee.export_predictions(model, loader, args, tmp_path / "par")


def test_label_free_items_export_the_plain_argmax(tmp_path):
    from cosa_amd import evaluation_engine as ee
    from cosa_amd.utils import seg_helper
    args, model, loader = _model_and_loader(n=3)
    free = [(n, img, img[:, 0], torch.tensor([0]) if k else None) for k, (n, img, _, _) in enumerate(loader)]      # the test stage's items
    res = ee.export_predictions(model, free, args, tmp_path / "t", what=("seg",))
    assert res["images"] == 3 and sorted(os.listdir(tmp_path / "t")) == ["manifest.json", "seg"]
    model.batch_invariant_heads = model.decoder.batch_invariant = True
    with torch.no_grad():
        for n, img, _, _ in free:
            x = torch.nn.functional.interpolate(img.cuda(), size=[64, 64], mode="bilinear", align_corners=False)
            _, _, seg, _, _ = seg_helper.multi_scale_camsegv3(model, x, ee.EVAL_SCALES, getcls=True)
            ones = torch.ones(1, args.num_classes - 1, device="cuda")                 # every class present: validation masks nothing
            _, lab_ps, _ = seg_helper.eval_label_maps(None, seg, ones, img.shape[2:], 0.5)
            assert np.array_equal(np.asarray(Image.open(tmp_path / "t" / "seg" / (n + ".png"))), lab_ps[0].cpu().numpy())
    model.batch_invariant_heads = model.decoder.batch_invariant = False
    with pytest.raises(ValueError, match="label row"):
        ee.export_predictions(model, free, args, tmp_path / "t2", what=("seg", "pseudo"))
    assert not (tmp_path / "t2" / "manifest.json").exists()


def test_vit_b8_export_equals_eval_label_maps(tmp_path):
    from cosa_amd import evaluation_engine as ee
    from cosa_amd.utils import seg_helper
    args, model, loader = _model_and_loader(backbone="dino_base_patch8_224", n=3)
    ee.export_predictions(model, loader, args, tmp_path / "b8", what=("seg",), eval_group=2)
    model.batch_invariant_heads = model.decoder.batch_invariant = True
    with torch.no_grad():
        for n, img, _, cls in loader:
            x = torch.nn.functional.interpolate(img.cuda(), size=[64, 64], mode="bilinear", align_corners=False)
            _, _, seg, _, _ = seg_helper.multi_scale_camsegv3(model, x, ee.EVAL_SCALES, getcls=True)
            _, _, lab_vd = seg_helper.eval_label_maps(None, seg, cls.cuda(), img.shape[2:], 0.5)
            assert np.array_equal(np.asarray(Image.open(tmp_path / "b8" / "seg" / (n + ".png"))), lab_vd[0].cpu().numpy())


def test_second_call_reuses_buffers(tmp_path):
    from cosa_amd import evaluation_engine as ee
    args, model, loader = _model_and_loader()
    mem = []
    for k in range(3):
        ee.export_predictions(model, loader, args, tmp_path / f"r{k}", what=("seg", "pseudo", "rawcam", "rawcam_aux"))
        gc.collect()
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
    assert mem[2] <= mem[1], mem


EVERYTHING = ("seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux", "pseudo_par", "pseudo_aux_par", "overlay", "camheat", "camheat_aux", "panel")
ONE_AT_A_TIME = [(("seg",), dict(getcrf=True, scores=True, boundary=True, boundary_d=2)), (("pseudo", "pseudo_aux", "rawcam", "rawcam_aux"), {}),
                 (("pseudo_par", "pseudo_aux_par"), {}), (("seg", "overlay"), {}), (("rawcam", "camheat"), {}), (("rawcam_aux", "camheat_aux"), {}),
                 (("panel",), {}), (("camheat_aux", "panel"), {})]
NOT_PRODUCTS = ("manifest.json", "scores.jsonl", "boundary_scores.jsonl")


@pytest.fixture(scope="module")
def all_at_once(tmp_path_factory):
    """three images with two present classes each and one with none (no pictures, k_live 0), every product in one run"""
    from cosa_amd import evaluation_engine as ee
    args, model, loader = _model_and_loader(C=4, S=64, n=3)
    rng = np.random.default_rng(9)
    img = torch.from_numpy(rng.standard_normal((1, 3, 37, 41)).astype(np.float32))
    lab = torch.from_numpy(rng.integers(0, 5, (1, 37, 41)).astype(np.int64))
    loader.append(("img_03", img, lab, torch.zeros(1, 4)))
    root = tmp_path_factory.mktemp("all_at_once")
    ee.export_predictions(model, loader, args, root, what=EVERYTHING, getcrf=True, scores=True, boundary=True, boundary_d=2)
    return args, model, loader, root, {k: b for k, b in _tree(root).items() if k not in NOT_PRODUCTS}


@pytest.mark.parametrize("what,kw", ONE_AT_A_TIME, ids=["+".join(w) for w, _ in ONE_AT_A_TIME])
def test_all_at_once_equals_one_at_a_time(all_at_once, tmp_path, what, kw):
    """every slot offset of the packed record at once (the pictures behind the overlay behind seg_crf, the panel's heat plane with and
    without camheat files) against runs that lay out one kind of slot each: the same bytes in every product file, the same counters"""
    from cosa_amd import evaluation_engine as ee
    from cosa_amd.utils import evaluation
    args, model, loader, root, everything = all_at_once
    ee.export_predictions(model, loader, args, tmp_path, what=what, **kw)
    files = {k: b for k, b in _tree(tmp_path).items() if k not in NOT_PRODUCTS}
    dirs = {os.path.dirname(k) for k in files}
    assert len(dirs) == len(what) + bool(kw.get("getcrf")) and len(files) >= 3 * len(dirs)          # the picture-free image has fewer files
    for k, b in files.items():
        assert k in everything and b == everything[k], k
    for f in ("scores.jsonl", "boundary_scores.jsonl") if kw else ():
        (st_a, rec_a), (st_b, rec_b) = evaluation.read_score_file(root / f), evaluation.read_score_file(tmp_path / f)
        assert st_b["maps"] == ["seg", "seg_crf"] and [r["name"] for r in rec_a] == [r["name"] for r in rec_b] == [it[0] for it in loader]
        for ra, rb in zip(rec_a, rec_b):
            (na, va, ca), (nb, vb, cb) = evaluation.split_row(ra["row"], args.num_classes), evaluation.split_row(rb["row"], args.num_classes)
            assert (na, va, ra.get("d")) == (nb, vb, rb.get("d"))
            for m, name in enumerate(st_b["maps"]):
                assert np.array_equal(ca[st_a["maps"].index(name)], cb[m]), (f, ra["name"], name)


def test_predict_command_line_end_to_end(tmp_path, capsys):
    """python -m cosa_amd.predict on a tiny VOC-shaped tree: checkpoint in the trainer's format, `val` with labels, `test` without"""
    from cosa_amd import predict
    from cosa_amd.main import _trainer_args
    from cosa_amd.models import build_model
    from cosa_amd.utils import torch_helper
    rng = np.random.default_rng(0)
    root, lists = tmp_path / "voc", tmp_path / "lists"
    names = ["2007_000001", "2007_000002", "2007_000003"]
    sizes = [(40, 60), (64, 48), (33, 35)]
    for d in ("JPEGImages", "JPEGImages_test"):
        os.makedirs(root / d)
        for n, (H, W) in zip(names, sizes):
            Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(root / d / (n + ".jpg"))
    os.makedirs(lists)
    for split in ("val", "test"):
        (lists / (split + ".txt")).write_text("\n".join(names) + "\n")
    onehot = {n: np.eye(4, dtype=np.float32)[k] + np.eye(4, dtype=np.float32)[3] * (k < 3) for k, n in enumerate(names)}
    np.save(lists / "cls_labels_onehot.npy", onehot, allow_pickle=True)
    common = ["--pretrained", "false", "--crop_size", "64", "--num_classes", "5", "--voc12_root", str(root), "--name_list_dir", str(lists),
              "--num_workers", "0"]
    args, _ = predict.parse(["run", "--checkpoint", "x", "--out", "x"] + common)
    torch.manual_seed(0)
    ckpt = torch_helper.save_best(tmp_path, build_model(_trainer_args(args)), 1, 0.0, args, 't', comment='seg')
    res = predict.main(["run", "--checkpoint", ckpt, "--out", str(tmp_path / "val"), "--split", "val", "--what", "seg,pseudo,rawcam", "--writers", "2"] + common)
    assert res["images"] == 3 and json.loads(capsys.readouterr().out.strip().splitlines()[-1])["images"] == 3
    man = json.loads((tmp_path / "val" / "manifest.json").read_text())
    assert man["settings"]["split"] == "val" and man["settings"]["checkpoint"] == os.path.abspath(ckpt)
    assert man["images"] == [{"name": n, "H": H, "W": W} for n, (H, W) in zip(names, sizes)]
    for n, (H, W) in zip(names, sizes):
        seg = np.asarray(Image.open(tmp_path / "val" / "seg" / (n + ".png")))
        assert seg.shape == (H, W) and set(np.unique(seg).tolist()) <= {0} | {int(c) + 1 for c in np.nonzero(onehot[n])[0]}
        assert sorted(np.load(tmp_path / "val" / "camraw" / (n + ".npy"), allow_pickle=True).item()) == np.nonzero(onehot[n])[0].tolist()
    res = predict.main(["run", "--checkpoint", ckpt, "--out", str(tmp_path / "test"), "--split", "test"] + common)
    assert res["images"] == 3 and sorted(os.listdir(tmp_path / "test")) == ["manifest.json", "seg"]
    assert sorted(os.listdir(tmp_path / "test" / "seg")) == [n + ".png" for n in names]
