"""The host half of prediction export: colour map, sharding rule, the writer pool and its file formats, the
command line's argument errors.  No GPU."""
import json
import os
import threading

import numpy as np
import pytest
from PIL import Image


def test_voc_colormap_by_rule():
    from cosa_amd.utils.export_io import voc_colormap
    cm = voc_colormap()
    assert cm.shape == (256, 3) and cm.dtype == np.uint8
    assert [tuple(c) for c in cm[:5].tolist()] == [(0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0), (0, 0, 128)]
    assert tuple(cm[255].tolist()) == (224, 224, 192)
    assert len({tuple(c) for c in cm.tolist()}) == 256               # the rule permutes the 8 index bits into 3 channels: a bijection
    for i in (6, 21, 77, 200):                                         # the rule itself, restated bit by bit
        r = g = b = 0
        for j in range(8):
            r |= ((i >> (3 * j)) & 1) << (7 - j)
            g |= ((i >> (3 * j + 1)) & 1) << (7 - j)
            b |= ((i >> (3 * j + 2)) & 1) << (7 - j)
        assert tuple(cm[i].tolist()) == (r & 255, g & 255, b & 255)


@pytest.mark.parametrize("n", [0, 1, 7, 1449, 10582])
@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_export_shard_disjoint_and_covering(n, world):
    from cosa_amd.evaluation_engine import export_shard
    parts = [export_shard(n, r, world) for r in range(world)]
    flat = [i for p in parts for i in p]
    assert len(flat) == n and sorted(flat) == list(range(n))           # disjoint (no index twice) and covering
    assert all(i % world == r for r, p in enumerate(parts) for i in p)
    with pytest.raises(ValueError):
        export_shard(n, world, world)


def _label_map(rng, H, W):
    vals = np.array(list(range(21)) + [255], np.uint8)
    a = vals[rng.integers(0, len(vals), (H, W))]
    a.reshape(-1)[: min(a.size, len(vals))] = vals[: min(a.size, len(vals))]      # every value present where the map is large enough
    return a


def test_writer_round_trip(tmp_path):
    from cosa_amd.utils.export_io import PredictionWriter, voc_colormap
    rng = np.random.default_rng(0)
    w = PredictionWriter(tmp_path, ("seg", "seg_crf", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux"), writers=3)
    maps, cams = {}, {}
    for k, (H, W) in enumerate([(1, 1), (3, 5), (375, 500)]):
        name = f"img_{k}"
        maps[name] = {p: _label_map(rng, H, W) for p in ("seg", "seg_crf", "pseudo", "pseudo_aux")}
        planes = rng.random((2, H, W), dtype=np.float32)
        cams[name] = (planes, np.array([3, 17], np.int32))
        prod = dict(maps[name])
        prod["rawcam"] = cams[name]
        prod["rawcam_aux"] = (planes[:0], np.zeros(0, np.int32))                     # no present class: no file
        w.submit(name, H, W, prod)
    assert not (tmp_path / "manifest.json").exists()
    total = w.close(settings={"split": "val"})
    pal = voc_colormap().reshape(-1).tolist()
    on_disk = 0
    for name, prods in maps.items():
        for p, a in prods.items():
            path = tmp_path / p / (name + ".png")
            on_disk += os.path.getsize(path)
            im = Image.open(path)
            assert im.mode == "P" and im.size == (a.shape[1], a.shape[0])
            assert np.array_equal(np.asarray(im), a)
            assert im.getpalette()[: 3 * 22] == pal[: 3 * 22]
        d = np.load(tmp_path / "camraw" / (name + ".npy"), allow_pickle=True).item()
        on_disk += os.path.getsize(tmp_path / "camraw" / (name + ".npy"))
        assert sorted(d) == [3, 17]
        assert all(d[c].dtype == np.float32 and np.array_equal(d[c], cams[name][0][k]) for k, c in enumerate((3, 17)))
        assert not (tmp_path / "camraw_aux" / (name + ".npy")).exists()
    assert total == on_disk
    man = json.loads((tmp_path / "manifest.json").read_text())
    assert man["settings"] == {"split": "val"}
    assert man["images"] == [{"name": "img_0", "H": 1, "W": 1}, {"name": "img_1", "H": 3, "W": 5}, {"name": "img_2", "H": 375, "W": 500}]


def test_writer_palette_holds_ignore_colour(tmp_path):
    from cosa_amd.utils.export_io import write_png
    a = np.array([[0, 255], [15, 20]], np.uint8)
    write_png(tmp_path / "a.png", a)
    rgb = np.asarray(Image.open(tmp_path / "a.png").convert("RGB"))
    assert tuple(rgb[0, 1]) == (224, 224, 192) and tuple(rgb[0, 0]) == (0, 0, 0) and tuple(rgb[1, 0]) == (192, 128, 128)


def test_writer_error_surfaces_and_manifest_waits(tmp_path):
    from cosa_amd.utils.export_io import PredictionWriter
    w = PredictionWriter(tmp_path, ("seg",), writers=2)
    gate = threading.Event()
    released = []

    def slow():
        gate.wait(10)
        return {"seg": np.zeros((4, 4), np.uint8)}

    f = w.submit("late", 4, 4, slow, release=lambda: released.append("late"))
    closer = threading.Thread(target=lambda: w.close(settings={}))
    closer.start()
    closer.join(0.3)
    assert closer.is_alive() and not (tmp_path / "manifest.json").exists()       # the manifest waits for the last file
    gate.set()
    closer.join(10)
    assert f.result() > 0 and released == ["late"]
    assert (tmp_path / "seg" / "late.png").exists() and (tmp_path / "manifest.json").exists()

    bad_dir = tmp_path / "bad"
    w2 = PredictionWriter(bad_dir, ("seg",), writers=1)
    w2.submit("ok", 2, 2, {"seg": np.zeros((2, 2), np.uint8)})
    w2.submit("broken", 2, 2, {"seg": np.zeros((2, 2), np.float32)})           # not a label map: the worker raises
    with pytest.raises(ValueError, match="uint8"):
        w2.close(settings={})
    assert not (bad_dir / "manifest.json").exists()                             # a failed export is never marked complete
    w3 = PredictionWriter(tmp_path / "bad3", ("seg",), writers=1)
    f3 = w3.submit("broken", 2, 2, {"seg": np.zeros((2, 2), np.float32)})
    with pytest.raises(ValueError):
        f3.result()
    with pytest.raises(ValueError):                                            # ... and the next submit reports it as well
        w3.submit("next", 2, 2, {"seg": np.zeros((2, 2), np.uint8)})
    w3.pool.shutdown(wait=True)
    with pytest.raises(ValueError):
        PredictionWriter(tmp_path / "w", ("seg",), writers=9)
    with pytest.raises(ValueError):
        w3.submit("../escape", 2, 2, {"seg": np.zeros((2, 2), np.uint8)})


BASE = ["run", "--checkpoint", "best_seg.pth", "--out", "out"]


@pytest.mark.parametrize("extra,needle", [(["--split", "test", "--what", "pseudo"], "label"), (["--split", "test", "--what", "seg,rawcam"], "label"),
                                          (["--writers", "9"], "--writers"), (["--usepar", "true"], "PAR"), (["--what", "heatmap"], "--what")])
def test_predict_argument_errors(capsys, extra, needle):
    from cosa_amd import predict
    with pytest.raises(SystemExit) as e:
        predict.parse(BASE + extra)
    assert e.value.code == 2 and needle in capsys.readouterr().err


def test_predict_defaults_follow_the_run():
    from cosa_amd import predict
    args, what = predict.parse(BASE + ["--split", "test"])
    assert what == ("seg",) and args.writers == 4 and (args.high_thre, args.low_thre) == (0.7, 0.25) and args.crop_size == 448
    args, what = predict.parse(BASE + ["--dataset", "COCO", "--what", "seg,pseudo,rawcam_aux", "--low_thre", "0.3", "--crf"])
    assert what == ("seg", "pseudo", "rawcam_aux") and args.high_thre == 0.65 and args.low_thre == 0.3 and args.crf and args.num_classes == 81


def test_record_layout_is_aligned_and_refuses_bad_sizes():
    from cosa_amd._C import CosaError
    from cosa_amd.utils import seg_helper
    offs, n = seg_helper.export_record_layout(20, 375, 500, 2, ("seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux"))
    assert list(offs) == ["seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux", "rawcam_idx", "rawcam_aux_idx"]
    assert all(o % 16 == 0 for o in offs.values()) and n % 16 == 0
    hw = 375 * 500
    assert offs["pseudo"] >= hw and offs["rawcam_aux"] - offs["rawcam"] >= 2 * hw * 4 and n >= offs["rawcam_aux_idx"] + 8
    assert list(seg_helper.export_record_layout(20, 3, 5, 0, ("seg",))[0]) == ["seg"]
    for bad in ((255, 3, 3, 0), (20, 0, 3, 0), (20, 3, 0, 0), (20, 3, 3, 21)):
        with pytest.raises(CosaError):
            seg_helper.export_record_layout(*bad, ("seg",))
    with pytest.raises(ValueError):
        seg_helper.export_record_layout(20, 3, 3, 0, ("heatmap",))


def test_threshold_rule_restatement_equals_cam2mask_generic():
    """the per-pixel rule the export kernel and tests/test_export_gpu.py use -- max over the present classes > high: the class; > low:
    ignore; else background -- against the reference's own formulation (seg_helper._cam2mask_generic: threshold plane + softmax + argmax
    twice) at full resolution, without a refine model, on a CPU-checkable square case"""
    import torch
    from cosa_amd.utils import seg_helper
    rng = np.random.default_rng(11)
    C, S, hi, lo = 6, 48, 0.7, 0.25
    cams = rng.random((2, C, S, S), dtype=np.float32)
    cls = np.zeros((2, C), np.float32)
    cls[0, [1, 4]] = 1
    cls[1, [0, 2, 5]] = 1
    valid = cams * cls[:, :, None, None]
    ref = seg_helper._cam2mask_generic(torch.zeros(2, 3, S, S), [[0, S, 0, S]] * 2, torch.from_numpy(valid), torch.from_numpy(cls), hi, lo,
                                       None, 255, 0).numpy()
    for b in range(2):
        keys = np.nonzero(cls[b])[0]
        planes = valid[b, keys]
        m, k = planes.max(axis=0), keys[planes.argmax(axis=0)] + 1
        mine = np.where(m > np.float32(hi), k, np.where(m > np.float32(lo), 255, 0))
        assert np.array_equal(mine, ref[b])
        assert {0, 255}.issubset(set(np.unique(mine).tolist())) and len(np.unique(mine)) >= 4


def test_sharded_loader_gives_every_item_to_one_rank():
    import torch
    from cosa_amd import evaluation_engine as ee

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return 11

        def __getitem__(self, i):
            return f"n{i}", torch.zeros(3, 2, 2), 0, torch.ones(4)

    dl = torch.utils.data.DataLoader(DS(), batch_size=1, shuffle=False)
    as_list = [(f"n{i}", None, None, None) for i in range(11)]
    for src in (dl, as_list):
        assert ee._sharded(src, 0, 1) is src
        seen = [(r, item[0][0] if src is dl else item[0]) for r in range(3) for item in ee._sharded(src, r, 3)]
        assert sorted(n for _, n in seen) == sorted(f"n{i}" for i in range(11))
        assert all(int(n[1:]) % 3 == r for r, n in seen)


def test_checkpoint_is_read_with_the_restricted_unpickler(tmp_path):
    import torch
    from cosa_amd import predict
    from cosa_amd.main import _trainer_args
    from cosa_amd.models import build_model
    from cosa_amd.utils import torch_helper
    args, _ = predict.parse(BASE + ["--pretrained", "false", "--crop_size", "64", "--num_classes", "5"])
    torch.manual_seed(0)
    a = build_model(_trainer_args(args))
    path = torch_helper.save_best(tmp_path, a, 3, 1.0, args, 's', comment='seg')       # the trainer's own file, `args` namespace included
    torch.manual_seed(1)
    b = build_model(_trainer_args(args))
    ckpt = predict.load_checkpoint(b, path)
    assert ckpt["epoch"] == 3 and all(torch.equal(x, y) for x, y in zip(a.state_dict().values(), b.state_dict().values()))
    torch.save({"model": a.state_dict(), "hook": test_voc_colormap_by_rule}, tmp_path / "other.pth")       # a global the unpickler does not know
    with pytest.raises(RuntimeError, match="trust_checkpoint"):
        predict.load_checkpoint(b, tmp_path / "other.pth")
    sd = a.state_dict()
    sd.pop(next(iter(sd)))
    torch.save({"model": sd}, tmp_path / "short.pth")
    with pytest.raises(RuntimeError, match="Missing key"):                              # strict, as finaleval
        predict.load_checkpoint(b, tmp_path / "short.pth")
