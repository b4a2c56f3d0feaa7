"""PAR-refined export products on the GPU: `seg_helper.export_refine` (cosa_export_refine) byte for byte against
the numpy yardstick `export_par_ref.rect_refined_label` (itself pinned to the reference in tests/test_export_par_cpu.py) and against the
fused square cam2mask; the parent's generic path as a reported diagnostic; the engine, the writer and the command line."""
import gc
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import export_par_ref as R

pytestmark = pytest.mark.gpu
HI, LO = 0.7, 0.25
PAR_PRODUCTS = ("pseudo_par", "pseudo_aux_par")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, "profiles", "r09_export_par.json")
MIN = 16                                                   # COSA_EXPORT_REFINE_MIN_SIDE


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cls_row(rng, C, n):
    r = np.zeros(C, np.float32)
    if n:
        r[rng.choice(C, n, replace=False)] = 1
    return r


def _merge_report(key, value):
    doc = {}
    if os.path.exists(REPORT):
        with open(REPORT) as f:
            doc = json.load(f)
    doc[key] = value
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def test_spec_expf_copy_has_the_oracle_bits(oracle_c):
    """the copy of spec E in csrc/spec_math.hpp (the label path's own lives file-local in label_kernels.hip) against oracle_c.expf"""
    from cosa_amd import _C
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.uniform(-100, 0.5, 20000), rng.uniform(-1, 1, 20000), rng.uniform(-90, 90, 5000),
                        [0.0, -0.0, -87.0, -87.00001, -86.99999, 88.0, 88.5, -1e-8, 1e-8, -0.34657359, 0.34657359]]).astype(np.float32)
    dx = dev(x)
    dy = torch.empty_like(dx)
    _C.check(_C.lib().cosa_spec_expf(_C.ptr(dx), _C.ptr(dy), x.size, _C.stream_ptr()), "cosa_spec_expf")
    want = R.expf_array(oracle_c, x)
    assert np.array_equal(dy.cpu().numpy().view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("K,h,w", [(4, 8, 8), (6, 8, 9), (3, 18, 20), (5, 16, 16)])
def test_par_kernels_bit_exact_on_the_smallest_grids(oracle_c, K, h, w):
    """what the stated minimum rests on: the PAR grid of a MIN x MIN image is 8 x 8 at downscale 2 -- the tiled affinity and step kernels
    clamp every tap, so grids far smaller than the largest dilation hold the oracle's bits like the 30 x 31 of tests/test_label_gpu.py"""
    from cosa_amd.models.PAR import PAR
    rng = np.random.default_rng(100 * h + w)
    img = rng.uniform(0, 1, (1, 3, h, w)).astype(np.float32)
    masks = rng.uniform(0, 1, (1, K, h, w)).astype(np.float32)
    out = PAR(num_iter=R.NUM_ITER, dilations=list(R.DIL))(dev(img), dev(masks)).cpu().numpy()
    assert np.array_equal(out[0], oracle_c.par_forward(img[0], masks[0], list(R.DIL), R.NUM_ITER))


# (H, W, S, C, present classes, downscale, products): every size with both downscales, C in {4, 20, 80} with 0, 1, 2 and C present,
# one CAM set (main alone, auxiliary alone) and both.  The all-present C = 80 stacks (2 x 2 x 81 planes) run at the small sizes.
BOTH, MAIN, AUX = PAR_PRODUCTS, ("pseudo_par",), ("pseudo_aux_par",)
CASES = [(MIN, MIN, 28, 4, n, ds, BOTH) for n in (0, 1, 2, 4) for ds in (2, 0)]
CASES += [(MIN, MIN + 1, 28, 20, 2, 2, BOTH), (MIN + 1, MIN, 28, 80, 80, 0, AUX)]
CASES += [(37, 41, 28, 4, n, ds, BOTH) for n in (0, 1, 2, 4) for ds in (2, 0)]
CASES += [(37, 41, 28, 20, 20, 2, MAIN), (37, 41, 28, 20, 1, 0, AUX), (37, 41, 28, 80, 80, 2, BOTH), (37, 41, 28, 80, 2, 0, BOTH)]
CASES += [(64, 64, 28, 20, n, ds, BOTH) for n in (1, 2, 20) for ds in (2, 0)]
CASES += [(64, 64, 56, 80, 80, 2, BOTH), (64, 64, 56, 80, 0, 0, MAIN), (64, 64, 56, 4, 4, 0, AUX)]
CASES += [(375, 500, 56, 20, 2, 2, BOTH), (375, 500, 56, 20, 2, 0, BOTH), (375, 500, 28, 80, 1, 2, AUX), (375, 500, 28, 4, 4, 2, MAIN)]
CASES += [(500, 333, 56, 20, 1, 2, BOTH), (500, 333, 28, 20, 2, 0, MAIN), (500, 333, 28, 4, 0, 2, BOTH), (500, 333, 28, 80, 2, 2, BOTH)]
CASES += [(40, 1023, 28, 4, 2, 2, BOTH), (40, 1023, 28, 4, 2, 0, BOTH), (40, 1023, 56, 20, 20, 2, BOTH), (40, 1023, 28, 80, 1, 0, AUX)]


@pytest.mark.parametrize("H,W,S,C,n,ds,what", CASES)
def test_export_refine_equals_the_yardstick(oracle_c, H, W, S, C, n, ds, what):
    from cosa_amd.utils import seg_helper, torch_helper
    rng = np.random.default_rng(H * 100003 + W * 101 + C * 7 + n + ds)
    img, cam, aux = R.synth_inputs(oracle_c, rng, C, S, H, W)
    cls = _cls_row(rng, C, n)
    img01 = torch_helper.denormalize_img(dev(img))
    assert np.array_equal(img01.cpu().numpy(), oracle_c.denormalize_img(img))
    record_what = ("seg",) + what                                              # the PAR slots sit behind another product's
    _, nbytes = seg_helper.export_record_layout(C, H, W, n, record_what)
    out = torch.full((nbytes + 64,), 7, device="cuda", dtype=torch.uint8)
    v = seg_helper.export_refine(img01, dev(cam), dev(aux), dev(cls), record_what, HI, LO, downscale=ds, out=out, k_live=n)
    assert sorted(v) == sorted(what)
    for p in what:
        want = R.rect_refined_label(oracle_c, img, aux if "aux" in p else cam, cls, HI, LO, downscale=ds)
        got = v[p].cpu().numpy()
        diff = int((got != want).sum())
        print(f"{p} {H}x{W} S{S} C{C} n{n} ds{ds}: values {np.unique(want).tolist()} differing pixels {diff}")
        assert got.shape == (H, W) and got.dtype == np.uint8 and diff == 0, (p, diff)
        assert set(np.unique(got).tolist()) <= {0, 255} | {int(c) + 1 for c in np.nonzero(cls)[0]}
    host = out.cpu().numpy()
    assert (host[:H * W] == 7).all() and (host[nbytes:] == 7).all()           # only its own slots are written
    if n == 0:
        assert not any(v[p].any() for p in what)
    # the wrapper counts the label row itself when k_live is not given, and owns the record when `out` is not
    v2 = seg_helper.export_refine(img01, dev(cam), dev(aux), dev(cls), what, HI, LO, downscale=ds)
    assert all(torch.equal(v2[p], v[p]) for p in what)


def test_yardstick_cases_show_every_label_kind(oracle_c):
    """the synthetic inputs of the sweep are not degenerate: class, ignore and background all occur"""
    rng = np.random.default_rng(1)
    img, cam, aux = R.synth_inputs(oracle_c, rng, 4, 28, 64, 48)
    cls = np.array([1, 0, 1, 0], np.float32)
    for c in (cam, aux):
        vals = set(np.unique(R.rect_refined_label(oracle_c, img, c, cls, HI, LO)).tolist())
        assert {0, 255} <= vals and vals & {1, 3}, vals


@pytest.mark.parametrize("ds", [2, 0])
@pytest.mark.parametrize("S,C,n", [(64, 4, 2), (64, 20, 20), (96, 20, 1), (32, 80, 3)])
def test_even_square_equals_the_fused_cam2mask(oracle_c, S, C, n, ds):
    """H = W = S even: the identity resize is exact and the 2:1 resamplings have weights 0.5 / 0.25 / 0.75 through the same fmaf order,
    so the product is the training path's fused cam2mask with PAR, byte for byte"""
    from cosa_amd.models.PAR import PAR
    from cosa_amd.utils import seg_helper, torch_helper
    rng = np.random.default_rng(S + C + n)
    img, cam, aux = R.synth_inputs(oracle_c, rng, C, S, S, S)
    cls = _cls_row(rng, C, n)
    img01 = torch_helper.denormalize_img(dev(img))
    v = seg_helper.export_refine(img01, dev(cam), dev(aux), dev(cls), PAR_PRODUCTS, HI, LO, downscale=ds)
    par = PAR(num_iter=R.NUM_ITER, dilations=list(R.DIL))
    for p, c in (("pseudo_par", cam), ("pseudo_aux_par", aux)):
        valid = dev(c * cls[:, None, None])[None]
        sq = seg_helper.cam2mask(img01, [[0, S, 0, S]], valid, dev(cls)[None], HI, LO, refine_model=par, ignore_index=255, downscale=ds)
        assert sq.shape == (1, S, S) and torch.equal(v[p], sq[0].to(torch.uint8)), (p, int((v[p] != sq[0].to(torch.uint8)).sum()))
        assert len(torch.unique(v[p])) >= 2


def test_generic_path_diagnostic(oracle_c):
    """Against the parent's way to a refined rectangular label, `_cam2mask_generic` with the PAR module: ATen's exp and resize kernels, whose
    differences PAR carries through ten steps -- equality is not required and no bound on it can be derived.  REPORTED, not asserted: the
    share of differing pixels per case goes to profiles/r09_export_par.json.  Asserted: shapes, and the same set of label values."""
    from cosa_amd.models.PAR import PAR
    from cosa_amd.utils import seg_helper, torch_helper
    par = PAR(num_iter=R.NUM_ITER, dilations=list(R.DIL))
    rows = []
    for (H, W, S, C, n, ds) in ((37, 41, 28, 4, 2, 2), (64, 64, 28, 20, 2, 2), (375, 500, 56, 20, 2, 2), (375, 500, 56, 20, 2, 0),
                                (500, 333, 56, 20, 3, 2), (40, 1023, 28, 4, 2, 2)):
        rng = np.random.default_rng(H + W + C)
        img, cam, aux = R.synth_inputs(oracle_c, rng, C, S, H, W)
        cls = _cls_row(rng, C, n)
        img01 = torch_helper.denormalize_img(dev(img))
        v = seg_helper.export_refine(img01, dev(cam), dev(aux), dev(cls), PAR_PRODUCTS, HI, LO, downscale=ds)
        for p, c in (("pseudo_par", cam), ("pseudo_aux_par", aux)):
            valid = dev(cls)[None, :, None, None] * torch.nn.functional.interpolate(dev(c)[None], size=(H, W), mode="bilinear", align_corners=False)
            gen = seg_helper._cam2mask_generic(img01, [[0, H, 0, W]], valid, dev(cls)[None], HI, LO, par, 255, ds)
            assert gen.shape == (1, H, W) and v[p].shape == (H, W)
            g8 = gen[0].to(torch.uint8)
            share = float((g8 != v[p]).float().mean())
            rows.append({"H": H, "W": W, "S": S, "C": C, "present": n, "downscale": ds, "product": p, "differing_share": share})
            print(rows[-1])
            assert set(torch.unique(g8).tolist()) == set(torch.unique(v[p]).tolist())
    _merge_report("vs_generic_path", {"note": "share of pixels where export_refine differs from _cam2mask_generic + PAR module (ATen exp / resize); "
                                              "diagnostic, one run per case", "cases": rows})


def test_export_refine_refuses_outside_the_envelope():
    from cosa_amd._C import CosaError
    from cosa_amd.utils import seg_helper
    img = torch.rand(1, 3, 40, 48, device="cuda")
    cam, cls = torch.rand(4, 8, 8, device="cuda"), torch.tensor([1.0, 0, 0, 1], device="cuda")
    ok = seg_helper.export_refine(img, cam, cam, cls, PAR_PRODUCTS, HI, LO)
    assert sorted(ok) == sorted(PAR_PRODUCTS)
    with pytest.raises(CosaError, match="image"):
        seg_helper.export_refine(None, cam, cam, cls, PAR_PRODUCTS, HI, LO)
    for small in (torch.rand(3, MIN - 1, 48, device="cuda"), torch.rand(3, 40, MIN - 1, device="cuda")):
        with pytest.raises(CosaError, match="envelope"):
            seg_helper.export_refine(small, cam, cam, cls, PAR_PRODUCTS, HI, LO)
    for ds in (3, 4, 1):
        with pytest.raises(CosaError, match="downscale"):
            seg_helper.export_refine(img, cam, cam, cls, PAR_PRODUCTS, HI, LO, downscale=ds)
    with pytest.raises(CosaError, match="dilations"):
        seg_helper.export_refine(img, cam, cam, cls, PAR_PRODUCTS, HI, LO, dilations=list(range(1, 10)))
    with pytest.raises(ValueError, match="record"):
        seg_helper.export_refine(img, cam, cam, cls, PAR_PRODUCTS, HI, LO, out=torch.empty(64, device="cuda", dtype=torch.uint8))
    with pytest.raises(CosaError):
        seg_helper.export_refine(img.cpu(), cam.cpu(), cam.cpu(), cls.cpu(), PAR_PRODUCTS, HI, LO)              # device tensors only
    with pytest.raises(CosaError, match="auxiliary"):
        seg_helper.export_refine(img, cam, None, cls, ("pseudo_aux_par",), HI, LO)
    with pytest.raises(ValueError):
        seg_helper.export_refine(img, cam, cam, cls, ("seg", "pseudo"), HI, LO)                                 # no PAR product named
    with pytest.raises(ValueError, match="export_refine"):
        seg_helper.export_maps(cam, cam, None, cls, (40, 48), ("pseudo_par",), HI, LO)                          # not export_maps' products


def _model_and_loader(C=4, S=64, n=7, seed=0):
    """tests/test_export_gpu.py:_model_and_loader (every size is above the minimum side)"""
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    torch.manual_seed(seed)
    args = default_args("VOC12", crop_size=S, batch_size=1)
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


@pytest.mark.parametrize("ds", [2, 0])
def test_engine_writes_what_export_refine_gives(tmp_path, ds):
    from cosa_amd import evaluation_engine as ee
    from cosa_amd.utils import seg_helper, torch_helper
    args, model, loader = _model_and_loader()
    args.par_downscale = ds
    what = ("seg", "pseudo", "pseudo_par", "pseudo_aux_par")
    res = ee.export_predictions(model, loader, args, tmp_path / "a", what=what)
    assert res["images"] == 7
    files = _tree(tmp_path / "a")
    assert sorted(os.listdir(tmp_path / "a")) == ["manifest.json", "pseudo", "pseudo_aux_par", "pseudo_par", "seg"]
    assert res["bytes_written"] == sum(len(b) for k, b in files.items() if k != "manifest.json")
    man = json.loads((tmp_path / "a" / "manifest.json").read_text())
    assert man["settings"]["par"] == {"num_iter": 10, "dilations": [1, 2, 4, 8, 12, 24], "downscale": ds}
    assert man["settings"]["products"] == list(what)
    # each PNG is export_refine called directly on that item's maps
    model.batch_invariant_heads = model.decoder.batch_invariant = True
    kinds = set()
    with torch.no_grad():
        for n, img, _, cls in loader:
            x = torch.nn.functional.interpolate(img.cuda(), size=[64, 64], mode="bilinear", align_corners=False)
            cams, cams_aux, _, _, _ = seg_helper.multi_scale_camsegv3(model, x, ee.EVAL_SCALES, getcls=True)
            v = seg_helper.export_refine(torch_helper.denormalize_img(img.cuda()), cams[0], cams_aux[0], cls.cuda(), ("pseudo_par", "pseudo_aux_par"),
                                         args.high_thre, args.low_thre, downscale=ds)
            for p in ("pseudo_par", "pseudo_aux_par"):
                im = Image.open(tmp_path / "a" / p / (n + ".png"))
                assert im.mode == "P" and np.array_equal(np.asarray(im), v[p].cpu().numpy()), (n, p)
                kinds |= set(np.unique(np.asarray(im)).tolist())
    model.batch_invariant_heads = model.decoder.batch_invariant = False
    assert kinds <= {0, 1, 2, 3, 4, 255}
    if ds == 2:
        # grouping, graph capture and the writer count change no byte
        for tag, kw in (("g1", dict(eval_group=1)), ("g3", dict(eval_group=3)), ("eager", dict(use_graph=False)), ("w1", dict(writers=1))):
            ee.export_predictions(model, loader, args, tmp_path / tag, what=what, **kw)
            other = _tree(tmp_path / tag)
            assert sorted(other) == sorted(files)
            assert all(other[k] == files[k] for k in files if k != "manifest.json"), tag
        # the old products are what a run without the new ones writes
        ee.export_predictions(model, loader, args, tmp_path / "old", what=("seg", "pseudo"))
        old = _tree(tmp_path / "old")
        assert sorted(k for k in old if k != "manifest.json") == sorted(k for k in files if k.startswith(("seg", "pseudo" + os.sep)))
        assert all(files[k] == b for k, b in old.items() if k != "manifest.json")
        assert "par" not in json.loads((tmp_path / "old" / "manifest.json").read_text())["settings"]
        # PAR products alone: no export_maps call at all
        ee.export_predictions(model, loader, args, tmp_path / "only", what=("pseudo_aux_par",))
        only = _tree(tmp_path / "only")
        assert all(only[k] == files[k] for k in only if k != "manifest.json") and len(only) == 8


def test_engine_refusals(tmp_path):
    from cosa_amd import evaluation_engine as ee
    args, model, loader = _model_and_loader(n=3)
    free = [(n, img, img[:, 0], torch.tensor([0])) for n, img, _, _ in loader]              # the test stage's items: no label row
    with pytest.raises(ValueError, match="label row"):
        ee.export_predictions(model, free, args, tmp_path / "t", what=("seg", "pseudo_par"))
    assert not (tmp_path / "t" / "manifest.json").exists()
    args.par_downscale = 4
    with pytest.raises(ValueError, match="par_downscale"):
        ee.export_predictions(model, loader, args, tmp_path / "d4", what=("pseudo_par",))
    ee.export_predictions(model, loader, args, tmp_path / "d4ok", what=("pseudo",))            # the other products do not read it
    args.par_downscale = 2
    args.usepar = True
    with pytest.raises(NotImplementedError, match="pseudo_par"):
        ee.export_predictions(model, loader, args, tmp_path / "par", what=("pseudo_par",))


def test_memory_does_not_grow_over_three_calls(tmp_path):
    from cosa_amd import evaluation_engine as ee
    args, model, loader = _model_and_loader()
    mem = []
    for k in range(3):
        ee.export_predictions(model, loader, args, tmp_path / f"r{k}", what=("seg", "pseudo_par", "pseudo_aux_par", "rawcam"))
        gc.collect()
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
    assert mem[2] <= mem[1], mem


def test_predict_command_line_with_par_products(tmp_path, capsys):
    """python -m cosa_amd.predict --what seg,pseudo_par,pseudo_aux_par on a tiny VOC-shaped tree"""
    from cosa_amd import predict
    from cosa_amd.main import _trainer_args
    from cosa_amd.models import build_model
    from cosa_amd.utils import torch_helper
    rng = np.random.default_rng(0)
    root, lists = tmp_path / "voc", tmp_path / "lists"
    names = ["2007_000001", "2007_000002", "2007_000003"]
    sizes = [(40, 60), (64, 48), (33, 35)]
    os.makedirs(root / "JPEGImages")
    for n, (H, W) in zip(names, sizes):
        Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(root / "JPEGImages" / (n + ".jpg"))
    os.makedirs(lists)
    (lists / "val.txt").write_text("\n".join(names) + "\n")
    onehot = {n: np.eye(4, dtype=np.float32)[k] + np.eye(4, dtype=np.float32)[3] * (k < 3) for k, n in enumerate(names)}
    np.save(lists / "cls_labels_onehot.npy", onehot, allow_pickle=True)
    common = ["--pretrained", "false", "--crop_size", "64", "--num_classes", "5", "--voc12_root", str(root), "--name_list_dir", str(lists),
              "--num_workers", "0"]
    args, _ = predict.parse(["run", "--checkpoint", "x", "--out", "x"] + common)
    torch.manual_seed(0)
    ckpt = torch_helper.save_best(tmp_path, build_model(_trainer_args(args)), 1, 0.0, args, 't', comment='seg')
    res = predict.main(["run", "--checkpoint", ckpt, "--out", str(tmp_path / "val"), "--split", "val", "--what", "seg,pseudo_par,pseudo_aux_par",
                        "--writers", "2"] + common)
    assert res["images"] == 3 and json.loads(capsys.readouterr().out.strip().splitlines()[-1])["images"] == 3
    man = json.loads((tmp_path / "val" / "manifest.json").read_text())
    assert man["settings"]["par"]["downscale"] == 2 and man["settings"]["products"] == ["seg", "pseudo_par", "pseudo_aux_par"]
    assert sorted(os.listdir(tmp_path / "val")) == ["manifest.json", "pseudo_aux_par", "pseudo_par", "seg"]
    for n, (H, W) in zip(names, sizes):
        for d in ("pseudo_par", "pseudo_aux_par"):
            m = np.asarray(Image.open(tmp_path / "val" / d / (n + ".png")))
            assert m.shape == (H, W) and set(np.unique(m).tolist()) <= {0, 255} | {int(c) + 1 for c in np.nonzero(onehot[n])[0]}
