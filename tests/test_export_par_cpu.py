"""PAR-refined export products (pseudo_par / pseudo_aux_par), the host half: the numpy yardstick
`export_par_ref.rect_refined_label` against the reference's own cam2mask + PAR at non-square sizes, the command line, the record layout,
the writer.  No GPU."""
import numpy as np
import pytest
from PIL import Image

import export_par_ref as R

BASE = ["run", "--checkpoint", "best_seg.pth", "--out", "out"]
OLD = ("seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux")


def test_rect_refined_label_equals_the_reference(oracle_c, golden):
    """tests/golden/export_par_rect.npz: what the reference's cam2mask(..., refine_model=PAR(10, [1,2,4,8,12,24])) gives at 37x53, 64x48,
    50x75 and 64x64, 1 / 2 / 3 present classes of 4, downscale 2 and 0 (tools/gen_export_par_golden.py).  Every label equal."""
    g = golden("export_par_rect")
    hi, lo = (float(t) for t in g["thr"])
    n = 0
    for si, (H, W), pi, present, ds, tag in R.golden_cases():
        ref = g[tag]
        assert ref.shape == (H, W) and ref.dtype == np.uint8
        vals = set(np.unique(ref).tolist())
        assert 0 in vals and 255 in vals and vals & {p + 1 for p in present}, (tag, vals)          # a constant map cannot pass
        cls = np.zeros(R.GOLDEN_C, np.float32)
        cls[list(present)] = 1
        mine = R.rect_refined_label(oracle_c, g[f"s{si}_img"], g[f"s{si}_cam"], cls, hi, lo, downscale=ds)
        assert np.array_equal(mine, ref), (tag, int((mine != ref).sum()))
        n += 1
    assert n == 24
    assert not R.rect_refined_label(oracle_c, g["s0_img"], g["s0_cam"], np.zeros(R.GOLDEN_C), hi, lo).any()       # no present class: all zero


def test_even_square_case_equals_the_square_oracle(oracle_c, golden):
    """H = W = S even: the literal rectangular reading coincides with the square path's oracle (orc_cam2mask, pinned to the reference
    by tests/golden/cam2mask.npz): identity resize, 2:1 taps 0.5 / 0.25 / 0.75"""
    g = golden("export_par_rect")
    img, S = g["s3_img"], 64
    cam = oracle_c.resize_bilinear(g["s3_cam"], S, S)
    cls = np.array([1, 0, 1, 1], np.float32)
    img01 = oracle_c.denormalize_img(img)
    for ds in (2, 0):
        sq = oracle_c.cam2mask(img01, [[0, S, 0, S]], cam[None], cls[None], 0.7, 0.25, downscale=ds, par=(list(R.DIL), R.NUM_ITER))[0]
        assert np.array_equal(R.rect_refined_label(oracle_c, img, cam, cls, 0.7, 0.25, downscale=ds), sq.astype(np.uint8))


def test_new_products_parse_and_test_split_refuses_them(capsys):
    from cosa_amd import predict
    args, what = predict.parse(BASE + ["--what", "seg,pseudo_par,pseudo_aux_par", "--split", "train_aug"])
    assert what == ("seg", "pseudo_par", "pseudo_aux_par") and args.par_downscale == 2
    args, what = predict.parse(BASE + ["--what", "pseudo_aux_par,pseudo", "--par_downscale", "0"])
    assert what == ("pseudo_aux_par", "pseudo") and args.par_downscale == 0
    for extra, needle in ((["--split", "test", "--what", "pseudo_par"], "label"), (["--split", "test", "--what", "seg,pseudo_aux_par"], "label"),
                          (["--what", "pseudo_par", "--par_downscale", "3"], "par_downscale"), (["--what", "pseudo_par,pseudo_par"], "--what"),
                          (["--usepar", "true"], "--what pseudo_par")):
        with pytest.raises(SystemExit) as e:
            predict.parse(BASE + extra)
        err = capsys.readouterr().err
        assert e.value.code == 2 and needle in err, (extra, err)
    predict.parse(BASE + ["--what", "pseudo", "--par_downscale", "3"])                    # the other products do not read it


def test_layout_appends_the_par_slots():
    from cosa_amd._C import CosaError
    from cosa_amd.utils import seg_helper
    assert seg_helper.EXPORT_BITS["pseudo_par"] == 32 and seg_helper.EXPORT_BITS["pseudo_aux_par"] == 64
    for (C, H, W, K) in ((20, 375, 500, 2), (4, 37, 41, 1), (80, 17, 1023, 80), (20, 3, 5, 0)):
        old, n_old = seg_helper.export_record_layout(C, H, W, K, OLD)
        assert list(old) == ["seg", "pseudo", "pseudo_aux", "rawcam", "rawcam_aux", "rawcam_idx", "rawcam_aux_idx"]
        # the old slots by their rule: each product's size rounded up to 16 bytes, in slot order
        hw, off = H * W, 0
        for k, size in zip(old, (hw, hw, hw, 4 * K * hw, 4 * K * hw, 4 * K, 4 * K)):
            assert old[k] == off
            off += (size + 15) & ~15
        assert n_old == max(off, 16)
        both, n = seg_helper.export_record_layout(C, H, W, K, OLD + ("pseudo_par", "pseudo_aux_par"))
        assert list(both) == list(old) + ["pseudo_par", "pseudo_aux_par"] and all(both[k] == old[k] for k in old)
        assert both["pseudo_par"] == off and both["pseudo_aux_par"] == off + ((hw + 15) & ~15) and n == off + 2 * ((hw + 15) & ~15)
        assert all(o % 16 == 0 for o in both.values()) and n % 16 == 0
        only, n1 = seg_helper.export_record_layout(C, H, W, K, ("pseudo_aux_par",))
        assert only == {"pseudo_aux_par": 0} and n1 == (hw + 15) & ~15
        mixed, _ = seg_helper.export_record_layout(C, H, W, K, ("seg", "pseudo_par"))
        assert mixed == {"seg": 0, "pseudo_par": (hw + 15) & ~15}
    with pytest.raises(CosaError):
        seg_helper.export_record_layout(20, 8, 8, 0, 128)
    rec = np.arange(4 * 64, dtype=np.uint8)
    v = seg_helper.export_record_views(rec, 4, 6, 7, 1, ("seg", "pseudo_par"))
    assert v["pseudo_par"].shape == (6, 7) and int(v["pseudo_par"][0, 0]) == 48 and v["seg"].shape == (6, 7)


def test_refine_entry_refuses_on_the_host():
    """argument errors of cosa_export_refine are found before any launch: reachable without a device (fake but aligned addresses)"""
    import ctypes
    from cosa_amd import _C
    L = _C.lib()
    dil = _C.int_array(R.DIL)
    p = ctypes.c_void_p(4096)

    def call(image=p, cam=p, aux=p, cls=p, C=4, S=8, H=32, W=32, K=0, what=96, ds=2, nd=6, iters=10, rec_bytes=1 << 20, ws_bytes=0):
        return L.cosa_export_refine(image, cam, aux, cls, C, S, H, W, K, what, 0.7, 0.25, 255, ds, dil, nd, iters, p, rec_bytes, p, ws_bytes, None)

    for kw, needle in ((dict(image=None), "image"), (dict(H=15), "envelope"), (dict(W=8), "envelope"), (dict(ds=3), "downscale"), (dict(nd=9), "dilations"),
                       (dict(rec_bytes=100), "record"), (dict(what=31), "PAR product"), (dict(what=32, cam=None), "main CAM"),
                       (dict(what=64, aux=None), "auxiliary"), (dict(K=5), "K_live"), (dict(C=255), "C must")):
        assert call(**kw) == 1, kw
        assert needle in L.cosa_last_error().decode(), (kw, L.cosa_last_error())
    assert call(K=2) == 4 and "workspace" in L.cosa_last_error().decode()                 # COSA_ENOMEM: the workspace is too small
    assert L.cosa_export_refine_workspace_bytes(32, 32, 2, 96, 3, 6) == 0 and L.cosa_export_refine_workspace_bytes(32, 32, 2, 31, 2, 6) == 0
    hw = 16 * 16
    al = lambda n: (n + 255) // 256 * 256
    assert L.cosa_export_refine_workspace_bytes(32, 33, 2, 96, 2, 6) == 2 * al(4 * 3 * hw * 4) + al(3 * hw * 4) + al(48 * hw * 4)
    # cosa_export_maps is not to be asked for the new bits
    assert L.cosa_export_maps(p, p, p, p, 4, 8, 32, 32, 0, 33, 0.7, 0.25, 255, p, 1 << 20, None) == 1


def test_writer_takes_the_par_directories(tmp_path):
    from cosa_amd.utils.export_io import PredictionWriter
    rng = np.random.default_rng(5)
    vals = np.array([0, 1, 4, 255], np.uint8)
    a, b = vals[rng.integers(0, 4, (37, 41))], vals[rng.integers(0, 4, (37, 41))]
    w = PredictionWriter(tmp_path, ("pseudo", "pseudo_par", "pseudo_aux_par"), writers=2)
    w.submit("x", 37, 41, {"pseudo": a, "pseudo_par": a, "pseudo_aux_par": b})
    w.close(settings={"par": {"num_iter": 10}})
    for d, m in (("pseudo_par", a), ("pseudo_aux_par", b)):
        im = Image.open(tmp_path / d / "x.png")
        assert im.mode == "P" and np.array_equal(np.asarray(im), m)
    assert (tmp_path / "pseudo_par" / "x.png").read_bytes() == (tmp_path / "pseudo" / "x.png").read_bytes()
