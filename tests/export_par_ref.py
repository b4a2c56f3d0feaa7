"""Tests-side yardstick of the PAR-refined export products: `rect_refined_label`, a numpy restatement of the
reference's `cam2mask(..., refine_model=PAR(...))` read literally at H != W, built from the C oracle's exported pieces
(resize_bilinear = spec R, expf = spec E, denormalize_img, par_forward).  float32 throughout, sums in class order.
tests/test_export_par_cpu.py pins it to the reference's own output (tests/golden/export_par_rect.npz); the GPU tests hold
`seg_helper.export_refine` to it byte for byte."""
import numpy as np

DIL = (1, 2, 4, 8, 12, 24)
NUM_ITER = 10


def expf_array(oracle_c, x):
    """spec E element by element through the oracle's own function"""
    f = oracle_c.lib().orc_expf_export
    flat = np.ascontiguousarray(x, np.float32).ravel()
    return np.fromiter((f(v) for v in flat.tolist()), np.float32, count=flat.size).reshape(np.shape(x))


def softmax_present(oracle_c, stack):
    """softmax over axis 0 of [K1,h,w] as ATen and the C oracle evaluate it: subtract the maximum, exp, sum in plane order, divide"""
    stack = np.ascontiguousarray(stack, np.float32)
    e = expf_array(oracle_c, stack - stack.max(axis=0, keepdims=True))
    s = np.zeros(stack.shape[1:], np.float32)
    for k in range(stack.shape[0]):
        s = s + e[k]
    return (e / s[None]).astype(np.float32)


def rect_refined_label(oracle_c, img, cam, cls, thr_hi, thr_lo, downscale=2, ignore_index=255, dilations=DIL, num_iter=NUM_ITER):
    """img [1,3,H,W] / [3,H,W] ImageNet-normalised, cam [C,S,S], cls [C] -> uint8 [H,W] in {0..C, ignore_index}"""
    img = np.asarray(img, np.float32).reshape(1, 3, *np.shape(img)[-2:])
    cam, cls = np.asarray(cam, np.float32), np.asarray(cls, np.float32)
    H, W = img.shape[-2:]
    keys = np.nonzero(cls)[0]
    if len(keys) == 0:
        return np.zeros((H, W), np.uint8)
    img01 = oracle_c.denormalize_img(img)[0]
    v = cls[keys][:, None, None] * oracle_c.resize_bilinear(cam[keys], H, W)          # cam_validation of the resized CAM: the `rawcam` planes
    if downscale:
        h, w = H // downscale, W // downscale
        small = oracle_c.resize_bilinear(img01, h, w)
    else:
        h, w = H, W
        small = img01
    labels = []
    for thr in (thr_hi, thr_lo):
        stack = np.concatenate([np.full((1, H, W), np.float32(thr), np.float32), v.astype(np.float32)], axis=0)
        if downscale:
            stack = oracle_c.resize_bilinear(stack, h, w)
        p = softmax_present(oracle_c, stack)
        p = oracle_c.par_forward(small, p, list(dilations), num_iter)
        up = oracle_c.resize_bilinear(p, H, W)
        k = up.argmax(axis=0)                                                         # first maximum wins
        labels.append(np.concatenate([[0], keys + 1])[k])
    hi, lo = labels
    m = hi.copy()
    m[hi == 0] = ignore_index
    m[(hi + lo) == 0] = 0
    return m.astype(np.uint8)


# the cases of tests/golden/export_par_rect.npz (tools/gen_export_par_golden.py writes them from the reference)
GOLDEN_SIZES = ((37, 53), (64, 48), (50, 75), (64, 64))
GOLDEN_C, GOLDEN_S = 4, 32
GOLDEN_PRESENT = ((2,), (0, 3), (0, 1, 3))
GOLDEN_THR = (0.7, 0.25)


def golden_cases():
    for si, (H, W) in enumerate(GOLDEN_SIZES):
        for pi, present in enumerate(GOLDEN_PRESENT):
            for ds in (2, 0):
                yield si, (H, W), pi, present, ds, f"s{si}_p{pi}_ds{ds}"


def synth_inputs(oracle_c, rng, C, S, H, W):
    """a smooth normalised image [1,3,H,W] with pixel noise and two smooth CAM sets [C,S,S] in [0, 1.1] with empty regions"""
    mean = np.array([123.675, 116.28, 103.53], np.float32)[:, None, None]
    std = np.array([58.395, 57.12, 57.375], np.float32)[:, None, None]
    base = oracle_c.resize_bilinear(rng.random((3, H // 8 + 2, W // 8 + 2), dtype=np.float32), H, W) * 255.0
    img = ((np.clip(base + rng.normal(0, 2.0, base.shape), 0, 255).astype(np.float32) - mean) / std).astype(np.float32)[None]
    cams = [np.maximum(oracle_c.resize_bilinear(rng.random((C, 5, 5), dtype=np.float32), S, S) * 2.0 - 0.6, 0).astype(np.float32) for _ in range(2)]
    return img, cams[0], cams[1]
