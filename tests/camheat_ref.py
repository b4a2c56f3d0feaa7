"""Restatements in numpy of the CAM pictures of prediction export, written from the arithmetic's definition, for
tests/test_camheat_cpu.py (which pins the colour ramp) and tests/test_camheat_gpu.py (which holds the kernels to them, byte for byte).

Per class plane m (float32 [H,W]), pixel and colour c of R, G, B:
  1. idx = trunc(255 m), clamped to 0..255; a NaN gives 0                     (the product is one float32 multiplication)
  2. jet[idx][c] = (clamp(765 - |8 idx - k_c|, 0, 510) + 1) >> 1,  k = 1530, 1020, 510
  3. b = the image's byte: clamp(rint(x std_c + mean_c), 0, 255) of the normalised float32 image, product and sum each rounded once
  4. s = jet[idx][c] + b;  M = max of s over the picture's 3 H W values;  byte = (255 s) // M
"""
import numpy as np

MEAN = (123.675, 116.28, 103.53)                    # dataloaders.train_loader.normalize_img
STD = (58.395, 57.12, 57.375)
JET_K = (1530, 1020, 510)
PANEL_COLOUR = (10, 186, 181)


def jet_table():
    """int64 [256, 3]"""
    idx = np.arange(256, dtype=np.int64)[:, None]
    v = 765 - np.abs(8 * idx - np.array(JET_K, np.int64)[None, :])
    return (np.clip(v, 0, 510) + 1) >> 1


def heat_index(planes):
    """float32 [...] -> int64 [...] in 0..255"""
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.float32(255.0) * np.asarray(planes, dtype=np.float32)
        t = np.where(np.isnan(t), np.float32(0.0), t)
        return np.trunc(np.clip(t, np.float32(0.0), np.float32(255.0))).astype(np.int64)


def image_bytes(x):
    """normalised float32 [3, H, W] -> uint8 [H, W, 3]"""
    x = np.asarray(x, dtype=np.float32)
    out = np.empty(x.shape[1:] + (3,), np.uint8)
    for c in range(3):
        with np.errstate(invalid="ignore"):
            u = np.rint(x[c] * np.float32(STD[c]) + np.float32(MEAN[c]))          # two float32 roundings
            u = np.where(np.isnan(u), np.float32(0.0), u)
        out[..., c] = np.clip(u, 0, 255).astype(np.uint8)
    return out


def picture_max(planes, img_u8):
    """-> int64 [k]: M of every picture"""
    s = jet_table()[heat_index(planes)] + np.asarray(img_u8).astype(np.int64)[None]
    return s.reshape(s.shape[0], -1).max(axis=1)


def camheat_ref(planes, img_u8):
    """planes float32 [k, H, W], img_u8 uint8 [H, W, 3] -> uint8 [k, H, W, 3]"""
    s = jet_table()[heat_index(planes)] + np.asarray(img_u8).astype(np.int64)[None]        # [k, H, W, 3], 0..510
    M = s.reshape(s.shape[0], -1).max(axis=1)
    assert (M >= 128).all()
    return ((255 * s) // M[:, None, None, None]).astype(np.uint8)


def panel_ref(heat, seg, class_idx, img_u8, gt=None):
    """heat uint8 [k, H, W, 3], seg / gt uint8 [H, W], class_idx int [k] (0-based), img_u8 uint8 [H, W, 3] -> uint8 [k, H, cols W, 3]:
    heat | seg == class | gt == class (only with gt; a gt of 255 never matches) | image"""
    colour = np.array(PANEL_COLOUR, np.uint8)
    out = []
    for j, c in enumerate(class_idx):
        cols = [heat[j], (np.asarray(seg) == int(c) + 1)[..., None] * colour]
        if gt is not None:
            g = np.asarray(gt)
            cols.append(((g == int(c) + 1) & (g != 255))[..., None] * colour)
        cols.append(np.asarray(img_u8))
        out.append(np.concatenate([np.asarray(a, dtype=np.uint8) for a in cols], axis=1))
    return np.stack(out)
