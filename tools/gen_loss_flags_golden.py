"""Write tests/golden/loss_flags.npz: inputs and what the REFERENCE's own `seg_loss`, `seg_refine_by_label` and `cam_loss` give at the
loss-flag settings other than the defaults (authoring container only: needs the reference tree, loaded file by file through
oracle.ref_loader).  Data only.

    python tools/gen_loss_flags_golden.py [seed]

B = 2, K = 6, S = 64, a 4 x 4 CAM grid (tests/golden/misc.npz holds the default-flag vectors of the same functions at S = 32):
  segloss_pred [B,K,S,S], segloss_mask [B,S,S] u8 {0, 1, 3, 5, 255}      -> segloss_a0 / segloss_a03 / segloss_a1  (fg_alpha 0, 0.3, 1)
  refine_seg [B,K,S,S], refine_labels [B,K-1] (image 0: no class present, image 1: two) -> refine_after  (after_softmax=True, T = 0.01)
  camloss_cam [B,K-1,4,4]                                                -> camloss_after  (cam_loss on refine_after)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader                                # noqa: E402

B, K, S, G = 2, 6, 64, 4
TEMP = 0.01


def main(seed):
    assert ref_loader.available(), "reference tree not present"
    torch.set_num_threads(4)
    sh = ref_loader.seg_helper()
    rng = np.random.default_rng(seed)
    t = torch.from_numpy
    out = {"seed": np.int64(seed), "temp": np.float32(TEMP)}
    pred = rng.normal(0, 1, (B, K, S, S)).astype(np.float32)
    mask = rng.choice([0, 1, 3, 5, 255], size=(B, S, S)).astype(np.uint8)
    out["segloss_pred"], out["segloss_mask"] = pred, mask
    with torch.no_grad():
        for tag, a in (("a0", 0.0), ("a03", 0.3), ("a1", 1.0)):
            out["segloss_" + tag] = sh.seg_loss(t(pred), t(mask.astype(np.float32)), fg_alpha=a).numpy().astype(np.float32)
        seg = rng.normal(0, 1, (B, K, S, S)).astype(np.float32)
        labels = np.zeros((B, K - 1), np.float32)
        labels[1, [1, 3]] = 1
        ref = sh.seg_refine_by_label(t(seg), t(labels), softmaxtemp=TEMP, after_softmax=True)
        cam = rng.normal(0, 1, (B, K - 1, G, G)).astype(np.float32)
        out["refine_seg"], out["refine_labels"], out["refine_after"] = seg, labels, ref.numpy().astype(np.float32)
        out["camloss_cam"] = cam
        out["camloss_after"] = sh.cam_loss(t(cam), ref.float()).numpy().astype(np.float32)
    assert float(out["refine_after"][0, 1:].max()) == 0.0 and float(out["refine_after"][1, [2, 4]].max()) > 0.5
    path = os.path.join(ROOT, "tests", "golden", "loss_flags.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for k_ in ("segloss_a0", "segloss_a03", "segloss_a1", "camloss_after"):
        print(k_, float(out[k_]))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 41)
