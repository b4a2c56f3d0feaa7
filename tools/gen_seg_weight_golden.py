"""Write tests/golden/seg_weight.npz: inputs and what the REFERENCE's own `seg_weightloss` (utils/seg_helper.py:823-835) gives on them -- the
value and its gradient w.r.t. `seg_pred` (authoring container only: needs the reference tree, loaded file by file through
oracle.ref_loader).  Data only.

    python tools/gen_seg_weight_golden.py [seed]

B = 2, K = 6, S = 64:
  pred [B,K,S,S], mask [B,S,S] u8 {0, 1, 3, 5, 255}, weights [B,S,S] uniform in [0, 1] with exact 0s and 1s planted
  -> loss_a0 / loss_a03 / loss_a1 and grad_a0 / grad_a03 / grad_a1 [B,K,S,S]  (fg_alpha 0, 0.3, 1)
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader                                # noqa: E402

B, K, S = 2, 6, 64
ALPHAS = (("a0", 0.0), ("a03", 0.3), ("a1", 1.0))


def main(seed):
    assert ref_loader.available(), "reference tree not present"
    torch.set_num_threads(4)
    sh = ref_loader.seg_helper()
    rng = np.random.default_rng(seed)
    pred = rng.normal(0, 1, (B, K, S, S)).astype(np.float32)
    mask = rng.choice([0, 1, 3, 5, 255], size=(B, S, S)).astype(np.uint8)
    weights = rng.uniform(0, 1, (B, S, S)).astype(np.float32)
    plant = rng.uniform(0, 1, (B, S, S))
    weights[plant < 0.05] = 0.0
    weights[plant > 0.95] = 1.0
    out = {"seed": np.int64(seed), "pred": pred, "mask": mask, "weights": weights}
    for tag, a in ALPHAS:
        p = torch.from_numpy(pred).clone().requires_grad_(True)
        loss = sh.seg_weightloss(p, torch.from_numpy(mask.astype(np.float32)), torch.from_numpy(weights), fg_alpha=a)
        loss.backward()
        out["loss_" + tag] = loss.detach().numpy().astype(np.float32)
        out["grad_" + tag] = p.grad.numpy().astype(np.float32)
    labelled = mask != 255
    assert (weights[labelled] == 0).any() and (weights[labelled] == 1).any() and ((weights > 0) & (weights < 1)).mean() > 0.8
    path = os.path.join(ROOT, "tests", "golden", "seg_weight.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    for tag, _a in ALPHAS:
        print(tag, float(out["loss_" + tag]), float(np.abs(out["grad_" + tag]).max()))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 43)
