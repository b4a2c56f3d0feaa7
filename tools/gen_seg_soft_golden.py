"""Write tests/golden/seg_soft.npz: inputs and what the REFERENCE's own `seg_softloss` / `seg_softlossv2` (utils/seg_helper.py:837-861) give on
them -- the values and their gradients w.r.t. `seg_pred`, in float64 (authoring container only: needs the reference tree, loaded file by
file through oracle.ref_loader).  Data only.

    python tools/gen_seg_soft_golden.py [seed]

B = 2, K = 5, S = 32, float64:
  pred [B,K,S,S] ~ N(0, 1); probs [B,K,S,S] = softmax of N(0, 1) logits whose channel 0 is lifted on the left half of every image, so that
  both of seg_softloss's sets (argmax == 0, argmax != 0) hold at least 900 of the 2048 pixels
  -> loss_a05 / loss_a03 and grad_a05 / grad_a03 (seg_softloss, fg_alpha 0.5 and 0.3), loss_v2 and grad_v2 (seg_softlossv2), n_bg, n_fg
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import ref_loader                                # noqa: E402

B, K, S = 2, 5, 32
ALPHAS = (("a05", 0.5), ("a03", 0.3))
LIFT = 2.5


def main(seed):
    assert ref_loader.available(), "reference tree not present"
    torch.set_num_threads(4)
    sh = ref_loader.seg_helper()
    rng = np.random.default_rng(seed)
    pred = rng.normal(0, 1, (B, K, S, S))
    raw = rng.normal(0, 1, (B, K, S, S))
    raw[:, 0, :, :S // 2] += LIFT
    probs = torch.softmax(torch.from_numpy(raw), dim=1).numpy()
    lab = probs.argmax(1)
    n_bg, n_fg = int((lab == 0).sum()), int((lab != 0).sum())
    assert n_bg >= 900 and n_fg >= 900, (n_bg, n_fg)
    out = {"seed": np.int64(seed), "pred": pred, "probs": probs, "n_bg": np.int64(n_bg), "n_fg": np.int64(n_fg)}
    for tag, a in ALPHAS:
        p = torch.from_numpy(pred).clone().requires_grad_(True)
        loss = sh.seg_softloss(p, torch.from_numpy(probs), fg_alpha=a)
        loss.backward()
        out["loss_" + tag], out["grad_" + tag] = loss.detach().numpy(), p.grad.numpy()
    p = torch.from_numpy(pred).clone().requires_grad_(True)
    loss = sh.seg_softlossv2(p, torch.from_numpy(probs))
    loss.backward()
    out["loss_v2"], out["grad_v2"] = loss.detach().numpy(), p.grad.numpy()
    assert all(v.dtype == np.float64 for k, v in out.items() if k.startswith(("loss", "grad", "pred", "probs")))
    path = os.path.join(ROOT, "tests", "golden", "seg_soft.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; sets", n_bg, n_fg)
    for tag in ("a05", "a03", "v2"):
        print(tag, float(out["loss_" + tag]), float(np.abs(out["grad_" + tag]).max()))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 47)
