"""Write tests/golden/camloss.npz: inputs and what the REFERENCE's own `cam_lossv2` and `cam_lossv3_wrap` give for them, values and
gradients w.r.t. the CAMs, computed in float64 from fp32 inputs (authoring container only: needs the reference tree, loaded file by file
through oracle.ref_loader).  Data only.

    python tools/gen_camloss_golden.py [seed]

B = 2, C = 5, a 4 x 4 CAM grid, S = 64:
  cam [B,C,4,4] fp32 (tests/camloss_ref.special_cam: an all-positive plane, an all-non-positive one, a doubled maximum, a dead cell)
  seg_ps [B,C+1,S,S] fp32 = softmax(1.2 randn)
  v2_loss, v2_grad                                  cam_lossv2(cam, seg_ps)
  v3_loss_25 / v3_grad_25 / v3_label_25             cam_lossv3_wrap(cam, seg_ps, 0.25), its label map (u8)
  v3_loss_50 / v3_grad_50 / v3_label_50             ... at seg_confident_thre = 0.5
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_loader                                # noqa: E402
import camloss_ref                                           # noqa: E402

B, C, G, S = 2, 5, 4, 64


def main(seed):
    assert ref_loader.available(), "reference tree not present"
    torch.set_num_threads(4)
    sh = ref_loader.seg_helper()
    rng = np.random.default_rng(seed)
    cam = camloss_ref.special_cam(rng, B, C, G, G)
    seg_ps = torch.softmax(torch.from_numpy(1.2 * rng.normal(0, 1, (B, C + 1, S, S))), dim=1).float().numpy()
    out = {"seed": np.int64(seed), "cam": cam, "seg_ps": seg_ps}

    def run(fn):
        x = torch.from_numpy(cam).double().requires_grad_(True)
        loss = fn(x, torch.from_numpy(seg_ps).double())
        loss.backward()
        return np.float64(loss.item()), x.grad.numpy().astype(np.float64)

    out["v2_loss"], out["v2_grad"] = run(lambda x, p: sh.cam_lossv2(x, p))
    for tag, thre in (("25", 0.25), ("50", 0.5)):
        out["v3_loss_" + tag], out["v3_grad_" + tag] = run(lambda x, p: sh.cam_lossv3_wrap(x, p, thre))
        value, label = torch.max(torch.from_numpy(seg_ps).double(), dim=1)
        label[value <= thre] = 255
        out["v3_label_" + tag] = label.numpy().astype(np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "camloss.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    lab = out["v3_label_50"]
    print("v2", float(out["v2_loss"]), "v3", float(out["v3_loss_25"]), float(out["v3_loss_50"]))
    print("shares at 0.5: ignore %.3f background %.3f foreground %.3f" % ((lab == 255).mean(), (lab == 0).mean(), ((lab != 0) & (lab != 255)).mean()))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 24)
