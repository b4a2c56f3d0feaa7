"""Write tests/golden/export_par_rect.npz: inputs and the label maps the REFERENCE's own `cam2mask` + `PAR` produce at non-square sizes
(authoring container only: needs the reference tree, loaded file by file through oracle.ref_loader).  Data only.

    python tools/gen_export_par_golden.py [seed]

Per size one ImageNet-normalised image [1,3,H,W] and one CAM [C,S,S] (smooth synthetic fields, as oracle/gen_golden.py makes them); per
case (size x present classes x downscale) the reference's label map.  Every case must show a class, `ignore` and background, and
tests/export_par_ref.py:rect_refined_label must equal every label of it -- the script checks both and refuses to write otherwise.
Seeds tried (CAM planes max(1.5 f - 0.4, 0) of a smooth field f): 31 -- two cases without a background pixel; 32 -- one case without a
class pixel; 33 -- every case shows all three kinds: written.  With all three seeds (and with seed 31 at planes max(1.3 f - 0.15, 0))
the restatement equalled the reference in every pixel of every case: the seed was chosen for the label kinds only."""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import c_oracle, ref_loader                      # noqa: E402
from oracle.gen_golden import smooth_field, synth_image255   # noqa: E402
import export_par_ref as R                                   # noqa: E402

MEAN = np.array([123.675, 116.28, 103.53], np.float32)[:, None, None]
STD = np.array([58.395, 57.12, 57.375], np.float32)[:, None, None]


def main(seed):
    assert ref_loader.available(), "reference tree not present"
    c_oracle.build()
    torch.set_num_threads(4)
    sh, par_mod, th = ref_loader.seg_helper(), ref_loader.par_module(), ref_loader.torch_helper_fns()
    rng = np.random.default_rng(seed)
    out, ok = {"seed": np.int64(seed), "thr": np.array(R.GOLDEN_THR, np.float32)}, True
    for si, (H, W) in enumerate(R.GOLDEN_SIZES):
        out[f"s{si}_img"] = ((synth_image255(rng, 1, H, W) - MEAN) / STD).astype(np.float32)
        cam = smooth_field(rng, R.GOLDEN_C, R.GOLDEN_S, R.GOLDEN_S)
        out[f"s{si}_cam"] = np.maximum(cam * 1.5 - 0.4, 0).astype(np.float32)
    par = par_mod.PAR(num_iter=R.NUM_ITER, dilations=list(R.DIL))
    for si, (H, W), pi, present, ds, tag in R.golden_cases():
        img, cam = out[f"s{si}_img"], out[f"s{si}_cam"]
        cls = np.zeros(R.GOLDEN_C, np.float32)
        cls[list(present)] = 1
        t = torch.from_numpy
        with torch.no_grad():
            img01 = th.denormalize_img(t(img))
            v = t(cls)[None, :, None, None] * F.interpolate(t(cam)[None], size=(H, W), mode="bilinear", align_corners=False)
            ref = sh.cam2mask(img01, [[0, H, 0, W]], v, t(cls)[None], R.GOLDEN_THR[0], R.GOLDEN_THR[1], refine_model=par, ignore_index=255,
                              downscale=ds)[0].numpy()
        assert np.array_equal(ref, ref.astype(np.uint8))
        ref = ref.astype(np.uint8)
        mine = R.rect_refined_label(c_oracle, img, cam, cls, *R.GOLDEN_THR, downscale=ds)
        vals = set(np.unique(ref).tolist())
        shows = 0 in vals and 255 in vals and bool(vals & {p + 1 for p in present})
        diff = int((mine != ref).sum())
        print(f"{tag}: {H}x{W} present {present} ds {ds}: values {sorted(vals)} differing pixels {diff}")
        ok = ok and shows and diff == 0
        out[tag] = ref
    if not ok:
        raise SystemExit(f"seed {seed}: a case lacks a label kind or the restatement differs; nothing written")
    path = os.path.join(ROOT, "tests", "golden", "export_par_rect.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 33)
