"""A float64 torch restatement of the two --act_stats reductions (csrc/act_stats_kernels.hip) and of the summary's globals
(seg_helper.act_stats_summary), for tests/test_act_stats_gpu.py and tests/test_act_stats_cpu.py.  Needs no device and no reference tree.

The range words are integers and are restated exactly.  The attention statistics are restated per ROW in float64 (`attn_rows`), or, with
dtype=torch.float32, by a plain fp32 evaluation (fp32 matmul, softmax, entropy): the difference between the two is what the GPU test derives
its tolerance from."""
import math
import struct

import torch

SITES = ("q", "k", "v", "o", "h", "x")
F16_SITES = ("q", "k", "v", "o", "h")
RANGE_FIELDS = ("finite", "absmax", "over", "near", "tiny", "nonfinite")
HEAD_FIELDS = ("rows", "ent_fix", "top1_fix", "peaked", "smax", "sharp", "nonfinite_rows")
F16_MAX, F16_HALF, F16_MIN_NORMAL = 65504.0, 32768.0, 2.0 ** -14
UNIT = 2.0 ** 32


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", float(v)))[0]


def bits_f32(b):
    return struct.unpack("<f", struct.pack("<I", int(b) & 0xffffffff))[0]


def range_words(x, acc=None):
    """the six words of cosa_range_stats_f32 over every element of the fp32 tensor x (the window itself, not its padding), added to `acc`"""
    x = x.detach().cpu().float().contiguous()
    a = x.abs().double().reshape(-1)
    fin = torch.isfinite(a)
    absmax = float(a[fin].max()) if bool(fin.any()) else 0.0
    w = [int(fin.sum()), f32_bits(absmax), int((fin & (a > F16_MAX)).sum()), int((fin & (a > F16_HALF)).sum()),
         int(((a > 0) & (a < F16_MIN_NORMAL)).sum()), int((~fin).sum())]
    if acc is not None:
        w = [max(p, q) if i == 1 else p + q for i, (p, q) in enumerate(zip(acc, w))]
    return w


def attn_rows(qkv, B, N, H, scale=0.125, dtype=torch.float64):
    """per row of every (image, head): the statistics the kernel reduces, evaluated in `dtype` from the fp32 rows qkv [>= B*N, >= 3*H*64]
    (the projection's own [3, H, 64] layout) -> dict of [B, H, N] tensors in float64: `bad` (bool: a non-finite logit), `hn` (normalised
    entropy; 0 for N = 1), `top1`, `smax` (largest finite |logit| after the scale)"""
    x = qkv.detach().cpu()[:B * N, :3 * H * 64].to(dtype).reshape(B, N, 3, H, 64)
    q, k = x[:, :, 0].permute(0, 2, 1, 3), x[:, :, 1].permute(0, 2, 1, 3)                  # [B, H, N, 64]
    s = torch.matmul(q, k.transpose(-1, -2)) * scale                                      # [B, H, N, N]
    fin = torch.isfinite(s)
    bad = ~fin.all(-1)
    p = torch.softmax(s, dim=-1)
    ent = torch.special.entr(p).sum(-1)                                                   # -sum p log p, 0 log 0 = 0
    hn = ent / math.log(N) if N > 1 else torch.zeros_like(ent)
    smax = torch.where(fin, s.abs(), torch.zeros_like(s)).amax(-1)
    return {"bad": bad, "hn": hn.double(), "top1": p.amax(-1).double(), "smax": smax.double()}


def attn_heads(rows):
    """attn_rows' output reduced as the kernel reduces it -> per head a dict: rows, nonfinite_rows, peaked (counts over the good rows), ent and
    top1 (means), smax, sharpest (the lowest hn); None where a head has no good row"""
    out = []
    H = rows["bad"].shape[1]
    for h in range(H):
        good = ~rows["bad"][:, h]
        n = int(good.sum())
        e = {"rows": n, "nonfinite_rows": int((~good).sum()), "peaked": 0, "ent": None, "top1": None, "smax": 0.0, "sharpest": None}
        if n:
            hn, t1 = rows["hn"][:, h][good], rows["top1"][:, h][good]
            e.update(peaked=int((t1 > 0.5).sum()), ent=float(hn.mean()), top1=float(t1.mean()), smax=float(rows["smax"][:, h][good].max()),
                     sharpest=float(hn.min()))
        out.append(e)
    return out


def merge_heads(parts):
    """several calls' attn_heads (the scales of a pass, accumulated into one table row) as one"""
    out = []
    for hs in zip(*parts):
        n = sum(e["rows"] for e in hs)
        live = [e for e in hs if e["rows"]]
        e = {"rows": n, "nonfinite_rows": sum(e["nonfinite_rows"] for e in hs), "peaked": sum(e["peaked"] for e in hs), "ent": None, "top1": None,
             "smax": max([e["smax"] for e in live], default=0.0), "sharpest": min([e["sharpest"] for e in live], default=None)}
        if n:
            e["ent"] = sum(e_["ent"] * e_["rows"] for e_ in live) / n
            e["top1"] = sum(e_["top1"] * e_["rows"] for e_ in live) / n
        out.append(e)
    return out


def head_words_decoded(words7):
    """seven kernel words of one head -> the same dict as attn_heads gives"""
    rows = int(words7[0])
    return {"rows": rows, "nonfinite_rows": int(words7[6]), "peaked": int(words7[3]), "ent": int(words7[1]) / UNIT / rows if rows else None,
            "top1": int(words7[2]) / UNIT / rows if rows else None, "smax": bits_f32(words7[4]),
            "sharpest": 1.0 - bits_f32(words7[5]) if rows else None}


def summary_globals(layers):
    """the globals of seg_helper.act_stats_summary restated: layers[i] = ({site: six range words}, [attn_heads-style dict per head])"""
    g = {"headroom_bits": None, "headroom_at": None, "smax": 0.0, "smax_at": None, "ent_mean": None, "ent_min": None, "ent_min_at": None,
         "over": 0, "nonfinite": 0, "nonfinite_rows": 0}
    rows = ent = 0.0
    for i, (sites, heads) in enumerate(layers):
        for name in SITES:
            w = sites[name]
            g["nonfinite"] += w[5]
            if name in F16_SITES:
                g["over"] += w[2]
                amax = bits_f32(w[1])
                if amax > 0 and (g["headroom_bits"] is None or math.log2(F16_MAX / amax) < g["headroom_bits"]):
                    g["headroom_bits"], g["headroom_at"] = math.log2(F16_MAX / amax), [name, i]
        for h, e in enumerate(heads):
            g["nonfinite_rows"] += e["nonfinite_rows"]
            if not e["rows"]:
                continue
            rows += e["rows"]
            ent += e["ent"] * e["rows"]
            if g["smax_at"] is None or e["smax"] > g["smax"]:
                g["smax"], g["smax_at"] = e["smax"], [i, h]
            if g["ent_min"] is None or e["ent"] < g["ent_min"]:
                g["ent_min"], g["ent_min_at"] = e["ent"], [i, h]
    if rows:
        g["ent_mean"] = ent / rows
    return g


def attn_bars(qkv, B, N, H, scale=0.125):
    """-> (per-head float64 reference, {quantity: tolerance}, {quantity: fp32 deviation}).  The tolerance of a quantity is 4 x the deviation
    that the plain fp32 evaluation of the same rows shows against the float64 one, plus 2^-30 (the fixed-point rounding of the sums).
    For the two means (`ent`, `top1`) the deviation is that of the per-head mean, at its largest over the heads.  `smax` and `sharpest` are
    single rows picked by a maximum: which row wins and how its own fp32 evaluation happened to round are unrelated, so the deviation taken
    is the largest any row shows (of its largest |logit|, of its normalised entropy)."""
    r64, r32 = attn_rows(qkv, B, N, H, scale), attn_rows(qkv, B, N, H, scale, dtype=torch.float32)
    h64, h32 = attn_heads(r64), attn_heads(r32)
    good = ~r64["bad"]
    dev = {}
    for k in ("ent", "top1"):
        dev[k] = max([abs(a[k] - b[k]) for a, b in zip(h64, h32) if a["rows"] and b["rows"]], default=0.0)
    row_dev = lambda k: float((r64[k] - r32[k]).abs()[good & ~r32["bad"]].max()) if bool((good & ~r32["bad"]).any()) else 0.0
    dev["smax"], dev["sharpest"] = row_dev("smax"), row_dev("hn")
    return h64, {k: 4.0 * v + 2.0 ** -30 for k, v in dev.items()}, dev
