"""cam_lossv2 / cam_lossv3 / cam_lossv3_wrap restated from their formulas, in any float dtype, on the host.

Written from the closed forms, not from the reference's text: the normalisation with its extrema's first positions, the soft-margin terms,
the bilinear up-sampling as two interpolation matrices, the class-balanced cross-entropy, and the gradients in closed form.  Every loss has
an autograd-able value (`*_loss`) and a closed-form gradient (`*_grad`); tests/test_camloss_cpu.py pins the second against autograd of the
first and both against the golden vectors (tests/golden/camloss.npz) the reference itself wrote.
"""
import numpy as np
import torch

IGNORE = 255


def first_index(mask):
    """[..., n] bool -> the first true position of every row"""
    n = mask.shape[-1]
    idx = torch.arange(n).expand(mask.shape)
    return torch.where(mask, idx, torch.full_like(idx, n)).min(dim=-1)[0]


def normalise(x):
    """x [B,C,h,w] -> n, (r - mn, d2, argmin, argmax): r = relu(x), mn / mx per plane, d2 = mx + 1e-4 taken before the shift"""
    B, C, h, w = x.shape
    r = torch.relu(x).reshape(B, C, h * w)
    mn, mx = r.min(dim=-1, keepdim=True)[0], r.max(dim=-1, keepdim=True)[0]
    d2 = mx + 1e-4
    amin, amax = first_index(r == mn), first_index(r == mx)
    # (gather at the first positions: autograd then routes the extrema's gradients there, as adaptive_max_pool2d does)
    mn_g, mx_g = r.gather(-1, amin[..., None]), r.gather(-1, amax[..., None])
    n = (r - mn_g) / (mx_g + 1e-4)
    return n.reshape(B, C, h, w), ((r - mn).reshape(B, C, h, w), d2.reshape(B, C, 1, 1), amin, amax)


def normalise_adjoint(x, g, aux):
    """g = dL/dn -> dL/dx:  g_i / d2 - [i == argmin] G / d2 - [i == argmax] Gn / d2^2, masked by x > 0"""
    B, C, h, w = x.shape
    rm, d2, amin, amax = aux
    g, rm, d2 = g.reshape(B, C, -1), rm.reshape(B, C, -1), d2.reshape(B, C, 1)
    G, Gn = g.sum(-1, keepdim=True), (g * rm).sum(-1, keepdim=True)
    idx = torch.arange(h * w).expand(B, C, -1)
    d = g / d2 - (idx == amin[..., None]) * (G / d2) - (idx == amax[..., None]) * (Gn / (d2 * d2))
    return (d * (x.reshape(B, C, -1) > 0)).reshape(B, C, h, w)


def log_sigmoid(v):
    return torch.clamp(v, max=0) - torch.log1p(torch.exp(-v.abs()))


# ---- v2 ----------------------------------------------------------------------------------------------------------------------
def v2_loss(x, y):
    """mean over rows (b, pixel) and classes of -(y log s(n) + (1 - y) log s(-n))"""
    n, _ = normalise(x)
    return -(y * log_sigmoid(n) + (1 - y) * log_sigmoid(-n)).mean()


def v2_grad(x, y):
    n, aux = normalise(x)
    return normalise_adjoint(x, (torch.sigmoid(n) - y) / n.numel(), aux)


# ---- bilinear resizing (align_corners = False) as a matrix -------------------------------------------------------------------
def interp_matrix(n_in, n_out, dtype):
    """[n_out, n_in]: row d holds the two weights of source position scale (d + 0.5) - 0.5 clamped at 0"""
    scale = torch.tensor(n_in, dtype=dtype) / n_out
    src = torch.clamp(scale * (torch.arange(n_out, dtype=dtype) + 0.5) - 0.5, min=0)
    i0 = torch.clamp(src.floor().long(), max=n_in - 1)
    i1 = torch.clamp(i0 + 1, max=n_in - 1)
    l1 = src - i0.to(dtype)
    m = torch.zeros((n_out, n_in), dtype=dtype)
    m[torch.arange(n_out), i0] += 1 - l1
    m[torch.arange(n_out), i1] += l1
    return m


def resize(t, H, W):
    """[..., h, w] -> [..., H, W]"""
    return interp_matrix(t.shape[-2], H, t.dtype) @ t @ interp_matrix(t.shape[-1], W, t.dtype).T


# ---- v3 ----------------------------------------------------------------------------------------------------------------------
def _ce_groups(label):
    lab = label.long()
    bg, fg = lab == 0, (lab != 0) & (lab != IGNORE)
    return lab, bg, fg


def _mean_denominator(group, dtype):
    """count + 1e-6 as the reference's type promotion performs it: an integer tensor plus a Python float is an fp32 addition, whatever the
    dtype of the logits (so above 16 pixels the 1e-6 is rounded away)"""
    return (group.sum().float() + 1e-6).to(dtype)


def balanced_ce(z, label):
    """z [B,K,S,S], label [B,S,S]: 0.5 mean over background pixels + 0.5 mean over foreground pixels of -log softmax(z)[label]; a mean
    is sum / (count + 1e-6), so an empty group gives 0"""
    lab, bg, fg = _ce_groups(label)
    logp = z - torch.logsumexp(z, dim=1, keepdim=True)
    nll = -logp.gather(1, torch.where(lab == IGNORE, torch.zeros_like(lab), lab)[:, None])[:, 0]
    return 0.5 * (nll * bg).sum() / _mean_denominator(bg, z.dtype) + 0.5 * (nll * fg).sum() / _mean_denominator(fg, z.dtype)


def mix_of(n):
    """cat(1 - max_c n, n) and the first channel of the maximum per cell"""
    mx = n.max(dim=1, keepdim=True)[0]
    arg = first_index((n == mx).permute(0, 2, 3, 1))
    return torch.cat([1 - n.gather(1, arg[:, None]), n], dim=1), arg


def v3_loss(x, label):
    n, _ = normalise(x)
    mix, _ = mix_of(n)
    return balanced_ce(resize(mix, *label.shape[-2:]), label)


def v3_grad(x, label):
    n, aux = normalise(x)
    mix, arg = mix_of(n)
    H, W = label.shape[-2:]
    lab, bg, fg = _ce_groups(label)
    p = torch.softmax(resize(mix, H, W), dim=1)
    onehot = torch.zeros_like(p).scatter_(1, torch.where(lab == IGNORE, torch.zeros_like(lab), lab)[:, None], 1.0)
    coef = 0.5 * bg.to(x.dtype) / _mean_denominator(bg, x.dtype) + 0.5 * fg.to(x.dtype) / _mean_denominator(fg, x.dtype)
    g_full = coef[:, None] * (p - onehot)
    g_mix = interp_matrix(mix.shape[-2], H, x.dtype).T @ g_full @ interp_matrix(mix.shape[-1], W, x.dtype)       # the resize's transpose
    C = x.shape[1]
    g_n = g_mix[:, 1:] - (torch.arange(C)[None, :, None, None] == arg[:, None]) * g_mix[:, :1]
    return normalise_adjoint(x, g_n, aux)


# ---- the v3 label ------------------------------------------------------------------------------------------------------------
def refine(seg, cls_label, T, after_softmax):
    """seg [B,K,S,S] summed teacher logits, cls_label [B,K-1] -> probabilities; absent classes masked with -1e5 before the softmax, or
    (after_softmax) zeroed after a softmax over all K"""
    present = torch.cat([torch.ones_like(cls_label[:, :1]), cls_label], dim=1)[:, :, None, None] != 0
    if after_softmax:
        return torch.softmax(seg / T, dim=1) * present
    return torch.softmax(torch.where(present, seg, torch.full_like(seg, -1e5)) / T, dim=1)


def label_of(p, thre):
    """argmax_k p (lowest index at an exact tie), 255 where max_k p <= thre"""
    mx = p.max(dim=1, keepdim=True)[0]
    lab = first_index((p == mx).permute(0, 2, 3, 1))
    return torch.where(mx[:, 0] <= thre, torch.full_like(lab, IGNORE), lab)


def sum_scales(scales, S):
    """per-scale low-res teacher segs [2B,K,h_i,w_i] (original batch, then the flipped batch) -> [B,K,S,S]: up(original) + un-flipped
    up(flipped), summed over the scales in order"""
    tot = None
    for s in scales:
        B = s.shape[0] // 2
        up = resize(s, S, S)
        v = up[:B] + up[B:].flip(-1)
        tot = v if tot is None else tot + v
    return tot


def label_from_scales(scales, cls_label, S, T, thre, after_softmax):
    """-> (label [B,S,S], excusable [B,S,S] bool): a pixel of a lower-precision evaluation may differ where the top two logits among the
    candidates lie within 1e-5 relative, or the maximum probability within 1e-5 of the threshold"""
    z = sum_scales(scales, S)
    p = refine(z, cls_label, T, after_softmax)
    lab = label_of(p, thre)
    present = (torch.cat([torch.ones_like(cls_label[:, :1]), cls_label], dim=1) != 0)[:, :, None, None].expand_as(z)
    zc = torch.where(present, z, torch.full_like(z, -float("inf")))
    top = zc.topk(min(2, z.shape[1]), dim=1)[0]
    gap = top[:, 0] - top[:, 1] if top.shape[1] > 1 else torch.full_like(top[:, 0], float("inf"))
    near_tie = torch.isfinite(gap) & (gap <= 1e-5 * torch.maximum(top[:, 0].abs(), top[:, -1].abs()))     # (one candidate: no tie)
    near_thre = (p.max(dim=1)[0] - thre).abs() <= 1e-5
    return lab, near_tie | near_thre


# ---- the committed inputs ----------------------------------------------------------------------------------------------------
def special_cam(rng, B, C, h, w):
    """CAMs [B,C,h,w] fp32 with the planes every test wants: (0, 0) all positive (the minimum carries gradient), (0, 1) all non-positive,
    (1, 0) its positive maximum twice (the first position takes the gradient), and cell (1, :, 0, 0) non-positive in every class"""
    cam = rng.normal(0, 1, (B, C, h, w)).astype(np.float32)
    cam[0, 0] = np.abs(cam[0, 0]) + 0.25
    cam[0, 1] = -np.abs(cam[0, 1])
    flat = cam[1, 0].reshape(-1)
    flat[[1, flat.size - 2]] = np.float32(np.abs(flat).max() + 0.5)
    cam[1, :, 0, 0] = -np.abs(cam[1, :, 0, 0]) - 0.125
    return cam


def seg_scales_inputs(rng, B, K, sizes, sd=1.0):
    """three low-resolution scales [2B,K,s,s] with live flipped halves, and class labels [B,K-1] with image 0 empty"""
    scales = [rng.normal(0, sd, (2 * B, K, s, s)).astype(np.float32) for s in sizes]
    cls = np.zeros((B, K - 1), np.float32)
    for b in range(1, B):
        cls[b, rng.choice(K - 1, size=min(3, K - 1), replace=False)] = 1
    return scales, cls


# the label kernel's committed cases (tests/test_camloss_cpu.py checks their shares and the fp32 restatement on the host, tests/test_camloss_gpu.py
# runs the kernel on them): crop 64 at the scales 1.0, 0.5, 1.5 of a 16-pixel patch
LABEL_SEED, LABEL_B, LABEL_K, LABEL_S, LABEL_SIZES = 7, 2, 6, 64, (4, 2, 6)
LABEL_SETTINGS = ((0.01, 0.25), (1.0, 0.5))          # (temperature, segconf_thre)
LABEL_EXCUSED_MAX = 1e-3                              # at most 0.1 % of the pixels may be excused


def label_case():
    rng = np.random.default_rng(LABEL_SEED)
    return seg_scales_inputs(rng, LABEL_B, LABEL_K, LABEL_SIZES)
