"""Tests-side yardsticks of the attention backward (csrc/attn_kernels.hip: attn_bwd_prep / _dq / _dkv kernels), both in float64 torch on
the 16-bit-rounded inputs: `exact`, autograd of softmax(q k^T / 8) v, and `model`, the same mathematics with the kernels' rounding points
and no others.  `draw` makes the seeded inputs the tests share.  A helper, not a test."""
import math

import torch

SCALE = 0.125
HD = 64


def rd(x, dt):
    """round to the 16-bit operand type (nearest even, subnormals kept) and come back to float64"""
    return x.to(dt).to(torch.float64)


def rd32(x):
    return x.to(torch.float32).to(torch.float64)


def ulp(x, dt):
    """one unit in the last place of `dt` at magnitude x (a python float); the subnormal spacing below the normal range"""
    mant, emin = (7, -126) if dt == torch.bfloat16 else (10, -14)
    e = max(math.frexp(x)[1] - 1, emin) if x > 0 else emin
    return 2.0 ** (e - mant)


def draw(B, N, H, dt, seed, scale=1.0, go_scale=1.0, sharp=False, device="cuda"):
    """qkv [B,N,3*H*64] and dO [B,N,H*64] in the operand type.  sharp: key N-3 of image 0, head 0 is 40 x query 7 (one key dominates a row
    late in the sequence, in the tail tile: the construction of test_attention_fwd_sharp_rows)"""
    gen = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, N, 3 * H * HD, generator=gen) * scale
    if sharp:
        qkv[0, N - 3, H * HD:H * HD + HD] = qkv[0, 7, 0:HD] * 40
    go = torch.randn(B, N, H * HD, generator=gen) * go_scale
    return qkv.to(dt).to(device), go.to(dt).to(device)


def heads(t, H):
    """[B,N,H*64] -> [B,H,N,64]"""
    B, N, _ = t.shape
    return t.view(B, N, H, HD).transpose(1, 2)


def split(qkv, H):
    """[B,N,3*H*64] -> q, k, v, each [B,H,N,64]"""
    B, N, _ = qkv.shape
    return qkv.view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)


def pack(dq, dk, dv):
    """three [B,H,N,64] -> [B,N,3*H*64]"""
    B, H, N, _ = dq.shape
    return torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(B, N, 3 * H * HD)


def exact(qkv, go, H):
    """-> dqkv [B,N,3*H*64], out [B,N,H*64], lse [B,H,N], all float64 and unrounded"""
    B, N, _ = qkv.shape
    x = qkv.double().requires_grad_(True)
    q, k, v = split(x, H)
    att = (q @ k.transpose(-1, -2)) * SCALE
    o = (att.softmax(-1) @ v).transpose(1, 2).reshape(B, N, H * HD)
    o.backward(go.double())
    return x.grad, o.detach(), torch.logsumexp(att.detach(), -1)


def forward_model(qkv, H):
    """out and lse with the forward kernel's rounding points: the un-normalised probabilities exp(s - max) are rounded to the operand type for
    both the P V product and the row sum, out is rounded to the operand type, lse to fp32 -> out [B,N,H*64], lse [B,H,N] (float64 holders).
    It has to reproduce the SIZE of the forward's rounding for the coupled bar, not the kernel's bits: the kernel rounds tile by tile
    against a running maximum, this against the row's final one, and relative rounding does not care which."""
    dt = qkv.dtype
    B, N, _ = qkv.shape
    q, k, v = split(qkv.double(), H)
    s = (q @ k.transpose(-1, -2)) * SCALE
    m = s.amax(-1, keepdim=True)
    p = rd(torch.exp(s - m), dt)
    l = p.sum(-1, keepdim=True)
    o = rd((p @ v) / l, dt)
    return o.transpose(1, 2).reshape(B, N, H * HD), rd32(m + torch.log(l)).squeeze(-1)


def model(qkv, go, H, out, lse, parts=False):
    """The backward's arithmetic in float64 with the kernels' rounding points: `out` is what the kernel is given (already in the operand type),
    delta = rowsum(dO o out) and `lse` are fp32; P = exp(s - lse) is rounded to the operand type for dV = P^T dO only; dS = P o (dP - delta) / 8
    is formed from the unrounded P and rounded to the operand type for dQ = dS K and dK = dS^T Q; the three results are rounded to the
    operand type.  -> dqkv [B,N,3*H*64] float64 (parts: also the unrounded dS)"""
    dt = qkv.dtype
    q, k, v = split(qkv.double(), H)
    do = heads(go.double(), H)
    s = (q @ k.transpose(-1, -2)) * SCALE
    p = torch.exp(s - rd32(lse.double()).unsqueeze(-1))
    delta = rd32((do * heads(rd(out.double(), dt), H)).sum(-1, keepdim=True))
    ds = p * (do @ v.transpose(-1, -2) - delta) * SCALE
    p16, ds16 = rd(p, dt), rd(ds, dt)
    g = rd(pack(ds16 @ k, ds16.transpose(-1, -2) @ q, p16.transpose(-1, -2) @ do), dt)
    return (g, ds) if parts else g


def slice_errors(g, ref, H):
    """per gradient and per (batch, head): -> rms [3,B,H], max [3,B,H] of g - ref, and max|ref| [3,B,H]"""
    B, N, _ = g.shape
    e = (g.double() - ref).view(B, N, 3, H, HD)
    r = ref.view(B, N, 3, H, HD)
    return e.pow(2).mean((1, 4)).sqrt().permute(1, 0, 2), e.abs().amax((1, 4)).permute(1, 0, 2), r.abs().amax((1, 4)).permute(1, 0, 2)
