"""The kernels of the "f32" operand family (csrc/f32_kernels.hip) one by one: derivable error bounds against float64,
the bit-for-bit properties the numerics contract promises, the argument envelope.  u = 2^-24, gamma_n = n u / (1 - n u).  The measured
error of every case relative to torch's fp32 evaluation on the CPU goes on record in profiles/fp32_teacher_parity.txt: one line per case,
replaced by the next run's."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "fp32_teacher_parity.txt")
U = 2.0 ** -24
SENT = -12345.5          # sentinel value: exactly representable, never a result


def gamma(n):
    return n * U / (1 - n * U)


def record(key, figures):
    """the line `key: figures` of the record, in place of the line an earlier run left under that key (a new key goes to the end)"""
    lines = open(RECORD).read().splitlines() if os.path.exists(RECORD) else []
    new, at = f"{key}: {figures}", [i for i, ln in enumerate(lines) if ln.startswith(key + ": ")]
    if at:
        lines[at[0]] = new
    else:
        lines.append(new)
    with open(RECORD, "w") as f:
        f.write("\n".join(lines) + "\n")


def _dev():
    return torch.device("cuda", 0)


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------
GEMM_CASES = [(1, 768, 768, 0, 0), (197, 2304, 768, 0, 0), (257, 3072, 768, 1, 0), (300, 768, 3072, 2, 0), (130, 768, 192, 0, 0), (513, 512, 768, 0, 32)]


def _gemm_inputs(M, N, K, seed=0):
    return _randn(M, K, seed=seed), _randn(N, K, seed=seed + 1, scale=0.05), _randn(N, seed=seed + 2), _randn(M, N, seed=seed + 3)


@pytest.mark.parametrize("M,N,K,epi,pad", GEMM_CASES)
def test_gemm_f32_within_the_fma_chain_bound_of_float64(M, N, K, epi, pad):
    """|y - y64| <= gamma_{K+2} (sum |x||w| + |bias| + |res|): K products in one chain plus the epilogue's one or two additions.  GELU: with the
    bias epilogue's own output x taken as given, |g - gelu64(x)| <= 4u (|x| + |g|).  Guard rows in front of and behind Y and the columns past N
    of a wider Y (ldy > N) keep their sentinels."""
    from cosa_amd import nn_ops
    dev = _dev()
    x, w, b, res = _gemm_inputs(M, N, K)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    buf = torch.full((M + 2, N + pad), SENT, device=dev)
    out = buf[1:M + 1, :N]
    if epi == 2:
        out.copy_(res.to(dev))
        nn_ops.gemm_f32(xd, wd, bd, M, N, K, nn_ops.EPI_RESIDUAL, residual=out, out=out)          # in place
    else:
        nn_ops.gemm_f32(xd, wd, bd, M, N, K, nn_ops.EPI_BIAS, out=out)
    y = out.cpu()
    assert bool((buf[0] == SENT).all()) and bool((buf[M + 1] == SENT).all()) and bool((buf[:, N:] == SENT).all())
    y64 = x.double() @ w.double().t() + b.double() + (res.double() if epi == 2 else 0)
    mag = x.abs().double() @ w.abs().double().t() + b.abs().double() + (res.abs().double() if epi == 2 else 0)
    err = (y.double() - y64).abs()
    worst = float((err / (gamma(K + 2) * mag)).max())
    ref32 = x @ w.t() + b + (res if epi == 2 else 0)                                           # torch's fp32 on the CPU
    e_ref = float((ref32.double() - y64).abs().max())
    record(f"gemm M={M} N={N} K={K} epi={epi}", f"max_err={float(err.max()):.3e} of_bound={worst:.3f} ref_fp32_max_err={e_ref:.3e} "
           f"ratio_to_ref={float(err.max()) / max(e_ref, 1e-30):.2f}")
    assert worst <= 1.0, worst
    if epi == 1:
        g = nn_ops.gemm_f32(xd, wd, bd, M, N, K, nn_ops.EPI_GELU).cpu()
        g64 = F.gelu(y.double())
        gw = float(((g.double() - g64).abs() / (4 * U * (y.abs().double() + g.abs().double()) + 1e-300)).max())
        record(f"gemm gelu M={M} N={N} K={K}", f"of_bound={gw:.3f}")
        assert gw <= 1.0, gw


def test_gemm_f32_rows_do_not_see_each_other():
    """row r of an M-row call == the same row run alone == the same row at another index of another call, bit for bit; two runs are identical;
    NaN and 6e4 in the other rows leave it unchanged"""
    from cosa_amd import nn_ops
    dev = _dev()
    M, N, K = 300, 768, 768
    x, w, b, _ = _gemm_inputs(M, N, K, seed=10)
    xd, wd, bd = x.to(dev), w.to(dev), b.to(dev)
    for epi in (nn_ops.EPI_BIAS, nn_ops.EPI_GELU):
        full = nn_ops.gemm_f32(xd, wd, bd, M, N, K, epi)
        assert _bits_equal(full, nn_ops.gemm_f32(xd, wd, bd, M, N, K, epi))
        for r in (0, 131, 255, 299):
            alone = nn_ops.gemm_f32(xd[r:r + 1].contiguous(), wd, bd, 1, N, K, epi)
            assert _bits_equal(alone[0], full[r]), (epi, r)
            other = torch.zeros((200, K), device=dev)
            other[137] = xd[r]
            assert _bits_equal(nn_ops.gemm_f32(other, wd, bd, 200, N, K, epi)[137], full[r]), (epi, r)
            poisoned = xd.clone()
            poisoned[:r:2] = float("nan")
            poisoned[1:r:2] = 6e4
            poisoned[r + 1::2] = float("nan")
            poisoned[r + 2::2] = 6e4
            assert _bits_equal(nn_ops.gemm_f32(poisoned, wd, bd, M, N, K, epi)[r], full[r]), (epi, r)


def test_gemm_f32_refuses_what_it_does_not_cover():
    from cosa_amd import _C
    dev = _dev()
    x, w, b = torch.ones((8, 64), device=dev), torch.ones((64, 64), device=dev), torch.ones(64, device=dev)
    y = torch.full((8, 64), SENT, device=dev)
    call = lambda X, W, Y, M, N, K, epi=0, res=None: _C.lib().cosa_gemm_f32(_C.ptr(X), _C.ptr(W), _C.ptr(b), _C.ptr(res), _C.ptr(Y), M, N, K, 64, 64, 64, 64,
                                                                            epi, _C.stream_ptr())
    assert call(x, w, y, 8, 64, 24) != 0 and call(x, w, y, 8, 32, 64) != 0 and call(x, w, y, 0, 64, 64) != 0          # K % 16, N % 64, M >= 1
    assert call(None, w, y, 8, 64, 64) != 0 and call(x, None, y, 8, 64, 64) != 0 and call(x, w, None, 8, 64, 64) != 0
    assert call(x, w, y, 8, 64, 64, epi=2) != 0 and call(x, w, y, 8, 64, 64, epi=3) != 0                               # residual missing; no such epilogue
    torch.cuda.synchronize()
    assert bool((y == SENT).all())
    assert call(x, w, y, 8, 64, 64) == 0 and bool((y == 65.0).all())


# ---- attention ------------------------------------------------------------------------------------------------------------------------
ATTN_CASES = [(2, 1, 12, "plain"), (1, 25, 12, "plain"), (2, 197, 12, "plain"), (1, 785, 2, "plain"), (1, 1765, 1, "sharp")]


def _attn_inputs(B, N, H, kind, seed=20):
    qkv = _randn(B, N, 3, H, 64, seed=seed)
    if kind == "sharp":          # scores up to ~10, and one query whose softmax is a single key
        qkv[:, :, :2] *= 2.0 ** 0.5
        k0 = qkv[0, N // 3, 1, 0]
        qkv[0, 7, 0, 0] = k0 * (30.0 / (0.125 * float(k0 @ k0)))
    return qkv


def _attn_ref(qkv, dtype):
    """models/vit/vit.py:128-134 in `dtype` on the CPU -> [B, N, H*64]"""
    B, N, _, H, hd = qkv.shape
    q, k, v = qkv.to(dtype).permute(2, 0, 3, 1, 4)
    attn = (q @ k.transpose(-2, -1)) * hd ** -0.5
    return (attn.softmax(dim=-1) @ v).transpose(1, 2).reshape(B, N, H * hd)


def _attn_hip(qkv):
    from cosa_amd import nn_ops
    B, N, _, H, hd = qkv.shape
    q2 = qkv.reshape(B * N, 3 * H * hd).to(_dev())
    buf = torch.full((B * N + 2, H * hd), SENT, device=_dev())
    nn_ops.attn_fwd_f32(q2, B, N, H, buf[1:B * N + 1])
    assert bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all())
    return buf[1:B * N + 1].view(B, N, H * hd)


@pytest.mark.parametrize("B,N,H,kind", ATTN_CASES)
def test_attn_f32_vs_float64_and_vs_the_reference_arithmetic(B, N, H, kind):
    """per (b, h) slice: the worst-case bound |delta| <= [2 gamma_{N+2} + 2 (gamma_66 S + 4u)] max|v| with S = max scale sum_d |q_d||k_jd|
    (numerator and denominator are chains of length N; a score error d perturbs exp by e^d - 1), and the slice's RMS error <= 10 x that of
    torch's fp32 evaluation of the reference expression on the CPU (floor u max|out|)."""
    qkv = _attn_inputs(B, N, H, kind)
    out = _attn_hip(qkv).cpu()
    o64, o32 = _attn_ref(qkv, torch.float64), _attn_ref(qkv, torch.float32)
    worst_b, worst_r = 0.0, 0.0
    for b in range(B):
        for h in range(H):
            q, k, v = (qkv[b, :, i, h].double() for i in range(3))
            S = float((q.abs() @ k.abs().t()).max()) * 0.125
            bound = (2 * gamma(N + 2) + 2 * (gamma(66) * S + 4 * U)) * float(v.abs().max())
            sl = slice(64 * h, 64 * h + 64)
            d = (out[b, :, sl].double() - o64[b, :, sl])
            dref = (o32[b, :, sl].double() - o64[b, :, sl])
            rms, rms_ref = float(d.pow(2).mean().sqrt()), float(dref.pow(2).mean().sqrt())
            floor = U * float(o64[b, :, sl].abs().max())
            worst_b = max(worst_b, float(d.abs().max()) / bound)
            worst_r = max(worst_r, rms / max(10 * rms_ref, floor))
    record(f"attn B={B} N={N} H={H} {kind}", f"worst_of_bound={worst_b:.4f} rms_over_10x_ref_rms={worst_r:.3f}")
    assert worst_b <= 1.0, worst_b
    assert worst_r <= 1.0, worst_r
    if N == 1:          # softmax of one key is 1: the output is v
        assert _bits_equal(out, qkv[:, :, 2].reshape(B, N, H * 64))


def test_attn_f32_slices_do_not_see_each_other():
    """a (batch, head) slice computed alone, and with NaN in every other slice, has the bits it has inside the full call; two runs are identical"""
    B, N, H = 2, 197, 12
    qkv = _attn_inputs(B, N, H, "plain", seed=21)
    full = _attn_hip(qkv)
    assert _bits_equal(full, _attn_hip(qkv))
    for b, h in ((0, 0), (1, 5), (1, 11)):
        alone = _attn_hip(qkv[b:b + 1, :, :, h:h + 1].contiguous())
        assert _bits_equal(alone[0], full[b, :, 64 * h:64 * h + 64]), (b, h)
        poisoned = torch.full_like(qkv, float("nan"))
        poisoned[b, :, :, h] = qkv[b, :, :, h]
        assert _bits_equal(_attn_hip(poisoned)[b, :, 64 * h:64 * h + 64], full[b, :, 64 * h:64 * h + 64]), (b, h)


def test_attn_f32_refuses_what_it_does_not_cover():
    from cosa_amd import _C
    dev = _dev()
    qkv, out = torch.ones((4, 192), device=dev), torch.full((4, 64), SENT, device=dev)
    call = lambda Q, O, B, N, H, hd=64, ldq=192, ldo=64: _C.lib().cosa_attn_fwd_f32(_C.ptr(Q), _C.ptr(O), B, N, H, hd, 0.125, ldq, ldo, _C.stream_ptr())
    assert call(None, out, 1, 4, 1) != 0 and call(qkv, None, 1, 4, 1) != 0 and call(qkv, out, 1, 4, 1, hd=32) != 0
    assert call(qkv, out, 1, 0, 1) != 0 and call(qkv, out, 1, 4, 1, ldq=128) != 0 and call(qkv, out, 1, 4, 1, ldo=32) != 0
    torch.cuda.synchronize()
    assert bool((out == SENT).all())
    assert call(qkv, out, 1, 4, 1) == 0 and bool((out == 1.0).all())


# ---- LayerNorm ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 394])
def test_layernorm_f32out_has_the_bits_of_the_x3_by_product(rows):
    from cosa_amd import nn_ops
    dev = _dev()
    x = _randn(rows, 768, seed=30, scale=3.0).to(dev) + 0.5
    g, b = (_randn(768, seed=31) * 0.2 + 1).to(dev), _randn(768, seed=32, scale=0.1).to(dev)
    split = torch.empty((rows, nn_ops.split_ld(768)), device=dev, dtype=torch.float16)
    _, want = nn_ops.layernorm_split(x, g, b, 1e-6, out=split, want_f32=True)
    buf = torch.full((rows + 2, 768), SENT, device=dev)
    got = nn_ops.layernorm_f32out(x, g, b, 1e-6, out=buf[1:rows + 1])
    assert _bits_equal(got, want) and bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all())
    ref = F.layer_norm(x.double().cpu(), (768,), g.double().cpu(), b.double().cpu(), 1e-6)
    assert float((got.cpu().double() - ref).abs().max()) <= 1e-5


# ---- token assembly ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 8])
def test_f32_token_im2col_and_patch_projection(P):
    """both built backbones (K = 768 and K = 192): the token-shaped fp32 im2col is an exact copy (images, then their mirror images; class-token
    rows untouched), and the patch projection through the residual epilogue, in place, keeps the chain bound"""
    from cosa_amd import _C, nn_ops
    dev = _dev()
    B, C, H, W, D = 2, 3, 2 * P, 3 * P, 768
    h, w, K = H // P, W // P, C * P * P
    x = _randn(B, C, H, W, seed=40)
    rows = torch.full((2 * B * (h * w + 1), K), SENT, device=dev)
    _C.check(_C.lib().cosa_im2col_flip_f32_tokens(_C.ptr(x.to(dev)), _C.ptr(rows), B, C, H, W, P, 2, 1, _C.stream_ptr()), "im2col")
    xx = torch.cat([x, x.flip(-1)], 0)
    want = xx.reshape(2 * B, C, h, P, w, P).permute(0, 2, 4, 1, 3, 5).reshape(2 * B, h * w, K)
    got = rows.view(2 * B, h * w + 1, K).cpu()
    assert bool((got[:, 0] == SENT).all()) and _bits_equal(got[:, 1:], want)
    rows.view(2 * B, h * w + 1, K)[:, 0] = 0
    wgt, bias = _randn(D, K, seed=41, scale=0.05), _randn(D, seed=42)
    stream = _randn(rows.shape[0], D, seed=43)
    xr = stream.to(dev)
    nn_ops.gemm_f32(rows, wgt.to(dev), bias.to(dev), rows.shape[0], D, K, nn_ops.EPI_RESIDUAL, residual=xr, out=xr)
    r64 = rows.cpu().double()
    y64 = r64 @ wgt.double().t() + bias.double() + stream.double()
    mag = r64.abs() @ wgt.abs().double().t() + bias.abs().double() + stream.abs().double()
    assert float(((xr.cpu().double() - y64).abs() / (gamma(K + 2) * mag)).max()) <= 1.0


# ---- decoder convolutions ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(6, 4), (7, 5)])
def test_conv3x3_dilated_f32_vs_float64_and_batch_invariance(h, w):
    """LargeFOV conv6 geometry (768 -> 512, dilation 5, zero padding, ReLU) on the token view the network hands it (class-token rows in between):
    |y - y64| <= gamma_{9 Cin + 2} sum |x||w|; an image alone has the bits it has inside the batch"""
    from cosa_amd import nn_ops
    dev = _dev()
    B, Cin, Cout, d = 2, 768, 512, 5
    tokens = _randn(B, h * w + 1, Cin, seed=50)
    wgt = _randn(Cout, Cin, 3, 3, seed=51, scale=0.02)
    tok = tokens.to(dev)[:, 1:]
    y = nn_ops.conv3x3_dilated_f32(tok, wgt.to(dev), B, h, w, d, relu=True).view(B, h * w, Cout)
    x64 = tokens[:, 1:].double().transpose(1, 2).reshape(B, Cin, h, w)
    y64 = F.relu(F.conv2d(x64, wgt.double(), padding=d, dilation=d)).flatten(2).transpose(1, 2)
    mag = F.conv2d(x64.abs(), wgt.abs().double(), padding=d, dilation=d).flatten(2).transpose(1, 2)
    err = (y.cpu().double() - y64).abs()
    worst = float((err / (gamma(9 * Cin + 2) * mag)).max())
    y32 = F.relu(F.conv2d(x64.float(), wgt, padding=d, dilation=d)).flatten(2).transpose(1, 2)
    e_ref = float((y32.double() - y64).abs().max())
    record(f"conv h={h} w={w} Cin={Cin} Cout={Cout}", f"max_err={float(err.max()):.3e} of_bound={worst:.3f} ref_fp32_max_err={e_ref:.3e} "
           f"ratio_to_ref={float(err.max()) / max(e_ref, 1e-30):.2f}")
    assert worst <= 1.0, worst
    assert float(y.min()) >= 0.0
    for b in range(B):
        alone = nn_ops.conv3x3_dilated_f32(tok[b:b + 1].contiguous(), wgt.to(dev), 1, h, w, d, relu=True)
        assert _bits_equal(alone, y[b]), b
    lin = nn_ops.conv3x3_dilated_f32(tok, wgt.to(dev), B, h, w, d, relu=False).view(B, h * w, Cout)
    assert torch.equal(torch.clamp_min(lin, 0), y) and float(lin.min()) < 0.0          # (values: a -0 of the chain is +0 after ReLU)
