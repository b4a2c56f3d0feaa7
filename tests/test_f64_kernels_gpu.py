"""The kernels of the "f64" operand family (csrc/f64_kernels.hip) one by one: derived error bounds against a numpy
longdouble evaluation (u = 2^-53, gamma_n = n u / (1 - n u)), the bit-for-bit independence the numerics contract promises, the argument
envelope, and -- where the bound cannot be derived in one line -- the rule `distance of the f64 kernel <= 64 x 2^-29 x distance of its fp32
counterpart`, both measured against the same high-precision reference on the same inputs: 2^-29 is the ratio of the unit roundoffs, the 64 x
is for different association orders and the exp / erf implementations.  The yardstick is the existing fp32 kernel, never the kernel under
test.  Every measured ratio goes on record in profiles/fp64_teacher_parity.txt: one line per case, replaced by the next run's."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "profiles", "fp64_teacher_parity.txt")
U = 2.0 ** -53
RULE = 64 * 2.0 ** -29
SENT = -12345.5          # sentinel value: exactly representable, never a result
LD = np.longdouble


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


def _randn(*shape, seed, scale=1.0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=dtype) * scale


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float64 and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _ld(t):
    return t.detach().cpu().double().numpy().astype(LD)


# ---- GEMM ---------------------------------------------------------------------------------------------------------------------------
GEMM_NK = [(64, 16), (192, 192), (2304, 768), (768, 3072)]
GEMM_M = (1, 17, 129, 300)
_GEMM_REF = {}


def _gemm_case(N, K, wdt):
    """inputs of 300 rows and their longdouble products, once per (N, K, weight type): a row's result does not depend on M, so the first M
    rows serve every M"""
    key = (N, K, wdt)
    if key not in _GEMM_REF:
        x, res = _randn(300, K, seed=K), _randn(300, N, seed=K + 3)
        w, b = _randn(N, K, seed=K + 1, scale=0.05).to(wdt), _randn(N, seed=K + 2).to(wdt)
        v = _ld(x) @ _ld(w).T + _ld(b)
        mag = x.abs() @ w.double().abs().t() + b.double().abs()
        _GEMM_REF[key] = (x, w, b, res, v, mag.numpy())
    return _GEMM_REF[key]


@pytest.mark.parametrize("wdt", [torch.float32, torch.float64], ids=["w32", "w64"])
@pytest.mark.parametrize("N,K", GEMM_NK)
def test_gemm_f64_within_the_derived_bound_of_longdouble(N, K, wdt):
    """|y - y_ld| <= gamma_{K+2} (sum |x||w| + |bias| + |res|): K products into one accumulator (any order) plus the epilogue's one or two
    additions.  GELU: with the bias epilogue's own output v taken as given, |g - gelu(v)| <= 8u |v| (gelu(v) = v/2 erfc(-v / sqrt 2) evaluated by
    mpmath-free float64 erfc, which has no cancellation: 3u |v| of the 8).  Padded strides on X, W and Y; guard rows and the columns past N
    keep their sentinels; fp32 weights (the masters, widened in the kernel) and float64 weights."""
    from cosa_amd import nn_ops
    dev = _dev()
    x, w, b, res, v_ld, mag = _gemm_case(N, K, wdt)
    xp = torch.zeros((300, K + 6), dtype=torch.float64)
    xp[:, :K] = x
    wp = torch.full((N, K + 8), 7.0, dtype=wdt)          # (the padding is never read: it would show)
    wp[:, :K] = w
    xd, wd, bd = xp.to(dev)[:, :K], wp.to(dev)[:, :K], b.to(dev)
    worst = {0: 0.0, 1: 0.0, 2: 0.0}
    for M in GEMM_M:
        for epi in (0, 1, 2):
            buf = torch.full((M + 2, N + 10), SENT, device=dev, dtype=torch.float64)
            out = buf[1:M + 1, :N]
            if epi == 2:
                out.copy_(res[:M].to(dev))
                nn_ops.gemm_f64(xd, wd, bd, M, N, K, nn_ops.EPI_RESIDUAL, residual=out, out=out)          # in place
            else:
                nn_ops.gemm_f64(xd, wd, bd, M, N, K, epi, out=out)
            y = out.cpu()
            assert bool((buf[0] == SENT).all()) and bool((buf[M + 1] == SENT).all()) and bool((buf[:, N:] == SENT).all()), (M, epi)
            if epi == 1:
                lin = nn_ops.gemm_f64(xd, wd, bd, M, N, K, 0).cpu()
                g64 = 0.5 * lin * torch.special.erfc(-lin * 0.70710678118654752440)
                worst[1] = max(worst[1], float(((y - g64).abs() / (8 * U * lin.abs() + 1e-300)).max()))
                continue
            ref = v_ld[:M] + (_ld(res[:M]) if epi == 2 else 0)
            bound = gamma(K + 2) * (mag[:M] + (res[:M].abs().numpy() if epi == 2 else 0))
            worst[epi] = max(worst[epi], float((np.abs(y.numpy().astype(LD) - ref) / bound).max()))
    record(f"gemm N={N} K={K} {'w32' if wdt == torch.float32 else 'w64'}", f"of_bound bias={worst[0]:.4f} gelu={worst[1]:.4f} residual={worst[2]:.4f}")
    assert max(worst.values()) <= 1.0, worst


def test_gemm_f64_head_width_and_conv_vs_float64_torch():
    """N = 21 (a head width taken directly: columns past N guarded) and the LargeFOV conv6 geometry (768 -> 512, dilation 5, ReLU) at h = w = 5
    and 9 on the token view the network hands it (class-token rows in between), against float64 torch on the CPU by the same derived bounds
    (the torch sum is itself within gamma_K of exact: 2 gamma); an image alone has the bits it has inside the batch; padded taps are zeros"""
    from cosa_amd import nn_ops
    dev = _dev()
    x, w = _randn(130, 768, seed=60), _randn(21, 768, seed=61, scale=0.05).float()
    y = nn_ops.gemm_f64(x.to(dev), w.to(dev), None, 130, 21, 768).cpu()
    y64, mag = x @ w.double().t(), x.abs() @ w.double().abs().t()
    worst = float(((y - y64).abs() / (2 * gamma(770) * mag)).max())
    record("gemm head N=21 K=768", f"of_bound={worst:.4f}")
    assert worst <= 1.0
    B, Cin, Cout, d = 2, 768, 512, 5
    wgt = _randn(Cout, Cin, 3, 3, seed=51, scale=0.02).float()
    for hw in (5, 9):
        tokens = _randn(B, hw * hw + 1, Cin, seed=50 + hw)
        tok = tokens.to(dev)[:, 1:]
        y = nn_ops.conv3x3_dilated_f64(tok, wgt.to(dev), B, hw, hw, d, relu=True).view(B, hw * hw, Cout)
        x64 = tokens[:, 1:].transpose(1, 2).reshape(B, Cin, hw, hw)
        y64 = F.relu(F.conv2d(x64, wgt.double(), padding=d, dilation=d)).flatten(2).transpose(1, 2)
        mag = F.conv2d(x64.abs(), wgt.double().abs(), padding=d, dilation=d).flatten(2).transpose(1, 2)
        worst = float(((y.cpu() - y64).abs() / (2 * gamma(9 * Cin + 2) * mag)).max())
        record(f"conv h=w={hw} Cin={Cin} Cout={Cout}", f"of_bound={worst:.4f}")
        assert worst <= 1.0 and float(y.min()) >= 0.0
        for b in range(B):
            alone = nn_ops.conv3x3_dilated_f64(tok[b:b + 1].contiguous(), wgt.to(dev), 1, hw, hw, d, relu=True)
            assert _bits_equal(alone, y[b]), (hw, b)
    # h = w = 5 with dilation 5: every tap but the centre is padding -> the conv IS the centre tap's 1x1 GEMM, bit for bit (exact zeros added)
    tokens = _randn(1, 26, Cin, seed=55).to(dev)
    lin = nn_ops.conv3x3_dilated_f64(tokens[:, 1:], wgt.to(dev), 1, 5, 5, d, relu=False)
    centre = nn_ops.gemm_f64(tokens[0, 1:], wgt[:, :, 1, 1].contiguous().to(dev), None, 25, Cout, Cin)
    assert _bits_equal(lin, centre)


def test_gemm_f64_rows_do_not_see_each_other():
    """row r of an M-row call == the same row run alone == the same row at another index of another call, bit for bit; two runs are identical;
    NaN and 1e300 in the other rows leave it unchanged"""
    from cosa_amd import nn_ops
    dev = _dev()
    M, N, K = 300, 768, 768
    x, w, b = _randn(M, K, seed=10).to(dev), _randn(N, K, seed=11, scale=0.05).float().to(dev), _randn(N, seed=12).float().to(dev)
    for epi in (nn_ops.EPI_BIAS, nn_ops.EPI_GELU):
        full = nn_ops.gemm_f64(x, w, b, M, N, K, epi)
        assert torch.isfinite(full).all() and _bits_equal(full, nn_ops.gemm_f64(x, w, b, M, N, K, epi))
        for r in (0, 63, 64, 131, 299):
            alone = nn_ops.gemm_f64(x[r:r + 1].contiguous(), w, b, 1, N, K, epi)
            assert _bits_equal(alone[0], full[r]), (epi, r)
            other = torch.zeros((200, K), device=dev, dtype=torch.float64)
            other[137] = x[r]
            assert _bits_equal(nn_ops.gemm_f64(other, w, b, 200, N, K, epi)[137], full[r]), (epi, r)
            poisoned = x.clone()
            poisoned[:r:2] = float("nan")
            poisoned[1:r:2] = 1e300
            poisoned[r + 1::2] = float("nan")
            poisoned[r + 2::2] = 1e300
            assert _bits_equal(nn_ops.gemm_f64(poisoned, w, b, M, N, K, epi)[r], full[r]), (epi, r)


def test_f64_kernels_refuse_what_they_do_not_cover():
    """null pointers, K outside the envelope, M = 0, a missing residual, head_dim != 64, N = 0: a status, and the sentinel-filled outputs untouched"""
    from cosa_amd import _C
    dev = _dev()
    L = _C.lib()
    x, w, b = (torch.ones(s, device=dev, dtype=torch.float64) for s in ((8, 64), (64, 64), (64,)))
    y = torch.full((8, 64), SENT, device=dev, dtype=torch.float64)
    gemm = lambda X, W, Y, M, N, K, epi=0, res=None, ldx=64: L.cosa_gemm_f64(_C.ptr(X), _C.ptr(W), _C.ptr(b), _C.ptr(res), _C.ptr(Y), M, N, K, ldx, 64, 64,
                                                                             64, epi, 0, _C.stream_ptr())
    assert gemm(x, w, y, 8, 64, 24) != 0 and gemm(x, w, y, 8, 64, 0) != 0 and gemm(x, w, y, 0, 64, 64) != 0 and gemm(x, w, y, 8, 0, 64) != 0
    assert gemm(None, w, y, 8, 64, 64) != 0 and gemm(x, None, y, 8, 64, 64) != 0 and gemm(x, w, None, 8, 64, 64) != 0
    assert gemm(x, w, y, 8, 64, 64, epi=2) != 0 and gemm(x, w, y, 8, 64, 64, epi=3) != 0 and gemm(x, w, y, 8, 64, 64, ldx=48) != 0
    conv = lambda T, Cin: L.cosa_conv3x3_dilated_f64(_C.ptr(T), _C.ptr(w), _C.ptr(y), 1, 2, 2, Cin, 8, 5, 4, 64, 1, 0, _C.stream_ptr())
    assert conv(None, 64) != 0 and conv(x, 24) != 0
    qkv, out = torch.ones((4, 192), device=dev, dtype=torch.float64), torch.full((4, 64), SENT, device=dev, dtype=torch.float64)
    attn = lambda Q, O, B, N, H, hd=64, ldq=192, ldo=64: L.cosa_attn_fwd_f64(_C.ptr(Q), _C.ptr(O), B, N, H, hd, 0.125, ldq, ldo, _C.stream_ptr())
    assert attn(None, out, 1, 4, 1) != 0 and attn(qkv, None, 1, 4, 1) != 0 and attn(qkv, out, 1, 4, 1, hd=32) != 0
    assert attn(qkv, out, 1, 0, 1) != 0 and attn(qkv, out, 1, 4, 1, ldq=128) != 0 and attn(qkv, out, 1, 4, 1, ldo=32) != 0
    g32 = torch.ones(64, device=dev)
    assert L.cosa_layernorm_f64(_C.ptr(x), _C.ptr(g32), None, _C.ptr(y), 8, 64, 1e-6, _C.stream_ptr()) != 0
    assert L.cosa_layernorm_f64(_C.ptr(x), _C.ptr(g32), _C.ptr(g32), _C.ptr(y), 0, 64, 1e-6, _C.stream_ptr()) != 0
    assert L.cosa_im2col_flip_f64_tokens(_C.ptr(x), _C.ptr(y), 1, 1, 8, 8, 3, 1, 0, _C.stream_ptr()) != 0                  # P % 4
    assert L.cosa_resize_bilinear_f64(_C.ptr(g32), None, 1, 8, 8, 4, 4, _C.stream_ptr()) != 0
    assert L.cosa_cam_flip_merge_upsample_f64(_C.ptr(x), _C.ptr(y), 1, 1, 2, 2, 8, 2, 0, None, None, _C.stream_ptr()) != 0  # mode 2
    assert L.cosa_cam_minmax_norm_f64(_C.ptr(y), 0, 64, None, None, _C.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((y == SENT).all()) and bool((out == SENT).all())
    assert gemm(x, w, y, 8, 64, 64) == 0 and bool((y == 65.0).all())
    assert attn(qkv, out, 1, 4, 1) == 0 and bool((out == 1.0).all())


# ---- attention ------------------------------------------------------------------------------------------------------------------------
def _attn_inputs(B, N, H, sharp, seed=20):
    """fp32-representable values, so that the f64 kernel and its fp32 counterpart read the SAME numbers"""
    qkv = _randn(B, N, 3, H, 64, seed=seed, dtype=torch.float32)
    if sharp and N > 2:          # one query whose softmax is a single key: logit +30
        k0 = qkv[0, N // 3, 1, 0]
        qkv[0, 2, 0, 0] = k0 * (30.0 / (0.125 * float(k0 @ k0)))
    return qkv


def _attn_ld(qkv):
    """softmax(q k^T / 8) v in longdouble -> [B, N, H*64]"""
    B, N, _, H, hd = qkv.shape
    a = qkv.double().numpy().astype(LD)
    out = np.zeros((B, N, H * hd), LD)
    for b in range(B):
        for h in range(H):
            q, k, v = a[b, :, 0, h], a[b, :, 1, h], a[b, :, 2, h]
            s = (q @ k.T) * LD(0.125)
            p = np.exp(s - s.max(axis=1, keepdims=True))
            out[b, :, hd * h:hd * h + hd] = (p @ v) / p.sum(axis=1, keepdims=True)
    return out


def _attn_hip(qkv, f64=True):
    from cosa_amd import nn_ops
    B, N, _, H, hd = qkv.shape
    dt = torch.float64 if f64 else torch.float32
    q2 = qkv.reshape(B * N, 3 * H * hd).to(dt).to(_dev())
    buf = torch.full((B * N + 2, H * hd), SENT, device=_dev(), dtype=dt)
    (nn_ops.attn_fwd_f64 if f64 else nn_ops.attn_fwd_f32)(q2, B, N, H, buf[1:B * N + 1])
    assert bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all())
    return buf[1:B * N + 1].view(B, N, H * hd)


@pytest.mark.parametrize("sharp", [False, True], ids=["random", "sharp"])
@pytest.mark.parametrize("N", [1, 5, 33, 64, 197])
def test_attn_f64_vs_longdouble_by_the_fp32_kernels_yardstick(N, sharp):
    """d64 = max |f64 kernel - longdouble| <= 64 x 2^-29 x d32, d32 = max |cosa_attn_fwd_f32 - longdouble| on the same (fp32-representable)
    inputs.  N = 1: the softmax of one key is 1 and the output is v, bit for bit (d32 = 0 there too)."""
    B, H = 2, 3
    qkv = _attn_inputs(B, N, H, sharp)
    ref = _attn_ld(qkv)
    o64 = _attn_hip(qkv).cpu()
    d64 = float(np.abs(o64.numpy().astype(LD) - ref).max())
    d32 = float(np.abs(_attn_hip(qkv, f64=False).cpu().double().numpy().astype(LD) - ref).max())
    record(f"attn B={B} H={H} N={N} {'sharp' if sharp else 'random'}", f"d64={d64:.3e} d32={d32:.3e} ratio_to_rule={d64 / max(RULE * d32, 1e-300):.4f}")
    assert torch.isfinite(o64).all()
    if N == 1:
        assert _bits_equal(o64, qkv[:, :, 2].reshape(B, N, H * 64).double())
    assert d64 <= RULE * d32, (d64, d32)


def test_attn_f64_slices_do_not_see_each_other():
    """a (batch, head) slice computed alone, and with NaN in every other slice, has the bits it has inside the full call; two runs are identical"""
    B, N, H = 2, 197, 3
    qkv = _attn_inputs(B, N, H, False, seed=21).double()
    full = _attn_hip(qkv)
    assert _bits_equal(full, _attn_hip(qkv))
    for b, h in ((0, 0), (1, 1), (1, 2)):
        alone = _attn_hip(qkv[b:b + 1, :, :, h:h + 1].contiguous())
        assert _bits_equal(alone[0], full[b, :, 64 * h:64 * h + 64]), (b, h)
        poisoned = torch.full_like(qkv, float("nan"))
        poisoned[b, :, :, h] = qkv[b, :, :, h]
        assert _bits_equal(_attn_hip(poisoned)[b, :, 64 * h:64 * h + 64], full[b, :, 64 * h:64 * h + 64]), (b, h)


# ---- LayerNorm, token assembly, the tail: float64 torch on the CPU, the fp32 counterpart as the yardstick; exact where the operation is a
# selection or one rounding per element ------------------------------------------------------------------------------------------------
def _by_rule(key, got64, got32, ref64):
    d64, d32 = float((got64.cpu() - ref64).abs().max()), float((got32.cpu().double() - ref64).abs().max())
    record(key, f"d64={d64:.3e} d32={d32:.3e} ratio_to_rule={d64 / max(RULE * d32, 1e-300):.4f}")
    assert torch.isfinite(got64).all() and d32 > 0 and d64 <= RULE * d32, (key, d64, d32)


@pytest.mark.parametrize("rows", [1, 3, 394])
def test_layernorm_f64(rows):
    from cosa_amd import nn_ops
    dev = _dev()
    x = _randn(rows, 768, seed=30, scale=3.0, dtype=torch.float32) + 0.5
    g, b = _randn(768, seed=31, dtype=torch.float32) * 0.2 + 1, _randn(768, seed=32, scale=0.1, dtype=torch.float32)
    buf = torch.full((rows + 2, 768), SENT, device=dev, dtype=torch.float64)
    got = nn_ops.layernorm_f64(x.double().to(dev), g.to(dev), b.to(dev), 1e-6, out=buf[1:rows + 1])
    assert bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all())
    ref = F.layer_norm(x.double(), (768,), g.double(), b.double(), 1e-6)
    _by_rule(f"layernorm rows={rows}", got, nn_ops.layernorm_f32out(x.to(dev), g.to(dev), b.to(dev), 1e-6), ref)


@pytest.mark.parametrize("P", [16, 8])
def test_f64_token_im2col_is_an_exact_copy(P):
    """both built backbones: images, then their mirror images; zero class-token rows stay untouched"""
    from cosa_amd import _C
    dev = _dev()
    B, C, H, W = 2, 3, 2 * P, 3 * P
    h, w, K = H // P, W // P, C * P * P
    x = _randn(B, C, H, W, seed=40)
    rows = torch.full((2 * B * (h * w + 1), K), SENT, device=dev, dtype=torch.float64)
    _C.check(_C.lib().cosa_im2col_flip_f64_tokens(_C.ptr(x.to(dev)), _C.ptr(rows), B, C, H, W, P, 2, 1, _C.stream_ptr()), "im2col")
    xx = torch.cat([x, x.flip(-1)], 0)
    want = xx.reshape(2 * B, C, h, P, w, P).permute(0, 2, 4, 1, 3, 5).reshape(2 * B, h * w, K)
    got = rows.view(2 * B, h * w + 1, K).cpu()
    assert bool((got[:, 0] == SENT).all()) and _bits_equal(got[:, 1:].contiguous(), want.contiguous())


@pytest.mark.parametrize("out", [32, 96])
def test_resize_bilinear_f64(out):
    from cosa_amd.utils import seg_helper
    x = _randn(2, 3, 64, 64, seed=70, dtype=torch.float32)
    got = seg_helper.resize_bilinear_f64(x.to(_dev()), (out, out))
    ref = F.interpolate(x.double(), size=(out, out), mode="bilinear", align_corners=False)
    assert got.dtype == torch.float64
    _by_rule(f"resize 64->{out}", got, seg_helper.resize_bilinear(x.to(_dev()), (out, out)), ref)


@pytest.mark.parametrize("h,S", [(2, 32), (4, 64)])
def test_flip_merge_upsample_f64_and_rawmax(h, S):
    """modes 0 (max of the two un-flipped maps, ReLU) and 1 (sum), accumulation over two calls, the `active` flags (absent planes: zeros); rawmax
    is a selection followed by one addition per call: exact"""
    from cosa_amd.utils import seg_helper
    dev = _dev()
    B, C = 2, 4
    srcs = [_randn(2 * B, C, h, h, seed=80 + i, dtype=torch.float32) for i in range(2)]
    act = torch.tensor([[1, 0, 1, 1], [0, 1, 1, 0]], dtype=torch.float32)
    up = lambda t: F.interpolate(t, size=(S, S), mode="bilinear", align_corners=False)
    for mode in (0, 1):
        for use_act in (False, True):
            a = act.to(dev) if use_act else None
            dst64 = torch.full((B, C, S, S), SENT, device=dev, dtype=torch.float64)
            dst32 = torch.full((B, C, S, S), SENT, device=dev)
            raw = torch.full((B, C), SENT, device=dev, dtype=torch.float64)
            ref, raw_ref = 0, 0
            for i, s in enumerate(srcs):
                seg_helper._flip_merge_upsample_f64(s.double().to(dev), dst64, B, S, mode, i > 0, a, raw)
                seg_helper._flip_merge_upsample(s.to(dev), dst32, B, S, mode, i > 0, a)
                u = up(s.double())
                m = torch.maximum(u[:B], u[B:].flip(-1)).clamp_min(0) if mode == 0 else u[:B] + u[B:].flip(-1)
                ref = ref + m
                raw_ref = raw_ref + torch.maximum(s[:B].double().abs().amax(dim=(2, 3)), s[B:].double().abs().amax(dim=(2, 3)))
            if use_act:
                ref = ref * act[:, :, None, None]
                assert bool((dst64.cpu()[act == 0] == 0).all())
            assert _bits_equal(raw.cpu(), raw_ref)
            _by_rule(f"flip_merge h={h} S={S} mode={mode} active={int(use_act)}", dst64, dst32, ref)


@pytest.mark.parametrize("S", [7, 32])
def test_minmax_norm_f64_and_peak_are_exact(S):
    """(x - min) / (max(x - min) + 1e-5): a selection and one rounding per operation -- the bits of float64 torch; peak = that divisor; absent
    planes are skipped (plane and peak untouched)"""
    from cosa_amd.utils import seg_helper
    dev = _dev()
    x = _randn(2, 3, S, S, seed=90).abs()
    act = torch.tensor([[1, 0, 1], [1, 1, 0]], dtype=torch.float32)
    t = x - x.amin(dim=(2, 3), keepdim=True)
    den = t.amax(dim=(2, 3), keepdim=True) + 1e-5
    for a in (None, act):
        cam, peak = x.clone().to(dev), torch.full((2, 3), SENT, device=dev, dtype=torch.float64)
        seg_helper.cam_minmax_norm_f64_(cam, a.to(dev) if a is not None else None, peak)
        live = torch.ones(2, 3, dtype=torch.bool) if a is None else a.bool()
        assert _bits_equal(cam.cpu()[live], (t / den)[live]) and _bits_equal(peak.cpu()[live], den[:, :, 0, 0][live])
        assert _bits_equal(cam.cpu()[~live], x[~live]) and bool((peak.cpu()[~live] == SENT).all())
