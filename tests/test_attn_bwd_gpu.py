"""Attention backward (cosa_attn_bwd / cosa_attn_bwd_f16: attn_bwd_prep / _dq / _dkv kernels of csrc/attn_kernels.hip) against float64, per
gradient and per (batch, head), in both operand types, with a bar that follows the kernels' own rounding (tests/attn_bwd_ref.py), plus the
exact properties that follow from a backward without atomics and without coupling between (batch, head) groups: slice independence,
neighbouring images that do not leak, linearity in dO, writes that stay inside their buffers, refused arguments.

Parity bar (per slice, per gradient): RMS and maximum of kernel - exact <= 2 x the same figure of model - exact, the maximum with an added
floor of one unit in the last place of the operand type at the slice's max|exact|.  The model has the kernels' rounding points; what it
leaves out (fp32 accumulation order, v_exp_f32 against exp, the folded log2 e) is below 2^-18 relative, so a factor 2 over a figure that
output rounding dominates is out of reach of those and below any indexing, masking or scaling error.  Every case appends its worst
kernel / model ratios to out/attn_bwd_parity.txt, or to the file that COSA_ATTN_BWD_RECORD names; profiles/attn_bwd_parity.txt is a copy of
one full run."""
import functools
import os

import pytest
import torch

import attn_bwd_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.environ.get("COSA_ATTN_BWD_RECORD") or os.path.join(ROOT, "out", "attn_bwd_parity.txt")      # the ratios of the last run
DTYPES = [torch.bfloat16, torch.float16]
COSA_ENOMEM = 4
FACTOR = 2.0


def _ids(dt):
    return "bf16" if dt == torch.bfloat16 else "fp16"


# ---- the kernels through the C ABI ---------------------------------------------------------------------------------------------------------
def _bwd(qkv, out, go, lse, H, dqkv=None, ws=None, ws_bytes=None, head_dim=64, check=True):
    from cosa_amd import _C
    dt = qkv.dtype
    B, N, _ = qkv.shape
    assert out.dtype == dt and go.dtype == dt and lse.dtype == torch.float32
    assert qkv.is_contiguous() and out.is_contiguous() and go.is_contiguous() and lse.is_contiguous()
    need = _C.fn16("cosa_attn_bwd_workspace_bytes", dt)(B, N, H)
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    if ws is None:
        ws = _C.workspace(need, qkv.device, "test_attn_bwd")
    rc = _C.fn16("cosa_attn_bwd", dt)(_C.ptr(qkv), _C.ptr(out), _C.ptr(go), _C.ptr(lse), _C.ptr(dqkv), B, N, H, head_dim, R.SCALE,
                                      _C.ptr(ws), need if ws_bytes is None else ws_bytes, _C.stream_ptr())
    if check:
        _C.check(rc, "cosa_attn_bwd")
        return dqkv
    return rc


def _fwd(qkv, H):
    """the training variant of the forward (flags = 0: keeps LSE)"""
    from cosa_amd import _C
    dt = qkv.dtype
    B, N, _ = qkv.shape
    out = torch.empty((B, N, H * 64), device=qkv.device, dtype=dt)
    lse = torch.empty((B, H, N), device=qkv.device, dtype=torch.float32)
    ws = _C.workspace(_C.fn16("cosa_attn_workspace_bytes", dt)(B, N, H), qkv.device, "test_attn_fwd")
    _C.check(_C.fn16("cosa_attn_fwd", dt)(_C.ptr(qkv), _C.ptr(out), _C.ptr(lse), B, N, H, 64, R.SCALE, 0, None, _C.ptr(ws), ws.numel(),
                                          _C.stream_ptr()), "cosa_attn_fwd")
    return out, lse


def _bits(t):
    return t.contiguous().view(torch.int16)


def _isolated_inputs(B, N, H, dt, seed, **kw):
    """qkv, dO and the exact reference's out / lse in the types the kernel takes"""
    qkv, go = R.draw(B, N, H, dt, seed, **kw)
    _, o, lse = R.exact(qkv, go, H)
    return qkv, go, o.to(dt), lse.float()


# ---- 2. parity ------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(2, 197, 4), (1, 1, 1), (1, 63, 1), (1, 64, 2), (1, 65, 1), (2, 128, 3), (1, 129, 2), (3, 130, 3), (1, 257, 9), (1, 785, 2)]
CASES = [("rand", s, {}) for s in SHAPES] + [("wide", (2, 197, 2), {"scale": 1.5}), ("smalldo", (2, 197, 2), {"go_scale": 0.01}),
                                              ("sharp", (1, 300, 1), {"scale": 0.5, "sharp": True})]


@pytest.fixture(scope="module", autouse=True)
def _record():
    os.makedirs(os.path.dirname(os.path.abspath(RECORD)), exist_ok=True)
    with open(RECORD, "w") as f:
        f.write("# attention backward, kernel error / model error against exact float64 (tests/test_attn_bwd_gpu.py), worst (batch, head) slice\n"
                "# rms = rms(kernel - exact) / rms(model - exact);  max = max|kernel - exact| / (max|model - exact| + ulp(max|exact|) / 2)\n"
                "# N = 1: dq, dk against 2 |model| + 2^-18 of the scale of dS K (exact value 0), dv bit-equal to dO.  The bar is 2 for every figure.\n")
    yield


@functools.lru_cache(maxsize=None)
def _references(name, shape, dt):
    """exact and model gradients of a case, computed once and shared by its isolated and coupled runs; never modified"""
    B, N, H = shape
    kw = dict([c for c in CASES if c[0] == name and c[1] == shape][0][2])
    qkv, go = R.draw(B, N, H, dt, seed=N, **kw)
    ref, o, lse = R.exact(qkv, go, H)
    iso = (o.to(dt), lse.float())
    fo, fl = R.forward_model(qkv, H)
    return qkv, go, ref, iso, R.model(qkv, go, H, *iso), R.model(qkv, go, H, fo.to(dt), fl.float())


def _ratios(g, mod, ref, H, dt):
    """-> [3, 2] worst-slice kernel / model ratios (rms, max) and the list of slices over the bar"""
    k_rms, k_max, scale = R.slice_errors(g, ref, H)
    m_rms, m_max, _ = R.slice_errors(mod, ref, H)
    floor = torch.tensor([[[R.ulp(x, dt) for x in row] for row in part] for part in scale.tolist()], dtype=torch.float64, device=g.device)

    def ratio(k, m):
        return torch.where(k > 0, k / m, torch.zeros_like(k))       # 0 / 0: the kernel is exact where the model is
    r_rms, r_max = ratio(k_rms, m_rms), ratio(k_max, m_max + floor / FACTOR)
    bad = [("dq dk dv".split()[i], b, h, kind, float(r[i, b, h])) for kind, r in (("rms", r_rms), ("max", r_max))
           for i, b, h in (r > FACTOR).nonzero().tolist()]
    return torch.stack([r_rms.amax((1, 2)), r_max.amax((1, 2))], 1), bad


def _note(name, shape, dt, mode, worst, extra=""):
    line = f"{name:8s} B,N,H={shape[0]},{shape[1]},{shape[2]:<3d} {_ids(dt)} {mode:8s} " + "  ".join(
        f"{n} rms {worst[i, 0]:.3f} max {worst[i, 1]:.3f}" for i, n in enumerate(("dq", "dk", "dv"))) + extra
    print(line)
    with open(RECORD, "a") as f:
        f.write(line + "\n")


def _single_token(g, mod, qkv, go, H):
    """N = 1: the softmax is the constant 1.  dV == dO bit for bit; dq and dk are exactly 0 in exact arithmetic, in the kernel
    dS = (dP - delta) / 8 with dP and delta two fp32 sums of the same 64 products in different orders, so |dq|, |dk| are bounded by the
    model's own values (its delta is the fp32 rounding of dP) plus the fp32 accumulation-order term the model leaves out, 2^-18 of the scale
    of dS K, sum|dO v| / 8 x max|k| (x max|q|) -- at max|exact| = 0 an ulp of the operand type is no floor."""
    q, k, v = R.split(qkv.double(), H)
    do = R.heads(go.double(), H)
    dq, dk, dv = R.split(g, H)
    assert torch.equal(_bits(dv), _bits(R.heads(go, H))), "N = 1: dV != dO"
    s = (do.abs() * v.abs()).sum(-1, keepdim=True) * R.SCALE * 2.0 ** -18
    worst, seen = torch.zeros(3, 2, dtype=torch.float64), ""
    mq, mk, _ = R.split(mod, H)
    for i, (got, m, other) in enumerate(((dq, mq, k), (dk, mk, q))):
        bound = FACTOR * m.abs().amax(-1, keepdim=True) + s * other.abs().amax(-1, keepdim=True)
        r = (got.double().abs().amax(-1, keepdim=True) / bound).max().item() * FACTOR      # on the file's scale: the bar is 2
        worst[i] = r
        seen += f"  max|d{'qk'[i]}| kernel {got.double().abs().max().item():.3e} model {m.abs().max().item():.3e} order term {(bound - FACTOR * m.abs().amax(-1, keepdim=True)).max().item():.3e}"
        assert r <= FACTOR, (i, r, seen)
    return worst, seen


@pytest.mark.parametrize("mode", ["isolated", "coupled"])
@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
@pytest.mark.parametrize("name,shape", [(c[0], c[1]) for c in CASES], ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}x{c[1][2]}" for c in CASES])
def test_backward_parity_per_gradient_and_slice(name, shape, dt, mode):
    """kernel - exact against model - exact, per gradient and per (batch, head): RMS and maximum within 2 x the model's, the maximum with a
    floor of one ulp of the operand type at the slice's max|exact|.  isolated: out / lse from the exact reference (rounded); coupled: from
    the project's own forward (bf16: through nn_ops.attention(...).backward(...)), the model then carries the forward's rounding points."""
    from cosa_amd import nn_ops
    B, N, H = shape
    qkv, go, ref, iso, mod_iso, mod_cpl = _references(name, shape, dt)
    if mode == "isolated":
        g, mod = _bwd(qkv, iso[0], go, iso[1], H), mod_iso
    elif dt == torch.bfloat16:
        x = qkv.clone().requires_grad_(True)
        nn_ops.attention(x, H).backward(go)
        g, mod = x.grad, mod_cpl
    else:
        out, lse = _fwd(qkv, H)
        g, mod = _bwd(qkv, out, go, lse, H), mod_cpl
    torch.cuda.synchronize()
    assert torch.isfinite(g).all()
    if N == 1:
        _note(name, shape, dt, mode, *_single_token(g, mod, qkv, go, H))
        return
    worst, bad = _ratios(g, mod, ref, H, dt)
    _note(name, shape, dt, mode, worst)
    assert not bad, bad[:8]


# ---- 3. exact properties --------------------------------------------------------------------------------------------------------------------
def _slice_of(t, b, h, H, parts):
    """(b, h) of a [B,N,parts*H*64] tensor as a contiguous [1,N,parts*64] one"""
    B, N, _ = t.shape
    return t.view(B, N, parts, H, 64)[b:b + 1, :, :, h].reshape(1, N, parts * 64).contiguous()


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_slices_are_independent(dt):
    """(B, H) = (3, 5), N = 130: every (batch, head) slice of the big run -- dq, dk, dv, and the training forward's out and lse -- equals the
    run of that slice alone as (1, N, 1) bit for bit: the workgroup -> (block, batch, head) map, the row strides and the per-image ranges"""
    B, N, H = 3, 130, 5
    qkv, go, o, lse = _isolated_inputs(B, N, H, dt, seed=5)
    g = _bwd(qkv, o, go, lse, H).clone()
    fo, fl = _fwd(qkv, H)
    for b in range(B):
        for h in range(H):
            q1, o1, go1, lse1 = _slice_of(qkv, b, h, H, 3), _slice_of(o, b, h, H, 1), _slice_of(go, b, h, H, 1), lse[b:b + 1, h:h + 1].contiguous()
            g1 = _bwd(q1, o1, go1, lse1, 1)
            assert torch.equal(_bits(_slice_of(g, b, h, H, 3)), _bits(g1)), (b, h)
            fo1, fl1 = _fwd(q1, 1)
            assert torch.equal(_bits(_slice_of(fo, b, h, H, 1)), _bits(fo1)), (b, h)
            assert torch.equal(fl[b:b + 1, h:h + 1].view(torch.int32), fl1.view(torch.int32)), (b, h)


@pytest.mark.parametrize("fill", [float("nan"), 6e4], ids=["nan", "6e4"])
@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_neighbouring_images_do_not_leak(dt, fill):
    """B = 3, N = 65 (a one-row tail tile: the range-checked LDS-DMA reads 63 rows past image 1's last one), images 0 and 2 filled with NaN
    (then with +-6e4) in qkv, out, dO and lse: image 1's gradients equal its B = 1 run bit for bit and are finite"""
    B, N, H = 3, 65, 2
    qkv, go, o, lse = _isolated_inputs(B, N, H, dt, seed=65)
    alone = _bwd(qkv[1:2].contiguous(), o[1:2].contiguous(), go[1:2].contiguous(), lse[1:2].contiguous(), H).clone()
    for t in (qkv, go, o, lse):
        for b in (0, 2):
            t[b] = fill
            if fill == fill:
                t[b].view(-1)[1::2] = -fill
    g = _bwd(qkv, o, go, lse, H)
    assert torch.isfinite(g[1]).all()
    assert torch.equal(_bits(g[1]), _bits(alone[0]))


# seeds of the linearity draws (fp16: the first of 0, 1, 2, ... that meets _linear_draw's condition; bf16 meets it at once)
LINEAR_SEEDS = {(torch.bfloat16, 197): 0, (torch.bfloat16, 64): 0, (torch.float16, 197): 3, (torch.float16, 64): 0}


def _linear_draw(B, N, H, dt):
    """a draw on which scaling dO by 2 commutes with every rounding of the backward: by the float64 model, no dS and no result of dO is a
    non-zero value below the operand type's smallest normal one (1 % margin: the kernel's fp32 dS is within 1e-6 of the model's), and
    none of 2 dO reaches its largest value.  fp16 needs dO at 2^12 for that (dS = P (dP - delta) / 8 sits near 2^-8 at unit scale) and,
    as values close to zero always occur, a seed that has none inside the band: LINEAR_SEEDS.  The condition is asserted, so a change
    of the draw shows here and not as a failed bit comparison."""
    tiny, big = (2.0 ** -125, 1e38) if dt == torch.bfloat16 else (1.01 * 2.0 ** -14, 6e4)
    qkv, go, o, lse = _isolated_inputs(B, N, H, dt, LINEAR_SEEDS[dt, N], go_scale=1.0 if dt == torch.bfloat16 else 4096.0)
    g, ds = R.model(qkv, go, H, o, lse, parts=True)
    for x in (ds, g, go.double()):
        assert x[x != 0].abs().min() >= tiny and 2 * x.abs().max() <= big, "the pinned seed no longer keeps the draw in the normal range"
    return qkv, go, o, lse


@pytest.mark.parametrize("B,N,H", [(2, 197, 3), (1, 64, 1)])
@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_backward_is_linear_in_dout(dt, B, N, H):
    """bwd(2 dO) == 2 bwd(dO) bit for bit (a power of two commutes with every rounding while nothing leaves the normal range: _linear_draw),
    and bwd(0) is all +0 / -0"""
    qkv, go, o, lse = _linear_draw(B, N, H, dt)
    g1 = _bwd(qkv, o, go, lse, H).clone()
    g2 = _bwd(qkv, o, go * 2, lse, H).clone()
    assert torch.isfinite(g2).all()
    assert torch.equal(_bits(g1 * 2), _bits(g2))
    g0 = _bwd(qkv, o, torch.zeros_like(go), lse, H)
    assert ((_bits(g0) & 0x7fff) == 0).all()


def _guarded(n_inner, row, dtype, device, sentinel, rows=4):
    """a buffer of n_inner elements between `rows` sentinel rows of `row` elements each -> (whole, inner view)"""
    whole = torch.full((2 * rows * row + n_inner,), sentinel, dtype=dtype, device=device)
    return whole, whole[rows * row:rows * row + n_inner]


@pytest.mark.parametrize("B,N,H", [(2, 129, 3), (1, 1, 1)])
@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_writes_stay_inside(dt, B, N, H):
    """dqkv and the workspace are views into larger buffers, sentinel rows before and after, the interior pre-filled with NaN: afterwards
    the sentinels are intact, every element of dqkv is finite and so is every delta the workspace holds"""
    from cosa_amd import _C
    qkv, go, o, lse = _isolated_inputs(B, N, H, dt, seed=11)
    row = 3 * H * 64
    whole, inner = _guarded(B * N * row, row, dt, qkv.device, 1024.0)
    inner.fill_(float("nan"))
    need = _C.fn16("cosa_attn_bwd_workspace_bytes", dt)(B, N, H)
    assert need >= B * H * N * 4 and need % 256 == 0
    ws_whole, ws = _guarded(need // 4, 64, torch.float32, qkv.device, 1024.0)
    ws.fill_(float("nan"))
    _bwd(qkv, o, go, lse, H, dqkv=inner.view(B, N, row), ws=ws)
    torch.cuda.synchronize()
    assert torch.isfinite(inner).all() and torch.isfinite(ws[:B * H * N]).all()
    for w, n in ((whole, 4 * row), (ws_whole, 4 * 64)):
        assert (w[:n] == 1024.0).all() and (w[-n:] == 1024.0).all()


@pytest.mark.parametrize("dt", DTYPES, ids=_ids)
def test_bad_arguments_are_refused_before_any_launch(dt):
    """head_dim = 32 is an error code, a workspace one byte short is COSA_ENOMEM; neither touches dqkv"""
    from cosa_amd import _C
    B, N, H = 1, 65, 2
    qkv, go, o, lse = _isolated_inputs(B, N, H, dt, seed=3)
    dqkv = torch.full_like(qkv, 1024.0)
    need = _C.fn16("cosa_attn_bwd_workspace_bytes", dt)(B, N, H)
    assert _bwd(qkv, o, go, lse, H, dqkv=dqkv, head_dim=32, check=False) not in (0, COSA_ENOMEM)
    assert "head_dim" in _C.lib().cosa_last_error().decode()
    assert _bwd(qkv, o, go, lse, H, dqkv=dqkv, ws_bytes=need - 1, check=False) == COSA_ENOMEM
    assert "workspace" in _C.lib().cosa_last_error().decode()
    torch.cuda.synchronize()
    assert (dqkv == 1024.0).all()
