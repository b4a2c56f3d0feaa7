"""The three-term attention forward (attn_fwd_x3_kernel) and the attention backward (attn_bwd_dq_kernel and its two neighbours) keep their
bits: SHA-256 of the output bytes against digests recorded from the build BEFORE the accumulators of those two kernels moved from AGPRs to
VGPRs (tests/golden/attn_regs_digests.json).  The kernels have no atomics and a fixed MFMA order, so equality of bytes is the bar.

Inputs are integers from a seeded CPU generator scaled by powers of two (exact in fp32 on every host), split on the device by
nn_ops.split_rows.  Forward, both operand types, B = 2, H = 2: N = 1 (tail tile only), 64 (one full tile, no tail), 65 (a full tile and a
tail of one), 129 (a second query block holding one query), 197, and at N = 197 two constructed score patterns: "rising", where the keys of
each 64-key tile score higher than all keys before (every row's maximum moves in every tile: the rescale branch is taken each time), and
"falling", the mirror order (the maximum never moves after the first tile).  Backward, both operand types: (B, N, H) = (1, 65, 1),
(1, 129, 1), (2, 197, 2), with out / lse from the training forward (cosa_attn_fwd).

Recording (on a GPU, from the build that is to be the reference; twice, the two files must be equal):
    python tests/test_attn_regs_gpu.py path/to/libcosa_hip.so digests.json"""
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "attn_regs_digests.json")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
HD = 64
FWD_CASES = [("N1", 1, None), ("N64", 64, None), ("N65", 65, None), ("N129", 129, None), ("N197", 197, None),
             ("N197rising", 197, "rising"), ("N197falling", 197, "falling")]
BWD_CASES = [(1, 65, 1), (1, 129, 1), (2, 197, 2)]
FB, FH = 2, 2


def _ints(gen, *shape):
    """uniform on [-2, 2) in steps of 2^-14: 16 significant bits, so the lo halves of the split carry something"""
    return torch.randint(-32768, 32768, shape, generator=gen).float() / 16384.0


def _fwd_input(N, pattern, seed):
    """fp32 qkv [B * N, 3 * H * 64]"""
    gen = torch.Generator().manual_seed(seed)
    x = _ints(gen, FB, N, 3, FH, HD)
    if pattern is not None:
        # q = 4 u + noise / 4, k = 2 s(tile) u + noise / 32 with u = (1/8, ..., 1/8), |u| = 1: q.u lies in 4 +- 1.2, so a raw score is
        # 2 s q.u +- 0.5 (|q| < 6, |k noise| <= 0.5 / sqrt 3 ... in practice a few tenths) and a step of 1 in s moves it by more than 5.6.
        tile = torch.arange(N) // 64
        s = (tile + 1.0) if pattern == "rising" else (4.0 - tile)
        x[:, :, 0] = 0.5 + x[:, :, 0] / 4
        x[:, :, 1] = 0.25 * s.view(1, N, 1, 1) + x[:, :, 1] / 32
    return x.reshape(FB * N, 3 * FH * HD)


def _sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def _run_fwd(N, pattern, dt, seed):
    from cosa_amd import nn_ops
    qkv_s = nn_ops.split_rows(_fwd_input(N, pattern, seed).cuda(), dtype=dt)
    out_s = torch.zeros(FB * N, nn_ops.split_ld(FH * HD), device="cuda", dtype=dt)
    lse = torch.zeros(FB, FH, N, device="cuda")
    nn_ops.attn_fwd_x3(qkv_s, FB, N, FH, out_s, lse)
    torch.cuda.synchronize()
    return {"out": _sha(out_s), "lse": _sha(lse)}


def _run_bwd(B, N, H, dt, seed):
    from cosa_amd import _C
    gen = torch.Generator().manual_seed(seed)
    qkv = _ints(gen, B, N, 3 * H * HD).to(dt).cuda()
    go = _ints(gen, B, N, H * HD).to(dt).cuda()
    out = torch.zeros(B, N, H * HD, device="cuda", dtype=dt)
    lse = torch.zeros(B, H, N, device="cuda")
    ws = _C.workspace(_C.fn16("cosa_attn_workspace_bytes", dt)(B, N, H), qkv.device, "test_attn_regs_fwd")
    _C.check(_C.fn16("cosa_attn_fwd", dt)(_C.ptr(qkv), _C.ptr(out), _C.ptr(lse), B, N, H, HD, 0.125, 0, None, _C.ptr(ws), ws.numel(),
                                          _C.stream_ptr()), "cosa_attn_fwd")
    dqkv = torch.zeros_like(qkv)
    need = _C.fn16("cosa_attn_bwd_workspace_bytes", dt)(B, N, H)
    wb = _C.workspace(need, qkv.device, "test_attn_regs_bwd")
    _C.check(_C.fn16("cosa_attn_bwd", dt)(_C.ptr(qkv), _C.ptr(out), _C.ptr(go), _C.ptr(lse), _C.ptr(dqkv), B, N, H, HD, 0.125,
                                          _C.ptr(wb), need, _C.stream_ptr()), "cosa_attn_bwd")
    torch.cuda.synchronize()
    return {"dqkv": _sha(dqkv)}


def _fwd_key(name, dtn):
    return f"fwd/{dtn}/{name}"


def _bwd_key(B, N, H, dtn):
    return f"bwd/{dtn}/B{B}N{N}H{H}"


def _all_digests():
    d = {}
    for dtn, dt in DTYPES.items():
        for i, (name, N, pattern) in enumerate(FWD_CASES):
            d[_fwd_key(name, dtn)] = _run_fwd(N, pattern, dt, 100 + i)
        for i, (B, N, H) in enumerate(BWD_CASES):
            d[_bwd_key(B, N, H, dtn)] = _run_bwd(B, N, H, dt, 200 + i)
    return d


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_patterns_do_what_they_say():
    """float64 on the host (no GPU): in "rising" every query's tile maximum exceeds all earlier ones, in "falling" none does after the first"""
    for pattern in ("rising", "falling"):
        x = _fwd_input(197, pattern, 105).double().view(FB, 197, 3, FH, HD)
        s = torch.einsum("bqhd,bkhd->bhqk", x[:, :, 0], x[:, :, 1])
        tmax = torch.stack([s[..., k0:k0 + 64].max(dim=-1).values for k0 in range(0, 197, 64)], dim=-1)      # [B, H, q, 4 tiles]
        step = tmax[..., 1:] - tmax[..., :-1]
        assert (step > 1.0).all() if pattern == "rising" else (step < -1.0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0] for c in FWD_CASES])
def test_fwd_x3_bits(case, dtn):
    name, N, pattern = case
    got = _run_fwd(N, pattern, DTYPES[dtn], 100 + FWD_CASES.index(case))
    assert got == _golden()[_fwd_key(name, dtn)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtn", list(DTYPES))
@pytest.mark.parametrize("case", BWD_CASES, ids=["B%dN%dH%d" % c for c in BWD_CASES])
def test_bwd_bits(case, dtn):
    B, N, H = case
    got = _run_bwd(B, N, H, DTYPES[dtn], 200 + BWD_CASES.index(case))
    assert got == _golden()[_bwd_key(B, N, H, dtn)]


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    from cosa_amd import _C
    _C.LIB_PATH = os.path.abspath(sys.argv[1])           # every kernel of the recording, the split included, comes from that build
    with open(sys.argv[2], "w") as f:
        json.dump(_all_digests(), f, indent=0, sort_keys=True)
        f.write("\n")
