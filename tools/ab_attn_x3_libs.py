"""A/B of builds of libcosa_hip.so on the three-term attention forward (cosa_attn_fwd_f16x3 / cosa_attn_fwd_bf16x3: B = 32, 12 heads,
N = 1765 / 785 / 197, split rows in and out) and on the attention backward at the student's shape (cosa_attn_bwd / _f16: B = 16, N = 785),
INTERLEAVED in one process: half a second of warm-up, then six rounds of ten launches per build.  Every output buffer of every build (out, lse, dqkv) is compared byte for
byte with the first build's, and every build with a second run of itself.  A build "wins" a shape when the slowest of its six rounds is
faster than the fastest of the first build's six.
usage (GPU box): python tools/ab_attn_x3_libs.py parent.so new.so [more.so ...]        (exit status 1 if any bytes differ)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd import _C, nn_ops
names = [os.path.basename(p).replace("libcosa_hip_", "").replace(".so", "") for p in sys.argv[1:]]
libs = [_C.load(os.path.abspath(p), strict=False) for p in sys.argv[1:]]          # signatures from include/cosa_hip.h
if len(libs) < 2:
    sys.exit(__doc__)
FWD = {torch.float16: "cosa_attn_fwd_f16x3", torch.bfloat16: "cosa_attn_fwd_bf16x3"}
BWD = {torch.float16: ("cosa_attn_fwd_f16", "cosa_attn_bwd_f16", "cosa_attn_bwd_workspace_bytes_f16", "cosa_attn_workspace_bytes_f16"),
       torch.bfloat16: ("cosa_attn_fwd", "cosa_attn_bwd", "cosa_attn_bwd_workspace_bytes", "cosa_attn_workspace_bytes")}
dev = torch.device("cuda", 0)
st, ptr = _C.stream_ptr, _C.ptr
tag = {torch.float16: "fp16", torch.bfloat16: "bf16"}
differ = 0


def bytes_of(t):
    return t.contiguous().view(torch.uint8)


def ab(label, fs, outs, flops):
    """fs[i]() launches build i once; outs[i] = its output buffers.  Bits against the first build and a second run, then the interleaved timing."""
    global differ
    for f in fs:
        for _ in range(3):
            assert f() == 0
    torch.cuda.synchronize()
    same = []
    for name, f, o in zip(names, fs, outs):
        keep = [t.clone() for t in o]
        for t in o:
            t.zero_()
        assert f() == 0
        torch.cuda.synchronize()
        det = all(torch.equal(bytes_of(a), bytes_of(b)) for a, b in zip(keep, o))
        eq = [torch.equal(bytes_of(a), bytes_of(b)) for a, b in zip(outs[0], o)]
        if not det:
            print(f"{label} {name}: NOT deterministic run to run")
        for k, (a, b) in enumerate(zip(outs[0], o)):
            if not eq[k]:
                print(f"{label} {name}: buffer {k}: {int((bytes_of(a) != bytes_of(b)).sum())} of {bytes_of(a).numel()} bytes differ from the first build")
        same.append(det and all(eq))
        differ += not same[-1]
    t0 = time.time()
    while time.time() - t0 < 0.5:            # bring the clocks to their loaded state before the first timed round: the builds alternate here too
        for f in fs:
            for _ in range(10):
                f()
        torch.cuda.synchronize()
    ts = [[] for _ in libs]
    for _ in range(6):
        for f, acc in zip(fs, ts):
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                f()
            e.record()
            torch.cuda.synchronize()
            acc.append(a.elapsed_time(e) / 10 * 1e3)
    base = sorted(ts[0])[3]
    for name, t, s in zip(names, ts, same):
        med = sorted(t)[3]
        win = "" if t is ts[0] else ("  WINS (slowest round < first build's fastest)" if max(t) < min(ts[0]) else "  no clear gain")
        print(f"{label} {name:14s} {med:8.1f} us (min {min(t):8.1f}, max {max(t):8.1f}, {flops / med / 1e6:5.0f} TF)  vs first {med / base:.4f}  "
              f"bits {'equal, deterministic' if s else 'DIFFER'}{win}", flush=True)


B, H = 32, 12
for N in (1765, 785, 197):
    g = torch.Generator(device="cpu").manual_seed(N)
    src = (torch.randn(B * N, 3 * H * 64, generator=g) * 1.5).to(dev)
    for dt in (torch.float16, torch.bfloat16):
        qkv = nn_ops.split_rows(src, dtype=dt)
        outs = [(torch.zeros(B * N, nn_ops.split_ld(H * 64), device=dev, dtype=dt), torch.zeros(B, H, N, device=dev)) for _ in libs]
        fs = [(lambda L=L, o=o: getattr(L, FWD[dt])(ptr(qkv), ptr(o[0]), ptr(o[1]), B, N, H, 64, 0.125, qkv.stride(0), o[0].stride(0), None, st()))
              for L, o in zip(libs, outs)]
        ab(f"fwd x3 {tag[dt]} N={N:5d}", fs, outs, 4.0 * N * N * 64 * B * H)
        del qkv, outs, fs
    del src

B, N = 16, 785
g = torch.Generator(device="cpu").manual_seed(7)
qkv32, go32 = torch.randn(B, N, 3 * H * 64, generator=g), torch.randn(B, N, H * 64, generator=g)
for dt in (torch.bfloat16, torch.float16):
    fwd, bwd, bws, fws = BWD[dt]
    L0 = libs[0]
    qkv, go = qkv32.to(dt).to(dev), go32.to(dt).to(dev)
    out, lse = torch.empty(B, N, H * 64, device=dev, dtype=dt), torch.empty(B, H, N, device=dev)
    ws = torch.zeros(max(getattr(L0, fws)(B, N, H), 256), device=dev, dtype=torch.uint8)
    assert getattr(L0, fwd)(ptr(qkv), ptr(out), ptr(lse), B, N, H, 64, 0.125, 0, None, ptr(ws), ws.numel(), st()) == 0      # the first build's forward feeds all
    need = getattr(L0, bws)(B, N, H)
    wss = [torch.zeros(need, device=dev, dtype=torch.uint8) for _ in libs]
    outs = [(torch.zeros_like(qkv),) for _ in libs]
    fs = [(lambda L=L, o=o, w=w: getattr(L, bwd)(ptr(qkv), ptr(out), ptr(go), ptr(lse), ptr(o[0]), B, N, H, 64, 0.125, ptr(w), need, st()))
          for L, o, w in zip(libs, outs, wss)]
    ab(f"bwd    {tag[dt]} N={N:5d}", fs, outs, 10.0 * N * N * 64 * B * H)
sys.exit(1 if differ else 0)
