"""A/B of two builds of libcosa_hip.so on the monitor kernels and the fp32 attention forward, INTERLEAVED in one process.

    python tools/ab_monitor_libs.py parent.so new.so [--json profiles/monitor_kernels_ab.json] [--bits-only]

Bits: cosa_attn_fwd_f32 and cosa_attn_stats_f32 at B = 2, H = 2, N in {1, 33, 161} (a single key, a tail tile, two query blocks with six key
tiles) and cosa_range_stats_f32 at 3 x 7 and 3 x 64: every output byte of the second build against the first's.  Speed: the same entry
points and cosa_teacher_check / cosa_gt_stats at the workload's shapes (b = 16 x 448^2, K = 21; attention B = 32, H = 12, N = 785), one
HIP event pair per call, the builds taking turns, 5 warm-up and 30 timed calls each, the median per entry point.  The first build is
loaded a second time from a copy of its file (`again`): what its median differs from the first's by, or the first's own interquartile
range if that is larger, is this machine's spread, and the second build passes an entry point if its median is not slower by more than
that.  The counters of the two timed monitors are compared as well.  Exit status 1 if a byte differs or an entry point fails."""
import argparse, ctypes, json, os, shutil, statistics, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd import _C

P, I, L, F, Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_size_t
SIGS = {"cosa_attn_fwd_f32": [P, P, I, I, I, I, F, I, I, P], "cosa_attn_stats_f32": [P, I, I, I, I, F, L, P, P],
        "cosa_range_stats_f32": [P, L, I, L, P, P], "cosa_gt_stats": [P] * 6 + [I] * 6 + [P, P],
        "cosa_teacher_check": [P] * 12 + [I] * 7 + [F, P, P, Z, P]}
WARMUP, TIMED = 5, 30


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, sig in SIGS.items():
        getattr(lib, name).argtypes, getattr(lib, name).restype = sig, I
    lib.cosa_teacher_check_workspace_bytes.argtypes, lib.cosa_teacher_check_workspace_bytes.restype = [I, I], Z
    for name in ("cosa_teacher_check_layout", "cosa_gt_stats_layout"):
        getattr(lib, name).argtypes, getattr(lib, name).restype = [I, P], Z
    return lib


ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
dev = torch.device("cuda", 0)
rand = lambda g, *shape: torch.randn(*shape, generator=g, device=dev)


def attention(B, H, N, seed):
    """{entry point: (lib) -> (call, the output it writes)} of the two fp32 attention kernels on one packed qkv"""
    g = torch.Generator(device=dev).manual_seed(seed)
    qkv = rand(g, B, N, 3 * H * 64) * 1.5

    def fwd(lib):
        out = torch.zeros(B, N, H * 64, device=dev)
        return (lambda: lib.cosa_attn_fwd_f32(ptr(qkv), ptr(out), B, N, H, 64, 0.125, 3 * H * 64, H * 64, _C.stream_ptr())), out

    def stats(lib):
        out = torch.zeros(H, 7, dtype=torch.int64, device=dev)
        return (lambda: lib.cosa_attn_stats_f32(ptr(qkv), B, N, H, 64, 0.125, 3 * H * 64, ptr(out), _C.stream_ptr())), out

    return {"cosa_attn_fwd_f32": fwd, "cosa_attn_stats_f32": stats}


def range_stats(rows, cols, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    x = rand(g, rows, cols) * 300.0                                                     # some elements over 65504 / 32768, some tiny
    x.view(-1)[::5] *= 1e-6
    x.view(-1)[3::11] *= 200.0

    def run(lib):
        out = torch.zeros(6, dtype=torch.int64, device=dev)
        return (lambda: lib.cosa_range_stats_f32(ptr(x), rows, cols, cols, ptr(out), _C.stream_ptr())), out

    return {"cosa_range_stats_f32": run}


def monitors(B, K, S, h, w, seed):
    """cosa_teacher_check and cosa_gt_stats on one step's tensors: CAM pairs that differ in the last bits, label maps with an ignore share"""
    g = torch.Generator(device=dev).manual_seed(seed)
    C = K - 1
    cam, aux, tgt = rand(g, B, C, S, S).sigmoid_(), rand(g, B, C, S, S).sigmoid_(), rand(g, B, C, h, w)
    other = lambda t: t * (1 + 1e-4 * rand(g, *t.shape))
    cam_b, aux_b, tgt_b = other(cam), other(aux), other(tgt)

    def blocks():                                                                       # 16 x 16 patches of one class, one in K + 1 of them 255
        m = torch.randint(0, K + 1, (B, S // 16, S // 16), generator=g, device=dev).repeat_interleave(16, 1).repeat_interleave(16, 2)
        return torch.where(m == K, 255, m).contiguous()

    main_a, laux_a, gt = blocks().float(), blocks().float(), blocks().to(torch.uint8)
    flip = lambda m: torch.where(torch.rand(m.shape, generator=g, device=dev) < 0.01, (m + 1) % K, m).contiguous()
    main_b, laux_b = flip(main_a), flip(laux_a)
    cls = (torch.rand(B, C, generator=g, device=dev) < 0.15).float()
    cls[:, 0] = 1
    seg = rand(g, B, K, h, w)
    boxes = torch.tensor([[8 * (b % 3), S - 4 * (b % 5), 4 * (b % 4), S - 8 * (b % 2)] for b in range(B)], dtype=torch.int32, device=dev)

    def teacher(lib):
        out = torch.zeros(lib.cosa_teacher_check_layout(K, (Z * 64)()), dtype=torch.int64, device=dev)
        ws = torch.zeros(lib.cosa_teacher_check_workspace_bytes(B, C), dtype=torch.uint8, device=dev)
        return (lambda: lib.cosa_teacher_check(*(ptr(t) for t in (cam, cam_b, aux, aux_b, tgt, tgt_b, main_a, main_b, laux_a, laux_b, cls, boxes)),
                                               B, C, K, S, h, w, 255, 1e-3, ptr(out), ptr(ws), ws.numel(), _C.stream_ptr())), out

    def gt_stats(lib):
        out = torch.zeros(lib.cosa_gt_stats_layout(K, (Z * 16)()), dtype=torch.int64, device=dev)
        return (lambda: lib.cosa_gt_stats(ptr(gt), ptr(main_a), ptr(laux_a), ptr(seg), ptr(cls), ptr(boxes), B, K, S, h, w, 255, ptr(out),
                                          _C.stream_ptr())), out

    return {"cosa_teacher_check": teacher, "cosa_gt_stats": gt_stats}


def same_bytes(case, makers, libs):
    """one call per build on zeroed outputs -> {entry point: whether every build's output equals the first's byte for byte}"""
    res = {}
    for name, make in makers.items():
        outs = []
        for lib in libs:
            call, out = make(lib)
            assert call() == 0, name
            outs.append(out)
        torch.cuda.synchronize()
        res[name] = all(torch.equal(outs[0].view(torch.uint8), o.view(torch.uint8)) for o in outs[1:])
        print(f"bits  {name:22s} {case:24s} {'equal' if res[name] else 'DIFFER'}", flush=True)
    return res


def timed(makers, libs):
    """{entry point: [[microseconds of each timed call] per build]}: a warm-up of every build, then the builds take turns call by call"""
    res = {}
    for name, make in makers.items():
        calls = [make(lib)[0] for lib in libs]
        for call in calls:
            for _ in range(WARMUP):
                assert call() == 0, name
        torch.cuda.synchronize()
        ts = [[] for _ in libs]
        for _ in range(TIMED):
            for call, acc in zip(calls, ts):
                a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                e.record()
                e.synchronize()
                acc.append(a.elapsed_time(e) * 1e3)
        res[name] = ts
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--json", default=None, help="write the figures there")
    ap.add_argument("--bits-only", action="store_true")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        again = shutil.copy(a.parent, os.path.join(tmp, "libcosa_hip_again.so"))          # a second code object of the same build
        parent, new, again = load(a.parent), load(a.new), load(again)
        ok, bits = True, {}
        for N in (1, 33, 161):
            bits[f"B2 H2 N{N}"] = same_bytes(f"B=2 H=2 N={N}", attention(2, 2, N, seed=N), (parent, new))
        for rows, cols in ((3, 7), (3, 64)):
            bits[f"{rows}x{cols}"] = same_bytes(f"{rows} x {cols}", range_stats(rows, cols, seed=cols), (parent, new))
        ok = all(v for case in bits.values() for v in case.values())
        report = {"device": torch.cuda.get_device_name(0), "bits_equal": bits, "warmup": WARMUP, "timed": TIMED, "unit": "us", "speed": {}}
        if not a.bits_only:
            work = {}
            work.update(attention(32, 12, 785, seed=7))
            work.update(range_stats(32 * 785, 768, seed=8))
            work.update(monitors(16, 21, 448, 28, 28, seed=9))
            bits["workload"] = same_bytes("workload", work, (parent, new))
            ok = ok and all(bits["workload"].values())
            for name, (tp, tn, ta) in timed(work, (parent, new, again)).items():
                med = statistics.median
                q = statistics.quantiles(tp, n=4)
                spread = max(abs(med(ta) - med(tp)), q[2] - q[0])
                passed = med(tn) - med(tp) <= spread
                ok = ok and passed
                report["speed"][name] = dict(parent=round(med(tp), 2), new=round(med(tn), 2), again=round(med(ta), 2), parent_iqr=round(q[2] - q[0], 2),
                                             spread=round(spread, 2), new_minus_parent=round(med(tn) - med(tp), 2), passed=passed)
                print(f"speed {name:22s} parent {med(tp):9.2f} us  new {med(tn):9.2f} us  again {med(ta):9.2f} us  spread {spread:7.2f} us  "
                      f"new - parent {med(tn) - med(tp):+8.2f} us  {'pass' if passed else 'FAIL'}", flush=True)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(report, f, indent=1, sort_keys=True)
                f.write("\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
