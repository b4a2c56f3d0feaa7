"""A/B of two builds of libcosa_hip.so on the monitor kernels and the fp32 attention forward, INTERLEAVED in one process.

    python tools/ab_monitor_libs.py parent.so new.so [--json profiles/monitor_kernels_ab.json] [--bits-only] [--cases monitors|losses]

Bits: cosa_attn_fwd_f32 and cosa_attn_stats_f32 at B = 2, H = 2, N in {1, 33, 161} (a single key, a tail tile, two query blocks with six key
tiles) and cosa_range_stats_f32 at 3 x 7 and 3 x 64: every output byte of the second build against the first's.  Speed: the same entry
points and cosa_teacher_check / cosa_gt_stats at the workload's shapes (b = 16 x 448^2, K = 21; attention B = 32, H = 12, N = 785), one
HIP event pair per call, the builds taking turns, 5 warm-up and 30 timed calls each, the median per entry point.  The first build is
loaded a second time from a copy of its file (`again`): what its median differs from the first's by, or the first's own interquartile
range if that is larger, is this machine's spread, and the second build passes an entry point if its median is not slower by more than
that.  The counters of the two timed monitors are compared as well.  Exit status 1 if a byte differs or an entry point fails.

--cases losses (-> profiles/loss_kernels_ab.json): the dense losses of csrc/loss_kernels.hip by the same rules.  Their
sums are integers, so every output is the same bytes whatever the scheduling.  Bits: cosa_seg_loss_forward_w then _backward_w at B = 2 with
and without the second label map, weights 0.25 x 4 and (0.21, 0.49, 0.09, 0.21), at (K, hs, ws, S) = (6, 4, 4, 64) (factor 16: grouped
adds), (3, 8, 8, 64) (factor 8), (5, 5, 7, 64) (quads straddle cells: per-pixel adds), (6, 4, 4, 72) (edge blocks) and (21, 12, 12, 192);
cosa_cam_lossv3 at tests/test_camloss_gpu.py's V3_SHAPES and at a 5 x 7 plane; cosa_cam_loss_targets_m and cosa_cam_label on one and on
three scales, K = 6 and 70, both after_softmax modes.  Speed: the same entry points at b = 16, K = 21, 28 x 28 -> 448, scales of 28, 14, 42."""
import argparse, ctypes, json, os, shutil, statistics, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from cosa_amd import _C

Z = ctypes.c_size_t
WARMUP, TIMED = 5, 30
load = lambda path: _C.load(os.path.abspath(path), strict=False)          # signatures from include/cosa_hip.h; an older build may lack entry points


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


def label_maps(g, n, B, K, S):
    """n float label maps [B,S,S] of 4 x 4 patches of one class, one patch in K + 1 ignored (255)"""
    m = torch.randint(0, K + 1, (n, B, S // 4, S // 4), generator=g, device=dev).repeat_interleave(4, 2).repeat_interleave(4, 3)
    return [t.contiguous() for t in torch.where(m == K, 255, m).float()]


def seg_loss(B, K, hs, ws, S, seed, settings):
    """cosa_seg_loss_forward_w / _backward_w per (second map given, weights): random logits and AS, non-unit upstream gradients, boxes that
    cut into the image -> {"seg_loss ... <output>": forward then backward, one entry per output} and the two entry points alone (for the clock)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    Sq = S // 2
    seg, simg, AS = rand(g, B, K, hs, ws) * 2, rand(g, B, 3, S, S), rand(g, B, K, Sq, Sq) * 1e4
    mA, mB = label_maps(g, 2, B, K, S)
    boxes = torch.tensor([[8 * (b % 3), S - 4 * (b % 5), 4 * (b % 4), S - 8 * (b % 2)] for b in range(B)], dtype=torch.int32, device=dev)
    gs, gr = torch.tensor([0.1], device=dev), torch.tensor([0.05 * 1e-7], device=dev)

    def make(lib, has_b, w, part, which):
        wsp = torch.zeros(lib.cosa_seg_loss_workspace_bytes(B, K, hs, ws), dtype=torch.uint8, device=dev)
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, dtype=dt, device=dev)
        out = dict(sums=z(8), s_seg=z(B, K, Sq, Sq), s_img=z(B, 3, Sq, Sq), roi=z(B, Sq, Sq), unlabel=z(B, Sq, Sq, dt=torch.uint8),
                   grad_seg_lr=z(B, K, hs, ws))
        b_map = mB if has_b else None
        fwd = lambda: lib.cosa_seg_loss_forward_w(ptr(seg), ptr(mA), ptr(b_map), ptr(simg), ptr(boxes), ptr(out["sums"]), ptr(out["s_seg"]),
                                                  ptr(out["s_img"]), ptr(out["roi"]), ptr(out["unlabel"]), B, K, hs, ws, S, ptr(wsp), wsp.numel(),
                                                  _C.stream_ptr())
        bwd = lambda: lib.cosa_seg_loss_backward_w(ptr(seg), ptr(mA), ptr(b_map), ptr(out["sums"]), ptr(AS), ptr(out["roi"]), ptr(gs), ptr(gr),
                                                   ptr(out["grad_seg_lr"]), *w, B, K, hs, ws, S, ptr(wsp), wsp.numel(), _C.stream_ptr())
        if part == "backward":                                                          # (its inputs are a forward's outputs)
            assert fwd() == 0
        return {"both": lambda: fwd() or bwd(), "forward": fwd, "backward": bwd}[part], out[which]

    res = {}
    for has_b, w in settings:
        tag = f"{'AB' if has_b else 'A'} {'/'.join(f'{x:g}' for x in w)}"
        for which in OUTPUTS:                                                           # one entry per output: the record names what differed
            res[f"seg_loss {tag} {which}"] = lambda lib, has_b=has_b, w=w, which=which: make(lib, has_b, w, "both", which)
    return res, {"cosa_seg_loss_forward_w": lambda lib: make(lib, *settings[0], "forward", "sums"),
                 "cosa_seg_loss_backward_w": lambda lib: make(lib, *settings[0], "backward", "grad_seg_lr")}


def cam_lossv3(B, C, h, w, S, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    cam = rand(g, B, C, h, w)
    label = label_maps(g, 1, B, C + 1, S)[0].to(torch.uint8)

    def run(lib, which):
        wsp = torch.zeros(lib.cosa_cam_lossv3_workspace_bytes(B, C, h, w), dtype=torch.uint8, device=dev)
        out = dict(loss=torch.zeros(1, device=dev), grad=torch.zeros(B, C, h, w, device=dev))
        return (lambda: lib.cosa_cam_lossv3(ptr(cam), ptr(label), ptr(out["grad"]), ptr(out["loss"]), B, C, h, w, S, ptr(wsp), wsp.numel(),
                                            _C.stream_ptr())), out[which]

    return {f"cosa_cam_lossv3 {which}": (lambda lib, which=which: run(lib, which)) for which in ("loss", "grad")}


def scale_kernels(B, K, S, cells, oh, temp, thre, after, seed):
    """cosa_cam_loss_targets_m and cosa_cam_label on per-scale teacher segs [2B,K,c,c] (live flipped halves), a third of the classes present"""
    g = torch.Generator(device=dev).manual_seed(seed)
    scales = [rand(g, 2 * B, K, c, c) for c in cells]
    n = len(scales)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in scales])
    hw = (ctypes.c_int * n)(*cells)
    labels = (torch.rand(B, K - 1, generator=g, device=dev) < 0.33).float()
    labels[:, 0] = 1

    def targets(lib):
        out = torch.zeros(B, K - 1, oh, oh, device=dev)
        return (lambda: lib.cosa_cam_loss_targets_m(ptrs, hw, hw, n, ptr(labels), ptr(out), B, K, S, oh, oh, temp, after, _C.stream_ptr())), out

    def label(lib):
        out = torch.zeros(B, S, S, dtype=torch.uint8, device=dev)
        return (lambda: lib.cosa_cam_label(ptrs, hw, hw, n, ptr(labels), ptr(out), B, K, S, temp, thre, after, _C.stream_ptr())), out

    targets.keep = label.keep = scales                                                  # (the pointer array does not own the tensors)
    return {"cosa_cam_loss_targets_m": targets, "cosa_cam_label": label}


OUTPUTS = ("sums", "s_seg", "s_img", "roi", "unlabel", "grad_seg_lr")
SEG_SETTINGS = [(has_b, w) for has_b in (True, False) for w in ((0.25, 0.25, 0.25, 0.25), (0.21, 0.49, 0.09, 0.21))]


def loss_cases():
    """[(key in the record, printed case, makers)] of the bit comparison, and a function that builds the makers of the timed workload"""
    bits = []
    for i, (K, hs, ws, S) in enumerate([(6, 4, 4, 64), (3, 8, 8, 64), (5, 5, 7, 64), (6, 4, 4, 72), (21, 12, 12, 192)]):
        bits.append((f"K={K} {hs}x{ws} S={S}", seg_loss(2, K, hs, ws, S, 20 + i, SEG_SETTINGS)[0]))
    for i, (C, h, w, S) in enumerate([(5, 4, 4, 64), (2, 8, 8, 64), (20, 12, 12, 192), (4, 5, 7, 64)]):      # V3_SHAPES of tests/test_camloss_gpu.py, + 5 x 7
        bits.append((f"C={C} {h}x{w} S={S}", cam_lossv3(2, C, h, w, S, 40 + i)))
    i = 0
    for cells in ((4,), (4, 2, 6)):
        for K in (6, 70):                                                               # K = 70: the second class slot of a lane, k >= 64
            for temp, thre in ((0.01, 0.25), (1.0, 0.5)):                               # LABEL_SETTINGS of tests/camloss_ref.py
                for after in (0, 1):
                    bits.append((f"{len(cells)} scales K={K} T={temp:g} after={after}", scale_kernels(2, K, 64, cells, 4, temp, thre, after, 60 + i)))
                    i += 1
    work = lambda: {**seg_loss(16, 21, 28, 28, 448, 7, SEG_SETTINGS[:1])[1], "cosa_cam_lossv3": cam_lossv3(16, 20, 28, 28, 448, 8)["cosa_cam_lossv3 grad"],
                    **scale_kernels(16, 21, 448, (28, 14, 42), 28, 0.01, 0.25, 0, 9)}
    return [(case, case, makers) for case, makers in bits], work


def monitor_cases():
    bits = [(f"B2 H2 N{N}", f"B=2 H=2 N={N}", attention(2, 2, N, seed=N)) for N in (1, 33, 161)]
    bits += [(f"{rows}x{cols}", f"{rows} x {cols}", range_stats(rows, cols, seed=cols)) for rows, cols in ((3, 7), (3, 64))]
    work = lambda: {**attention(32, 12, 785, seed=7), **range_stats(32 * 785, 768, seed=8), **monitors(16, 21, 448, 28, 28, seed=9)}
    return bits, work


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
    ap.add_argument("--cases", choices=("monitors", "losses"), default="monitors")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        again = shutil.copy(a.parent, os.path.join(tmp, "libcosa_hip_again.so"))          # a second code object of the same build
        parent, new, again = load(a.parent), load(a.new), load(again)
        cases, work = monitor_cases() if a.cases == "monitors" else loss_cases()
        bits = {key: same_bytes(case, makers, (parent, new)) for key, case, makers in cases}
        ok = all(v for case in bits.values() for v in case.values())
        report = {"device": torch.cuda.get_device_name(0), "bits_equal": bits, "warmup": WARMUP, "timed": TIMED, "unit": "us", "speed": {}}
        if not a.bits_only:
            work = work()
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
