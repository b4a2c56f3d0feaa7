"""The --act_stats_iters monitor on the GPU: the two reductions of csrc/act_stats_kernels.hip against their float64
restatement (tests/act_stats_ref.py), the encoder's probe on a network in mode fp32 at crop 64, and the trainer.

Range words are integers: every comparison is exact.  The attention words that are sums or maxima of floating-point row statistics are held to
4 x the deviation a plain fp32 evaluation (torch on the host: fp32 matmul, softmax, entropy) of the same rows shows against the float64
restatement, plus 2^-30 (act_stats_ref.attn_bars says per quantity which deviation that is); each test prints both figures."""
import functools
import math
import os

import pytest
import torch

import act_stats_ref as ref

pytestmark = pytest.mark.gpu

SENTINEL = -0x0123456789abcdef
EINVAL = 1
INF, NAN = float("inf"), float("nan")
NEXT_ABOVE_F16_MAX = ref.bits_f32(ref.f32_bits(65504.0) + 1)
# +-inf, NaN, exactly 65504 (not over), the next float (over), exactly 32768 (not near), 2^-14 (not tiny), 2^-15 (tiny), +-0, and ordinary large ones
PLANTED = (INF, -INF, NAN, 65504.0, -NEXT_ABOVE_F16_MAX, 32768.0, 2.0 ** -14, -2.0 ** -15, 0.0, -0.0, 40000.0, -70000.0)


def _dev():
    return torch.device("cuda", 0)


# ---- the range kernel ---------------------------------------------------------------------------------------------------------------------
def _matrix(rows, width, seed, plant_cols=None):
    """random fp32 rows with PLANTED spread over the columns `plant_cols` (a range) of as many rows as it takes"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, width, generator=g) * 3.0
    lo, hi = plant_cols if plant_cols is not None else (0, width)
    cells = torch.randperm(rows * (hi - lo), generator=g)[:len(PLANTED)].tolist()
    for v, c in zip(PLANTED, cells):
        x[c // (hi - lo), lo + c % (hi - lo)] = v
    return x


def _raw_range(base_ptr, rows, cols, ld, out):
    from cosa_amd import _C
    rc = _C.lib().cosa_range_stats_f32(_C.c_void_p(base_ptr), rows, cols, ld, _C.ptr(out), _C.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _guarded(n):
    return torch.full((n + 2,), SENTINEL, dtype=torch.int64, device=_dev())


def test_range_one_element():
    from cosa_amd import nn_ops
    for v in (3.5, -0.0, INF, 2.0 ** -20):
        out = torch.zeros(6, dtype=torch.int64, device=_dev())
        x = torch.tensor([[v]], dtype=torch.float32)
        nn_ops.range_stats(x.to(_dev()), out)
        assert out.cpu().tolist() == ref.range_words(x), v


def test_range_window_with_padding_reads_nothing_outside_it():
    """3 x 5 at row stride 8 on a 16-byte aligned base (one float4 and one tail column per row): inf in the three padding columns of every
    row and in the four floats before and after the window stay uncounted; sentinels around the six words survive"""
    g = torch.Generator().manual_seed(5)
    buf = torch.full((4 + 3 * 8 + 4,), INF)
    win = torch.randn(3, 5, generator=g)
    win[1, 4], win[2, 0], win[0, 3] = 2.0 ** -15, -NEXT_ABOVE_F16_MAX, NAN
    buf[4:4 + 24].view(3, 8)[:, :5] = win
    d = buf.to(_dev())
    out = _guarded(6)
    out[1:7] = 0
    assert d.data_ptr() % 16 == 0 and _raw_range(d.data_ptr() + 16, 3, 5, 8, out[1:7]) == 0
    got = out.cpu().tolist()
    assert got[0] == SENTINEL and got[7] == SENTINEL and got[1:7] == ref.range_words(win)
    assert got[1] == 14 and got[6] == 1 and got[3] == 1 and got[5] == 1


@pytest.mark.parametrize("col0", [0, 768, 1536])
def test_range_qkv_windows(col0):
    """37 x 768 out of 37 x 2304: what reads q / k / v out of the packed qkv rows; the planted values sit in the window under test"""
    from cosa_amd import nn_ops
    x = _matrix(37, 2304, 11 + col0, plant_cols=(col0, col0 + 768))
    out = torch.zeros(6, dtype=torch.int64, device=_dev())
    nn_ops.range_stats(x.to(_dev()), out, col0, 768)
    want = ref.range_words(x[:, col0:col0 + 768])
    assert out.cpu().tolist() == want and want[5] == 3 and want[2] == 2 and want[3] == 4 and want[4] >= 1


@pytest.mark.parametrize("rows,width,col0,cols", [(9, 12, 1, 7),        # base not 16-byte aligned: the scalar path
                                                  (5, 7, 0, 6),         # aligned base, row stride no multiple of 4: the scalar path
                                                  (6, 16, 4, 3),        # fewer than four columns
                                                  (197, 3072, 0, 3072)])  # more than one block, several float4 per thread
def test_range_paths_and_sizes(rows, width, col0, cols):
    from cosa_amd import nn_ops
    x = _matrix(rows, width, 100 + rows, plant_cols=(col0, col0 + cols))
    out = torch.zeros(6, dtype=torch.int64, device=_dev())
    nn_ops.range_stats(x.to(_dev()), out, col0, cols)
    assert out.cpu().tolist() == ref.range_words(x[:, col0:col0 + cols])


def test_range_two_calls_accumulate_and_two_runs_give_identical_bytes():
    from cosa_amd import nn_ops
    x = _matrix(197, 3072, 7)
    d = x.to(_dev())
    one, runs = ref.range_words(x), []
    for _ in range(2):
        out = torch.zeros(6, dtype=torch.int64, device=_dev())
        nn_ops.range_stats(d, out)
        first = out.cpu().tolist()
        nn_ops.range_stats(d, out)
        runs.append((first, out.cpu().numpy().tobytes(), out.cpu().tolist()))
    assert runs[0] == runs[1] and runs[0][0] == one
    assert runs[0][2] == ref.range_words(x, one) == [2 * w if i != 1 else w for i, w in enumerate(one)]


def test_range_refusals_leave_the_output_untouched():
    from cosa_amd import _C, nn_ops
    L = _C.lib()
    d = torch.zeros(4, 8, device=_dev())
    for kw in (dict(rows=0), dict(rows=-1), dict(cols=0), dict(ld=7), dict(x=0), dict(out=0)):
        out = torch.full((6,), 3, dtype=torch.int64, device=_dev())
        a = dict(x=d.data_ptr(), rows=4, cols=8, ld=8, out=out.data_ptr())
        a.update(kw)
        rc = L.cosa_range_stats_f32(_C.c_void_p(a["x"]), a["rows"], a["cols"], a["ld"], _C.c_void_p(a["out"]), _C.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL and b"cosa_range_stats_f32" in L.cosa_last_error(), kw
        assert bool((out == 3).all())
    with pytest.raises(_C.CosaError):
        nn_ops.range_stats(d, torch.zeros(5, dtype=torch.int64, device=_dev()))
    with pytest.raises(_C.CosaError):
        nn_ops.range_stats(d, torch.zeros(6, dtype=torch.int64, device=_dev()), 4, 5)
    with pytest.raises(_C.CosaError):
        nn_ops.range_stats(d.cpu(), torch.zeros(6, dtype=torch.int64))


# ---- the attention kernel -----------------------------------------------------------------------------------------------------------------
B = 2
ATTN_SHAPES = [(1, 1), (5, 12), (32, 2), (33, 12), (37, 12), (129, 3), (197, 12)]      # (N, H): one key, tails of every kind, two query blocks


@functools.lru_cache(maxsize=None)
def _attn_case(N, H):
    """random q / k / v of unit variance [B * N, 3 * H * 64] (host) and its reference: (qkv, per-head float64 figures, bars, fp32 deviations)"""
    g = torch.Generator().manual_seed(4000 + 16 * N + H)
    qkv = torch.randn(B * N, 3 * H * 64, generator=g)
    rows = ref.attn_rows(qkv, B, N, H)
    # `peaked` is exact only where no row sits at the threshold: asserted of the float64 reference (seeds chosen so that it holds)
    assert float((rows["top1"] - 0.5).abs().min()) > 1e-3, (N, H)
    return (qkv,) + ref.attn_bars(qkv, B, N, H)


def _attn_words(qkv_dev, N, H, batch=B):
    from cosa_amd import nn_ops
    out = torch.zeros(7 * H, dtype=torch.int64, device=_dev())
    nn_ops.attn_stats(qkv_dev, batch, N, H, out)
    return out.cpu().view(H, 7)


def _check_heads(words, want, bars, tag):
    worst = {k: 0.0 for k in bars}
    for h, (w, e) in enumerate(zip(words.tolist(), want)):
        got = ref.head_words_decoded(w)
        assert (got["rows"], got["nonfinite_rows"], got["peaked"]) == (e["rows"], e["nonfinite_rows"], e["peaked"]), (tag, h, got, e)
        for k in bars:
            if e[k] is not None:
                worst[k] = max(worst[k], abs(got[k] - e[k]))
    return worst


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("N,H", ATTN_SHAPES)
def test_attn_words_against_the_float64_restatement(N, H, pad):
    qkv, want, bars, dev32 = _attn_case(N, H)
    ld = 3 * H * 64 + pad
    x = torch.full((B * N, ld), NAN)                      # (padding columns a kernel must not read as data)
    x[:, :3 * H * 64] = qkv
    words = _attn_words(x.to(_dev()), N, H)
    assert all(e["rows"] == B * N and e["nonfinite_rows"] == 0 for e in want)
    worst = _check_heads(words, want, bars, (N, H, pad))
    for k in bars:
        print("attn N=%d H=%d ldq=%d %-8s: kernel vs float64 %.3e, fp32 vs float64 %.3e, bar %.3e" % (N, H, ld, k, worst[k], dev32[k], bars[k]))
    assert all(worst[k] <= bars[k] for k in bars), (worst, bars)


def _planted():
    """B = 1, N = 37, H = 3.  Head 0: every q is zero (uniform rows).  Head 1: q_i = 8 e_i, k_j = 40 e_j, so s_ii = 40 and every other logit
    is 0 (one-hot rows, 40 above the rest).  Head 2: random."""
    N, H = 37, 3
    g = torch.Generator().manual_seed(9)
    x = torch.randn(N, 3 * H * 64, generator=g).view(N, 3, H, 64)
    x[:, 0, 0] = 0
    x[:, 0, 1] = 8.0 * torch.eye(N, 64)
    x[:, 1, 1] = 40.0 * torch.eye(N, 64)
    return x.reshape(N, -1).contiguous(), N, H


def test_attn_planted_rows_with_known_answers():
    x, N, H = _planted()
    got = [ref.head_words_decoded(w) for w in _attn_words(x.to(_dev()), N, H, batch=1).tolist()]
    uni, hot = got[0], got[1]
    assert uni["rows"] == hot["rows"] == N and uni["peaked"] == 0 and hot["peaked"] == N
    assert abs(uni["top1"] - 1.0 / N) <= 1e-6 and abs(uni["ent"] - 1.0) <= 1e-6 and uni["smax"] == 0.0 and abs(uni["sharpest"] - 1.0) <= 1e-6
    assert abs(hot["top1"] - 1.0) <= 1e-6 and abs(hot["ent"]) <= 1e-6 and hot["smax"] == 40.0 and abs(hot["sharpest"]) <= 1e-6


def test_attn_a_nan_row_is_counted_and_left_out():
    """a NaN in q of the row that holds head 1's largest logit: it lands in nonfinite_rows, and every other word of the head is what the
    other rows alone give (the float64 restatement without that row); heads 0 and 2 keep their bytes"""
    N, H = 37, 3
    qkv = _attn_case(37, 12)[0][:N, :3 * H * 64].contiguous()       # (any random rows will do: head h here is not head h there)
    clean = _attn_words(qkv.to(_dev()), N, H, batch=1)
    rows = ref.attn_rows(qkv, 1, N, H)
    r = int(rows["smax"][0, 1].argmax())
    bad = qkv.clone()
    bad[r, 1 * 64 + 3] = NAN
    words = _attn_words(bad.to(_dev()), N, H, batch=1)
    assert torch.equal(words[0], clean[0]) and torch.equal(words[2], clean[2])
    want, bars, _ = ref.attn_bars(bad, 1, N, H)
    assert want[1]["rows"] == N - 1 and want[1]["nonfinite_rows"] == 1 and want[1]["smax"] < float(rows["smax"][0, 1].max())
    worst = _check_heads(words, want, bars, "nan row")
    assert all(worst[k] <= bars[k] for k in bars), (worst, bars)
    # a NaN in a k row reaches every query of its head and image
    bad = qkv.clone()
    bad[4, (H + 2) * 64] = NAN
    words = _attn_words(bad.to(_dev()), N, H, batch=1)
    assert words[2].tolist() == [0, 0, 0, 0, 0, 0, N] and torch.equal(words[:2], clean[:2])


def test_attn_heads_are_independent_and_runs_give_identical_bytes():
    qkv, _, _, _ = _attn_case(33, 12)
    N, H = 33, 12
    a, a2 = _attn_words(qkv.to(_dev()), N, H), _attn_words(qkv.to(_dev()), N, H)
    assert a.numpy().tobytes() == a2.numpy().tobytes()
    other = qkv.clone().view(B * N, 3, H, 64)
    other[:, :, 0] += 1.0                                   # q, k and v of head 0
    b = _attn_words(other.reshape(B * N, -1).to(_dev()), N, H)
    assert not torch.equal(a[0], b[0]) and torch.equal(a[1:], b[1:])
    # two calls into the same words: counts and sums double, maxima stay
    from cosa_amd import nn_ops
    out = torch.zeros(7 * H, dtype=torch.int64, device=_dev())
    d = qkv.to(_dev())
    nn_ops.attn_stats(d, B, N, H, out)
    nn_ops.attn_stats(d, B, N, H, out)
    twice = out.cpu().view(H, 7)
    assert torch.equal(twice[:, [0, 1, 2, 3, 6]], 2 * a[:, [0, 1, 2, 3, 6]]) and torch.equal(twice[:, [4, 5]], a[:, [4, 5]])


def test_attn_sentinels_and_refusals():
    from cosa_amd import _C
    L = _C.lib()
    N, H = 5, 12
    d = _attn_case(N, H)[0].to(_dev())
    out = _guarded(7 * H)
    out[1:-1] = 0
    assert L.cosa_attn_stats_f32(_C.ptr(d), B, N, H, 64, 0.125, d.stride(0), _C.ptr(out[1:-1]), _C.stream_ptr()) == 0
    torch.cuda.synchronize()
    got = out.cpu()
    assert int(got[0]) == SENTINEL and int(got[-1]) == SENTINEL and torch.equal(got[1:-1].view(H, 7), _attn_words(d, N, H))
    ld = d.stride(0)
    for kw in (dict(B=0), dict(N=0), dict(H=0), dict(hd=32), dict(ldq=ld - 4), dict(ldq=ld + 2), dict(q=d.data_ptr() + 4), dict(q=0), dict(out=0)):
        w = torch.full((7 * H,), 3, dtype=torch.int64, device=_dev())
        a = dict(q=d.data_ptr(), B=B, N=N, H=H, hd=64, ldq=ld, out=w.data_ptr())
        a.update(kw)
        rc = L.cosa_attn_stats_f32(_C.c_void_p(a["q"]), a["B"], a["N"], a["H"], a["hd"], 0.125, a["ldq"], _C.c_void_p(a["out"]), _C.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL and b"cosa_attn_stats_f32" in L.cosa_last_error(), kw
        assert bool((w == 3).all())


# ---- the encoder's probe ------------------------------------------------------------------------------------------------------------------
CROP, SCALES = 64, [1.0, 0.5, 1.5]                          # 16-pixel patches: N = 17 / 5 / 37, every batch doubled by its mirror images


FC1_SCALE = 4.0


def _network(mode="fp32", seed=3):
    """the seeded initialisation with every block's fc1 (weight and bias) times FC1_SCALE, the same rule for all twelve blocks.  Why: the
    std-0.02 initialisation behind a LayerNorm gives fc1 pre-activations of standard deviation 0.02 sqrt(768) = 0.55, so its largest fc1 + GELU value over
    the 236 x 3072 elements of a pass is 2.5 (measured: 2.51 at block 7), 14.7 bits under 65504 -- a network on which the overflow case below,
    one fc1 times 2^14, cannot overflow whatever the seed or the images (it needs a clean |h| above 65504 / 2^14 = 4, a 7-sigma value).
    Times 4, a power of two, the MLP activations peak near 10, the order of a trained ViT's, and that case exercises what it is there for;
    every other test of this section reads the same network."""
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    from cosa_amd.utils import torch_helper
    torch_helper.setup_seed(seed)
    m = build_model(default_args("VOC12", crop_size=CROP, batch_size=2)).to(_dev()).eval()
    for p in m.parameters():
        p.requires_grad = False
    for blk in m.encoder.blocks:
        blk.mlp.fc1.weight *= FC1_SCALE
        blk.mlp.fc1.bias *= FC1_SCALE
    return m.set_nograd_precision(mode)


def _images():
    from cosa_amd.train_step import synthetic_batch
    wimg, _simg, lab, _box = synthetic_batch(2, CROP, 20, _dev(), seed=41)
    return wimg, lab


def _pass(m, probe=None, tag="probe"):
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    wimg, lab = _images()
    m.encoder.act_probe = probe
    try:
        with torch.no_grad(), _C.workspace_scope(tag):
            cam, aux, seg = seg_helper.multi_scale_camseg(m, wimg, SCALES, _active_labels=lab, _seg_scales=True)
        torch.cuda.synchronize()
        return [t.clone() for t in (cam, aux, *seg)]
    finally:
        m.encoder.act_probe = None


class _CloneProbe:
    """a probe at the Python level: what the encoder hands to its two calls, cloned"""

    def __init__(self):
        self.sites, self.attn_calls = [], []

    def site(self, layer, name, x, col0=0, cols=None):
        cols = x.shape[1] - col0 if cols is None else cols
        self.sites.append((layer, name, x[:, col0:col0 + cols].detach().cpu().clone()))

    def attn(self, layer, qkv, B_, N, H):
        self.attn_calls.append((layer, qkv.detach().cpu().clone(), B_, N, H))


@functools.lru_cache(maxsize=None)
def _probed():
    from cosa_amd.models.vit import ActProbe
    m = _network()
    depth, H = len(m.encoder.blocks), m.encoder.num_heads
    plain = _pass(m)
    probe = ActProbe(depth, H, device=_dev())
    probed = _pass(m, probe)
    clones = _CloneProbe()
    _pass(m, clones)
    return dict(m=m, depth=depth, H=H, plain=plain, probed=probed, table=probe.table.cpu().clone(), clones=clones)


def test_probe_changes_no_bit_of_the_pass_and_counts_every_row():
    p = _probed()
    assert len(p["plain"]) == len(p["probed"]) and all(torch.equal(a, b) for a, b in zip(p["plain"], p["probed"]))
    b, H, depth = 2, p["H"], p["depth"]
    rows = 2 * b * sum((int(s * CROP) // 16) ** 2 + 1 for s in SCALES)
    t = p["table"].view(depth, -1)
    assert t.shape == (12, 36 + 7 * 12) and rows == 2 * 2 * (17 + 5 + 37)
    heads = t[:, 36:].view(depth, H, 7)
    assert bool((heads[:, :, 0] == rows).all()) and bool((heads[:, :, 6] == 0).all())
    for j, width in enumerate((768, 768, 768, 768, 3072, 768)):
        assert bool((t[:, 6 * j] == rows * width).all()) and bool((t[:, 6 * j + 5] == 0).all()), j


def test_probe_table_equals_the_restatement_on_the_buffers():
    """layer index, site order, column windows and per-scale offsets: the table against act_stats_ref on clones taken at the same sites"""
    p = _probed()
    depth, H, t = p["depth"], p["H"], p["table"]
    sites = {}
    for layer, name, x in p["clones"].sites:
        assert (layer, name) not in sites
        sites[layer, name] = ref.range_words(x)
    assert len(sites) == depth * 6
    for i in range(depth):
        for j, name in enumerate(ref.SITES):
            assert t[i, 6 * j:6 * j + 6].tolist() == sites[i, name], (i, name)
    by_layer = {}
    for layer, qkv, B_, N, H_ in p["clones"].attn_calls:
        assert H_ == H and B_ == 4 and qkv.shape == (B_ * N, 3 * 768)
        assert float((ref.attn_rows(qkv, B_, N, H)["top1"] - 0.5).abs().min()) > 1e-3, (layer, N)      # (`peaked` is exact away from its threshold)
        by_layer.setdefault(layer, []).append((N, ref.attn_bars(qkv, B_, N, H)))
    assert sorted(by_layer) == list(range(depth)) and all([n for n, _ in v] == [17, 5, 37] for v in by_layer.values())
    worst_all = {}
    for i in range(depth):
        want = ref.merge_heads([w for _, (w, _, _) in by_layer[i]])
        bars = {k: max(b[k] for _, (_, b, _) in by_layer[i]) for k in ("ent", "top1", "smax", "sharpest")}
        worst = _check_heads(t[i, 36:].view(H, 7), want, bars, ("layer", i))
        assert all(worst[k] <= bars[k] for k in bars), (i, worst, bars)
        worst_all = {k: max(worst[k], worst_all.get(k, 0.0)) for k in worst}
    print("encoder probe, worst over the blocks:", {k: "%.2e" % v for k, v in worst_all.items()})


def test_probe_on_another_operand_mode_raises():
    from cosa_amd.models.vit import ActProbe
    m = _network("fp16x3")
    with pytest.raises(RuntimeError, match="act_probe"):
        _pass(m, ActProbe(len(m.encoder.blocks), m.encoder.num_heads, device=_dev()), tag="x3")


def _table_of(m):
    from cosa_amd.models.vit import ActProbe
    probe = ActProbe(len(m.encoder.blocks), m.encoder.num_heads, device=_dev())
    _pass(m, probe)
    return probe.table.cpu().clone()


def test_gain_on_the_q_rows_scales_the_logits_bit_for_bit():
    """block 5's q rows (weight and bias) times 8: the f32 GEMM is one ascending fma chain per element and 8 is a power of two, so the scaling
    commutes with every rounding -- block 5's smax words are exactly 8 x the unscaled run's, blocks 0-4 keep every byte"""
    p = _probed()
    m, H = _network(), p["H"]
    qkv = m.encoder.blocks[5].attn.qkv
    qkv.weight[:768] *= 8.0
    qkv.bias[:768] *= 8.0
    t = _table_of(m)
    assert torch.equal(t[:5], p["table"][:5])
    smax = lambda tab: [ref.bits_f32(v) for v in tab[5, 36:].view(H, 7)[:, 4].tolist()]
    assert smax(t) == [8.0 * v for v in smax(p["table"])] and all(v > 0 for v in smax(t))
    assert not torch.equal(t[6], p["table"][6])


def _scaled_fc1_summary(power):
    """the summary of a pass with block 7's fc1 (weight and bias) times 2^power, and of the clean pass"""
    from cosa_amd.utils import seg_helper
    p = _probed()
    depth, H = p["depth"], p["H"]
    one = torch.ones(1, dtype=torch.int64)
    clean = seg_helper.act_stats_summary(torch.cat([p["table"].reshape(-1), one]), depth, H)
    m = _network()
    fc1 = m.encoder.blocks[7].mlp.fc1
    fc1.weight *= 2.0 ** power
    fc1.bias *= 2.0 ** power
    s = seg_helper.act_stats_summary(torch.cat([_table_of(m).reshape(-1), one]), depth, H)
    h0, h1 = clean["layers"][7]["sites"]["h"], s["layers"][7]["sites"]["h"]
    print("fc1 of block 7 x 2^%d: max |h| %.4g -> %.4g, near %d, over %d, headroom %.2f bits at %s (clean: %.2f bits at %s)" % (
        power, h0["absmax"], h1["absmax"], h1["near"], h1["over"], s["headroom_bits"], s["headroom_at"], clean["headroom_bits"], clean["headroom_at"]))
    return clean, s


def test_a_scaled_fc1_shows_as_overflow_at_its_site():
    """fc1 of block 7 times 2^14: block 7's h site reports over > 0 and the summary's minimum headroom, now negative, names (h, 7); the
    blocks before it keep their sites; and the clean table's globals against their restatement"""
    from cosa_amd.utils import seg_helper
    p = _probed()
    depth, H = p["depth"], p["H"]
    clean, s = _scaled_fc1_summary(14)
    assert s["layers"][7]["sites"]["h"]["over"] > 0 and s["headroom_at"] == ["h", 7] and s["checks"] == 1
    assert s["headroom_bits"] < 0 and s["over"] >= s["layers"][7]["sites"]["h"]["over"] and s["layers"][6]["sites"] == clean["layers"][6]["sites"]
    assert clean["over"] == 0 and clean["nonfinite"] == 0 and clean["headroom_bits"] > 0
    layers = [({n: p["table"][i, 6 * j:6 * j + 6].tolist() for j, n in enumerate(ref.SITES)},
               [ref.head_words_decoded(w) for w in p["table"][i, 36:].view(H, 7).tolist()]) for i in range(depth)]
    g = ref.summary_globals(layers)
    for k in ("headroom_at", "smax_at", "ent_min_at", "over", "nonfinite", "smax"):
        assert clean[k] == g[k], k
    for k in ("headroom_bits", "ent_mean", "ent_min"):
        assert abs(clean[k] - g[k]) <= 1e-12, k
    print("the encoder fixture at crop 64:", seg_helper.act_stats_line(clean))


# ---- the trainer --------------------------------------------------------------------------------------------------------------------------
LOSSES = ("cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")


def _trainer(seed=3, **over):
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=CROP, batch_size=2, lr=1e-3, **over)              # (teacher graph and side stream on: the defaults)
    return CoSATrainer(args, _dev(), seed=seed)


def _step(tr, k, n_iter=None):
    from cosa_amd.train_step import synthetic_batch
    logs = tr.step(*synthetic_batch(2, CROP, 20, tr.device, seed=700 + k), n_iter=tr.args.warmup_iters + 1 + k if n_iter is None else n_iter)
    return torch.stack([logs[n].reshape(()).float() for n in LOSSES]).clone()


def _state(tr):
    out = {}
    for tag, net in (("ON", tr.student), ("AN", tr.model_AN)):
        for n, p in net.named_parameters():
            out[f"{tag}.{n}"] = p.detach().clone()
    names = {id(p): n for n, p in tr.student.named_parameters()}
    for p, st in tr.optimizer.state.items():
        for k in ("exp_avg", "exp_avg_sq"):
            out[f"opt.{names[id(p)]}.{k}"] = st[k].clone()
    return out


@functools.lru_cache(maxsize=None)
def _monitored_run(directory):
    tr = _trainer(act_stats_iters=1)
    assert tr.model_AK is not None and tr.model_AK.encoder.precision == "f32" and tr.model_AK.encoder.act_probe is not None
    assert not {id(p) for p in tr.model_AK.parameters()} & {id(p) for p in tr.model_AN.parameters()}
    assert tr.extra_state["act_stats.counters"] is tr.act_stats_state
    losses = torch.stack([_step(tr, k) for k in (1, 2)])
    path = os.path.join(directory, "state_00000002.cosa")
    tr.save_state(path, n_iter=tr.args.warmup_iters + 3)
    tr.wait_state()
    return dict(losses=losses, state=_state(tr), counters=tr.act_stats_state.cpu().clone(), summary=tr.act_stats(), path=path)


@pytest.fixture(scope="module")
def monitored_run(tmp_path_factory):
    return _monitored_run(str(tmp_path_factory.mktemp("act_stats")))


@functools.lru_cache(maxsize=None)
def _plain_run(directory):
    tr = _trainer()
    assert tr.act_stats_state is None and tr.model_AK is None and tr.act_stats() is None and "act_stats.counters" not in getattr(tr, "extra_state", {})
    losses = torch.stack([_step(tr, k) for k in (1, 2)])
    path = os.path.join(directory, "plain", "state_00000002.cosa")
    os.makedirs(os.path.dirname(path))
    tr.save_state(path, n_iter=tr.args.warmup_iters + 3)
    tr.wait_state()
    return dict(losses=losses, state=_state(tr), path=path)


def test_the_flag_changes_no_bit_of_the_run(monitored_run):
    """two steps: the five losses of each, the student's weights, the AdamW moments and the EMA teacher"""
    plain = _plain_run(os.path.dirname(monitored_run["path"]))
    assert torch.equal(plain["losses"].view(torch.int32), monitored_run["losses"].view(torch.int32))
    a, b = plain["state"], monitored_run["state"]
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k].reshape(-1).view(torch.uint8), b[k].reshape(-1).view(torch.uint8)), k


def test_the_counters_hold_two_passes_of_finite_numbers(monitored_run):
    s = monitored_run["summary"]
    rows = 2 * 2 * 2 * (17 + 5 + 37)
    assert s["checks"] == 2 and s["nonfinite"] == 0 and s["nonfinite_rows"] == 0 and s["over"] == 0
    assert all(h["rows"] == rows for layer in s["layers"] for h in layer["heads"])
    flat = [s["headroom_bits"], s["smax"], s["ent_mean"], s["ent_min"]] + \
        [h[k] for layer in s["layers"] for h in layer["heads"] for k in ("ent", "top1", "peaked", "smax", "sharpest")] + \
        [e["absmax"] for layer in s["layers"] for e in layer["sites"].values()]
    assert all(v is not None and math.isfinite(v) for v in flat)
    assert 0 < s["ent_min"] <= s["ent_mean"] <= 1 and s["smax"] > 0 and s["headroom_bits"] > 0


def test_a_state_file_restores_the_table_and_notes_say_what_differs(monitored_run, capsys):
    from cosa_amd import monitors
    row = monitors.BY_NAME["act_stats"]
    plain = _plain_run(os.path.dirname(monitored_run["path"]))
    tr = _trainer(seed=77, act_stats_iters=1)                # another seed: nothing of its own survives a load
    tr.act_stats_state.fill_(9)
    capsys.readouterr()
    tr.load_state(plain["path"])                             # only the run has the entry: its counters start at zero
    assert row.notes[1] in capsys.readouterr().out and int(tr.act_stats_state.abs().sum()) == 0
    assert tr.load_state(monitored_run["path"])["n_iter"] == tr.args.warmup_iters + 3
    assert row.notes[0] not in capsys.readouterr().out
    assert torch.equal(tr.act_stats_state.cpu(), monitored_run["counters"]) and tr.extra_state["act_stats.counters"] is tr.act_stats_state
    assert int(tr.act_stats_state[-1]) == 2
    tr = _trainer(seed=77)                                   # the file has the entry, the run does not: ignored, with a note
    capsys.readouterr()
    tr.load_state(monitored_run["path"])
    assert row.notes[0] in capsys.readouterr().out


def test_accum_steps_probes_on_the_closing_micro_batch_only():
    tr = _trainer(act_stats_iters=2, accum_steps=2)
    seen = []
    for it in (1, 2, 3, 4):
        for micro in (0, 1):
            _step(tr, 2 * it + micro, n_iter=tr.args.warmup_iters + it)
            seen.append(int(tr.act_stats_state[-1]))
    # optimizer steps n_iter = warmup + 1 .. 4: (n_iter + 1) % 2 == 0 selects every second one, on its last micro-batch
    want, checks = [], 0
    for it in (1, 2, 3, 4):
        for micro in (0, 1):
            checks += int((tr.args.warmup_iters + it + 1) % 2 == 0 and micro == 1)
            want.append(checks)
    assert seen == want and seen[-1] == 2


# ---- the tool and the launcher --------------------------------------------------------------------------------------------------------------
def test_the_tool_prints_the_table_and_one_json_summary():
    """tools/act_stats.py --synthetic at crop 64 on the seeded initialisation, gain 1 and gain 16, in fresh child processes"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    recs = {}
    for gain in ("1", "16"):
        cmd = [sys.executable, os.path.join(root, "tools", "act_stats.py"), "--synthetic", "--crop_size", "64", "--batch_size", "2", "--batches", "2",
               "--qk_gain", gain]
        res = subprocess.run(cmd, cwd=root, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stderr[-2000:]
        lines = res.stdout.strip().splitlines()
        assert len(lines) == 12 + 2 and all(lines[i].startswith("L%d " % i) for i in range(12)) and lines[12].startswith("act: headroom ")
        recs[gain] = json.loads(lines[-1])
    a, b = recs["1"], recs["16"]
    for key in ("checks", "layers", "headroom_bits", "headroom_at", "smax", "smax_at", "ent_mean", "ent_min", "over", "nonfinite", "mode", "qk_gain"):
        assert key in a, key
    assert a["checks"] == b["checks"] == 2 and a["mode"] == "fp32" and a["qk_gain"] == 1.0 and b["qk_gain"] == 16.0 and a["nonfinite"] == 0
    assert all(h["rows"] == 2 * 2 * 2 * (17 + 5 + 37) for h in a["layers"][0]["heads"])
    # block 0 sees the same stream in both runs: its logits are 16 x larger to rounding, and sharper
    s0 = lambda r: max(h["smax"] for h in r["layers"][0]["heads"])
    assert abs(s0(b) / s0(a) - 16.0) < 1e-3 and b["ent_mean"] < a["ent_mean"] and b["smax"] > a["smax"]


def test_the_launcher_logs_the_line_and_writes_the_jsonl_file(tmp_path, make_voc_tree):
    """python -m cosa_amd.main ... --act_stats_iters 2 --log_iters 4: one interval of four steps holds two passes"""
    import json
    import subprocess
    import sys
    root_dir = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import shutil
    import numpy as np
    from PIL import Image
    root, lists, names, _labels = make_voc_tree(tmp_path, n=6)
    os.makedirs(f"{root}/SegmentationClassAug")                 # (the launcher builds its validation loader whether or not it evaluates)
    for n in names:
        im = np.asarray(Image.open(f"{root}/JPEGImages/{n}.jpg"))
        Image.fromarray((im[..., 0] // 13).astype(np.uint8)).save(f"{root}/SegmentationClassAug/{n}.png")
    shutil.copy(f"{lists}/train_aug.txt", f"{lists}/val.txt")
    work = str(tmp_path / "work")
    env = dict(os.environ, PYTHONPATH=root_dir + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "cosa_amd.main", "EXP_A", "--work_dir", work, "--dataset", "VOC12", "--voc12_root", root, "--name_list_dir", lists,
           "--max_iters", "4", "--warmup_iters", "1", "--eval_iters", "100", "--log_iters", "4", "--aux_layer", "-4", "--crop_size", "64",
           "--batch_size", "2", "--num_workers", "0", "--pretrained", "false", "--finalval", "false", "--act_stats_iters", "2"]
    r = subprocess.run(cmd, cwd=root_dir, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Iter: 4;" in r.stdout and " act: headroom " in r.stdout and "max|s| " in r.stdout, r.stdout[-3000:]
    recs = [json.loads(x) for x in open(os.path.join(work, "EXP_A", "act_stats.jsonl")).read().splitlines()]
    assert len(recs) == 1 and recs[0]["iters"] == 4 and recs[0]["checks"] == 2 and recs[0]["mode"] == "fp32" and recs[0]["nonfinite"] == 0
    assert len(recs[0]["layers"]) == 12 and recs[0]["layers"][11]["heads"][0]["rows"] == 2 * 2 * 2 * (17 + 5 + 37)
