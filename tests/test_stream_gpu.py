"""GPU tests of the student's fp32 residual stream (round 4): the LayerNorm-backward kernel with the fp32 skip gradient, the
(projection + residual add, LayerNorm) autograd node, the fp32 gradient junction at the final norm's output, grouped deferred weight
gradients, and the loud refusal of shapes / dtypes the HIP path does not cover.

Reference: models/vit/vit.py:154-158 (`x = x + attn(norm1(x)); x = x + mlp(norm2(x))`) under main.py:124-246 (fp32, no autocast)."""
import math

import pytest
import torch

from torch_reference import torch_reference_ops

pytestmark = pytest.mark.gpu


def _cos(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a @ b) / (a.norm() * b.norm() + 1e-300))


@pytest.mark.parametrize("rows,dy32,skip", [(1570, False, True), (12560, False, True), (777, True, False), (64, False, False), (3, True, True)])
def test_layernorm_bwd_f32_vs_torch(rows, dy32, skip):
    """cosa_layernorm_bwd_f32 against torch autograd of F.layer_norm in fp32 on the same (bf16-rounded) dy / gamma: dx within 2e-6 of the
    row's scale, dgamma / dbeta within 1e-5 relative, the bf16 copy equal to the rounded fp32 result bit for bit"""
    from cosa_amd import nn_ops
    g = torch.Generator(device="cpu").manual_seed(rows)
    dev = torch.device("cuda", 0)
    x = (torch.randn(rows, 768, generator=g) * 1.7 + 0.3).to(dev)
    gam = (1 + 0.2 * torch.randn(768, generator=g)).to(dev)
    dy = torch.randn(rows, 768, generator=g).to(dev)
    dy_in = dy if dy32 else dy.to(torch.bfloat16)
    dsk = torch.randn(rows, 768, generator=g).to(dev) if skip else None
    g16 = gam.to(torch.bfloat16)
    dx, dx16, dgamma, dbeta = nn_ops._ln_backward_f32(dy_in, x, g16, 1e-6, dsk, True)
    xr = x.clone().requires_grad_(True)
    wr = g16.float().clone().requires_grad_(True)
    br = torch.zeros(768, device=dev, requires_grad=True)
    y = torch.nn.functional.layer_norm(xr, (768,), wr, br, 1e-6)
    y.backward(dy_in.float())
    ref = xr.grad + (dsk if skip else 0)
    scale = ref.abs().amax(dim=1, keepdim=True)
    assert float(((dx - ref).abs() / scale).max()) < 2e-6
    assert torch.equal(dx16, dx.to(torch.bfloat16))
    assert float((dgamma - wr.grad).abs().max()) <= 1e-5 * float(wr.grad.abs().max()) + 1e-6
    assert float((dbeta - br.grad).abs().max()) <= 1e-5 * float(br.grad.abs().max()) + 1e-6


def _shadowed_linear(K, N, dev, seed):
    from cosa_amd import nn_ops
    torch.manual_seed(seed)
    lin = torch.nn.Linear(K, N).to(dev)
    torch.nn.init.normal_(lin.bias, std=0.1)
    norm = torch.nn.LayerNorm(N, eps=1e-6).to(dev)
    with torch.no_grad():
        norm.weight.add_(0.1 * torch.randn_like(norm.weight))
        norm.bias.add_(0.1 * torch.randn_like(norm.bias))
    holder = torch.nn.ModuleList([lin, norm])
    ss = nn_ops.ensure_shadows(holder)                       # bf16 shadows of W, b, gamma, beta
    wt = nn_ops.TransposedShadows([lin.weight])              # bf16 W^T for the input-gradient GEMM
    return lin, norm, (holder, ss, wt)


@pytest.mark.parametrize("M,K,y_f32", [(1570, 768, False), (12560, 3072, False), (12560, 768, True)])
def test_residual_linear_ln_vs_fp32_torch(M, K, y_f32):
    """ResidualLinearLNFn (persistent GEMM with the fp32 residual epilogue + LayerNorm, and its one-node backward) against fp32 torch
    autograd on the SAME bf16-rounded operands: x' within 1e-5 of its scale (fp32 accumulation order only), y within bf16 rounding,
    gradients w.r.t. a / x / W / b / gamma / beta by cosine >= 0.9999 and norm ratio within 1e-3 (the only extra rounding is dY -> bf16)"""
    from cosa_amd import nn_ops
    dev = torch.device("cuda", 0)
    lin, norm, keep = _shadowed_linear(K, 768, dev, seed=M + K)
    g = torch.Generator(device="cpu").manual_seed(K)
    a = torch.randn(M, K, generator=g).to(dev).to(torch.bfloat16).requires_grad_(True)
    x = (torch.randn(M, 768, generator=g) * 2).to(dev).requires_grad_(True)
    xn, y = nn_ops.residual_linear_ln(a, x, lin, norm, y_f32=y_f32)
    assert xn.dtype == torch.float32 and y.dtype == (torch.float32 if y_f32 else torch.bfloat16)
    gx = torch.randn(M, 768, generator=g).to(dev)
    gy = torch.randn(M, 768, generator=g).to(dev)
    gy_in = gy if y_f32 else gy.to(torch.bfloat16)
    torch.autograd.backward([xn, y], [gx, gy_in])
    got = dict(a=a.grad.float(), x=x.grad, W=lin.weight.grad, b=lin.bias.grad, gamma=norm.weight.grad, beta=norm.bias.grad)
    # fp32 reference on the rounded operands
    ar = a.detach().float().requires_grad_(True)
    xr = x.detach().clone().requires_grad_(True)
    W = lin.weight.detach().to(torch.bfloat16).float().requires_grad_(True)
    b = lin.bias.detach().to(torch.bfloat16).float().requires_grad_(True)
    gam = norm.weight.detach().to(torch.bfloat16).float().requires_grad_(True)
    bet = norm.bias.detach().to(torch.bfloat16).float().requires_grad_(True)
    xnr = xr + ar @ W.t() + b
    yr = torch.nn.functional.layer_norm(xnr, (768,), gam, bet, 1e-6)
    assert float((xn - xnr).abs().max()) <= 2e-5 * float(xnr.abs().max())
    tol = 1e-5 if y_f32 else 2 ** -8
    assert float((y.float() - yr).abs().max()) <= tol * float(yr.abs().max()) + 1e-6
    torch.autograd.backward([xnr, yr], [gx, gy_in.float()])
    ref = dict(a=ar.grad, x=xr.grad, W=W.grad, b=b.grad, gamma=gam.grad, beta=bet.grad)
    for k in got:
        cs, ratio = _cos(got[k], ref[k]), float(got[k].norm() / ref[k].norm())
        assert cs >= 0.9999 and abs(ratio - 1) < 2e-3, (k, cs, ratio)
    assert float((got["x"] - ref["x"]).abs().max()) <= 1e-5 * float(ref["x"].abs().max())      # the stream gradient stays fp32-exact


class _FanoutRef(torch.autograd.Function):
    """what nn_ops.patch_fanout_bf16 replaced (round 4's nn_ops.FanoutBf16Fn, kept here as the reference): fp32 x -> n views of one bf16 cast;
    backward: the consumers' bf16 gradients added up in fp32, in consumer order"""

    @staticmethod
    def forward(ctx, x, n):
        x16 = x.to(torch.bfloat16)
        return tuple(x16.view_as(x16) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        acc = None
        for g in gs:
            if g is not None:
                acc = g.float() if acc is None else acc.add_(g)
        return acc, None


@pytest.mark.parametrize("live", [(0, 1, 2), (0, 2), (1,)])
def test_patch_fanout_equals_the_sliced_fanout(live):
    """nn_ops.patch_fanout_bf16 (one bf16 copy of the patch tokens, the consumers' gradients summed by cosa_token_junction_bwd) against what it
    replaced: a fan-out of the whole token tensor (_FanoutRef above) + a [:, 1:] slice per consumer -- same forward bits, same gradient bits (fp32 adds in
    consumer order, zero class-token row), also when some consumers take no part in the backward pass (ragged N)"""
    from cosa_amd import nn_ops
    dev = torch.device("cuda", 0)
    B, N = 3, 198
    x = torch.randn(B, N, 768, device=dev, requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    outs = nn_ops.patch_fanout_bf16(x, 3)
    refs = [t[:, 1:] for t in _FanoutRef.apply(x2, 3)]
    assert all(o.shape == (B, N - 1, 768) and o.is_contiguous() and torch.equal(o, r) for o, r in zip(outs, refs))
    assert outs[0].data_ptr() == outs[1].data_ptr() == outs[2].data_ptr()
    gs = [torch.randn(B, N - 1, 768, device=dev).to(torch.bfloat16) for _ in range(3)]
    torch.autograd.backward([outs[i] for i in live], [gs[i] for i in live])
    torch.autograd.backward([refs[i] for i in live], [gs[i] for i in live])
    assert x.grad.dtype == torch.float32 and torch.equal(x.grad, x2.grad) and float(x.grad[:, 0].abs().max()) == 0.0


def _student_grads(tr, batch, n_iter, stream, groups):
    enc = tr.student.encoder
    enc.residual_stream, enc.defer_groups = stream, groups
    tr.optimizer.zero_grad(set_to_none=True)
    loss, logs = tr.forward_losses(*batch, n_iter)
    loss.backward()
    return float(loss), {n: p.grad.detach().clone() for n, p in tr.student.named_parameters() if p.grad is not None}


def test_grouped_deferred_wgrad_is_bit_identical_and_streams_agree():
    """(a) the blocks' weight gradients through 1, 3, 4 or 12 DeferredWgrad groups are the same bits (every 256 x 128 tile of dW runs the
    whole token loop whatever launch it is part of) -- the grouped form is what runs under data parallelism; (b) fp32-stream and bf16-stream
    students agree closely (cosine >= 0.97 everywhere) -- they are the same network, the difference is rounding"""
    from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch
    dev = torch.device("cuda", 0)
    S, b = 224, 4
    args = default_args("VOC12", crop_size=S, batch_size=b, teacher_graph=False, teacher_async=False)
    tr = CoSATrainer(args, dev, seed=11)
    batch = synthetic_batch(b, S, 20, dev, seed=13)
    n_iter = args.warmup_iters + 1
    l1, g1 = _student_grads(tr, batch, n_iter, "fp32", 1)
    assert len(g1) > 100 and all(torch.isfinite(v).all() for v in g1.values())
    for groups in (3, 4, 12):
        lg, gg = _student_grads(tr, batch, n_iter, "fp32", groups)
        assert lg == l1
        for n, v in g1.items():
            assert torch.equal(gg[n], v), (groups, n)
    tr.student.encoder.defer_wgrad = False
    ln, gn = _student_grads(tr, batch, n_iter, "fp32", 1)
    tr.student.encoder.defer_wgrad = True
    for n, v in g1.items():           # per-layer launches split the token range (fixed-order slab sums): same value up to fp32 summation order
        assert float((gn[n] - v).abs().max()) <= 1e-4 * float(v.abs().max()) + 1e-9, n
    lb, gb = _student_grads(tr, batch, n_iter, "bf16", 1)
    assert lb == pytest.approx(l1, rel=5e-3)
    for n in ("encoder.blocks.0.attn.qkv.weight", "encoder.blocks.6.mlp.fc1.weight", "encoder.blocks.11.mlp.fc2.weight", "decoder.conv6.weight",
              "classifier.weight", "encoder.norm.weight"):
        assert _cos(gb[n], g1[n]) >= 0.97, (n, _cos(gb[n], g1[n]))


def test_shapes_outside_the_hip_path_raise_instead_of_falling_back():
    """north_star: "no dual backend" -- a CUDA tensor that no kernel of this repository covers raises CosaError; torch's own operators run
    only inside torch_reference_ops() (tests)"""
    from cosa_amd import nn_ops, _C
    dev = torch.device("cuda", 0)
    qkv32 = torch.randn(1, 65, 3 * 2 * 64, device=dev)
    with pytest.raises(_C.CosaError):
        nn_ops.attention(qkv32, 2)
    lin = torch.nn.Linear(96, 40).to(dev)                    # no shadows, odd shape
    x = torch.randn(7, 96, device=dev, dtype=torch.bfloat16)
    with pytest.raises(_C.CosaError):
        nn_ops.linear(x, lin.weight, lin.bias, torch.bfloat16)
    with torch_reference_ops():
        y = nn_ops.linear(x, lin.weight, lin.bias, torch.bfloat16)
        o = nn_ops.attention(qkv32, 2)
    assert y.shape == (7, 40) and o.shape == (1, 65, 128) and math.isfinite(float(o.sum()))
    with pytest.raises(_C.CosaError):                        # the switch is scoped
        nn_ops.attention(qkv32, 2)


@pytest.mark.parametrize("S,mode,use_act", [(64, "fp16c8-x2", True), (64, "bf16", False), (224, "fp16c8-x2", True), (64, "fp16x3", True)])
def test_teacher_graph_every_replay_equals_the_eager_pass(S, mode, use_act):
    """Round 6: the captured teacher pass must give the eager pass's bits on EVERY replay, not only on the first.  It did not: the min-max
    normalisation initialised its per-plane keys with hipMemsetAsync, and inside a captured hipGraph those memset nodes were not ordered with the
    kernels around them from the second replay on -- the auxiliary CAM came out NaN (and the main CAM altered at 224^2 / 448^2) in every step
    of the benchmarked loop but the one that captured the graph; every test before this one looked at eager passes or at the first replay.
    The keys are now set by a kernel (csrc/label_kernels.hip: minmax_init_kernel)."""
    from cosa_amd import nn_ops
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args, synthetic_batch
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    wimg, _, lab, _ = synthetic_batch(2, S, 20, dev, seed=100)
    args = default_args("VOC12", crop_size=S, batch_size=2)
    torch.manual_seed(0)
    net = build_model(args).to(dev).eval()
    net.set_nograd_precision(mode)
    nn_ops.ensure_shadows(net, net.compute_dtype)
    bufs = {} if use_act else None
    run = lambda: seg_helper.multi_scale_camseg(net, wimg, args.pseudo_scales, _active_labels=lab if use_act else None, _seg_scales=True, _buffers=bufs)
    with torch.no_grad():
        for _ in range(2):
            e = run()
        torch.cuda.synchronize()
        ref = [e[0].clone(), e[1].clone()] + [t.clone() for t in e[2]]
        assert all(torch.isfinite(t).all() for t in ref)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            out = run()
        for rep in range(4):
            g.replay()
            torch.cuda.synchronize()
            for name, c, r in zip(("cam", "cam_aux", "seg0", "seg1", "seg2"), [out[0], out[1]] + list(out[2]), ref):
                assert torch.equal(c, r), (rep + 1, name, float((c - r).abs().max()))


def test_captured_teacher_keeps_its_operand_buffers_through_evictions():
    """the activation-buffer cache pins what a captured graph replays into: a captured fp16x3 pass (the trainer's mode), then nine other
    token geometries eagerly -- more than the cache's bound, one of them with the SAME row count and another (images, tokens) split, whose
    token-shaped patch operand has its zero class-token rows elsewhere -- and the replay still gives the eager pass's bits"""
    from cosa_amd.models import build_model
    from cosa_amd.train_step import default_args
    torch.manual_seed(0)
    net = build_model(default_args("VOC12", crop_size=64)).cuda().eval()
    net.set_nograd_precision("fp16x3")
    xa, xb = torch.randn(2, 3, 64, 64, device="cuda"), torch.randn(1, 3, 48, 176, device="cuda")       # 34 token rows each
    others = [xb] + [torch.randn(1, 3, 16, 16 * wd, device="cuda") for wd in range(1, 9)]
    with torch.no_grad():
        for _ in range(2):
            e = net.forward_multi([xa], need_cls=False)[0]
        torch.cuda.synchronize()
        ref = [t.clone() for t in e if t is not None]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            out = [t for t in net.forward_multi([xa], need_cls=False)[0] if t is not None]
        for x in others:
            net.forward_multi([x], need_cls=False)
        assert len(net.encoder._operand_bufs) <= net.encoder._BUFS_MAX
        g.replay()
        torch.cuda.synchronize()
    assert len(out) == len(ref) == 4                       # feature map, seg, cam, cam_aux
    for j, (c, r) in enumerate(zip(out, ref)):
        assert torch.equal(c, r), j


def test_trainer_with_the_captured_teacher_trains_the_same_weights_as_with_the_eager_one():
    """the same at the level of the training loop: six steps with the teacher as a replayed hipGraph on the side stream (the benchmarked
    configuration) and six with the eager teacher give bit-identical student and teacher weights and the same label maps in every step"""
    from cosa_amd.train_step import CoSATrainer, default_args, synthetic_batch
    dev = torch.device("cuda", 0)
    wimg, simg, lab, box = synthetic_batch(2, 64, 20, dev, seed=100)
    res = {}
    for graph in (False, True):
        tr = CoSATrainer(default_args("VOC12", crop_size=64, batch_size=2, teacher_graph=graph, lr=1e-3), dev, seed=0)
        masks = []
        for _ in range(6):
            logs = tr.step(wimg, simg, lab, box, n_iter=10 ** 6)
            masks.append(logs["mask"].clone())
        torch.cuda.synchronize()
        assert (tr._graph is not None) == graph
        res[graph] = (masks, {k: v.detach().clone() for k, v in tr.student.named_parameters()}, {k: v.detach().clone() for k, v in tr.model_AN.named_parameters()})
    for a, b in zip(res[False][0], res[True][0]):
        assert torch.equal(a, b) and int(((a > 0) & (a < 255)).sum()) > 0
    for i in (1, 2):
        for k in res[False][i]:
            assert torch.equal(res[False][i][k], res[True][i][k]), k
