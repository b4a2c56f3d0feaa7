"""ViT-B/16 encoder of the CoSA network, MI355X-native execution.

Reference: models/vit/vit.py:86-181 (Mlp/Attention/Block/PatchEmbed), :219-330 (VisionTransformer,
prepare_tokens, forward_features), :365-377 (vit_base_patch16_224).  Module / parameter names are
kept so the reference's state_dict (and the released checkpoints) load unchanged.

Execution differs from the reference on purpose:
  * tokens stay [B, N, 768] (== NHWC) end to end; no NCHW transposes
  * patch embedding is an im2col view + one GEMM (the 16x16/16 conv is exactly that)
  * attention is the fused HIP kernel on the packed qkv buffer (no [B,12,N,N] tensor, no permutes)
  * the bicubic position-embedding resize is cached per token grid (pos_embed is frozen)
  * bf16 compute with fp32 master weights (compute_dtype=torch.float32 is the parity mode)
"""
import typing
from functools import partial

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import nn_ops


_OP16 = (torch.bfloat16, torch.float16)       # MFMA operand types of the HIP path (fp16: no-grad passes only)


class FP32Tokens:
    """what the training path on the fp32 residual stream hands to VITNetwork._heads instead of the (cls, tokens, aux tokens, fp32 tokens)
    tuple: the final norm's output and the auxiliary layer's output, both fp32 [B, N, 768] including the class-token row"""

    def __init__(self, final, aux):
        self.final, self.aux = final, aux


class OperandMap(typing.NamedTuple):
    """operand formats of a no-grad pass (VisionTransformer._operand_map): of the patch projection -- the family that assembles the tokens and
    closes with its LayerNorm -- and per block of the attention half and the MLP half: "plain", "x3", "c8", "c4" (qkv / fc1 / fc2 on fp16c4
    operands in an otherwise fp16c8 half), "f32" (fp32 operands read from the fp32 masters: all of the pass or none of it) or "f64" (float64
    activations on the f64 MFMA, the fp32 masters widened inside the kernels: all or none likewise)"""
    patch: str
    attn: tuple
    mlp: tuple
    plain_qkv: bool            # the qkv projections of the c8 / c4 halves on plain fp16 operands (the output projection keeps its terms)
    c4_proj: bool              # the output projections of the c4 halves on fp16c4 operands too (default: fp16c8)
    dt16: object               # type of the plain operands
    hdt: object                # type of the hi / lo halves of the x3 operands

    def of(self, i, name):
        """operand format of projection `name` ("qkv", "proj", "fc1", "fc2") of block i"""
        half = (self.attn if name in ("qkv", "proj") else self.mlp)[i]
        if half in ("c8", "c4") and name == "qkv" and self.plain_qkv:
            return "plain"
        if half == "c4" and name == "proj" and not self.c4_proj:
            return "c8"
        return half

    def uses(self, fmt):
        return fmt in self.attn or fmt in self.mlp


class TokenPack(typing.NamedTuple):
    """the token rows of several image batches in one [M, D] buffer: batch i is `shapes[i]` = (images, tokens per image) at rows offs[i]:offs[i+1]"""
    shapes: tuple
    offs: tuple
    M: int
    Kp: int                    # width of an im2col row
    nf: int                    # 2: every batch stands for cat(x, x.flip(-1))
    dev: object

    def scales(self):
        return [(B, N, o0, o1) for (B, N), o0, o1 in zip(self.shapes, self.offs[:-1], self.offs[1:])]

    def cut(self, a16, xn32, aux, D):
        """per batch (cls fp32, 16-bit tokens, aux tokens, fp32 tokens); a16 may be operand rows whose first D columns are the tokens"""
        outs = []
        for B, N, o0, o1 in self.scales():
            t16, a32, ax = a16[o0:o1].view(B, N, -1)[:, :, :D], xn32[o0:o1].view(B, N, D), aux[o0:o1].view(B, N, D)
            outs.append((a32[:, 0], t16[:, 1:], ax[:, 1:], a32[:, 1:]))
        return outs


ACT_SITES = ("q", "k", "v", "o", "h", "x")      # the range sites of a block, in the table's order (seg_helper.act_stats_layout)


class ActProbe:
    """what `VisionTransformer.act_probe` holds: an int64 table [depth][6 * 6 + H * 7] on the device, row i = block i:
    six words per range site (ACT_SITES), then seven per head.  The fp32 no-grad path calls `site` after the launch that produced a site
    and `attn` per scale before the attention launch's output is consumed; both add into row `layer` (nn_ops.range_stats / attn_stats),
    on the current stream, without a host sync.  `table` may be a view of a longer vector (the trainer's counters)."""

    def __init__(self, depth, heads, device=None, table=None):
        self.depth, self.heads, self.width = int(depth), int(heads), 6 * len(ACT_SITES) + 7 * int(heads)
        self.table = torch.zeros((self.depth, self.width), dtype=torch.int64, device=device) if table is None else table
        assert self.table.shape == (self.depth, self.width) and self.table.dtype == torch.int64 and self.table.is_contiguous()

    def site(self, layer, name, x, col0=0, cols=None):
        j = ACT_SITES.index(name)
        nn_ops.range_stats(x, self.table[layer, 6 * j:6 * j + 6], col0, cols)

    def attn(self, layer, qkv, B, N, H):
        assert H == self.heads
        nn_ops.attn_stats(qkv, B, N, H, self.table[layer, 6 * len(ACT_SITES):])


@torch.no_grad()
def qk_gain_(module, gain):
    """multiply the q rows and the k rows (weights and biases) of every Block's qkv projection under `module` by sqrt(gain), in place: every
    attention logit becomes `gain` times larger, nothing else of the network is touched (v, the output projection and the MLP read the
    same inputs; only the softmax sharpens).  The "sharp attention" recipe of the conformance tools (--qk_gain); 1 touches nothing."""
    gain = float(gain)
    if not gain > 0 or gain == float("inf"):
        raise ValueError(f"qk_gain {gain!r}: a positive finite factor")
    if gain == 1.0:
        return module
    f = gain ** 0.5
    for blk in module.modules():
        if isinstance(blk, Block):
            two_d = 2 * blk.attn.qkv.weight.shape[0] // 3
            blk.attn.qkv.weight[:two_d] *= f
            if blk.attn.qkv.bias is not None:
                blk.attn.qkv.bias[:two_d] *= f
    return module


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features)
        self.fc2 = nn.Linear(hidden_features, in_features)


class Attention(nn.Module):
    def __init__(self, dim, num_heads, qkv_bias=True):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.proj = nn.Linear(dim, dim)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio=4.0, qkv_bias=True, eps=1e-6):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = Attention(dim, num_heads, qkv_bias)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))


class PatchEmbed(nn.Module):
    def __init__(self, img_size=224, patch_size=16, in_chans=3, embed_dim=768):
        super().__init__()
        self.img_size = (img_size, img_size)
        self.patch_size = (patch_size, patch_size)
        self.num_patches = (img_size // patch_size) ** 2
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=patch_size)


def _trunc_normal_(t, std=0.02):
    return nn.init.trunc_normal_(t, std=std)


class VisionTransformer(nn.Module):
    """models/vit/vit.py:219-330"""

    def __init__(self, img_size=224, patch_size=16, in_chans=3, num_classes=1000, embed_dim=768, depth=12, num_heads=12,
                 mlp_ratio=4.0, qkv_bias=True, aux_layer=-3, eps=1e-6, compute_dtype=torch.bfloat16):
        super().__init__()
        self.num_classes = num_classes
        self.num_features = self.embed_dim = embed_dim
        self.patch_embed = PatchEmbed(img_size, patch_size, in_chans, embed_dim)
        num_patches = self.patch_embed.num_patches
        self.cls_token = nn.Parameter(torch.zeros(1, 1, embed_dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, num_patches + 1, embed_dim))
        self.pos_embed.requires_grad = False                      # vit.py:237
        self._size = img_size // patch_size
        self.patch_size = patch_size
        self.aux_layer = aux_layer
        self.num_heads = num_heads
        self.blocks = nn.ModuleList([Block(embed_dim, num_heads, mlp_ratio, qkv_bias, eps) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=eps)
        self.head = nn.Linear(embed_dim, num_classes) if num_classes > 0 else nn.Identity()   # unused by the path (vit.py:257,325)
        self.compute_dtype = compute_dtype
        self.precision = None          # "bf16x3" / "fp16c8" / "fp16c4": parity-grade operand representations of the no-grad passes;
        #                                "f32": fp32 operands on the f32-input MFMA (mode string "fp32")
        #                                "f64": float64 operands on the f64 MFMA (mode string "fp64", section 20: a check mode)
        # residual stream of the TRAINING path: "fp32" (default since round 4: the reference trains in fp32, main.py:124-246 -- the sums
        # x + attn(..), x + mlp(..) and the gradient sums of the skip connections are formed and kept in fp32; MFMA operands stay bf16) or
        # "bf16" (rounds 1-3: the stream itself rounded to 8 significant bits after every add; kept for A/B measurements)
        self.residual_stream = "fp32"
        self.defer_wgrad = True        # the blocks' weight gradients in batched launches (nn_ops.DeferredWgrad) ...
        self.defer_groups = None       # ... one launch per group of depth / defer_groups blocks; None: 1 on a single GPU, 6 under data parallelism
        self.c8_plain_from = None      # fp16c8 / fp16c4: blocks with index >= this run on plain fp16 operands ("fp16c8-9": the last three)
        self.c8_plain_mlp_from = None  # ... their MLP halves (norm2, fc1, fc2) already from this block on (None: as c8_plain_from)
        self.x3_until = None           # fp16c8 / fp16c4: blocks with index < this run on bf16x3 operands ("fp16c8-x6"); x3_mlp_until: their MLP halves
        self.x3_mlp_until = None
        self.x3_dtype = torch.bfloat16   # type of the hi / lo halves of the three-term path: bf16 ("bf16x3") or fp16 ("fp16x3")
        self.c4_from = None            # fp16c8: blocks with index >= this take their qkv / fc1 / fc2 on fp16c4 operands ("fp16c8-x2c6": mixed maps, round 5)
        self.c8_plain_qkv = False      # ... the qkv projections of the corrected blocks on plain fp16 operands too (the output projection keeps its terms)
        # fp16c4: the output projection too on fp16c4 operands (the attention kernel then writes c4 rows)?  Measured (round 4, three seeds, 448^2):
        # the auxiliary CAM's worst error goes from 4.5e-4 to 5.1e-4 (margin on the 1e-3 bar 2.2x -> 1.95x) for 0.15 ms per step, so it is off:
        # proj stays on fp16c8 operands (e5m2 corrections), 10 % of the projection work
        self.c4_proj = False
        self.act_probe = None          # an ActProbe: the fp32 no-grad path reports every block's q / k / v / o / h / x and its attention logits to it
        #                                (--act_stats_iters); None: nothing is launched.  Only the "f32" family is probed
        self._pos_cache = {}
        _trunc_normal_(self.pos_embed)
        _trunc_normal_(self.cls_token)
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            _trunc_normal_(m.weight)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    # -- vit.py:283-300 ---------------------------------------------------------------------------
    def _pos_for_grid(self, h, w, dtype):
        """bicubic resize of the 14x14 position grid (vit.py:288-291).  The resize is linear in pos_embed, so it is
        applied as a cached [h*w,196] interpolation matrix (built once per grid with the same bicubic kernel) times
        the current pos_embed -- the teacher's pos_embed is EMA-touched every step, so caching the RESULT would go
        stale, and torch's bicubic kernel costs ~3 ms per call on this shape."""
        pe = self.pos_embed
        key = (h, w, pe.device)
        ent = self._pos_cache.get(key)
        if ent is None:
            n0 = self._size * self._size
            with torch.no_grad():
                eye = torch.eye(n0, device=pe.device, dtype=torch.float32).reshape(1, n0, self._size, self._size)
                mat = F.interpolate(eye, size=(h, w), mode="bicubic", align_corners=False).reshape(n0, h * w).t().contiguous()
                # bicubic: at most 4 x 4 source cells per output token -> the 16 largest-magnitude entries of a row are all its non-zeros
                wgt, idx = torch.topk(mat.abs(), 16, dim=1)
                wgt = torch.gather(mat, 1, idx)
                assert float((mat.abs().sum(1) - wgt.abs().sum(1)).abs().max()) < 1e-6
            ent = {"mat": mat, "idx": idx.to(torch.int32).contiguous(), "wgt": wgt.contiguous()}
            self._pos_cache[key] = ent
        with torch.no_grad():      # recomputed every pass so a captured graph never holds a stale value
            src = pe[0, 1:, :].float().contiguous()
            if pe.is_cuda and self.embed_dim % 4 == 0:
                from .. import _C
                grid = torch.empty((h * w, self.embed_dim), device=pe.device, dtype=torch.float32)
                _C.check(_C.lib().cosa_pos_resize(_C.ptr(src), _C.ptr(ent["idx"]), _C.ptr(ent["wgt"]), _C.ptr(grid), h * w, self.embed_dim,
                                                  _C.stream_ptr()), "cosa_pos_resize")
            else:
                grid = ent["mat"] @ src
            return torch.cat((pe[0, :1, :].float(), grid), dim=0).unsqueeze(0).to(dtype)

    def prepare_tokens(self, x, stream_f32=False):
        """stream_f32 (training on the fp32 residual stream): class token, position rows and their sum in fp32; the patch projection itself
        runs on bf16 operands like every other projection"""
        B, nc, H, W = x.shape
        p = self.patch_size
        h, w = H // p, W // p
        dt = self.compute_dtype
        # im2col view of the stride-16 conv: [B, h*w, 3*16*16] @ W^T
        cols = x.to(dt).reshape(B, nc, h, p, w, p).permute(0, 2, 4, 1, 3, 5).reshape(B, h * w, nc * p * p)
        wgt = nn_ops.cast_param(self.patch_embed.proj.weight, dt).reshape(self.embed_dim, -1)
        bias = nn_ops.cast_param(self.patch_embed.proj.bias, dt)
        if dt in _OP16 and x.is_cuda and not torch.is_grad_enabled() and wgt.shape[0] % 128 == 0 and wgt.shape[1] % 64 == 0:
            # no-grad (teacher / evaluation): the patch projection on our own MFMA GEMM -- like every other kernel of the CAM / seg
            # path its result for a token does not depend on the batch around it
            tok = nn_ops.gemm_bf16(cols.reshape(B * h * w, -1).contiguous(), wgt.contiguous(), bias.contiguous(), nn_ops.EPI_BIAS).view(B, h * w, -1)
        elif dt == torch.bfloat16 and x.is_cuda and torch.is_grad_enabled() and self.patch_embed.proj.weight.requires_grad:
            # training: the same GEMM kernels with autograd (LinearShadowFn on the [768, 3*16*16] view of the conv weight)
            tok = nn_ops.linear_view2d(cols, self.patch_embed.proj.weight, self.patch_embed.proj.bias, dt)
        else:
            tok = nn_ops.reference_op("linear", f"patch projection ({dt}, embed {self.embed_dim})", cols, wgt, bias)
        if stream_f32:
            tok = torch.cat((self.cls_token.float().expand(B, -1, -1), tok.float()), dim=1)
            return tok + self._pos_for_grid(h, w, torch.float32), h, w
        cls = nn_ops.cast_param(self.cls_token, dt).expand(B, -1, -1)
        tok = torch.cat((cls, tok), dim=1)
        return tok + self._pos_for_grid(h, w, dt), h, w

    def _block(self, blk, x):
        dt = self.compute_dtype
        c = nn_ops.cast_param
        ln = lambda t, n: nn_ops.reference_op("layer_norm", f"LayerNorm({self.embed_dim}) on {dt}", t, c(n.weight, dt), c(n.bias, dt), n.eps)
        y = ln(x, blk.norm1)
        qkv = nn_ops.linear(y, blk.attn.qkv.weight, blk.attn.qkv.bias, dt)
        y = nn_ops.attention(qkv, self.num_heads)
        x = x + nn_ops.linear(y, blk.attn.proj.weight, blk.attn.proj.bias, dt)
        y = ln(x, blk.norm2)
        y = nn_ops.linear(y, blk.mlp.fc1.weight, blk.mlp.fc1.bias, dt, act=True)
        return x + nn_ops.linear(y, blk.mlp.fc2.weight, blk.mlp.fc2.bias, dt)

    def _block_fused_ln(self, blk, x, delta):
        """training-path block on the bf16 stream with the residual adds folded into the LayerNorm kernels: takes the stream x and the
        not-yet-added output `delta` of the previous block's MLP (None for the first block), returns (x_in, x', delta'):
        x_in = x + delta is the previous block's output as it materialises here, the block's own output is x' + delta'."""
        dt = self.compute_dtype
        x, y = nn_ops.add_layernorm(x, delta, blk.norm1.weight, blk.norm1.bias, blk.norm1.eps)
        x_in = x
        qkv = nn_ops.linear(y, blk.attn.qkv.weight, blk.attn.qkv.bias, dt)
        y = nn_ops.attention(qkv, self.num_heads)
        d1 = nn_ops.linear(y, blk.attn.proj.weight, blk.attn.proj.bias, dt)
        x, y = nn_ops.add_layernorm(x, d1, blk.norm2.weight, blk.norm2.bias, blk.norm2.eps)
        y = nn_ops.linear(y, blk.mlp.fc1.weight, blk.mlp.fc1.bias, dt, act=True)
        return x_in, x, nn_ops.linear(y, blk.mlp.fc2.weight, blk.mlp.fc2.bias, dt)

    # -- fused no-grad path (the teacher's 6 passes, evaluation): fp32 residual stream, HIP GEMM / LN / attention kernels ----------------
    #    Operand formats of a projection: "plain" (bf16 or fp16), "x3" (hi + lo 16-bit halves, three MFMA terms: bf16x3 / fp16x3), "c8" (fp16 +
    #    8-bit correction terms, csrc/c8.hpp; attention on plain fp16 q, k, v, its OUTPUT leaves as c8 rows) and "c4" (fp16 + FP4 MX-block
    #    correction terms, csrc/c4.hpp).  tools/sim_precision_map.py is the sensitivity study behind the mixed maps.
    def _plain_from(self):
        """(first block whose attention half, first block whose MLP half) runs on plain fp16 operands in the fp16c8 / fp16c4 modes"""
        a = self.c8_plain_from if self.c8_plain_from is not None else len(self.blocks)
        return a, (self.c8_plain_mlp_from if self.c8_plain_mlp_from is not None else a)

    def _x3_until(self):
        """(xa, xm): the attention halves of blocks < xa and the MLP halves of blocks < xm of an fp16c8 / fp16c4 pass run on bf16x3 operands
        (16 significant bits: "fp16c8-x6", "fp16c8-x6m4") -- the early blocks, whose rounding passes through the most layers"""
        xa = self.x3_until if getattr(self, "x3_until", None) is not None else 0
        return xa, (self.x3_mlp_until if getattr(self, "x3_mlp_until", None) is not None else xa)

    def _is_c4(self, i):
        """does block i take its qkv / fc1 / fc2 projections on fp16c4 operands?  (every block in the fp16c4 modes; blocks >= c4_from in the mixed
        fp16c8 maps: the late blocks, whose rounding passes through the fewest layers)"""
        return self.precision == "fp16c4" or (self.precision == "fp16c8" and self.c4_from is not None and i >= self.c4_from)

    def _operand_map(self):
        """which projection of which block runs on which operand format, from the fields `set_nograd_precision` sets: the ONE place that
        decides it (weight sets, buffers and the block loop all read the result).  Reads no tensor, launches nothing."""
        depth = len(self.blocks)
        if self.precision == "f32":                   # (no 16-bit type anywhere: weights are the masters, activations fp32 buffers)
            return OperandMap("f32", ("f32",) * depth, ("f32",) * depth, False, False, None, None)
        if self.precision == "f64":                   # (float64 activation buffers; no weight set, no shadows: the masters are widened as they are read)
            return OperandMap("f64", ("f64",) * depth, ("f64",) * depth, False, False, None, None)
        if self.precision not in ("bf16x3", "fp16c8", "fp16c4"):
            return OperandMap("plain", ("plain",) * depth, ("plain",) * depth, False, False, self.compute_dtype, None)
        if self.precision == "bf16x3":                # (hi / lo halves of x3_dtype: "bf16x3" or "fp16x3")
            return OperandMap("x3", ("x3",) * depth, ("x3",) * depth, False, False, None, self.x3_dtype)
        (pa, pm), (xa, xm) = self._plain_from(), self._x3_until()
        # the early blocks on bf16x3 operands (the bf16 build's split-row kernels on the same fp32 stream); the last blocks on plain fp16
        # operands (the fused 1x path): rounding injected there passes through the fewest layers and never reaches the auxiliary CAM
        half = lambda i, x, p_: "x3" if i < x else "plain" if i >= p_ else "c4" if self._is_c4(i) else "c8"
        return OperandMap("c8", tuple(half(i, xa, pa) for i in range(depth)), tuple(half(i, xm, pm) for i in range(depth)),
                          bool(self.c8_plain_qkv), bool(self.c4_proj), torch.float16, torch.bfloat16)

    def _operand_items(self, fmap, fmt):
        """(name, weight, bias) of every projection that `fmap` puts on operand format `fmt`, the patch projection first"""
        items = [("patch", self.patch_embed.proj.weight.reshape(self.embed_dim, -1), self.patch_embed.proj.bias)] if fmap.patch == fmt else []
        for i, blk in enumerate(self.blocks):
            for n, m in (("qkv", blk.attn.qkv), ("proj", blk.attn.proj), ("fc1", blk.mlp.fc1), ("fc2", blk.mlp.fc2)):
                if fmap.of(i, n) == fmt:
                    items.append((f"{i}.{n}", m.weight, m.bias))
        return items

    def _operand_rows(self, fmap, fmt):
        """{name: weight operand} of format `fmt` ("x3", "c8" or "c4"), rebuilt from the fp32 masters on every pass (the teacher's masters move
        every step; ~0.5 GB of traffic, part of the captured graph)"""
        items = self._operand_items(fmap, fmt)
        return self._split_weights(items, fmap.hdt) if fmt == "x3" else self._batched_rows(fmt, items)

    def _split_weights(self, items, dtype):
        """split rows [N, 2K+64] (bias in the augmentation block), one launch per tensor"""
        ws = self.__dict__.setdefault("_x3_w", {}).setdefault(dtype, {})          # (bf16 halves: bf16x3 and the early blocks of fp16c8-xN; fp16: fp16x3)
        for name, w, b in items:
            buf = ws.get(name)
            if buf is None or buf.device != w.device:
                buf = ws[name] = torch.empty((w.shape[0], nn_ops.split_ld(w.shape[1])), device=w.device, dtype=dtype)
            nn_ops.split_rows(w.detach(), bias=b.detach(), out=buf)
        return ws

    def _batched_rows(self, fmt, items):
        """c8 rows [N, 2K+64 fp16 units] (bias in the augmentation block), or fp16c4 rows + their scale tensors (csrc/c4.hpp; the patch
        projection never: its operand comes out of the im2col kernel as c8 rows), by ONE batched launch"""
        import numpy as np
        from .. import _C
        c4 = fmt == "c4"
        ent = self.__dict__.get(f"_{fmt}_w")
        key = tuple((n, w.data_ptr(), b.data_ptr()) for n, w, b in items)
        if ent is None or ent["key"] != key:
            dev = items[0][1].device
            rows = lambda w: (torch.zeros if c4 else torch.empty)((w.shape[0], nn_ops.split_ld(w.shape[1])), device=dev, dtype=torch.float16)
            bufs = {n: (rows(w), nn_ops.c4_scales(w.shape[0], w.shape[1], dev)) if c4 else rows(w) for n, w, _ in items}
            rec_dt = np.dtype([("src", "u8"), ("bias", "u8"), ("dst", "u8")] + ([("sc", "u8")] if c4 else []) +
                              [("rows", "i4"), ("K", "i4"), ("row0", "i4"), ("qrows", "i4")])
            assert rec_dt.itemsize == (_C.lib().cosa_c4_record_bytes() if c4 else _C.lib().cosa_c8_record_bytes())
            rec, row0 = np.zeros(len(items), rec_dt), 0
            for j, (n, w, b) in enumerate(items):
                assert w.dtype == torch.float32 and w.is_contiguous() and w.shape[1] % (256 if c4 else 128) == 0 and (not c4 or w.shape[0] % 256 == 0)
                dst = tuple(t.data_ptr() for t in bufs[n]) if c4 else (bufs[n].data_ptr(),)
                # (qkv: the attention scale is folded into the q rows -- the attention kernel is then called with scale = ln 2, nn_ops.LN2)
                rec[j] = (w.data_ptr(), b.data_ptr()) + dst + (w.shape[0], w.shape[1], row0, w.shape[0] // 3 if n.endswith(".qkv") else 0)
                row0 += w.shape[0]
            ent = self.__dict__[f"_{fmt}_w"] = {"key": key, "bufs": bufs, "rec": torch.from_numpy(rec.view(np.uint8).copy()).to(dev),
                                                "n": len(items), "rows": row0}
        fn = "cosa_c4_rows_batched" if c4 else "cosa_c8_rows_batched"
        _C.check(getattr(_C.lib(), fn)(_C.ptr(ent["rec"]), ent["n"], ent["rows"], _C.stream_ptr()), fn)
        return ent["bufs"]

    _BUFS_MAX = 8          # cached geometries (each holds ~M x 7 KB of activations): evaluation over many image sizes must not pin them all

    def _operand_buffers(self, fmt, dtype, pk, cols=False):
        """persistent "x3" / "c8" / "f32" / "f64" activations for the token rows of `pk` ("f32" / "f64": plain fp32 / float64 rows, no augmentation block); the (1, 1, 0, ...) augmentation block of the fc1 output is set once
        here (the GEMM epilogues write the operand halves only), the other buffers get theirs from their producing kernels.  Keyed on the FULL
        token geometry (the (images, tokens) split per scale and the patch width), not on M alone: the token-shaped patch operand `cols`
        relies on its class-token rows staying zero, and another split of the same M puts class tokens where stale patch rows sit (ADVICE
        r4).  Least recently used entries are dropped beyond _BUFS_MAX, except those a captured hipGraph replays into."""
        bufs = self.__dict__.setdefault("_operand_bufs", {})
        key = (fmt, dtype, pk.M, pk.dev, (pk.shapes, pk.Kp))
        ent = bufs.pop(key, None)
        mk = lambda n: torch.zeros((pk.M, n), device=pk.dev, dtype=dtype)
        if ent is None:
            D, Hd = self.embed_dim, self.blocks[0].mlp.fc1.weight.shape[0]
            if fmt in ("f32", "f64"):
                ent = {"y": mk(D), "qkv": mk(3 * D), "o": mk(D), "h": mk(Hd)}
            else:
                ent = {"y": mk(nn_ops.split_ld(D)), "qkv": mk((2 if fmt == "x3" else 1) * 3 * D), "o": mk(nn_ops.split_ld(D)), "h": mk(nn_ops.split_ld(Hd))}
                ent["h"][:, 2 * Hd:2 * Hd + 2] = 1
        if cols and "cols" not in ent:
            ent["cols"] = mk(pk.Kp if fmt in ("f32", "f64") else nn_ops.split_ld(pk.Kp))      # (class-token rows: zero for good)
        bufs[key] = ent                             # (re-inserted last: the dict is the LRU order)
        if torch.cuda.is_current_stream_capturing():
            ent["pinned"] = True
        elif len(bufs) > self._BUFS_MAX:
            for k in [k for k, e in bufs.items() if not e.get("pinned") and k != key][:len(bufs) - self._BUFS_MAX]:
                del bufs[k]
        return ent

    def _token_pack(self, xs, flip_pairs):
        p = self.patch_size
        nf = 2 if flip_pairs else 1                  # flip_pairs: every batch stands for cat(x, x.flip(-1)) (the teacher's passes)
        shapes = [(nf * x.shape[0], (x.shape[2] // p) * (x.shape[3] // p) + 1) for x in xs]
        offs = [0]
        for B, N in shapes:
            offs.append(offs[-1] + B * N)
        return TokenPack(tuple(shapes), tuple(offs), offs[-1], xs[0].shape[1] * p * p, nf, xs[0].device)

    def _forward_features_fused(self, x):
        return self._forward_features_fused_multi([x])[0]

    def _forward_features_fused_multi(self, xs, flip_pairs=False):
        """Several image batches (the teacher's three scales) through the encoder TOGETHER: LayerNorm and the four
        projections are token-wise, so all tokens of all scales go through one launch each per block (M = sum B_i N_i:
        better tile quantisation on 256 CUs, a third of the launches); only attention runs per scale, on its slice of
        the packed qkv buffer.  Token assembly and the closing LayerNorm belong to the operand family of the patch projection."""
        fmap, pk = self._operand_map(), self._token_pack(xs, flip_pairs)
        D = self.embed_dim
        if self.act_probe is not None and fmap.patch != "f32":
            raise RuntimeError(f"act_probe: only the fp32 no-grad path (mode \"fp32\") is probed -- its qkv / o / h buffers are plain fp32; "
                               f"this network runs its passes on {fmap.patch!r} operands")
        f = lambda t: t.detach()
        if fmap.patch == "x3":
            W = {"x3": self._operand_rows(fmap, "x3")}
            bufs = {"x3": self._operand_buffers("x3", fmap.hdt, pk, cols=True)}
            xr, aux = self._blocks_nograd(self._tokens_x3(xs, pk, bufs["x3"], W["x3"]["patch"], fmap.hdt), pk, fmap, W, bufs)
            a16 = torch.empty_like(bufs["x3"]["y"])      # (its hi halves: 16-bit tokens for the decoder convs, a strided view)
            _, xn32 = nn_ops.layernorm_split(xr, f(self.norm.weight), f(self.norm.bias), self.norm.eps, out=a16, want_f32=True)
        elif fmap.patch == "c8":
            W = {"c8": self._operand_rows(fmap, "c8")}
            if fmap.uses("c4"):
                W["c4"] = self._operand_rows(fmap, "c4")
            bufs = {"c8": self._operand_buffers("c8", torch.float16, pk, cols=True)}
            xr = self._tokens_c8(xs, pk, bufs["c8"], W["c8"]["patch"])
            if "c4" in W and "y_sc" not in bufs["c8"]:
                # the scale tensors of the c4 activation operands (LayerNorm, attention and GELU outputs), created when first needed: the
                # buffers may stem from another precision setting
                M, Hd = pk.M, self.blocks[0].mlp.fc1.weight.shape[0]
                bufs["c8"].update(y_sc=nn_ops.c4_scales(M, D, pk.dev), o_sc=nn_ops.c4_scales(M, D, pk.dev), h_sc=nn_ops.c4_scales(M, Hd, pk.dev))
            if fmap.uses("x3"):
                W["x3"], bufs["x3"] = self._operand_rows(fmap, "x3"), self._operand_buffers("x3", fmap.hdt, pk)
            xr, aux = self._blocks_nograd(xr, pk, fmap, W, bufs)
            a16 = torch.empty_like(bufs["c8"]["y"])      # (its hi parts: fp16 tokens for the decoder convs, a strided view)
            _, xn32 = nn_ops.layernorm_c8(xr, f(self.norm.weight), f(self.norm.bias), self.norm.eps, out=a16, want_f32=True)
        elif fmap.patch == "f32":
            bufs = {"f32": self._operand_buffers("f32", torch.float32, pk, cols=True)}
            xr, aux = self._blocks_nograd(self._tokens_f32(xs, pk, bufs["f32"]), pk, fmap, {}, bufs)
            a16 = xn32 = nn_ops.layernorm_f32out(xr, f(self.norm.weight), f(self.norm.bias), self.norm.eps)      # (no 16-bit tokens: the decoder runs fp32 too)
        elif fmap.patch == "f64":
            bufs = {"f64": self._operand_buffers("f64", torch.float64, pk, cols=True)}
            xr, aux = self._blocks_nograd(self._tokens_f64(xs, pk, bufs["f64"]), pk, fmap, {}, bufs)
            a16 = xn32 = nn_ops.layernorm_f64(xr, f(self.norm.weight), f(self.norm.bias), self.norm.eps)      # (float64 tokens for every head)
        else:
            c = lambda p_: nn_ops.cast_param(p_, fmap.dt16)
            xr, aux = self._blocks_nograd(self._tokens_plain(xs, pk, fmap.dt16, flip_pairs), pk, fmap, {}, {})
            a16, xn32 = nn_ops.layernorm_f32(xr, c(self.norm.weight), c(self.norm.bias), self.norm.eps, True, True)
        return pk.cut(a16, xn32, xn32 if aux is None else aux, D)

    def _tokens_plain(self, xs, pk, dt16, flip_pairs):
        """fp32 residual stream [sum M_i, 768] of the plain 16-bit family (dt16: bf16, or fp16 -- no-grad passes only: same kernels)"""
        c = lambda p_: nn_ops.cast_param(p_, dt16)
        D, p = self.embed_dim, self.patch_size
        if not (all(x.is_cuda for x in xs) and D % 128 == 0 and (3 * p * p) % 64 == 0 and p % 8 == 0):
            toks = []
            for x in ([torch.cat([x, x.flip(-1)], dim=0) for x in xs] if flip_pairs else xs):
                tok, h, w = self.prepare_tokens(x)                   # 16-bit [B,N,768]
                toks.append(tok.float().reshape(-1, tok.shape[-1]))
            return toks[0].contiguous() if len(toks) == 1 else torch.cat(toks, 0)
        # patch projection on the own GEMM, then ONE pass per scale that adds the class token and the position rows and writes the fp32
        # residual stream in place (cosa_embed_finish) -- instead of cat(cls, tok) + pos, .float() and the concatenation of the scales
        from .. import _C
        xr = torch.empty((pk.M, D), device=pk.dev, dtype=torch.float32)
        wgt = c(self.patch_embed.proj.weight).reshape(D, -1).contiguous()
        bias, cls = c(self.patch_embed.proj.bias).contiguous(), c(self.cls_token).reshape(-1).contiguous()
        code = 1 if dt16 == torch.bfloat16 else 2
        for x, (B, N, o0, o1) in zip(xs, pk.scales()):
            h, w = x.shape[2] // p, x.shape[3] // p
            xf = x.float().contiguous()
            cols = torch.empty((B * h * w, x.shape[1] * p * p), device=x.device, dtype=dt16)
            _C.check(_C.lib().cosa_im2col_flip(_C.ptr(xf), _C.ptr(cols), x.shape[0], x.shape[1], x.shape[2], x.shape[3], p, pk.nf, code,
                                               _C.stream_ptr()), "cosa_im2col_flip")
            tok = nn_ops.gemm_bf16(cols, wgt, bias, nn_ops.EPI_BIAS)
            pos = self._pos_for_grid(h, w, dt16).reshape(N, D).contiguous()
            _C.check(_C.lib().cosa_embed_finish(_C.ptr(tok), _C.ptr(cls), _C.ptr(pos), _C.ptr(xr[o0:o1]), B, N - 1, D, code, _C.stream_ptr()),
                     "cosa_embed_finish")
        return xr

    def _stream_and_cols(self, xs, pk, cols, im2col, name):
        """token assembly without ATen passes or concatenations: the residual stream xr [sum_i B_i (n_i + 1), D] starts as (cls + pos_0 | pos rows)
        per image, and the im2col kernel writes the operand rows of the patches (images and their mirror images) into the token-shaped `cols`,
        whose class-token rows stay zero (augmentation block included: no bias there) -- the patch projection then adds into xr in place
        through its fp32 residual epilogue"""
        from .. import _C
        D, p = self.embed_dim, self.patch_size
        xr = torch.empty((pk.M, D), device=pk.dev, dtype=torch.float32)
        cls = self.cls_token.detach().float().reshape(1, 1, D)
        for x, (B, N, o0, o1) in zip(xs, pk.scales()):
            pos = self._pos_for_grid(x.shape[2] // p, x.shape[3] // p, torch.float32)   # [1, n+1, D]
            first = torch.cat((cls + pos[:, :1], pos[:, 1:]), dim=1).contiguous()       # (a [n+1, D] tensor: small)
            _C.check(_C.lib().cosa_broadcast_rows(_C.ptr(first), _C.ptr(xr[o0:o1]), B, N * D, _C.stream_ptr()), "cosa_broadcast_rows")
            xf = x.float().contiguous()
            _C.check(im2col(_C.ptr(xf), _C.ptr(cols[o0:o1]), x.shape[0], x.shape[1], x.shape[2], x.shape[3], p, pk.nf, 1, _C.stream_ptr()), name)
        return xr

    def _tokens_x3(self, xs, pk, bf, w_patch, hdt):
        xr = self._stream_and_cols(xs, pk, bf["cols"], nn_ops._x3_fn("cosa_im2col_flip_split_tokens", hdt), "cosa_im2col_flip_split_tokens")
        # One launch per scale: cosa_gemm_bf16x3 picks its kernel by M (the 128 x 128 kernel below 4096 rows: another summation order than the
        # persistent one), so per token row the same products are summed in the same order as with one projection per scale on materialised
        # im2col rows: bit-identical CAMs.
        for B, N, o0, o1 in pk.scales():
            nn_ops.gemm_x3(bf["cols"][o0:o1], w_patch, B * N, self.embed_dim, pk.Kp, nn_ops.EPI_RESIDUAL, residual=xr[o0:o1], out=xr[o0:o1])
        return xr

    def _tokens_f32(self, xs, pk, bf):
        """the fp32 family's token assembly: fp32 im2col rows, the patch projection on the fp32 master weight through the residual epilogue into
        the stream in place, all scales in one launch (a row's chain does not depend on M).  The bias is an epilogue operand here, not an
        augmentation column, so the class-token rows (zero operand rows) receive it too: they are written again afterwards as cls + pos_0"""
        from .. import _C
        D = self.embed_dim
        xr = self._stream_and_cols(xs, pk, bf["cols"], _C.lib().cosa_im2col_flip_f32_tokens, "cosa_im2col_flip_f32_tokens")
        first = [xr[o0].clone() for _, _, o0, _ in pk.scales()]             # cls + pos_0 of each scale ([D]: small)
        pe = self.patch_embed.proj
        nn_ops.gemm_f32(bf["cols"], pe.weight.detach().reshape(D, -1), pe.bias.detach(), pk.M, D, pk.Kp, nn_ops.EPI_RESIDUAL, residual=xr, out=xr)
        for row, (B, N, o0, o1) in zip(first, pk.scales()):
            xr[o0:o1].view(B, N, D)[:, 0] = row
        return xr

    def _pos_f64(self, h, w):
        """the position rows [h*w + 1, D] of a token geometry in float64: F.interpolate(bicubic) on the float64 copy of pos_embed, formed once
        per geometry and kept until pos_embed is written again (its version counter: frozen for the student, EMA-touched for a teacher)"""
        pe = self.pos_embed
        key = (h, w, pe.device, "f64")
        ent = self._pos_cache.get(key)
        if ent is None or ent["version"] != pe._version or ent["ptr"] != pe.data_ptr():
            with torch.no_grad():
                g = pe[0, 1:].double().reshape(1, self._size, self._size, -1).permute(0, 3, 1, 2)
                g = F.interpolate(g, size=(h, w), mode="bicubic", align_corners=False).reshape(-1, h * w).t()
                rows = torch.cat((pe[0, :1].double(), g), dim=0).contiguous()
            ent = self._pos_cache[key] = {"version": pe._version, "ptr": pe.data_ptr(), "rows": rows}
        return ent["rows"]

    def _tokens_f64(self, xs, pk, bf):
        """the float64 family's token assembly, as `_tokens_f32`: the stream starts as the position rows, the float64 im2col rows go through
        the patch projection on the fp32 master weight (widened in the kernel) and its residual epilogue into the stream in place, all scales
        in one launch; the class-token rows (zero operand rows that received the bias) are written afterwards as cls + pos_0"""
        from .. import _C
        D, p = self.embed_dim, self.patch_size
        xr = torch.empty((pk.M, D), device=pk.dev, dtype=torch.float64)
        cls = self.cls_token.detach().double().reshape(D)
        first = []
        for x, (B, N, o0, o1) in zip(xs, pk.scales()):
            pos = self._pos_f64(x.shape[2] // p, x.shape[3] // p)
            xr[o0:o1].view(B, N, D).copy_(pos.unsqueeze(0).expand(B, N, D))
            first.append(cls + pos[0])
            xd = x.double().contiguous()                 # (fp32 inputs widen exactly; the rescaled ones arrive as float64 planes)
            _C.check(_C.lib().cosa_im2col_flip_f64_tokens(_C.ptr(xd), _C.ptr(bf["cols"][o0:o1]), x.shape[0], x.shape[1], x.shape[2], x.shape[3], p,
                                                          pk.nf, 1, _C.stream_ptr()), "cosa_im2col_flip_f64_tokens")
        pe = self.patch_embed.proj
        nn_ops.gemm_f64(bf["cols"], pe.weight.detach().reshape(D, -1), pe.bias.detach(), pk.M, D, pk.Kp, nn_ops.EPI_RESIDUAL, residual=xr, out=xr)
        for row, (B, N, o0, o1) in zip(first, pk.scales()):
            xr[o0:o1].view(B, N, D)[:, 0] = row
        return xr

    def _tokens_c8(self, xs, pk, bf, w_patch):
        from .. import _C
        xr = self._stream_and_cols(xs, pk, bf["cols"], _C.lib().cosa_im2col_flip_c8_tokens, "cosa_im2col_flip_c8_tokens")
        # the patch projection of ALL scales in one launch, token-wise like the block projections
        nn_ops.gemm_c8(bf["cols"], w_patch, pk.M, self.embed_dim, pk.Kp, nn_ops.EPI_RESIDUAL, residual=xr, out=xr)
        return xr

    def _blocks_nograd(self, xr, pk, fmap, W, bufs):
        """the blocks on the fp32 stream xr, each half on the operand format `fmap` gives it -> (stream, aux-layer output or None)"""
        depth = len(self.blocks)
        aux_idx = self.aux_layer % depth
        aux = None
        o16 = torch.empty((pk.M, self.embed_dim), device=xr.device, dtype=fmap.dt16) if "plain" in fmap.attn else None
        for i, blk in enumerate(self.blocks):
            # the stream is updated in place, except right after the auxiliary layer: its output stays where it is (it IS the aux
            # feature) and the next residual GEMM writes the stream to a fresh buffer -- no 270-MB clone
            xn = torch.empty_like(xr) if aux is xr else xr
            if fmap.attn[i] == "plain":
                self._attn_plain(xr, xn, blk, pk, o16, fmap.dt16)
            elif fmap.attn[i] == "x3":
                self._attn_x3(xr, xn, blk, pk, bufs["x3"], W["x3"], i)
            elif fmap.attn[i] == "f32":
                self._attn_f32(xr, xn, blk, pk, bufs["f32"], i)
            elif fmap.attn[i] == "f64":
                self._attn_f64(xr, xn, blk, pk, bufs["f64"])
            else:
                self._attn_c8(xr, xn, blk, pk, bufs["c8"], W, i, fmap)
            xr = xn
            if fmap.mlp[i] == "plain":
                self._mlp_plain(xr, blk, fmap.dt16)
            elif fmap.mlp[i] == "x3":
                self._mlp_x3(xr, blk, pk, bufs["x3"], W["x3"], i)
            elif fmap.mlp[i] == "f32":
                self._mlp_f32(xr, blk, pk, bufs["f32"], i)
            elif fmap.mlp[i] == "f64":
                self._mlp_f64(xr, blk, pk, bufs["f64"])
            else:
                self._mlp_c8(xr, blk, pk, bufs["c8"], W, i, fmap.mlp[i] == "c4")
            if i == aux_idx and aux_idx != depth - 1:
                aux = xr
        return xr, aux

    def _attn_plain(self, xr, xn, blk, pk, o16, dt16):
        c = lambda p_: nn_ops.cast_param(p_, dt16)
        D = self.embed_dim
        y, _ = nn_ops.layernorm_f32(xr, c(blk.norm1.weight), c(blk.norm1.bias), blk.norm1.eps)
        qkv = nn_ops.gemm_bf16(y, c(blk.attn.qkv.weight), c(blk.attn.qkv.bias), nn_ops.EPI_BIAS)
        for B, N, o0, o1 in pk.scales():
            nn_ops._attn_fwd(qkv[o0:o1].view(B, N, 3 * D), B, N, self.num_heads, out=o16[o0:o1].view(B, N, D), nograd=True)
        nn_ops.gemm_bf16(o16, c(blk.attn.proj.weight), c(blk.attn.proj.bias), nn_ops.EPI_RESIDUAL, residual=xr, out=xn)

    def _mlp_plain(self, xr, blk, dt16):
        c = lambda p_: nn_ops.cast_param(p_, dt16)
        y, _ = nn_ops.layernorm_f32(xr, c(blk.norm2.weight), c(blk.norm2.bias), blk.norm2.eps)
        hmid = nn_ops.gemm_bf16(y, c(blk.mlp.fc1.weight), c(blk.mlp.fc1.bias), nn_ops.EPI_GELU)
        nn_ops.gemm_bf16(hmid, c(blk.mlp.fc2.weight), c(blk.mlp.fc2.bias), nn_ops.EPI_RESIDUAL, residual=xr, out=xr)

    def _attn_x3(self, xr, xn, blk, pk, bf, W, i):
        M, D = pk.M, self.embed_dim
        nn_ops.layernorm_split(xr, blk.norm1.weight.detach(), blk.norm1.bias.detach(), blk.norm1.eps, out=bf["y"])
        nn_ops.gemm_x3(bf["y"], W[f"{i}.qkv"], M, 3 * D, D, nn_ops.EPI_BIAS, out=bf["qkv"], ldy=2 * 3 * D)
        for B, N, o0, o1 in pk.scales():
            nn_ops.attn_fwd_x3(bf["qkv"][o0:o1], B, N, self.num_heads, bf["o"][o0:o1])
        nn_ops.gemm_x3(bf["o"], W[f"{i}.proj"], M, D, D, nn_ops.EPI_RESIDUAL, residual=xr, out=xn)

    def _mlp_x3(self, xr, blk, pk, bf, W, i):
        M, D, Hd = pk.M, self.embed_dim, blk.mlp.fc1.weight.shape[0]
        nn_ops.layernorm_split(xr, blk.norm2.weight.detach(), blk.norm2.bias.detach(), blk.norm2.eps, out=bf["y"])
        nn_ops.gemm_x3(bf["y"], W[f"{i}.fc1"], M, Hd, D, nn_ops.EPI_GELU, out=bf["h"], ldy=bf["h"].shape[1])
        nn_ops.gemm_x3(bf["h"], W[f"{i}.fc2"], M, D, Hd, nn_ops.EPI_RESIDUAL, residual=xr, out=xr)

    def _attn_f32(self, xr, xn, blk, pk, bf, i):
        """fp32 attention half: the projections read the fp32 master weights and biases themselves -- no weight set, nothing rebuilt per pass.
        `act_probe`, when set, reads block i's q / k / v windows, the logits per scale and o after the launches that produced them"""
        M, D = pk.M, self.embed_dim
        d = lambda p_: None if p_ is None else p_.detach()
        probe = self.act_probe
        nn_ops.layernorm_f32out(xr, d(blk.norm1.weight), d(blk.norm1.bias), blk.norm1.eps, out=bf["y"])
        nn_ops.gemm_f32(bf["y"], d(blk.attn.qkv.weight), d(blk.attn.qkv.bias), M, 3 * D, D, nn_ops.EPI_BIAS, out=bf["qkv"])
        if probe is not None:
            for j, name in enumerate(("q", "k", "v")):
                probe.site(i, name, bf["qkv"][:M], j * D, D)
        for B, N, o0, o1 in pk.scales():
            nn_ops.attn_fwd_f32(bf["qkv"][o0:o1], B, N, self.num_heads, bf["o"][o0:o1])
            if probe is not None:
                probe.attn(i, bf["qkv"][o0:o1], B, N, self.num_heads)
        if probe is not None:
            probe.site(i, "o", bf["o"][:M])
        nn_ops.gemm_f32(bf["o"], d(blk.attn.proj.weight), d(blk.attn.proj.bias), M, D, D, nn_ops.EPI_RESIDUAL, residual=xr, out=xn)

    def _mlp_f32(self, xr, blk, pk, bf, i):
        M, D, Hd = pk.M, self.embed_dim, blk.mlp.fc1.weight.shape[0]
        d = lambda p_: p_.detach()
        probe = self.act_probe
        nn_ops.layernorm_f32out(xr, d(blk.norm2.weight), d(blk.norm2.bias), blk.norm2.eps, out=bf["y"])
        nn_ops.gemm_f32(bf["y"], d(blk.mlp.fc1.weight), d(blk.mlp.fc1.bias), M, Hd, D, nn_ops.EPI_GELU, out=bf["h"])
        if probe is not None:
            probe.site(i, "h", bf["h"][:M])                  # fc1 + GELU
        nn_ops.gemm_f32(bf["h"], d(blk.mlp.fc2.weight), d(blk.mlp.fc2.bias), M, D, Hd, nn_ops.EPI_RESIDUAL, residual=xr, out=xr)
        if probe is not None:
            probe.site(i, "x", xr[:M])                       # the stream after the block

    def _attn_f64(self, xr, xn, blk, pk, bf):
        """float64 attention half: float64 activations, the fp32 master weights and biases widened inside the kernels -- no weight set"""
        M, D = pk.M, self.embed_dim
        d = lambda p_: None if p_ is None else p_.detach()
        nn_ops.layernorm_f64(xr, d(blk.norm1.weight), d(blk.norm1.bias), blk.norm1.eps, out=bf["y"])
        nn_ops.gemm_f64(bf["y"], d(blk.attn.qkv.weight), d(blk.attn.qkv.bias), M, 3 * D, D, nn_ops.EPI_BIAS, out=bf["qkv"])
        for B, N, o0, o1 in pk.scales():
            nn_ops.attn_fwd_f64(bf["qkv"][o0:o1], B, N, self.num_heads, bf["o"][o0:o1])
        nn_ops.gemm_f64(bf["o"], d(blk.attn.proj.weight), d(blk.attn.proj.bias), M, D, D, nn_ops.EPI_RESIDUAL, residual=xr, out=xn)

    def _mlp_f64(self, xr, blk, pk, bf):
        M, D, Hd = pk.M, self.embed_dim, blk.mlp.fc1.weight.shape[0]
        d = lambda p_: p_.detach()
        nn_ops.layernorm_f64(xr, d(blk.norm2.weight), d(blk.norm2.bias), blk.norm2.eps, out=bf["y"])
        nn_ops.gemm_f64(bf["y"], d(blk.mlp.fc1.weight), d(blk.mlp.fc1.bias), M, Hd, D, nn_ops.EPI_GELU, out=bf["h"])
        nn_ops.gemm_f64(bf["h"], d(blk.mlp.fc2.weight), d(blk.mlp.fc2.bias), M, D, Hd, nn_ops.EPI_RESIDUAL, residual=xr, out=xr)

    def _attn_c8(self, xr, xn, blk, pk, bf, W, i, fmap):
        """fp16c8 attention half; its qkv projection may run on plain fp16 (`c8_plain_qkv`) or fp16c4 operands, its output projection on
        fp16c4 operands (`c4_proj`: the attention kernel then writes c4 rows + scale bytes)"""
        M, D, H = pk.M, self.embed_dim, self.num_heads
        n1w, n1b = blk.norm1.weight.detach(), blk.norm1.bias.detach()
        fq, fp = fmap.of(i, "qkv"), fmap.of(i, "proj")
        if fq == "plain":
            c16 = lambda p_: nn_ops.cast_param(p_, torch.float16)
            y, _ = nn_ops.layernorm_f32(xr, c16(blk.norm1.weight), c16(blk.norm1.bias), blk.norm1.eps)
            nn_ops.gemm_bf16(y, c16(blk.attn.qkv.weight), c16(blk.attn.qkv.bias), nn_ops.EPI_BIAS, out=bf["qkv"])
        elif fq == "c4":
            # fp16c4: LayerNorm and the GELU epilogue write c4 rows + scale bytes; qkv / fc1 / fc2 run on the FP4 block-scaled MFMA
            nn_ops.layernorm_c4(xr, n1w, n1b, blk.norm1.eps, out=bf["y"], scales=bf["y_sc"])
            nn_ops.gemm_c4(bf["y"], bf["y_sc"], *W["c4"][f"{i}.qkv"], M, 3 * D, D, nn_ops.EPI_BIAS, out=bf["qkv"], ldy=3 * D)
        else:
            nn_ops.layernorm_c8(xr, n1w, n1b, blk.norm1.eps, out=bf["y"])
            nn_ops.gemm_c8(bf["y"], W["c8"][f"{i}.qkv"], M, 3 * D, D, nn_ops.EPI_BIAS, out=bf["qkv"], ldy=3 * D)
        for B, N, o0, o1 in pk.scales():                 # (the q rows of the c8 / c4 weight operands are pre-scaled: _batched_rows)
            if fp == "c4":
                nn_ops.attn_fwd_c4(bf["qkv"][o0:o1].view(B, N, 3 * D), B, N, H, bf["o"][o0:o1], bf["o_sc"], o0, q_prescaled=fq != "plain")
            else:
                nn_ops.attn_fwd_c8(bf["qkv"][o0:o1].view(B, N, 3 * D), B, N, H, bf["o"][o0:o1], q_prescaled=fq != "plain")
        if fp == "c4":
            nn_ops.gemm_c4(bf["o"], bf["o_sc"], *W["c4"][f"{i}.proj"], M, D, D, nn_ops.EPI_RESIDUAL, residual=xr, out=xn)
        else:
            nn_ops.gemm_c8(bf["o"], W["c8"][f"{i}.proj"], M, D, D, nn_ops.EPI_RESIDUAL, residual=xr, out=xn)

    def _mlp_c8(self, xr, blk, pk, bf, W, i, c4):
        """fp16c8 MLP half, or (c4) the same on fp16c4 operands"""
        M, D, Hd = pk.M, self.embed_dim, blk.mlp.fc1.weight.shape[0]
        n2w, n2b = blk.norm2.weight.detach(), blk.norm2.bias.detach()
        if c4:
            nn_ops.layernorm_c4(xr, n2w, n2b, blk.norm2.eps, out=bf["y"], scales=bf["y_sc"])
            nn_ops.gemm_c4(bf["y"], bf["y_sc"], *W["c4"][f"{i}.fc1"], M, Hd, D, nn_ops.EPI_GELU, out=bf["h"], out_scales=bf["h_sc"],
                           ldy=nn_ops.split_ld(Hd))
            nn_ops.gemm_c4(bf["h"], bf["h_sc"], *W["c4"][f"{i}.fc2"], M, D, Hd, nn_ops.EPI_RESIDUAL, residual=xr, out=xr)
        else:
            nn_ops.layernorm_c8(xr, n2w, n2b, blk.norm2.eps, out=bf["y"])
            nn_ops.gemm_c8(bf["y"], W["c8"][f"{i}.fc1"], M, Hd, D, nn_ops.EPI_GELU, out=bf["h"], ldy=nn_ops.split_ld(Hd))
            nn_ops.gemm_c8(bf["h"], W["c8"][f"{i}.fc2"], M, D, Hd, nn_ops.EPI_RESIDUAL, residual=xr, out=xr)

    def _n_defer_groups(self):
        g = self.defer_groups
        if g is None:
            import torch.distributed as dist
            # under data parallelism the gradient buckets must fill while the backward pass is still running: 6 groups of 2 blocks.
            # A block is 108 jobs of 256 x 256, so 1, 2, 3 and 6 groups all cost the same six rounds of the 256 CUs (1296 jobs = 5.06 rounds -> 6;
            # 216 jobs per group -> one round each); 4 groups would cost eight, 12 groups twelve (tools/step_only.py ... groupsN)
            g = 6 if (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) else 1
        return max(1, min(int(g), len(self.blocks)))

    def _features_train_f32(self, img):
        """training forward on the fp32 residual stream (vit.py:302-321 with autograd): per block
            qkv = Linear(y); o = attention(qkv); (x, y) = x + proj(o), norm2(.);  h = gelu(fc1(y)); (x, y) = x + fc2(h), next norm1(.)
        every (projection + residual add, following LayerNorm) pair is ONE autograd node (nn_ops.ResidualLinearLNFn).  The blocks' weight
        gradients are computed per group of blocks by one batched launch when the backward pass leaves the group: the DeferredWgrad node
        sits on the group's first LayerNorm OUTPUT, whose gradient (from the qkv projection) is the last thing the group's backward
        produces."""
        dt = self.compute_dtype
        x, h, w = self.prepare_tokens(img, stream_f32=True)
        depth = len(self.blocks)
        aux_idx = self.aux_layer % depth
        aux = None
        defer = torch.is_grad_enabled() and x.requires_grad and self.defer_wgrad
        groups = self._n_defer_groups() if defer else 0
        per = -(-depth // groups) if groups else depth
        n1 = self.blocks[0].norm1
        x, y = nn_ops.stream_layernorm(x, n1.weight, n1.bias, n1.eps)
        scope = None
        try:
            for i, blk in enumerate(self.blocks):
                if groups and i % per == 0:
                    if scope is not None:
                        scope.__exit__(None, None, None)
                    mods = [m for b_ in self.blocks[i:i + per] for m in (b_.attn.qkv, b_.attn.proj, b_.mlp.fc1, b_.mlp.fc2)]
                    y, coll = nn_ops.defer_wgrads(y, mods)
                    scope = nn_ops.collecting(coll)
                    scope.__enter__()
                qkv = nn_ops.linear(y, blk.attn.qkv.weight, blk.attn.qkv.bias, dt)
                o = nn_ops.attention(qkv, self.num_heads)
                x, y = nn_ops.residual_linear_ln(o, x, blk.attn.proj, blk.norm2)
                hmid = nn_ops.linear(y, blk.mlp.fc1.weight, blk.mlp.fc1.bias, dt, act=True)
                last = i + 1 == depth
                x, y = nn_ops.residual_linear_ln(hmid, x, blk.mlp.fc2, self.norm if last else self.blocks[i + 1].norm1, y_f32=last)
                if i == aux_idx and not last:
                    aux = x
        finally:
            if scope is not None:
                scope.__exit__(None, None, None)
        xn = y                                                  # the final norm's output, FP32: its consumers (decoder, CAM head, pooled
        aux = xn if aux is None else aux                        # classification head) take bf16 copies through nn_ops.fanout_bf16, so that
        return FP32Tokens(xn, aux)                              # their gradients are summed in fp32; aux = block aux_idx's output, pre-norm

    def use_fused(self, x):
        return (not torch.is_grad_enabled()) and (self.compute_dtype in _OP16 or self.precision in ("f32", "f64")) and x.is_cuda and self.embed_dim == 768

    # -- vit.py:302-321: returns cls token, final tokens, aux-layer tokens (pre final norm unless aux is the last) --
    def forward_features(self, x):
        f = self.features_ex(x)
        if isinstance(f, FP32Tokens):
            return f.final[:, 0], f.final[:, 1:], f.aux[:, 1:]
        return f[:3]

    def features_ex(self, x):
        """-> (cls, tokens, aux tokens, fp32 tokens or None).  No-grad bf16 passes take the fused HIP path."""
        if self.use_fused(x):
            return self._forward_features_fused(x)
        if self.compute_dtype == torch.bfloat16 and x.is_cuda and self.embed_dim == 768 and self.residual_stream == "fp32" \
                and torch.is_grad_enabled():
            return self._features_train_f32(x)
        x, h, w = self.prepare_tokens(x)
        depth = len(self.blocks)
        aux_idx = self.aux_layer % depth
        aux = None
        if self.compute_dtype == torch.bfloat16 and x.is_cuda and self.embed_dim == 768 and x.dtype == torch.bfloat16:
            # student training path: the stream is (x, pending delta); x + delta materialises inside the next LayerNorm kernel
            delta = None
            # the 48 weight gradients of the blocks are computed in one batched launch when the backward pass reaches this point
            # (nn_ops.DeferredWgrad) instead of 48 split-K launches + 48 reductions
            defer = torch.is_grad_enabled() and x.requires_grad and self.defer_wgrad
            if defer:
                x, coll = nn_ops.defer_wgrads(x, [m for blk in self.blocks for m in (blk.attn.qkv, blk.attn.proj, blk.mlp.fc1, blk.mlp.fc2)])
            with nn_ops.collecting(coll if defer else None):
                for i, blk in enumerate(self.blocks):
                    x_in, x, delta = self._block_fused_ln(blk, x, delta)
                    if i - 1 == aux_idx:
                        aux = x_in                                          # output of block aux_idx, materialised in this block's norm1
            x, xn = nn_ops.add_layernorm(x, delta, self.norm.weight, self.norm.bias, self.norm.eps)
            if aux_idx == depth - 1:
                aux = xn
            return xn[:, 0], xn[:, 1:], aux[:, 1:], None
        # not ViT-B on 16-bit operands: outside the HIP path's envelope -- the block below is module wiring only, every operator of it is
        # nn_ops.reference_op (raises in the product; the host-logic tests install torch's operators: tests/torch_reference.py)
        for i, blk in enumerate(self.blocks):
            x = self._block(blk, x)
            if i == aux_idx:
                aux = x
        dt = self.compute_dtype
        x = nn_ops.reference_op("layer_norm", f"LayerNorm({self.embed_dim}) on {dt}", x, nn_ops.cast_param(self.norm.weight, dt),
                                nn_ops.cast_param(self.norm.bias, dt), self.norm.eps)
        if aux_idx == depth - 1:
            aux = x
        return x[:, 0], x[:, 1:], aux[:, 1:], None


PRETRAINED_ENV = "COSA_VIT_PRETRAINED"        # path of a local timm ViT-B/16 checkpoint (jx_vit_base_p16_224-80ecf9dd.pth)


def load_pretrained_vit(model, path, strict_keys=True):
    """What timm's `load_pretrained(model, filter_fn=_conv_filter)` does for the reference (models/vit/vit.py:332-339,371-374), from a
    LOCAL file: the checkpoint's keys are the module names used here (timm ViT names); a linear-shaped patch projection is reshaped
    to the conv layout (`_conv_filter`); the 1000-way `head` is dropped when its shape differs (timm's `num_classes` handling)."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    sd = sd.get("model", sd.get("state_dict", sd))
    out = {}
    for k, v in sd.items():
        if "patch_embed.proj.weight" in k:
            v = v.reshape(v.shape[0], 3, model.patch_size, model.patch_size)
        out[k] = v
    own = model.state_dict()
    for k in ("head.weight", "head.bias"):
        if k in out and (k not in own or out[k].shape != own[k].shape):
            out.pop(k)
    missing, unexpected = model.load_state_dict(out, strict=False)
    missing = [k for k in missing if not k.startswith("head.")]
    if strict_keys and (missing or unexpected):
        raise RuntimeError(f"load_pretrained_vit({path}): missing keys {missing}, unexpected keys {list(unexpected)}")
    return model


def vit_base_patch16_224(pretrained=False, pretrained_path=None, **kwargs):
    """models/vit/vit.py:365-377.  The reference's `pretrained=True` downloads ImageNet weights through timm; there is no network
    here, so the weights come from a local file (`pretrained_path`, or $COSA_VIT_PRETRAINED) -- and a run that asks for pretrained
    weights without one FAILS instead of silently training from random initialisation."""
    import os
    model = VisionTransformer(patch_size=16, embed_dim=768, depth=12, num_heads=12, mlp_ratio=4, qkv_bias=True, eps=1e-6, **kwargs)
    if pretrained:
        path = pretrained_path or os.environ.get(PRETRAINED_ENV)
        if not path or not os.path.exists(path):
            raise FileNotFoundError(
                "vit_base_patch16_224(pretrained=True): no local checkpoint -- pass pretrained_path= or set $" + PRETRAINED_ENV +
                " to timm's jx_vit_base_p16_224-80ecf9dd.pth (the file the reference downloads, models/vit/vit.py:53-56), "
                "or build with pretrained=False")
        load_pretrained_vit(model, path)
    return model
