"""utils.torch_helper -- the hot-path subset of the reference module, MI355X-native.

Reference: utils/torch_helper.py:32-42 (setup_seed), :261-293 (PolyWarmupAdamW), :354-367
(denormalize_img_/denormalize_img).
"""
import random

import numpy as np
import torch

from .. import _C


def setup_seed(seed):
    """utils/torch_helper.py:32-42"""
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)


def denormalize_img(imgs):
    """utils/torch_helper.py:354-367: (x*std+mean) -> uint8 truncation -> /255, one fused kernel."""
    _C.require_cuda(imgs)
    imgs = imgs.contiguous().float()
    B, C, H, W = imgs.shape
    if C != 3:
        raise ValueError("denormalize_img expects [B,3,H,W]")
    out = torch.empty_like(imgs)
    _C.check(_C.lib().cosa_denormalize_img(_C.ptr(imgs), _C.ptr(out), B, H, W, _C.stream_ptr()), "cosa_denormalize_img")
    return out


def denormalize_img_(imgs, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375)):
    """uint8 image (utils/torch_helper.py:354-361); derived from the fused kernel's output."""
    if tuple(mean) != (123.675, 116.28, 103.53) or tuple(std) != (58.395, 57.12, 57.375):
        raise NotImplementedError("only the ImageNet mean/std of the reference are compiled in")
    return (denormalize_img(imgs) * 255.0).to(torch.uint8)


def poly_warmup_lr_mult(step, warmup_iter, max_iter, warmup_ratio, power, min_mult):
    """LR multiplier of PolyWarmupAdamW.step (utils/torch_helper.py:275-289); None = keep previous LR."""
    if step < warmup_iter:
        return 1 - (1 - step / warmup_iter) * (1 - warmup_ratio)
    if step < max_iter:
        return max((1 - step / max_iter) ** power, min_mult)
    return None


class PolyWarmupAdamW(torch.optim.AdamW):
    """utils/torch_helper.py:261-293, same constructor and schedule.

    The update itself is torch's fused multi-tensor AdamW (one launch per dtype group, no
    per-parameter Python loop); `ema_update()` applies the teacher EMA (main.py:250-252) with
    one foreach launch.
    """

    def __init__(self, params, lr, weight_decay, betas, warmup_iter, max_iter, warmup_ratio, power, min_mult=0, **kwargs):
        fused = kwargs.pop("fused", None)
        params = list(params)
        if fused is None:
            first = params[0]["params"][0] if isinstance(params[0], dict) else params[0]
            fused = bool(first.is_cuda)
        super().__init__(params, lr=lr, betas=betas, weight_decay=weight_decay, eps=1e-8, fused=fused)
        self.global_step = 0
        self.warmup_iter = warmup_iter
        self.warmup_ratio = warmup_ratio
        self.max_iter = max_iter
        self.power = power
        self.min_mult = min_mult
        self._init_lr = [group["lr"] for group in self.param_groups]

    def step(self, closure=None):
        mult = poly_warmup_lr_mult(self.global_step, self.warmup_iter, self.max_iter, self.warmup_ratio, self.power,
                                   self.min_mult)
        if mult is not None:
            for i, g in enumerate(self.param_groups):
                g["lr"] = self._init_lr[i] * mult
        super().step(closure)
        self.global_step += 1

    def skip_step(self):
        """A refused iteration (the gradient guard): nothing is updated, but the schedule and the bias-correction count advance exactly as
        in step(), because the fused path's host never learns that its kernel refused a step."""
        mult = poly_warmup_lr_mult(self.global_step, self.warmup_iter, self.max_iter, self.warmup_ratio, self.power,
                                   self.min_mult)
        for i, g in enumerate(self.param_groups):
            if mult is not None:
                g["lr"] = self._init_lr[i] * mult
            for p in g["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if "step" not in st:                        # as torch's AdamW creates them in its first step()
                    on_dev = bool(g.get("fused")) or bool(g.get("capturable"))
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if on_dev else torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
        self.global_step += 1


@torch.no_grad()
def ema_update(teacher_params, student_params, momentum):
    """main.py:250-252: a <- m*a + (1-m)*o over parameters, as two foreach launches."""
    teacher_params, student_params = list(teacher_params), list(student_params)
    torch._foreach_mul_(teacher_params, momentum)
    torch._foreach_add_(teacher_params, student_params, alpha=1 - momentum)


# --------------------------------------------------------------------------------------------
# the gradient guard: clip by the global norm, refuse a non-finite step
# --------------------------------------------------------------------------------------------
GUARD_WORDS = 5      # the guard record of include/cosa_hip.h as int64 words: {f32 norm, f32 coef | i32 skip, i32 pad | applied | skipped | clipped}


def new_guard_state(device):
    return torch.zeros(GUARD_WORDS, dtype=torch.int64, device=device)


def guard_norm(state):
    """the last step's global gradient norm: a 0-dim fp32 view of the guard record (no sync)"""
    return state.view(torch.float32)[0]


def guard_coef(state):
    return state.view(torch.float32)[1]


def guard_skip(state):
    return state.view(torch.int32)[2]


def guard_counters(state):
    """{applied, skipped, clipped} of the run so far; synchronises"""
    applied, skipped, clipped = state[2:5].tolist()
    return {"applied": applied, "skipped": skipped, "clipped": clipped}


@torch.no_grad()
def guard_decision(grads, max_norm, skip_nonfinite, state):
    """The guard's decision in plain torch, written into `state` the way cosa_grad_norm does: the global norm from a float64 sum of squares,
    coef = clamp(max_norm / (norm + 1e-6), max=1) in fp32 (1 without clipping), skip = skip_nonfinite and a non-finite sum, the counters.
    -> (coef as a 0-dim fp32 tensor, skip as a bool: this path, unlike the kernels, tells the host)."""
    dev = state.device
    if grads:
        total = torch.stack([g.detach().double().square().sum() for g in grads]).sum()
    else:
        total = torch.zeros((), dtype=torch.float64, device=dev)
    norm = total.sqrt().float()
    coef = (float(max_norm) / (norm + 1e-6)).clamp(max=1.0) if max_norm > 0 else torch.ones((), dtype=torch.float32, device=dev)
    skip = bool(skip_nonfinite) and not bool(torch.isfinite(total))
    f32 = state.view(torch.float32)
    f32[0], f32[1] = norm, coef
    state.view(torch.int32)[2] = int(skip)
    if skip:
        state[3] += 1
    else:
        state[2] += 1
        state[4] += (coef < 1).to(torch.int64)
    return coef, skip


@torch.no_grad()
def guarded_torch_step(optimizer, teacher_params, student_params, momentum, max_norm, skip_nonfinite, state):
    """optimizer.step() + ema_update behind the gradient guard, for the non-fused path and host trainers: the semantics of
    cosa_grad_norm + cosa_fused_adamw_ema_guarded (a refused step changes nothing and still counts for the schedule and the bias
    correction).  Clipping scales the gradients in place, as torch.nn.utils.clip_grad_norm_ does."""
    grads = [p.grad for g in optimizer.param_groups for p in g["params"] if p.grad is not None]
    coef, skip = guard_decision(grads, max_norm, skip_nonfinite, state)
    if skip:
        optimizer.skip_step()
        return
    if max_norm > 0 and grads:
        torch._foreach_mul_(grads, coef)
    optimizer.step()
    ema_update(teacher_params, student_params, momentum)


# --------------------------------------------------------------------------------------------
# gradient accumulation over micro-batches
# --------------------------------------------------------------------------------------------
def accum_mode(k, n):
    """cosa_grad_accumulate's mode for micro-step k of n > 1: 0 (acc = g) first, 2 (acc = (acc + g) * fl(1/n)) last, 1 (acc += g) between"""
    if not (n > 1 and 0 <= k < n):
        raise ValueError(f"micro-step {k} of {n}: accumulation needs n > 1 and 0 <= k < n")
    return 0 if k == 0 else (2 if k == n - 1 else 1)


def accum_scale(n):
    """fl(1/n) as a Python float: what the closing micro-step multiplies by, on the device and in torch"""
    return float(np.float32(1.0) / np.float32(n))


def check_same_grads(had, grads, names):
    """a parameter must have a gradient in every micro-step of an optimizer step or in none (the host knows: no sync)"""
    for i, (h, g) in enumerate(zip(had, grads)):
        if h != (g is not None):
            raise RuntimeError(f"{names[i]}: .grad is {'None' if g is None else 'set'} in this micro-step and was "
                               f"{'set' if h else 'None'} in the step's first one; a step's micro-batches must reach the same parameters")


@torch.no_grad()
def accumulate_grads_torch(acc, grads, k, n, names=None):
    """cosa_grad_accumulate in plain torch, for fused_optimizer=False and host trainers: the same fp32 sequence, one rounding per operation.
    acc: the list micro-step 0 returned (ignored for k == 0); grads: one gradient or None per tensor.  -> acc, one fp32 tensor or None per
    tensor: g1 after k = 0, fl(acc + g) in between, fl(fl(acc + g) * fl(1/n)) after k = n - 1.  RuntimeError (naming the tensor) when a
    tensor has a gradient in one micro-step and none in another."""
    mode = accum_mode(k, n)
    grads = list(grads)
    if mode == 0:
        return [None if g is None else g.detach().clone() for g in grads]
    names = names if names is not None else [f"param{i}" for i in range(len(grads))]
    if acc is None or len(acc) != len(grads):
        raise RuntimeError("accumulate_grads_torch: micro-step 0 has not run for this set of tensors")
    check_same_grads([a is not None for a in acc], grads, names)
    for a, g in zip(acc, grads):
        if a is not None:
            a.add_(g.detach())
            if mode == 2:
                a.mul_(accum_scale(n))
    return acc


# --------------------------------------------------------------------------------------------
# per-tensor diagnostics: norms, the EMA gap, the blame counters
# --------------------------------------------------------------------------------------------
TENSOR_STATS_SLOTS =("g_sq", "w_sq", "gap_sq", "g_absmax", "g_nonfinite", "w_nonfinite")      # cosa_tensor_stats_layout's order
assert len(TENSOR_STATS_SLOTS) == _C.constant("COSA_TENSOR_STATS_SLOTS")
TENSOR_STATS_F64 = 4         # the first four slots of a row hold float64 bits, the last two uint64 counts


def tensor_stats_layout():
    """cosa_tensor_stats_layout: ({slot name: offset in bytes}, bytes per row)"""
    off = (_C.c_size_t * len(TENSOR_STATS_SLOTS))()
    n = _C.lib().cosa_tensor_stats_layout(off)
    return {k: int(off[i]) for i, k in enumerate(TENSOR_STATS_SLOTS)}, int(n)


def new_tensor_stats(n_tensors, device):
    """the table of n_tensors rows as int64 [n_tensors, 6]: float64 bits in the first four columns, counts in the last two"""
    return torch.zeros((int(n_tensors), len(TENSOR_STATS_SLOTS)), dtype=torch.int64, device=device)


def tensor_stats_values(table):
    """the table's six columns as float64 [T, 6] (the sums and the maximum reinterpreted, the counts converted: exact below 2^53);
    on the table's device, no sync"""
    return torch.cat([table[:, :TENSOR_STATS_F64].contiguous().view(torch.float64), table[:, TENSOR_STATS_F64:].double()], dim=1)


@torch.no_grad()
def tensor_stats_torch(student, teacher, grads):
    """cosa_tensor_stats in plain torch, for fused_optimizer=False and host trainers (the role guarded_torch_step plays for the gradient
    guard): float64 sums, the same six slots, the same table layout.  student / teacher: the parameter lists of the fused step;
    grads: one gradient or None (frozen) per tensor.  -> int64 [T, 6] on the parameters' device."""
    student, teacher, grads = list(student), list(teacher), list(grads)
    assert len(student) == len(teacher) == len(grads)
    dev = student[0].device if student else "cpu"
    vals = torch.zeros((len(student), len(TENSOR_STATS_SLOTS)), dtype=torch.float64, device=dev)
    for i, (p, tp, g) in enumerate(zip(student, teacher, grads)):
        p, tp = p.detach().reshape(-1), tp.detach().reshape(-1)
        pf, tf = torch.isfinite(p), torch.isfinite(tp)
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        vals[i, 1] = torch.where(pf, p.double().square(), zero).sum()
        vals[i, 2] = torch.where(pf & tf, (tp.double() - p.double()).square(), zero).sum()
        vals[i, 5] = (~(pf & tf)).sum()
        if g is not None:
            g = g.detach().reshape(-1)
            gf = torch.isfinite(g)
            vals[i, 0] = torch.where(gf, g.double().square(), zero).sum()
            if g.numel():
                vals[i, 3] = torch.where(gf, g.abs().double(), zero).max()
            vals[i, 4] = (~gf).sum()
    return torch.cat([vals[:, :TENSOR_STATS_F64].contiguous().view(torch.int64), vals[:, TENSOR_STATS_F64:].to(torch.int64)], dim=1)


@torch.no_grad()
def grad_blame_torch(grads, blame):
    """cosa_grad_blame in plain torch: blame[t] advances by one when tensor t's gradient holds a non-finite element"""
    for i, g in enumerate(grads):
        if g is not None:
            blame[i] += (~torch.isfinite(g.detach())).any().to(blame.dtype)
    return blame


def _pooled(rows, sizes, blamed):
    """the figures of a set of rows (one tensor, a parameter group, all): square roots of the pooled sums"""
    g_sq, w_sq, gap_sq = (float(sum(r[k] for r in rows)) for k in range(3))
    weight_norm, ema_gap = w_sq ** 0.5, gap_sq ** 0.5
    return {"n": int(sum(sizes)) if all(s is not None for s in sizes) else None,
            "grad_norm": g_sq ** 0.5, "grad_absmax": float(max([r[3] for r in rows], default=0.0)),
            "weight_norm": weight_norm, "ema_gap": ema_gap,
            "ema_gap_rel": ema_gap / (weight_norm + 1e-12) if weight_norm > 0 else 0.0,          # an all-zero weight: zeros, not 1e12 or NaN
            "g_nonfinite": int(sum(r[4] for r in rows)), "w_nonfinite": int(sum(r[5] for r in rows)), "blamed": int(sum(blamed))}


def tensor_stats_summary(table, blame, names, group_idx, sizes=None):
    """What a table says, as plain Python (JSON-serialisable).  table: [T, 6], either the int64 table itself (a tensor or an array: the
    float64 bits are reinterpreted) or its values as floats (tensor_stats_values, a list out of the log interval's one sync); blame: [T]
    counts or None (no gradient guard: zeros); names: [T]; group_idx: [T] optimizer parameter group of each tensor (-1: in none);
    sizes: [T] element counts (None: `n` is None).  -> {"tensors": {name: figures}, "groups": {group: figures pooled, with square roots
    of the pooled sums}, "global": the same over all tensors, "worst": the name of the tensor with the largest `blamed`, then
    `g_nonfinite` (the first such; None when all are zero)}.  Figures: n, grad_norm, grad_absmax, weight_norm, ema_gap,
    ema_gap_rel = ema_gap / (weight_norm + 1e-12) (0 for a zero weight_norm), g_nonfinite, w_nonfinite, blamed.  A tensor synchronises."""
    if torch.is_tensor(table):
        table = table.detach().cpu().numpy()
    t = np.asarray(table)
    if t.dtype.kind in "iu":
        t = np.ascontiguousarray(t.astype(np.int64))
        t = np.concatenate([t[:, :TENSOR_STATS_F64].copy().view(np.float64), t[:, TENSOR_STATS_F64:].astype(np.float64)], axis=1)
    t = np.asarray(t, dtype=np.float64).reshape(-1, len(TENSOR_STATS_SLOTS))
    T = t.shape[0]
    names, group_idx = list(names), [int(g) for g in group_idx]
    if len(names) != T or len(group_idx) != T:
        raise ValueError(f"tensor_stats_summary: {T} rows, {len(names)} names, {len(group_idx)} group indices")
    if blame is None:
        blame = [0] * T
    elif torch.is_tensor(blame):
        blame = blame.detach().cpu().tolist()
    blame = [int(b) for b in blame]
    sizes = [None] * T if sizes is None else [int(s) for s in sizes]
    if len(blame) != T or len(sizes) != T:
        raise ValueError(f"tensor_stats_summary: {T} rows, {len(blame)} blame counters, {len(sizes)} sizes")
    rows = [tuple(float(v) for v in r) for r in t]
    tensors = {n: _pooled([rows[i]], [sizes[i]], [blame[i]]) for i, n in enumerate(names)}
    groups = {}
    for gi in sorted(set(group_idx)):
        idx = [i for i in range(T) if group_idx[i] == gi]
        groups[str(gi)] = _pooled([rows[i] for i in idx], [sizes[i] for i in idx], [blame[i] for i in idx])
    worst, key = None, (0, 0)
    for i, n in enumerate(names):
        k = (blame[i], int(rows[i][4]))
        if k > key:
            worst, key = n, k
    return {"tensors": tensors, "groups": groups, "global": _pooled(rows, sizes, blame), "worst": worst}


class FusedAdamWEMAStep:
    """optimizer.step() + the teacher EMA (main.py:250-252) + refresh of the bf16 shadow weights as ONE HIP kernel.

    State lives where torch keeps it (optimizer.state[p]['exp_avg'|'exp_avg_sq'], optimizer.param_groups[i]['lr']) so the
    PolyWarmupAdamW object stays the source of truth (state_dict compatible); this class only replaces the sweeps over
    memory.  The LR schedule is PolyWarmupAdamW's (utils/torch_helper.py:275-289).

    max_norm > 0 and / or skip_nonfinite: the gradient guard.  step() then launches the global-norm reduction and
    the guarded kernel, which clips by `coef` or refuses the whole step on the device; `self.guard` is the guard record (GUARD_WORDS int64).
    Without either, step() is the unguarded call.

    tensor_stats: per-tensor diagnostics.  The step then owns `first_chunk`, the table (`stats_table`, int64 [T, 6]),
    its workspace and -- with a guard -- `blame` (int64 [T]; None without one).  arm() makes the next step() run sample() in front of the
    optimizer kernel; with a guard every step() launches cosa_grad_blame behind cosa_grad_norm.  Without a guard and unarmed, step() does
    nothing it did not do before.  `names`: one per tensor (the stable parameter names of checkpoint.TrainState).

    accum_steps = N > 1: gradient accumulation.  The step then owns `acc`, one fp32 arena with a 16-byte-aligned
    slice per trainable tensor, and `d_acc_ptrs`; accumulate(k) adds micro-step k's gradients into it, and step() -- after accumulate(N - 1)
    -- reads the mean gradient from it instead of p.grad: norm, blame, the armed sample and the optimizer kernel are otherwise unchanged.
    With N == 1 nothing is allocated (`acc is None`) and step() is what it was."""

    def __init__(self, optimizer, student_params, teacher_params, momentum, shadow_of=None, max_norm=0.0, skip_nonfinite=False,
                 tensor_stats=False, names=None, accum_steps=1):
        import numpy as np
        self.opt = optimizer
        self.momentum = float(momentum)
        self.student = list(student_params)
        self.teacher = list(teacher_params)
        assert len(self.student) == len(self.teacher)
        dev = self.student[0].device
        L = _C.lib()
        self.rec_dtype = np.dtype([("p", "u8"), ("g", "u8"), ("m", "u8"), ("v", "u8"), ("tp", "u8"), ("p16", "u8"), ("t16", "u8"),
                                   ("lr", "f4"), ("wd", "f4"), ("n", "i8"), ("t16_f16", "i4"), ("p16_f16", "i4")])
        assert self.rec_dtype.itemsize == L.cosa_optim_record_bytes()
        group_of = {}
        for gi, g in enumerate(optimizer.param_groups):
            for p in g["params"]:
                group_of[id(p)] = gi
        self.group_idx = [group_of.get(id(p), -1) for p in self.student]
        shadow_of = shadow_of or (lambda p: None)
        n = len(self.student)
        # The trainer has no per-step host sync, so the host may run steps ahead of the GPU: the record table (gradient pointers,
        # scheduled lr / wd) is therefore kept in a ring of kRing pinned host tables + device tables.  Slot s is rewritten only after
        # the event recorded behind the H2D copy that last read it has completed, and every step's kernel reads its own device table.
        self.kRing = 4
        self.hosts = [torch.zeros(n * self.rec_dtype.itemsize, dtype=torch.uint8).pin_memory() for _ in range(self.kRing)]
        self.recs = [h.numpy().view(self.rec_dtype) for h in self.hosts]
        self.copied = [None] * self.kRing
        self.slot = 0
        self.rec = self.recs[0]
        self._step_t = torch.tensor(0.0)
        chunk = L.cosa_optim_chunk_elems()
        chunks, first_chunk = [], []
        for i, (p, tp) in enumerate(zip(self.student, self.teacher)):
            assert p.is_contiguous() and tp.is_contiguous() and p.dtype == torch.float32 and tp.dtype == torch.float32
            first_chunk.append(len(chunks))               # a tensor's chunks are contiguous and ascending in the list
            r = self.rec[i]
            r["p"], r["tp"], r["n"] = p.data_ptr(), tp.data_ptr(), p.numel()
            sp, st = shadow_of(p), shadow_of(tp)
            r["p16"] = sp.data_ptr() if sp is not None else 0
            r["t16"] = st.data_ptr() if st is not None else 0
            r["p16_f16"] = int(sp is not None and sp.dtype == torch.float16)
            r["t16_f16"] = int(st is not None and st.dtype == torch.float16)
            if self.group_idx[i] >= 0:
                stt = optimizer.state[p]
                if "exp_avg" not in stt:
                    stt["step"] = self._step_t
                    stt["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    stt["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                r["m"], r["v"] = stt["exp_avg"].data_ptr(), stt["exp_avg_sq"].data_ptr()
            chunks += [(i, c) for c in range((p.numel() + chunk - 1) // chunk)]
        self.n_chunks = len(chunks)
        self.d_chunks = torch.tensor(chunks, dtype=torch.int32, device=dev).contiguous()
        for r in self.recs[1:]:
            r[:] = self.recs[0]
        self.d_recs = [torch.empty(n * self.rec_dtype.itemsize, dtype=torch.uint8, device=dev) for _ in range(self.kRing)]
        self.max_norm, self.skip_nonfinite = float(max_norm), bool(skip_nonfinite)
        if not self.max_norm >= 0:
            raise ValueError(f"max_norm {max_norm!r}: 0 (no clipping) or a positive bound")
        self.guard = self.norm_ws = None
        if self.max_norm > 0 or self.skip_nonfinite:
            assert L.cosa_grad_guard_bytes() == GUARD_WORDS * 8
            self.guard = new_guard_state(dev)
            self.norm_ws = torch.empty(max(L.cosa_grad_norm_workspace_bytes(self.n_chunks), 8), dtype=torch.uint8, device=dev)
        self.tensor_stats = bool(tensor_stats)
        self.names = list(names) if names is not None else [f"param{i}" for i in range(n)]
        assert len(self.names) == n
        self.sizes = [int(p.numel()) for p in self.student]
        self.d_first_chunk = self.stats_table = self.stats_ws = self.blame = None
        self._armed = False
        self._last_rec = None
        if self.tensor_stats:
            assert tensor_stats_layout()[1] == 8 * len(TENSOR_STATS_SLOTS)
            self.d_first_chunk = torch.tensor(first_chunk + [len(chunks)], dtype=torch.int32, device=dev).contiguous()
            self.stats_table = new_tensor_stats(n, dev)
            self.stats_ws = torch.empty(max(L.cosa_tensor_stats_workspace_bytes(self.n_chunks), 8), dtype=torch.uint8, device=dev)
            if self.guard is not None:
                self.blame = torch.zeros(n, dtype=torch.int64, device=dev)
        self.accum_steps = int(accum_steps)
        if self.accum_steps < 1:
            raise ValueError(f"accum_steps {accum_steps!r}: a positive number of micro-steps")
        self.acc = self.acc_slices = self.d_acc_ptrs = None
        self._acc_next = 0                                 # the micro-step accumulate() expects; accum_steps: the mean is ready for step()
        self._acc_has = None                               # which tensors had a gradient in the step's first micro-step
        if self.accum_steps > 1:
            offs, total = [], 0
            for sz, gi in zip(self.sizes, self.group_idx):
                offs.append(total if gi >= 0 else None)
                if gi >= 0:
                    total += (sz + 3) // 4 * 4             # every slice starts on a 16-byte boundary
            self.acc = torch.empty(max(total, 4), dtype=torch.float32, device=dev)
            assert self.acc.data_ptr() % 16 == 0
            self.acc_slices = [None if o is None else self.acc[o:o + sz] for o, sz in zip(offs, self.sizes)]
            self.d_acc_ptrs = torch.tensor([0 if a is None else a.data_ptr() for a in self.acc_slices], dtype=torch.int64, device=dev)

    def _take_slot(self):
        """the next slot of the record-table ring, once the copy that last read its host table has completed"""
        slot = self.slot
        self.slot = (slot + 1) % self.kRing
        if self.copied[slot] is not None:
            self.copied[slot].synchronize()            # the copy issued kRing steps ago; never waits in practice
        return slot

    def _upload(self, slot):
        """host table -> device table of `slot`, and the event that guards the host table"""
        self.d_recs[slot].copy_(self.hosts[slot], non_blocking=True)
        if self.copied[slot] is None:
            self.copied[slot] = torch.cuda.Event()
        self.copied[slot].record()
        return self.d_recs[slot]

    def accumulate(self, k):
        """micro-step k of accum_steps: the current p.grad of every trainable tensor into the accumulator (cosa_grad_accumulate: acc = g
        for k == 0, acc += g, and acc = (acc + g) * fl(1/N) for the last), on the optimizer kernel's stream, no sync.  RuntimeError when a
        parameter has a gradient in one micro-step of a step and none in another."""
        n = self.accum_steps
        if n <= 1:
            raise RuntimeError("FusedAdamWEMAStep was built with accum_steps=1: there is no accumulator")
        if k != self._acc_next:
            raise RuntimeError(f"FusedAdamWEMAStep.accumulate({k}): micro-step {self._acc_next % n} of {n} is next"
                               + (" (after step())" if self._acc_next == n else ""))
        mode = accum_mode(k, n)
        grads = [p.grad if gi >= 0 else None for p, gi in zip(self.student, self.group_idx)]
        if k == 0:
            self._acc_has = [g is not None for g in grads]
        else:
            check_same_grads(self._acc_has, grads, self.names)
        slot = self._take_slot()
        rec = self.recs[slot]
        for i, g in enumerate(grads):
            rec[i]["g"] = g.data_ptr() if g is not None else 0
        d_rec = self._upload(slot)
        with _C.profiled("grad_accumulate"):
            _C.check(_C.lib().cosa_grad_accumulate(_C.ptr(d_rec), _C.ptr(self.d_chunks), self.n_chunks, _C.ptr(self.d_acc_ptrs), mode,
                                                   accum_scale(n), _C.stream_ptr()), "cosa_grad_accumulate")
        self._acc_next = k + 1

    def arm(self):
        """the next step() samples the table in front of its optimizer kernel"""
        if not self.tensor_stats:
            raise RuntimeError("FusedAdamWEMAStep was built with tensor_stats=False")
        self._armed = True

    def sample(self, d_rec=None):
        """cosa_tensor_stats on a step's device record table (default: the last step's, whose gradient pointers hold until the next
        zero_grad), on the optimizer kernel's stream, into `stats_table`.  The call does not wait for that stream; the host does wait, inside
        the call, for a read-back of first_chunk (T + 1 ints on a stream of the library's own: what cosa_tensor_stats checks before it
        launches), once per sample"""
        if not self.tensor_stats:
            raise RuntimeError("FusedAdamWEMAStep was built with tensor_stats=False")
        d_rec = self._last_rec if d_rec is None else d_rec
        if d_rec is None:
            raise RuntimeError("FusedAdamWEMAStep.sample: no step has filled a record table yet")
        with _C.profiled("tensor_stats"):
            _C.check(_C.lib().cosa_tensor_stats(_C.ptr(d_rec), _C.ptr(self.d_chunks), _C.ptr(self.d_first_chunk), len(self.student), self.n_chunks,
                                                _C.ptr(self.stats_ws), self.stats_ws.numel(), _C.ptr(self.stats_table), _C.stream_ptr()),
                     "cosa_tensor_stats")
        return self.stats_table

    def step(self):
        opt = self.opt
        acc = self.acc_slices                              # None without accumulation: the gradients are p.grad
        if acc is not None:
            if self._acc_next != self.accum_steps:
                raise RuntimeError(f"FusedAdamWEMAStep.step(): {self._acc_next} of {self.accum_steps} micro-steps accumulated")
            self._acc_next = 0
        mult = poly_warmup_lr_mult(opt.global_step, opt.warmup_iter, opt.max_iter, opt.warmup_ratio, opt.power, opt.min_mult)
        if mult is not None:
            for i, g in enumerate(opt.param_groups):
                g["lr"] = opt._init_lr[i] * mult
        groups = opt.param_groups
        slot = self._take_slot()
        rec = self.recs[slot]
        for i, p in enumerate(self.student):
            gi = self.group_idx[i]
            if gi >= 0 and (p.grad is not None if acc is None else self._acc_has[i]):
                rec[i]["g"] = p.grad.data_ptr() if acc is None else acc[i].data_ptr()
                rec[i]["lr"] = groups[gi]["lr"]
                rec[i]["wd"] = groups[gi]["weight_decay"]
            else:
                rec[i]["g"] = 0
        d_rec = self._upload(slot)
        b1, b2 = groups[0]["betas"]
        opt.global_step += 1
        self._step_t.fill_(float(opt.global_step))
        self._last_rec = d_rec
        if self._armed:                                    # the weights are the pre-step ones, the gradients (under DDP) already reduced
            self._armed = False
            self.sample(d_rec)
        if self.guard is None:
            _C.check(_C.lib().cosa_fused_adamw_ema(_C.ptr(d_rec), _C.ptr(self.d_chunks), self.n_chunks, float(b1), float(b2),
                                                   float(groups[0]["eps"]), int(opt.global_step), self.momentum, _C.stream_ptr()),
                     "cosa_fused_adamw_ema")
            return
        # behind loss.backward() (under DDP its hooks have all-reduced every gradient by now: each rank reduces the same values to the same
        # decision, no further collective), on the stream of the optimizer kernel
        with _C.profiled("grad_norm"):
            _C.check(_C.lib().cosa_grad_norm(_C.ptr(d_rec), _C.ptr(self.d_chunks), self.n_chunks, self.max_norm, int(self.skip_nonfinite),
                                             _C.ptr(self.norm_ws), self.norm_ws.numel(), _C.ptr(self.guard), _C.stream_ptr()), "cosa_grad_norm")
        if self.blame is not None:                         # which tensor: one small launch over the partials the norm has just left
            with _C.profiled("grad_blame"):
                _C.check(_C.lib().cosa_grad_blame(_C.ptr(self.norm_ws), _C.ptr(self.d_first_chunk), len(self.student), self.n_chunks,
                                                  _C.ptr(self.blame), _C.stream_ptr()), "cosa_grad_blame")
        with _C.profiled("adamw_ema_guarded"):
            _C.check(_C.lib().cosa_fused_adamw_ema_guarded(_C.ptr(d_rec), _C.ptr(self.d_chunks), self.n_chunks, float(b1), float(b2),
                                                           float(groups[0]["eps"]), int(opt.global_step), self.momentum, _C.ptr(self.guard),
                                                           _C.stream_ptr()), "cosa_fused_adamw_ema_guarded")


# --------------------------------------------------------------------------------------------
# evaluation helpers  (utils/torch_helper.py:12-30 format_tabs, :61-90 AverageMeter, :140-148 compute_mAP)
# --------------------------------------------------------------------------------------------
def average_precision(labels, outputs):
    """Per-sample average precision over the class axis, on the device: [b,C] {0,1} labels and scores -> ([b] AP, [b] valid).

    What sklearn's average_precision_score returns for each row (utils/torch_helper.py:146): sum over the distinct score
    thresholds, descending, of (R_n - R_{n-1}) * P_n; tied scores form ONE threshold.  Rows without a positive are invalid
    (the reference skips them)."""
    y = labels.double()
    s, order = torch.sort(outputs.double(), dim=1, descending=True, stable=True)
    yt = torch.gather(y, 1, order)
    C = y.shape[1]
    tps = yt.cumsum(1)
    last = torch.ones_like(s, dtype=torch.bool)
    last[:, :-1] = s[:, 1:] != s[:, :-1]                                  # last element of every run of equal scores
    npos = y.sum(1, keepdim=True)
    prec = tps / torch.arange(1, C + 1, device=y.device, dtype=torch.float64)
    rec = tps / npos.clamp_min(1.0)
    # recall at the previous threshold: running max of the recall at `last` positions strictly before i
    rec_at = torch.where(last, rec, torch.zeros_like(rec))
    prev = torch.cat([torch.zeros_like(rec[:, :1]), torch.cummax(rec_at, dim=1).values[:, :-1]], dim=1)
    ap = (torch.where(last, (rec - prev) * prec, torch.zeros_like(rec))).sum(1)
    return ap, npos[:, 0] > 0


def compute_mAP(labels, outputs):
    """utils/torch_helper.py:140-148: list of per-sample APs (samples without positives skipped).  One device->host copy."""
    ap, valid = average_precision(labels, outputs)
    return [float(a) for a, v in zip(ap.tolist(), valid.tolist()) if v]


class AverageMeter:
    """utils/torch_helper.py:61-90"""

    def __init__(self, *keys):
        self._data = {k: [0.0, 0] for k in keys}

    def add(self, d):
        for k, v in d.items():
            e = self._data.setdefault(k, [0.0, 0])
            e[0] += v
            e[1] += 1

    def get(self, *keys):
        vals = [self._data[k][0] / self._data[k][1] for k in keys]
        return vals[0] if len(vals) == 1 else tuple(vals)

    def pop(self, key=None):
        if key is None:
            for k in self._data:
                self._data[k] = [0.0, 0]
            return None
        v = self.get(key)
        self._data[key] = [0.0, 0]
        return v


def format_tabs(scores, name_list, cat_list=None, getmIoU_list=True):
    """utils/torch_helper.py:12-30 without the texttable dependency: (table text, last column's mIoU, list of mIoUs), values in
    per cent rounded to 2 decimals; the mIoU row is the plain mean over ALL classes of the rounded per-class values, as there."""
    import numpy as np
    keys = list(scores[0]["iou"].keys())
    vals = np.round(np.array([list(sc["iou"].values()) for sc in scores]) * 100, 2)
    names = [str(cat_list[i]) if cat_list is not None else str(k) for i, k in enumerate(keys)]
    wid = max([len(n) for n in names] + [5])
    lines = ["| " + "Class".ljust(wid) + " | " + " | ".join(n.rjust(8) for n in name_list) + " |"]
    for i, n in enumerate(names):
        lines.append("| " + n.ljust(wid) + " | " + " | ".join(f"{v:8.2f}" for v in vals[:, i]) + " |")
    means = vals.mean(1)
    lines.append("| " + "mIoU".ljust(wid) + " | " + " | ".join(f"{v:8.2f}" for v in means) + " |")
    return "\n".join(lines), means[-1], list(means)


# --------------------------------------------------------------------------------------------
# checkpoints  (utils/torch_helper.py:101-117 save_best; main.py:401-412 finaleval's load)
# --------------------------------------------------------------------------------------------
class EMAtracker:
    """utils/torch_helper.py:90-99.  `update` also takes a device scalar (the adaptive thresholds never visit the host); a
    non-finite new value (a fit that left an outer component empty -- the reference would have raised) leaves X as it is."""

    def __init__(self, initial_value=0, decay=0.9):
        self.X = initial_value
        self.decay = decay

    def update(self, value):
        keep, mix = self.decay, 1 - self.decay
        if torch.is_tensor(value):
            x = torch.as_tensor(self.X, dtype=value.dtype, device=value.device)
            self.X = torch.where(torch.isfinite(value), x * keep + value * mix, x)
        else:
            self.X = self.X * keep + value * mix

    def get(self):
        return self.X


def save_best(output_dir, model, finish_epoch, result, args, s_or_t, comment=''):
    """Same file name and dict layout as the reference ({'s_or_t','model','epoch','args','result'}), written by rank 0 only
    (utils.save_on_master).  `model.state_dict()` has the reference's key names, so either code base reads the other's files."""
    import os
    import torch.distributed as dist
    path = os.path.join(str(output_dir), f'best_{comment}.pth')
    if dist.is_available() and dist.is_initialized() and dist.get_rank() != 0:
        return path
    os.makedirs(str(output_dir), exist_ok=True)
    model = getattr(model, "module", model)                      # unwrap DistributedDataParallel
    torch.save({'s_or_t': s_or_t, 'model': {k: v.detach().cpu() for k, v in model.state_dict().items()}, 'epoch': finish_epoch,
                'args': args, 'result': result}, path)
    return path


def load_best(model, path, strict=True):
    """main.py:410-412: `ckpt["model"]` into the network (strict by default, as there); returns the checkpoint dict."""
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    getattr(model, "module", model).load_state_dict(ckpt["model"], strict=strict)
    return ckpt
