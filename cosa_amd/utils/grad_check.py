"""The --grad_check_iters check: the step's raw fp32 gradient g against central differences of the loss along g itself.

Per direction d (a set of parameter tensors) the check measures r = <grad L, g> / <g, g> restricted to d: 1 for an exact gradient,
1 / (1 + |e|^2 / |grad L|^2) for one that carries an orthogonal error e.  This module holds everything but the loss evaluations, which are
the trainer's (CoSATrainer._grad_check): the directions by parameter name, the record table and the two HIP streams over the parameters
(csrc/grad_check_kernels.hip; include/cosa_hip.h: the layouts), their torch composition for host tensors, and the host maths on a finished
record.  tests/grad_check_ref.py restates the two streams and the maths in float64 NumPy."""
import math
import re

import numpy as np
import torch

from .. import _C

CHUNK = _C.constant("COSA_GRAD_CHECK_CHUNK")
RECORD = _C.constant("COSA_GRAD_CHECK_RECORD")       # doubles per direction
G2, W2, S, FLAGS, T, LOSS, BAD_G, BAD_W = 0, 1, 2, 3, 4, 8, 33, 34
FLAG_ZERO_GRAD, FLAG_BAD_GRAD, FLAG_BAD_WEIGHT, FLAG_NO_STEP = 1, 2, 4, 8
FLAG_NAMES = ((FLAG_ZERO_GRAD, "zero_grad"), (FLAG_BAD_GRAD, "nonfinite_grad"), (FLAG_BAD_WEIGHT, "nonfinite_weight"), (FLAG_NO_STEP, "no_step"))
STEPS = (1.0, -1.0, 0.5, -0.5)                 # c of perturb's slots 0..3
TERMS = ("cls", "cls_aux", "seg", "cam", "reg")
MODES = ("fp32", "fp64")                       # a 16-bit forward is too noisy to difference
DIRS = ("all", "sites")
# the relative step |s g| / |w|: the decade of the sweep on the synthetic trainer at 448^2, b = 16 where r(1) and r(1/2) agree best in both
# modes (profiles/grad_check.json)
DEFAULT_RHO = 1e-5

_TABLE_DTYPE = np.dtype([("w", "<u8"), ("g", "<u8"), ("dst", "<u8"), ("n", "<i8"), ("dir", "<i4"), ("pad", "<i4")])
assert _TABLE_DTYPE.itemsize == _C.constant("COSA_GRAD_CHECK_RECORD_BYTES")


def check_mode(mode):
    mode = str(mode)
    if mode not in MODES:
        raise ValueError(f"grad_check_mode {mode!r}: one of {', '.join(MODES)} (differences of a 16-bit forward are rounding noise)")
    return mode


def check_dirs(dirs):
    dirs = str(dirs)
    if dirs not in DIRS:
        raise ValueError(f"grad_check_dirs {dirs!r}: one of {', '.join(DIRS)}")
    return dirs


def check_rho(rho):
    rho = float(rho)
    if not (math.isfinite(rho) and rho > 0):
        raise ValueError(f"grad_check_rho {rho!r}: a finite positive relative step")
    return rho


def site_of(name):
    """the site of a parameter by its name in the (unwrapped) network: embed | block<i> | norm | decoder | heads | other"""
    m = re.match(r"encoder\.blocks\.(\d+)\.", name)
    if m:
        return "block" + m.group(1)
    if name.startswith("encoder.patch_embed.") or name in ("encoder.cls_token", "encoder.pos_embed"):
        return "embed"
    if name.startswith("encoder.norm.") or name.startswith("norm."):
        return "norm"
    if name.startswith("decoder."):
        return "decoder"
    if name.startswith(("classifier.", "aux_classifier.", "encoder.head.")):
        return "heads"
    return "other"


def _site_key(site):
    order = {"embed": 0, "norm": 2, "decoder": 3, "heads": 4, "other": 5}
    return (1, int(site[5:])) if site.startswith("block") else (order[site], 0)


def plan(names, in_play, dirs="all"):
    """-> (direction names, passes): the directions of a check over the parameters `names`, of which `in_play[i]` says whether tensor i has
    a gradient (a frozen or gradient-less one belongs to no direction).  A tensor carries ONE direction per table, so `sites` is two
    passes: ("all",) and the sites.  passes: [(first row of the record, number of directions, [direction of tensor i within the pass | -1])]"""
    dirs = check_dirs(dirs)
    passes = [(0, 1, [0 if ok else -1 for ok in in_play])]
    dir_names = ["all"]
    if dirs == "sites":
        sites = sorted({site_of(n) for n, ok in zip(names, in_play) if ok}, key=_site_key)
        at = {s: i for i, s in enumerate(sites)}
        passes.append((1, len(sites), [at[site_of(n)] if ok else -1 for n, ok in zip(names, in_play)]))
        dir_names += sites
    return dir_names, passes


def n_chunks_of(sizes):
    return sum((int(n) + CHUNK - 1) // CHUNK for n in sizes)


def table_bytes(sizes):
    return len(sizes) * _TABLE_DTYPE.itemsize + 8 * n_chunks_of(sizes)


class Table:
    """one pass's record table on the host (pinned where the device is a GPU: the upload does not wait for the stream) and on the device,
    allocated once for a list of tensor sizes; fill() writes the live pointers"""

    def __init__(self, sizes, device):
        self.sizes = [int(n) for n in sizes]
        self.n_tensors, self.n_chunks = len(self.sizes), n_chunks_of(self.sizes)
        nb = table_bytes(self.sizes)
        self.host = torch.empty(nb, dtype=torch.uint8)
        if torch.device(device).type == "cuda":
            self.host = self.host.pin_memory()
        self.dev = torch.empty(nb, dtype=torch.uint8, device=device)
        arr = self.host.numpy()
        self.recs = arr[:self.n_tensors * 40].view(_TABLE_DTYPE)
        chunks = arr[self.n_tensors * 40:].view("<i4").reshape(-1, 2)
        at = 0
        for t, n in enumerate(self.sizes):
            k = (n + CHUNK - 1) // CHUNK
            chunks[at:at + k, 0] = t
            chunks[at:at + k, 1] = np.arange(k)
            at += k
        self.workspace = torch.empty(max(int(_C.lib().cosa_grad_check_workspace_bytes(self.n_chunks)), 8), dtype=torch.uint8, device=device)

    def fill(self, ws, gs, dsts, dirs):
        """the live pointers of one check: ws / dsts fp32 contiguous tensors, gs fp32 contiguous tensors or None, dirs as plan() gives them"""
        assert len(ws) == len(gs) == len(dsts) == len(dirs) == self.n_tensors
        for i, (w, g, d, k) in enumerate(zip(ws, gs, dsts, dirs)):
            for t in (w, g, d):
                if t is not None and not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == self.sizes[i]):
                    raise ValueError(f"grad_check: tensor {i} must be contiguous fp32 of {self.sizes[i]} elements, got {t.dtype} {tuple(t.shape)}")
            if g is None and k >= 0:
                raise ValueError(f"grad_check: tensor {i} is in direction {k} and has no gradient")
            self.recs[i] = (w.data_ptr(), g.data_ptr() if g is not None else 0, d.data_ptr(), self.sizes[i], k, 0)
        self.dev.copy_(self.host, non_blocking=True)
        return self


def norms(table, n_dirs, rho, rows):
    """cosa_grad_check_norms: G2, W2, s, flags and the non-finite counts of every direction into `rows`, the [n_dirs, RECORD] float64 rows
    of the record (contiguous, on the device)"""
    assert rows.dtype == torch.float64 and rows.is_contiguous() and tuple(rows.shape) == (n_dirs, RECORD)
    _C.check(_C.lib().cosa_grad_check_norms(table.host.data_ptr(), _C.ptr(table.dev), table.n_tensors, table.n_chunks, int(n_dirs), float(rho),
                                            _C.ptr(rows), _C.ptr(table.workspace), table.workspace.numel(), _C.stream_ptr()),
             "cosa_grad_check_norms")


def perturb(table, n_dirs, d, c, slot, rows):
    """cosa_grad_check_perturb: every dst of the table written (perturbed by c s g inside direction d, copied outside), t_c into rows[d, T + slot]"""
    assert rows.dtype == torch.float64 and rows.is_contiguous() and tuple(rows.shape) == (n_dirs, RECORD)
    _C.check(_C.lib().cosa_grad_check_perturb(table.host.data_ptr(), _C.ptr(table.dev), table.n_tensors, table.n_chunks, int(n_dirs), int(d),
                                              float(c), int(slot), _C.ptr(rows), _C.ptr(table.workspace), table.workspace.numel(),
                                              _C.stream_ptr()), "cosa_grad_check_perturb")


@torch.no_grad()
def norms_torch(ws, gs, dirs, n_dirs, rho, rows):
    """norms() as a torch composition, for host tensors: the same record fields by the same rules"""
    rho = check_rho(rho)
    for d in range(n_dirs):
        mine = [(w, g) for w, g, k in zip(ws, gs, dirs) if k == d and g is not None]
        g2 = sum((g.double().square().sum() for _, g in mine), torch.zeros((), dtype=torch.float64))
        w2 = sum((w.double().square().sum() for w, _ in mine), torch.zeros((), dtype=torch.float64))
        bad_g = sum(int((~torch.isfinite(g)).sum()) for _, g in mine)
        bad_w = sum(int((~torch.isfinite(w)).sum()) for w, _ in mine)
        g2, w2 = float(g2), float(w2)
        flags = (FLAG_ZERO_GRAD if g2 == 0 else 0) | (FLAG_BAD_GRAD if (not math.isfinite(g2) or bad_g) else 0) | \
            (FLAG_BAD_WEIGHT if (not math.isfinite(w2) or bad_w) else 0)
        s = 0.0
        if not flags:
            with np.errstate(over="ignore"):
                s = float(np.float32(rho * math.sqrt(w2 / g2)))
            if not math.isfinite(s) or s == 0.0:
                s, flags = 0.0, flags | FLAG_NO_STEP
        rows[d, G2], rows[d, W2], rows[d, S], rows[d, FLAGS], rows[d, BAD_G], rows[d, BAD_W] = g2, w2, s, flags, bad_g, bad_w


@torch.no_grad()
def perturb_torch(ws, gs, dsts, dirs, d, c, slot, rows):
    """perturb() as a torch composition, for host tensors: dst = w + fl32(fl32(c s) g), the product and the sum two fp32 operations"""
    if not math.isfinite(float(c)):
        raise ValueError(f"grad_check: c {c!r} must be finite")
    s = torch.tensor(float(rows[d, S]), dtype=torch.float32)
    cs = torch.tensor(float(c), dtype=torch.float32) * s
    t = torch.zeros((), dtype=torch.float64)
    for w, g, dst, k in zip(ws, gs, dsts, dirs):
        if k == d and g is not None and float(s) != 0.0:
            dst.copy_(w + cs * g)
            t += ((dst.double() - w.double()) * g.double()).sum()
        else:
            dst.copy_(w)
    rows[d, T + slot] = t


def _ratio(num, den):
    return num / den if den != 0 and math.isfinite(den) else float("nan")


def summarize(record, dir_names, weights):
    """the host maths on a finished record ([n_dirs][RECORD] numbers) -> one dict per direction.  weights: the five loss weights of the step
    (the objective is their dot product with the five terms, formed here in float64).  r1, r_half: central differences over the realised
    steps at c = 1, 1/2; r_star: their Richardson combination (the h^2 term cancels); rough = |r1 - r_half|; curv = (L(+1) + L(-1) -
    2 L(0)) / (s^2 G2); terms: r_star of each loss term alone (weight 1): the term's own directional derivative over <g, g>"""
    out = []
    wts = [float(w) for w in weights]
    for name, row in zip(dir_names, record):
        row = [float(v) for v in row]
        flags = int(row[FLAGS])
        t = row[T:T + 4]
        terms = [[row[LOSS + 5 * j + i] for i in range(5)] for j in range(5)]          # [evaluation][term]
        total = [sum(w * v for w, v in zip(wts, e)) for e in terms]

        def rs(L):
            r1 = _ratio(L[1] - L[2], t[0] - t[1])
            rh = _ratio(L[3] - L[4], t[2] - t[3])
            return r1, rh, (4.0 * rh - r1) / 3.0

        r1, rh, rstar = rs(total)
        s, g2 = row[S], row[G2]
        d = dict(dir=name, r1=r1, r_half=rh, r_star=rstar, rough=abs(r1 - rh), curv=_ratio(total[1] + total[2] - 2.0 * total[0], s * s * g2),
                 G2=g2, W2=row[W2], s=s, flags=flags, flag_names=[n for b, n in FLAG_NAMES if flags & b], nonfinite_g=int(row[BAD_G]),
                 nonfinite_w=int(row[BAD_W]), t=t, loss0=total[0],
                 terms={k: rs([e[i] for e in terms])[2] for i, k in enumerate(TERMS)})
        out.append(d)
    return out


def worst(summary):
    """the site direction whose r_star lies farthest from 1 (None without site directions or finite figures)"""
    sites = [d for d in summary[1:] if math.isfinite(d["r_star"])]
    return max(sites, key=lambda d: abs(d["r_star"] - 1.0)) if sites else None


def line(summary, mode):
    """` gcheck[fp64]: r 0.987 (worst 0.912 block7), curv 3.1e+00` -- r_star of `all`, the site farthest from 1 where sites were asked for"""
    a, w = summary[0], worst(summary)
    return " gcheck[%s]: r %.3f%s, curv %.1e" % (mode, a["r_star"], " (worst %.3f %s)" % (w["r_star"], w["dir"]) if w else "", a["curv"])


def jsonable(v):
    """NaN / inf as None: a record line stays strict JSON"""
    if isinstance(v, float):
        return v if math.isfinite(v) else None
    if isinstance(v, dict):
        return {k: jsonable(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [jsonable(x) for x in v]
    return v


def table_text(summary):
    rows = ["%-10s %9s %9s %9s %9s %10s %10s %10s  %s" % ("dir", "r_star", "r1", "r_half", "rough", "curv", "|g|", "s", "flags")]
    for d in summary:
        rows.append("%-10s %9.5f %9.5f %9.5f %9.1e %10.2e %10.3e %10.3e  %s" % (
            d["dir"], d["r_star"], d["r1"], d["r_half"], d["rough"], d["curv"], math.sqrt(d["G2"]) if d["G2"] >= 0 else float("nan"), d["s"],
            ",".join(d["flag_names"]) or "-"))
    return "\n".join(rows)
