"""Full-state checkpoints: a run saved at iteration k and continued in a new process produces the bits of the run that was never
interrupted.

`TrainState(trainer)` names every tensor that defines the future of a run -- parameters and buffers of both networks, the AdamW moments,
with --usegmm the queues and threshold trackers, with the gradient guard its record (the arena's last, optional tensor), with
--label_stats its counters and with --tensor_stats behind a guard its blame counters (optional too) -- and moves them as ONE byte arena: on the GPU with one launch of the gather / scatter kernel
of csrc/optim_kernels.hip (cosa_state_snapshot / cosa_state_restore, two 64-bit checksums per tensor), on a host-device trainer with
torch copies and the same checksums from numpy.  Everything derived (16-bit shadows, W^T copies, split rows, CAM buffers, the
captured teacher graph) is NOT state: load() rebuilds it.

File:  MAGIC | u32 version | u64 header bytes | u64 host-section bytes | u64 arena bytes | JSON header | host section | arena.
The host section holds the RNG states (and the launcher's blobs) as raw bytes; nothing in the file is ever unpickled.
"""
import ctypes
import glob
import json
import os
import random
import re
import struct
import threading

import numpy as np
import torch

from . import _C
from .monitors import BY_NAME, MONITORS

MAGIC = b"COSASTAT"
VERSION = 1
_PRE = struct.Struct("<8sIQQQ")
MAX_TENSORS = 4096
MAX_BYTES = 1 << 40
# a refusal names the field and both values
ID_FIELDS = ("backbone", "num_classes", "crop_size", "usegmm", "dataset", "teacher_precision", "max_iters")


# ---- the arena: one definition of layout and checksums for device and host ------------------------------------------------------------
def state_layout(nbytes):
    """-> (offsets, total) of the arena holding tensors of `nbytes` bytes each: 16-byte aligned slots in table order, tails zero.
    This IS cosa_state_layout: the library must be built (no second definition is consulted; `host_layout` below is the restatement
    the tests compare with it)."""
    nbytes = [int(b) for b in nbytes]
    n = len(nbytes)
    L = _C.lib()
    a = (ctypes.c_ulonglong * max(n, 1))(*nbytes)
    o = (ctypes.c_ulonglong * max(n, 1))()
    total = L.cosa_state_layout(n, a, o)
    if total == ctypes.c_size_t(-1).value:
        raise ValueError(L.cosa_last_error().decode("utf-8", "replace"))
    return [int(o[i]) for i in range(n)], int(total)


def host_layout(nbytes):
    if len(nbytes) > MAX_TENSORS:
        raise ValueError(f"state layout: {len(nbytes)} tensors (at most {MAX_TENSORS})")
    offs, off = [], 0
    for i, b in enumerate(nbytes):
        if b < 0 or b > MAX_BYTES:
            raise ValueError(f"state layout: tensor {i} has {b} bytes (at most 2^40)")
        offs.append(off)
        off += (b + 15) // 16 * 16
    return offs, off


def host_checksums(slot_bytes):
    """(s0, s1) of one zero-padded slot given as a uint8 array whose length is a multiple of 4: over its little-endian 32-bit words w_i,
    s0 = sum w_i and s1 = sum (i+1) w_i, both mod 2^64"""
    w = np.ascontiguousarray(slot_bytes).view("<u4").astype(np.uint64)
    with np.errstate(over="ignore"):
        s0 = np.add.reduce(w, dtype=np.uint64)
        s1 = np.add.reduce(w * np.arange(1, w.size + 1, dtype=np.uint64), dtype=np.uint64)
    return int(s0), int(s1)


def _as_bytes(t):
    """the bytes of a contiguous tensor as a flat uint8 view (shares memory)"""
    return t.detach().reshape(-1).view(torch.uint8)


# ---- RNG states and the launcher's blobs: raw bytes + JSON, never pickle ---------------------------------------------------------------
def capture_rng(device=None):
    """-> (meta, [bytes]) of Python `random`, NumPy's global generator, the torch CPU generator and the torch device generator"""
    ver, py, gauss = random.getstate()
    name, keys, pos, has_gauss, cached = np.random.get_state()
    meta = {"py_version": ver, "py_gauss": gauss, "np_name": name, "np_pos": int(pos), "np_has_gauss": int(has_gauss),
            "np_cached": float(cached), "device": None}
    blobs = [np.asarray(py, dtype="<u8").tobytes(), np.asarray(keys, dtype="<u4").tobytes(), torch.get_rng_state().numpy().tobytes()]
    if device is not None and torch.device(device).type == "cuda":
        meta["device"] = True
        blobs.append(torch.cuda.get_rng_state(device).numpy().tobytes())
    return meta, blobs


def restore_rng(meta, blobs, device=None):
    py = tuple(int(v) for v in np.frombuffer(blobs[0], dtype="<u8"))
    random.setstate((meta["py_version"], py, meta["py_gauss"]))
    np.random.set_state((meta["np_name"], np.frombuffer(blobs[1], dtype="<u4").copy(), meta["np_pos"], meta["np_has_gauss"], meta["np_cached"]))
    torch.set_rng_state(torch.from_numpy(np.frombuffer(blobs[2], dtype=np.uint8).copy()))
    if meta.get("device") and device is not None and torch.device(device).type == "cuda":
        torch.cuda.set_rng_state(torch.from_numpy(np.frombuffer(blobs[3], dtype=np.uint8).copy()), device)


def pack_rng(device=None):
    """the RNG states as one JSON-able value (for `extra`: the loader position carries states of an earlier moment)"""
    meta, blobs = capture_rng(device)
    return {"meta": meta, "blobs": [bytes(b) for b in blobs]}


def unpack_rng(packed, device=None):
    restore_rng(packed["meta"], packed["blobs"], device)


def _encode(obj, blobs):
    """JSON-able copy of `obj`: bytes / arrays / tensors move into the host section"""
    if isinstance(obj, (bytes, bytearray)):
        blobs.append(bytes(obj))
        return {"__blob__": len(blobs) - 1}
    if torch.is_tensor(obj):
        obj = obj.detach().cpu().numpy()
    if isinstance(obj, np.ndarray):
        blobs.append(np.ascontiguousarray(obj).tobytes())
        return {"__blob__": len(blobs) - 1, "dtype": obj.dtype.str, "shape": list(obj.shape)}
    if isinstance(obj, dict):
        return {str(k): _encode(v, blobs) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return [_encode(v, blobs) for v in obj]
    if isinstance(obj, (np.integer,)):
        return int(obj)
    if isinstance(obj, (np.floating,)):
        return float(obj)
    if obj is None or isinstance(obj, (bool, int, float, str)):
        return obj
    raise TypeError(f"state file: a value of type {type(obj).__name__} in `extra` cannot be stored (plain containers, numbers, strings, "
                    f"bytes, arrays and tensors can)")


def _decode(obj, blobs):
    if isinstance(obj, dict):
        if "__blob__" in obj:
            b = blobs[obj["__blob__"]]
            if "dtype" in obj:
                return np.frombuffer(b, dtype=np.dtype(obj["dtype"])).reshape(obj["shape"]).copy()
            return b
        return {k: _decode(v, blobs) for k, v in obj.items()}
    if isinstance(obj, list):
        return [_decode(v, blobs) for v in obj]
    return obj


# ---- the file ---------------------------------------------------------------------------------------------------------------------------
def write_file(path, header, blobs, arena):
    """header: dict (gets the blob table); blobs: list of bytes; arena: a uint8 array / buffer.  tmp + fsync + rename."""
    sizes = [len(b) for b in blobs]
    header = dict(header, blob_bytes=sizes)
    hj = json.dumps(header, allow_nan=True).encode("utf-8")
    arena = memoryview(arena).cast("B") if not isinstance(arena, (bytes, memoryview)) else arena
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        f.write(_PRE.pack(MAGIC, VERSION, len(hj), sum(sizes), len(arena)))
        f.write(hj)
        for b in blobs:
            f.write(b)
        f.write(arena)
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, path)


def read_header(path):
    """-> (header, blobs, arena offset in the file, arena bytes); ValueError for a bad magic or a truncated file.  Reads no arena bytes."""
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        pre = f.read(_PRE.size)
        if len(pre) < _PRE.size:
            raise ValueError(f"{path}: truncated file ({size} bytes, the preamble alone has {_PRE.size})")
        magic, version, hlen, blen, alen = _PRE.unpack(pre)
        if magic != MAGIC:
            raise ValueError(f"{path}: bad magic {magic!r} (expected {MAGIC!r})")
        if version != VERSION:
            raise ValueError(f"{path}: file version {version} (this build reads {VERSION})")
        want = _PRE.size + hlen + blen + alen
        if size != want:
            raise ValueError(f"{path}: truncated file ({size} bytes, the preamble announces {want})")
        header = json.loads(f.read(hlen).decode("utf-8"))
        blobs = [f.read(n) for n in header["blob_bytes"]]
    return header, blobs, _PRE.size + hlen + blen, alen


def sidecar_path(path, rank):
    """the per-rank file next to a state file written under a process group: that rank's RNG states, loader position, queues"""
    return f"{path}.rank{int(rank)}"


def is_complete(path):
    """the file is whole -- and, when it was written by a process group, so is the sidecar of every rank"""
    try:
        header = read_header(path)[0]
        world = int(header.get("world_size", 1))
        if world > 1 and header.get("part") == "shared":
            for r in range(world):
                read_header(sidecar_path(path, r))
        return True
    except (ValueError, OSError, KeyError, json.JSONDecodeError):
        return False


_STATE_RE = re.compile(r"state_(\d+)\.cosa$")


def state_path(output_dir, n_iter):
    return os.path.join(str(output_dir), f"state_{int(n_iter):08d}.cosa")


def list_states(output_dir):
    """complete state_*.cosa files of a directory, oldest first (by iteration); `.tmp` and cut-off files are not in the list"""
    found = []
    for p in glob.glob(os.path.join(str(output_dir), "state_*.cosa")):
        m = _STATE_RE.search(os.path.basename(p))
        if m and is_complete(p):
            found.append((int(m.group(1)), p))
    return [p for _, p in sorted(found)]


def newest_state(output_dir):
    """what `--resume auto` takes: the newest complete file, or None"""
    s = list_states(output_dir)
    return s[-1] if s else None


def prune_states(output_dir, keep):
    """remove all but the `keep` newest complete files; returns the removed paths"""
    s = list_states(output_dir)
    gone = s[:-keep] if keep > 0 else []
    for p in gone:
        for f in [p] + glob.glob(glob.escape(p) + ".rank*"):
            try:
                os.remove(f)
            except FileNotFoundError:      # (another writer thread of this process was quicker)
                pass
    return gone


class DeviceTable:
    """The record table and chunk list of the gather / scatter kernel for a fixed list of contiguous device tensors (any dtype, any
    alignment): snapshot() and restore() are ONE launch each on the current stream."""

    def __init__(self, tensors, names=None):
        self.tensors = list(tensors)
        self.names = list(names) if names is not None else [str(i) for i in range(len(self.tensors))]
        for n, t in zip(self.names, self.tensors):
            if not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"state table: tensor {n} must be a contiguous device tensor")
        self.nbytes = [t.numel() * t.element_size() for t in self.tensors]
        self.offsets, self.total = state_layout(self.nbytes)
        L, n = _C.lib(), len(self.tensors)
        dev = self.tensors[0].device if n else torch.device("cuda", torch.cuda.current_device())
        rec_dt = np.dtype([("ptr", "u8"), ("nbytes", "u8"), ("off", "u8")])
        assert rec_dt.itemsize == L.cosa_state_record_bytes()
        rec = np.zeros(max(n, 1), rec_dt)
        chunk = L.cosa_state_chunk_bytes()
        chunks = []
        for i, (t, nb, off) in enumerate(zip(self.tensors, self.nbytes, self.offsets)):
            rec[i] = (t.data_ptr(), nb, off)
            chunks += [(i, c) for c in range(((nb + 15) // 16 * 16 + chunk - 1) // chunk)]
        self.n_chunks = len(chunks)
        self.d_recs = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        self.d_chunks = torch.tensor(chunks if chunks else [(0, 0)], dtype=torch.int32, device=dev).contiguous()
        self.device = dev

    def new_sums(self):
        return torch.zeros((max(len(self.tensors), 1), 2), dtype=torch.int64, device=self.device)

    def snapshot(self, arena, sums):
        assert arena.numel() >= self.total and arena.dtype == torch.uint8 and sums.numel() >= 2 * len(self.tensors)
        _C.check(_C.lib().cosa_state_snapshot(_C.ptr(self.d_recs), _C.ptr(self.d_chunks), len(self.tensors), self.n_chunks, _C.ptr(arena),
                                              _C.ptr(sums), _C.stream_ptr()), "cosa_state_snapshot")

    def restore(self, arena, sums, scatter):
        """scatter False: only the checksums of the arena's slots (nothing else is written); True: the slots go back into the tensors"""
        assert arena.numel() >= self.total and arena.dtype == torch.uint8 and sums.numel() >= 2 * len(self.tensors)
        _C.check(_C.lib().cosa_state_restore(_C.ptr(self.d_recs), _C.ptr(self.d_chunks), len(self.tensors), self.n_chunks, _C.ptr(arena),
                                             _C.ptr(sums), 1 if scatter else 0, _C.stream_ptr()), "cosa_state_restore")

    def restore_checked(self, arena, expected, sums=None, what="arena"):
        """verify, then restore: `expected` [(s0, s1)] per tensor is compared with the checksums of the arena's bytes BEFORE any tensor is
        overwritten; a mismatch restores nothing and names the tensor (ValueError)"""
        sums = self.new_sums() if sums is None else sums
        self.restore(arena, sums, False)
        check_sums(sums.cpu().numpy().view(np.uint64), expected, self.names, what)
        self.restore(arena, sums, True)


def check_sums(got, expected, names, what):
    for i, (n, e) in enumerate(zip(names, expected)):
        g = (int(got[i, 0]), int(got[i, 1]))
        if g != (int(e[0]), int(e[1])):
            raise ValueError(f"{what}: checksum of tensor {n} differs: recorded ({int(e[0]):#x}, {int(e[1]):#x}), its bytes give "
                             f"({g[0]:#x}, {g[1]:#x}); nothing was restored")


# ---- the state of a trainer --------------------------------------------------------------------------------------------------------------
class TrainState:
    """Every tensor that defines the future of `trainer`'s run, by stable name, and its arena."""

    TRACKERS = ("ema_lowthre", "ema_highthre", "ema_auxlowthre", "ema_auxhighthre")
    GUARD = BY_NAME["guard"].state_name              # (the other optional entries: the `state_name`s of cosa_amd/monitors.py's table)

    def __init__(self, trainer, part="all"):
        """part: "all" (a world of one), or under a process group "shared" (networks and moments: identical on every rank, written by
        rank 0) / "local" (this rank's queues, trackers and launcher tensors: its sidecar)"""
        assert part in ("all", "shared", "local")
        self.part = part
        self.trainer = trainer
        self.device = trainer.device
        self.cuda = self.device.type == "cuda"
        tr, opt = trainer, trainer.optimizer
        entries = []
        for tag, net in (("ON", tr.student), ("AN", tr.model_AN)) if part != "local" else ():
            for n, p in net.named_parameters():
                entries.append((f"{tag}.{n}", p.data))
            for n, b in net.named_buffers():
                entries.append((f"{tag}.buffer.{n}", b))
        name_of = {id(p): n for n, p in tr.student.named_parameters()}
        self.opt_params = []
        for g in opt.param_groups if part != "local" else ():
            for p in g["params"]:
                st = opt.state[p]
                if "exp_avg" not in st:                 # torch creates the moments in the first step(): a fresh trainer that loads needs them now
                    on_dev = bool(g.get("fused")) or bool(g.get("capturable"))
                    st["step"] = torch.zeros((), dtype=torch.float32, device=p.device) if on_dev else torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                self.opt_params.append(p)
                for k in ("exp_avg", "exp_avg_sq"):
                    entries.append((f"opt.{name_of[id(p)]}.{k}", st[k]))
        self.trackers = []
        if getattr(tr.args, "usegmm", False) and part != "shared":
            entries.append(("gmm.cam_queue.queue", tr.cam_queue.queue))
            entries.append(("gmm.camaux_queue.queue", tr.camaux_queue.queue))
            self.trackers = [getattr(tr, n) for n in self.TRACKERS]
            # EMAtracker.update REPLACES X (a float, then a new device scalar every step): the table points at this staging row instead
            self._x_stage = torch.zeros(len(self.trackers), dtype=torch.float64, device=self.device)
            entries.append(("gmm.trackers.X", self._x_stage))
        if part != "shared":
            # tensors the launcher keeps on the device between iterations (CoSATrainer.extra_state: its running loss sums)
            for n, t in sorted(getattr(tr, "extra_state", {}).items()):
                entries.append((f"aux.{n}", t))
        if part != "local" and getattr(tr, "tensor_stats_state", None) is not None:
            # --tensor_stats' blame counters: in the shared part, because the gradients they are derived from are identical on every rank
            # behind the all-reduce.  Optional like the guard record that follows (_reconcile_optional)
            entries.append((BY_NAME["tensor_stats"].state_name, tr.tensor_stats_state))
        if part != "local" and getattr(tr, "guard_state", None) is not None:
            # the gradient guard's record (its counters; identical on every rank).  LAST, so that a file differs from one written without a
            # guard by its tail only: load() reconciles the two (_reconcile_optional), and with the guard off nothing here changes
            entries.append((self.GUARD, tr.guard_state))
        for n, t in entries:
            if not t.is_contiguous():
                raise ValueError(f"TrainState: {n} is not contiguous")
        self.names = [n for n, _ in entries]
        self.tensors = [t for _, t in entries]
        assert len(set(self.names)) == len(self.names)
        self.nbytes = [t.numel() * t.element_size() for t in self.tensors]
        self.offsets, self.total = state_layout(self.nbytes)
        self.state_bytes = sum(self.nbytes)
        self._arenas = self._hosts = self._sums = self._hsums = None
        self._writers = [None, None]
        self._errors = []
        self.n_saves = 0
        self._table = None

    # -- tables and buffers (built once: host and device memory do not grow from save to save) --
    def _ensure_buffers(self):
        if self._arenas is not None:
            return
        n, dev = len(self.tensors), self.device
        size = max(self.total, 16)
        self._arenas = [torch.zeros(size, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._sums = [torch.zeros((max(n, 1), 2), dtype=torch.int64, device=dev) for _ in range(2)]
        if self.cuda:
            self._hosts = [torch.zeros(size, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
            self._hsums = [torch.zeros((max(n, 1), 2), dtype=torch.int64, pin_memory=True) for _ in range(2)]
            self._table = DeviceTable(self.tensors, self.names)
            self._side = torch.cuda.Stream(device=dev)
            self._events = [(torch.cuda.Event(), torch.cuda.Event()) for _ in range(2)]
        else:
            self._hosts = self._arenas
            self._hsums = self._sums

    def _stage_trackers(self):
        if self.trackers:
            self._x_stage.copy_(torch.stack([torch.as_tensor(t.X, dtype=torch.float64, device=self.device).reshape(()) for t in self.trackers]))

    def _unstage_trackers(self):
        for i, t in enumerate(self.trackers):
            t.X = self._x_stage[i].clone()

    def snapshot(self, slot=0):
        """gather the state into arena `slot` and its checksums into sums `slot`, on the current stream (GPU: ONE launch)"""
        self._ensure_buffers()
        self._stage_trackers()
        arena, sums = self._arenas[slot], self._sums[slot]
        if self.cuda:
            self._table.snapshot(arena, sums)
        else:
            arena.zero_()
            for t, nb, off in zip(self.tensors, self.nbytes, self.offsets):
                if nb:
                    arena[off:off + nb].copy_(_as_bytes(t))
            self._host_sums(arena, sums)
        return arena, sums

    def _host_sums(self, arena, sums):
        a = arena.numpy()
        out = sums.numpy().view(np.uint64)
        for i, (nb, off) in enumerate(zip(self.nbytes, self.offsets)):
            out[i] = host_checksums(a[off:off + (nb + 15) // 16 * 16])

    def checksums(self):
        """{name: (s0, s1)} of the state as it is now (waits for pending files, synchronises)"""
        self.wait()
        _, sums = self.snapshot(0)
        h = sums.cpu().numpy().view(np.uint64)
        return {n: (int(h[i, 0]), int(h[i, 1])) for i, n in enumerate(self.names)}

    # -- what the header says about the run --
    def describe(self):
        tr, opt = self.trainer, self.trainer.optimizer
        import torch.distributed as dist
        world, rank = (dist.get_world_size(), dist.get_rank()) if dist.is_available() and dist.is_initialized() else (1, 0)
        fused = getattr(tr, "_fused_step", None) is not None
        steps = [float(opt.global_step)] * len(self.opt_params) if fused else [float(opt.state[p]["step"]) for p in self.opt_params]
        h = {"ident": {k: getattr(tr.args, k) for k in ID_FIELDS}, "world_size": world, "rank": rank, "part": self.part,
             "global_step": int(opt.global_step), "lr": [float(g["lr"]) for g in opt.param_groups], "opt_steps": steps,
             "tensors": [{"name": n, "dtype": str(t.dtype), "shape": list(t.shape), "offset": o, "nbytes": b}
                         for n, t, o, b in zip(self.names, self.tensors, self.offsets, self.nbytes)]}
        if self.trackers:
            h["queue_ptr"] = [int(tr.cam_queue.ptr), int(tr.camaux_queue.ptr)]
        return h

    # -- save --
    def wait(self):
        """until every file asked for so far is in place; raises what a writer thread raised"""
        for w in self._writers:
            if w is not None:
                w.join()
        self._writers = [None, None]
        if self._errors:
            e, self._errors = self._errors[0], []
            raise e

    def save(self, path, extra=None, keep=0, on_written=None):
        """Snapshot now (one launch on the current stream), copy and write behind the loop's back.  Two arenas rotate: the call waits only
        when the arena it needs belongs to a file that is not yet written.  keep > 0: older complete state files of the directory are
        removed once this one is renamed into place."""
        self._ensure_buffers()
        slot = self.n_saves % 2
        self.n_saves += 1
        if self._writers[slot] is not None:
            self._writers[slot].join()
            self._writers[slot] = None
        if self._errors:
            e, self._errors = self._errors[0], []
            raise e
        header = self.describe()
        rng_meta, blobs = capture_rng(self.device)
        header["rng"] = rng_meta
        header["n_rng_blobs"] = len(blobs)
        header["extra"] = _encode(extra or {}, blobs)
        arena, sums = self.snapshot(slot)
        host, hsums, done = self._hosts[slot], self._hsums[slot], None
        if self.cuda:
            taken, done = self._events[slot]
            taken.record()
            with torch.cuda.stream(self._side):
                self._side.wait_event(taken)
                host.copy_(arena, non_blocking=True)
                hsums.copy_(sums, non_blocking=True)
                done.record()
        else:
            host, hsums = arena.clone(), sums.clone()          # the host arena is the live one here: the writer gets its own copy
        total, names, path = self.total, self.names, str(path)

        def writer():
            try:
                if done is not None:
                    done.synchronize()
                s = hsums.numpy().view(np.uint64)
                for i, t in enumerate(header["tensors"]):
                    t["s0"], t["s1"] = int(s[i, 0]), int(s[i, 1])
                write_file(path, header, blobs, host.numpy()[:total])
                if keep > 0:
                    prune_states(os.path.dirname(path) or ".", keep)
                if on_written is not None:
                    on_written(path)
            except BaseException as e:          # surfaces in the next save() / wait()
                self._errors.append(e)

        th = threading.Thread(target=writer, name="cosa-state-writer", daemon=False)
        th.start()
        self._writers[slot] = th
        return path

    # -- load --
    def check_header(self, header, path="state file"):
        """every refusal (ValueError naming the field and both values) that needs no tensor data"""
        mine = self.describe()
        for k in ID_FIELDS:
            a, b = header["ident"].get(k), mine["ident"][k]
            if a != b:
                raise ValueError(f"{path}: {k} differs: the file has {a!r}, this run {b!r}")
        if header["world_size"] != mine["world_size"]:
            raise ValueError(f"{path}: world_size differs: the file has {header['world_size']!r}, this run {mine['world_size']!r}")
        if header.get("part", "all") != self.part:
            raise ValueError(f"{path}: part differs: the file has {header.get('part', 'all')!r}, this run reads {self.part!r}")
        if self.part == "local" and header["rank"] != mine["rank"]:
            raise ValueError(f"{path}: rank differs: the file has {header['rank']!r}, this run {mine['rank']!r}")
        theirs = {t["name"]: t for t in header["tensors"]}
        for n in self.names:
            if n not in theirs:
                raise ValueError(f"{path}: tensor {n} is missing from the file")
        mine_names = set(self.names)
        for n in theirs:
            if n not in mine_names:
                raise ValueError(f"{path}: tensor {n} of the file does not exist in this run")
        for t, m in zip(header["tensors"], mine["tensors"]):
            if t["name"] != m["name"]:
                raise ValueError(f"{path}: tensor order differs: the file has {t['name']!r} where this run has {m['name']!r}")
            for k in ("shape", "dtype", "offset", "nbytes"):
                if t[k] != m[k]:
                    raise ValueError(f"{path}: tensor {t['name']}: {k} differs: the file has {t[k]!r}, this run {m[k]!r}")

    def _optional_notes(self):
        """{name of an optional tensor: (note when the file has it and this run does not, note when only this run has it)}"""
        return {m.state_name: m.notes for m in MONITORS}

    def _reconcile_optional(self, header, a_len, path):
        """The monitors' tensors are optional (cosa_amd/monitors.py's `state_name`s): the guard record (the arena's last), --tensor_stats'
        blame counters (in front of it), and the counters the monitors keep in `extra_state` (among the launcher's tensors).  ->
        (header as this run would have written it, its arena bytes, [(file offset, arena offset, bytes)] to read, [(arena offset,
        bytes)] to zero).  A file without one of them loads into a run that has it with the tensor zero (counters start at zero); a
        file with one loads into a run without it, the entry ignored.  Each with a note.  Any other difference is left as it is, for
        check_header to refuse."""
        notes = self._optional_notes()
        theirs = header["tensors"]
        their_names, my_names = {t["name"] for t in theirs}, set(self.names)
        extra = [n for n in notes if n in their_names and n not in my_names]
        missing = [n for n in notes if n in my_names and n not in their_names]
        if not extra and not missing:
            return header, a_len, [(0, 0, a_len)], []
        slot = lambda nb: (int(nb) + 15) // 16 * 16
        for n in extra:
            print(f"note: {path}: {notes[n][0]}", flush=True)
        for n in missing:
            print(f"note: {path}: {notes[n][1]}", flush=True)
        kept = [t for t in theirs if t["name"] not in extra]
        out, segs, gaps, fi = [], [], [], 0
        for n, t, o, b in zip(self.names, self.tensors, self.offsets, self.nbytes):
            if n in missing:
                out.append({"name": n, "dtype": str(t.dtype), "shape": list(t.shape), "offset": o, "nbytes": b, "s0": 0, "s1": 0})
                gaps.append((o, slot(b)))
                continue
            if fi >= len(kept) or kept[fi]["name"] != n or int(kept[fi]["nbytes"]) != b:
                return dict(header, tensors=kept), a_len, [], []            # another run's file: check_header names the difference
            f_off, nb = int(kept[fi]["offset"]), slot(b)
            if f_off < 0 or f_off + nb > a_len:
                raise ValueError(f"{path}: tensor {n} lies outside the file's arena")
            if segs and segs[-1][0] + segs[-1][2] == f_off and segs[-1][1] + segs[-1][2] == o:
                segs[-1] = (segs[-1][0], segs[-1][1], segs[-1][2] + nb)
            else:
                segs.append((f_off, o, nb))
            out.append(dict(kept[fi], offset=o))
            fi += 1
        if fi != len(kept):
            return dict(header, tensors=kept), a_len, [], []
        return dict(header, tensors=out), self.total, segs, gaps

    def load(self, path):
        """-> extra.  Verify, then restore: the checksums of what arrived on the device are compared with the file's BEFORE any tensor is
        overwritten; then counters, everything derived, and the RNG states last."""
        path = str(path)
        header, blobs, a_off, a_len = read_header(path)              # bad magic / truncation: nothing has been touched
        header, a_len, segs, gaps = self._reconcile_optional(header, a_len, path)
        self.check_header(header, path)
        if a_len != self.total:
            raise ValueError(f"{path}: arena size differs: the file has {a_len!r}, this run {self.total!r}")
        self.wait()
        self._ensure_buffers()
        tr, opt = self.trainer, self.trainer.optimizer
        host, arena, sums = self._hosts[0], self._arenas[0], self._sums[1]
        f_len, got, view = sum(n for _, _, n in segs), 0, memoryview(host.numpy())
        with open(path, "rb") as f:
            for f_off, h_off, n in segs:
                f.seek(a_off + f_off)
                got += f.readinto(view[h_off:h_off + n]) if n else 0
        if got != f_len:
            raise ValueError(f"{path}: truncated file ({got} arena bytes read, {f_len} announced)")
        for h_off, n in gaps:
            host[h_off:h_off + n].zero_()                            # (an optional tensor the file does not have)
        if self.cuda:
            arena.copy_(host, non_blocking=True)
            self._table.restore(arena, sums, False)
        else:
            self._host_sums(arena, sums)
        check_sums(sums.cpu().numpy().view(np.uint64), [(t["s0"], t["s1"]) for t in header["tensors"]], self.names, path)
        if self.cuda:
            torch.cuda.current_stream().wait_stream(self._side)
            if getattr(tr, "_side", None) is not None:       # a teacher replay in flight reads the masters
                torch.cuda.current_stream().wait_stream(tr._side)
            self._table.restore(arena, sums, True)
        else:
            for t, nb, off in zip(self.tensors, self.nbytes, self.offsets):
                if nb:
                    _as_bytes(t).copy_(arena[off:off + nb])
        self._unstage_trackers()
        if self.trackers:
            tr.cam_queue.ptr, tr.camaux_queue.ptr = (int(v) for v in header["queue_ptr"])
        if self.part != "local":
            # counters
            opt.global_step = int(header["global_step"])
            for g, lr in zip(opt.param_groups, header["lr"]):
                g["lr"] = float(lr)
            fused = getattr(tr, "_fused_step", None)
            if fused is not None:
                fused._step_t.fill_(float(opt.global_step))
            else:
                for p, v in zip(self.opt_params, header["opt_steps"]):
                    opt.state[p]["step"].fill_(float(v))
            # everything derived: a stale shadow after a load is a silent wrong run
            for sh in (getattr(tr, "_student_shadows", None), getattr(tr, "_teacher_shadows", None)):
                if sh is not None:
                    sh.refresh(force=True)
            tr._graph = None
            tr._graph_calls = 0
            tr._teacher_pending = False
        if self.part == "shared":           # the RNG states and `extra` of this rank are in its sidecar
            return {}
        nb = header["n_rng_blobs"]
        extra = _decode(header["extra"], blobs)
        extra["rng_at_save"] = {"meta": header["rng"], "blobs": blobs[:nb]}
        restore_rng(header["rng"], blobs[:nb], self.device)
        return extra


# ---- a trainer's files: one in a world of one; under a process group the shared arena from rank 0 and a sidecar from every rank ------------
def _world():
    import torch.distributed as dist
    return (dist.get_world_size(), dist.get_rank()) if dist.is_available() and dist.is_initialized() else (1, 0)


def _states(trainer):
    st = trainer.__dict__.setdefault("_train_states", {})
    if not st:
        if _world()[0] == 1:
            st["all"] = TrainState(trainer, "all")
        else:
            st["shared"], st["local"] = TrainState(trainer, "shared"), TrainState(trainer, "local")
    return st


def trainer_state(trainer):
    """the TrainState that holds the networks and moments of `trainer` ("all", or "shared" under a process group)"""
    st = _states(trainer)
    return st.get("all") or st["shared"]


def _settle(trainer, keep):
    """process group only: every rank's files of the saves so far are in place (own writers joined, then a barrier) before rank 0 prunes"""
    import torch.distributed as dist
    st = _states(trainer)
    for s_ in st.values():
        s_.wait()
    dist.barrier()
    directory = trainer.__dict__.get("_state_dir")
    if keep > 0 and directory is not None and dist.get_rank() == 0:
        prune_states(directory, keep)
    dist.barrier()


def save_trainer(trainer, path, extra=None, keep=0):
    path = str(path)
    st = _states(trainer)
    world, rank = _world()
    if world == 1:
        return st["all"].save(path, extra, keep=keep)
    # Rank 0 writes the shared arena, every rank its sidecar.  Pruning needs all of them: it happens at the NEXT save (or wait), after a
    # barrier, so a state file is never removed while the sidecars of its successor are still being written.
    if trainer.__dict__.get("_state_dir") is not None:
        _settle(trainer, keep)
    trainer.__dict__["_state_dir"] = os.path.dirname(path) or "."
    if rank == 0:
        st["shared"].save(path, {}, keep=0)
    st["local"].save(sidecar_path(path, rank), extra, keep=0)
    return path


def wait_trainer(trainer, keep=0):
    st = trainer.__dict__.get("_train_states") or {}
    if _world()[0] > 1 and trainer.__dict__.get("_state_dir") is not None:
        _settle(trainer, keep)
    for s_ in st.values():
        s_.wait()


def load_trainer(trainer, path):
    path = str(path)
    st = _states(trainer)
    world, rank = _world()
    if world == 1:
        return st["all"].load(path)
    if not is_complete(path):
        raise ValueError(f"{path}: truncated file or missing sidecar (a state of a process group needs the sidecar of every rank)")
    st["shared"].load(path)
    return st["local"].load(sidecar_path(path, rank))
