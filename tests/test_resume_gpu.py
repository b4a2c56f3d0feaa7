"""Full-state checkpoints on the GPU: the gather / scatter kernel on a ragged table, the contract (a run saved at
iteration k and continued by a fresh trainer -- another process in the launcher test -- produces the bits of the uninterrupted run), saves
that do not disturb the run, the launcher end to end, and the refusals."""
import copy
import functools
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the kernel on a ragged table ------------------------------------------------------------------------------------------------------
def _ragged_table(dev):
    """tensors of every listed size and dtype as views at assorted element offsets of one larger buffer per dtype -> (buffers, views)"""
    from cosa_amd import _C
    chunk_bytes = _C.lib().cosa_state_chunk_bytes()
    g = torch.Generator().manual_seed(5)
    bufs, views = [], []
    for dt in (torch.uint8, torch.bfloat16, torch.float32, torch.float64, torch.int64):
        es = torch.empty((), dtype=dt).element_size()
        chunk = chunk_bytes // es
        sizes = [0, 1, 3, 5, 255, 256, 257, chunk - 1, chunk, chunk + 1, 2 * chunk + 5]
        gaps = [1, 3, 4, 8, 16, 1, 5, 7, 2, 16, 3]                        # elements in front of each tensor: odd and aligned starts
        total = sum(sizes) + sum(gaps) + 9
        buf = torch.randint(0, 256, (total * es,), dtype=torch.uint8, generator=g).to(dev).view(dt)
        bufs.append(buf)
        at = 0
        for n, gap in zip(sizes, gaps):
            at += gap
            views.append(buf[at:at + n])
            at += n
    return bufs, views


def test_state_kernel_on_a_ragged_table():
    from cosa_amd import checkpoint as ck
    dev = torch.device("cuda", 0)
    bufs, views = _ragged_table(dev)
    tab = ck.DeviceTable(views)
    assert tab.total % 16 == 0 and len({v.data_ptr() % 16 for v in views}) > 4 and any(nb % 4 for nb in tab.nbytes)
    GUARD = 256
    full = torch.full((tab.total + GUARD,), 0xA5, dtype=torch.uint8, device=dev)
    arena, sums = full[:tab.total], tab.new_sums()
    tab.snapshot(arena, sums)
    # the arena is the host concatenation by cosa_state_layout, padding zero; the guard behind it is untouched
    want = np.zeros(tab.total, np.uint8)
    host_sums = []
    for v, nb, off in zip(views, tab.nbytes, tab.offsets):
        want[off:off + nb] = v.reshape(-1).view(torch.uint8).cpu().numpy()
        host_sums.append(ck.host_checksums(want[off:off + (nb + 15) // 16 * 16]))
    got = full.cpu().numpy()
    assert np.array_equal(got[:tab.total], want)
    assert (got[tab.total:] == 0xA5).all()
    s = sums.cpu().numpy().view(np.uint64)
    assert [(int(a), int(b)) for a, b in s[:len(views)]] == host_sums
    # two snapshots of the same state: identical arena and sums
    full2 = torch.full_like(full, 0x3C)
    sums2 = tab.new_sums()
    tab.snapshot(full2[:tab.total], sums2)
    assert torch.equal(full2[:tab.total], arena) and torch.equal(sums2, sums)
    # restore into poisoned tensors: every bit comes back, bytes between the tensors stay as they are
    orig = [b.clone() for b in bufs]
    for b in bufs:
        b.view(torch.uint8).fill_(0x5A)
    # one arena byte flipped: the tensor is named, NOTHING is overwritten
    j = 29
    bad = arena.clone()
    bad[tab.offsets[j] + tab.nbytes[j] - 1] ^= 0x01
    with pytest.raises(ValueError, match=r"tensor 29 differs.*nothing was restored"):
        tab.restore_checked(bad, host_sums)
    pad = arena.clone()
    k = next(i for i, nb in enumerate(tab.nbytes) if nb % 16 and nb > 0)
    pad[tab.offsets[k] + tab.nbytes[k]] = 7                                 # a padding byte counts too
    with pytest.raises(ValueError, match=f"tensor {k} differs"):
        tab.restore_checked(pad, host_sums)
    assert all(bool((b.view(torch.uint8) == 0x5A).all()) for b in bufs)
    tab.restore_checked(arena, host_sums)
    is_view = [torch.zeros(b.numel() * b.element_size(), dtype=torch.bool, device=dev) for b in bufs]
    per = len(views) // len(bufs)
    for i, v in enumerate(views):
        b = bufs[i // per]
        o = v.data_ptr() - b.data_ptr()
        is_view[i // per][o:o + v.numel() * v.element_size()] = True
    for b, o, m in zip(bufs, orig, is_view):
        bb, ob = b.view(torch.uint8), o.view(torch.uint8)
        assert torch.equal(bb[m], ob[m])
        assert bool((bb[~m] == 0x5A).all())
    assert (full.cpu().numpy()[tab.total:] == 0xA5).all()


def test_state_kernel_envelope():
    from cosa_amd import _C, checkpoint as ck
    dev = torch.device("cuda", 0)
    empty = ck.DeviceTable([torch.empty(0, device=dev), torch.empty(0, dtype=torch.int64, device=dev)])
    sums = torch.full((2, 2), -1, dtype=torch.int64, device=dev)
    empty.snapshot(torch.empty(0, dtype=torch.uint8, device=dev), sums)       # zero-length tensors only: accepted, checksums 0
    assert empty.total == 0 and int(sums.abs().sum()) == 0
    L = _C.lib()
    rc = L.cosa_state_snapshot(None, None, 4097, 0, None, None, None)
    assert rc != 0 and b"4097" in L.cosa_last_error()
    with pytest.raises(ValueError, match="2\\^40"):
        ck.state_layout([(1 << 40) + 16])


# ---- 2. the contract ------------------------------------------------------------------------------------------------------------------------
LOSSES = ("overall_loss", "cls_loss", "cls_aux_loss", "seg_loss", "cam_loss", "reg_loss")
CONFIGS = {"default": {}, "usegmm": {"usegmm": True}, "usepar": {"usepar": True}}


def _trainer(config, precision, seed):
    from cosa_amd.train_step import CoSATrainer, default_args
    args = default_args("VOC12", crop_size=64, batch_size=2, lr=1e-3, teacher_precision=precision, **CONFIGS[config])
    return CoSATrainer(args, torch.device("cuda", 0), seed=seed)


def _steps(tr, first, last, after=None):
    from cosa_amd.train_step import synthetic_batch
    store = torch.zeros((last - first + 1, len(LOSSES)), dtype=torch.float32, device=tr.device)   # no allocation per step, no sync per step
    for k in range(first, last + 1):
        batch = synthetic_batch(2, 64, 20, tr.device, seed=500 + k)
        logs = tr.step(*batch, n_iter=tr.args.warmup_iters + k)                # past the warm-up: all five losses live
        for j, n in enumerate(LOSSES):
            store[k - first, j] = logs[n].float()
        del logs, batch
        if after is not None:
            after(k)
    torch.cuda.synchronize()
    return [{n: store[i, j] for j, n in enumerate(LOSSES)} for i in range(last - first + 1)]


@functools.lru_cache(maxsize=None)
def _run_a(config, precision):
    """A: six uninterrupted steps on the fixed batch sequence -> (losses per step, checksums of the full state) -- computed once per case"""
    tr = _trainer(config, precision, seed=3)
    losses = _steps(tr, 1, 6)
    return losses, tr.train_state().checksums()


def _same_losses(got, want):
    for step, (g, w) in enumerate(zip(got, want)):
        for n in LOSSES:
            assert torch.equal(g[n], w[n]), (step, n, float(g[n]), float(w[n]))
    assert len(got) == len(want)


@pytest.mark.parametrize("precision", ["auto", "bf16"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_saved_and_resumed_run_equals_the_uninterrupted_run(tmp_path, config, precision):
    losses_a, sums_a = _run_a(config, precision)
    assert all(float(l["seg_loss"]) != 0 and float(l["cam_loss"]) != 0 for l in losses_a)
    path = str(tmp_path / "state_00000003.cosa")
    b = _trainer(config, precision, seed=3)
    losses_b = _steps(b, 1, 3)
    b.save_state(path, n_iter=2)
    b.wait_state()
    _same_losses(losses_b, losses_a[:3])
    del b
    c = _trainer(config, precision, seed=77)                                  # ANOTHER seed: nothing of C's own survives the load
    try:
        extra = c.load_state(path)
    finally:
        os.remove(path)
    assert extra["n_iter"] == 2
    _same_losses(_steps(c, 4, 6), losses_a[3:])
    assert c.train_state().checksums() == sums_a
    assert c.optimizer.global_step == 6
    sh = c._teacher_shadows
    for p, s16 in zip(sh.params, sh.shadows):                                 # the teacher's shadows are op16(master)
        assert torch.equal(s16, p.detach().to(sh.dtype))
    for p, s16 in zip(c._student_shadows.params, c._student_shadows.shadows):
        assert torch.equal(s16, p.detach().to(torch.bfloat16))


# ---- 3. saving does not disturb ---------------------------------------------------------------------------------------------------------------
def test_saving_every_step_changes_nothing_and_keeps_two_files(tmp_path):
    from cosa_amd import checkpoint as ck
    import gc
    losses_a, sums_a = _run_a("default", "auto")
    gc.collect()                                   # trainers of earlier tests die in reference cycles: not while this test reads the allocator
    tr = _trainer("default", "auto", seed=3)
    assert tr.args.__dict__.setdefault("keep_states", 2) == 2
    mem, grew = {}, {}

    def save(k):
        before = torch.cuda.memory_allocated()
        tr.save_state(ck.state_path(tmp_path, k), n_iter=k - 1)
        mem[k] = torch.cuda.memory_allocated()
        grew[k] = mem[k] - before

    try:
        def after(k):
            save(k)
            if k == 6:                             # saves 7 and 8 from the same place as the others: the memory figures are comparable
                save(7)
                save(8)

        _same_losses(_steps(tr, 1, 6, after=after), losses_a)
        tr.wait_state()
        assert tr.train_state().checksums() == sums_a
        assert sorted(os.listdir(tmp_path)) == [os.path.basename(ck.state_path(tmp_path, k)) for k in (7, 8)]
        assert ck.list_states(tmp_path) == [ck.state_path(tmp_path, k) for k in (7, 8)]
        print("memory_allocated after each save:", mem, "growth across each save:", grew)
        assert mem[8] == mem[3]                                              # device memory does not grow from save to save
        assert grew[1] > 0 and all(grew[k] == 0 for k in range(2, 9))
        h7, h8 = (ck.read_header(ck.state_path(tmp_path, k))[0] for k in (7, 8))
        assert [(t["s0"], t["s1"]) for t in h7["tensors"]] == [(t["s0"], t["s1"]) for t in h8["tensors"]] == list(sums_a.values())
        assert h8["extra"]["n_iter"] == 7 and h8["global_step"] == 6 and h8["ident"]["teacher_precision"] == "fp16x3"
    finally:
        tr.wait_state()
        for p in glob.glob(str(tmp_path / "state_*")):
            os.remove(p)


# ---- 4. the launcher end to end -----------------------------------------------------------------------------------------------------------------
def _launch(work, root, lists, workers, *more):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "cosa_amd.main", "EXP_R", "--work_dir", work, "--dataset", "VOC12", "--voc12_root", root, "--name_list_dir", lists,
           "--max_iters", "8", "--warmup_iters", "2", "--eval_iters", "4", "--log_iters", "1", "--aux_layer", "-4", "--crop_size", "64",
           "--batch_size", "2", "--num_workers", str(workers), "--pretrained", "false", "--finalval", "false"] + list(more)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)   # a fresh child under its own time limit
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("workers", [0, 2])
def test_launcher_resumes_bit_for_bit(tmp_path, make_voc_tree, workers):
    from PIL import Image
    from cosa_amd import checkpoint as ck
    # ten images = five batches per pass: the state of iteration 4 lies inside the first pass (four batches to draw and drop on resume), the
    # resumed run crosses the end of that pass at iteration 6; two validation images keep the evaluation rounds short
    root, lists, names, labels = make_voc_tree(tmp_path, n=10)
    os.makedirs(f"{root}/SegmentationClassAug")
    for n in names[:2]:
        im = np.asarray(Image.open(f"{root}/JPEGImages/{n}.jpg"))
        Image.fromarray((im[..., 0] // 13).astype(np.uint8)).save(f"{root}/SegmentationClassAug/{n}.png")
    open(f"{lists}/val.txt", "w").write("\n".join(names[:2]) + "\n")
    straight, saved, resumed = (str(tmp_path / d) for d in ("straight", "saved", "resumed"))
    _launch(straight, root, lists, workers, "--save_iters", "8")              # uninterrupted; its only file is the final state
    _launch(saved, root, lists, workers, "--save_iters", "4")                 # the same max_iters (the schedule depends on it) ...
    out_r = os.path.join(resumed, "EXP_R")
    os.makedirs(out_r)
    shutil.move(ck.state_path(os.path.join(saved, "EXP_R"), 4), ck.state_path(out_r, 4))      # ... of which only the file of iteration 4 is kept
    shutil.rmtree(saved)
    open(os.path.join(out_r, "state_00000006.cosa.tmp"), "wb").write(b"cut off")
    open(os.path.join(out_r, "log_val.txt"), "w").write("earlier lines\n")
    stdout = _launch(resumed, root, lists, workers, "--save_iters", "4", "--resume", "auto")
    assert "Resumed from" in stdout and "continuing at iteration 4" in stdout and "Iter: 5;" in stdout and "Iter: 4;" not in stdout
    df_s = torch.load(os.path.join(straight, "EXP_R", "loss_dataframe.pt"), weights_only=False)
    df_r = torch.load(os.path.join(out_r, "loss_dataframe.pt"), weights_only=False)
    assert df_r["iters"] == df_s["iters"] == list(range(1, 9))
    for k in df_s:
        assert df_r[k][4:] == df_s[k][4:], k                                 # rows 5-8: the very same doubles
    assert all(v > 0 for k in ("seg_loss", "cam_loss") for v in df_s[k][4:])
    hs, hr = (ck.read_header(ck.state_path(d, 8))[0] for d in (os.path.join(straight, "EXP_R"), out_r))
    assert [(t["name"], t["s0"], t["s1"]) for t in hr["tensors"]] == [(t["name"], t["s0"], t["s1"]) for t in hs["tensors"]]
    assert hr["global_step"] == hs["global_step"] == 8 and hr["lr"] == hs["lr"]
    log = open(os.path.join(out_r, "log_val.txt")).read()
    assert log.startswith("earlier lines\n") and log.count("iters:7") == 1 and "iters:3" not in log
    for d in (straight, resumed):
        shutil.rmtree(d)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_their_field_and_touch_nothing(tmp_path):
    from cosa_amd import checkpoint as ck
    tr = _trainer("default", "auto", seed=5)
    path = str(tmp_path / "state_00000000.cosa")
    tr.save_state(path)
    tr.wait_state()
    before = tr.train_state().checksums()
    try:
        for field, value in (("backbone", "dino_base_patch8_224"), ("num_classes", 81), ("crop_size", 128), ("usegmm", True), ("dataset", "COCO"),
                             ("teacher_precision", "bf16"), ("max_iters", 40000)):
            old = getattr(tr.args, field)
            setattr(tr.args, field, value)
            try:
                with pytest.raises(ValueError, match=field) as e:
                    tr.load_state(path)
                assert repr(old) in str(e.value) and repr(value) in str(e.value)
            finally:
                setattr(tr.args, field, old)
        header, blobs, a_off, a_len = ck.read_header(path)
        small = str(tmp_path / "variant.cosa")

        def variant(mutate):
            h = copy.deepcopy(header)
            mutate(h)
            ck.write_file(small, h, blobs, b"")                             # (header-only refusals never reach the arena)
            return small

        gone = header["tensors"][3]["name"]
        for mutate, word in ((lambda h: h.update(world_size=8), "world_size"), (lambda h: h["tensors"].pop(3), gone),
                             (lambda h: h["tensors"].append(dict(h["tensors"][0], name="ON.extra.weight")), "ON.extra.weight"),
                             (lambda h: h["tensors"][0].update(shape=[1, 2]), "shape")):
            with pytest.raises(ValueError, match=word.replace(".", r"\.")):
                tr.load_state(variant(mutate))
        # one flipped byte of the arena: the tensor is named, nothing is restored
        t9 = header["tensors"][9]
        with open(path, "r+b") as f:
            f.seek(a_off + t9["offset"] + 2)
            b = f.read(1)
            f.seek(a_off + t9["offset"] + 2)
            f.write(bytes([b[0] ^ 0x40]))
        with pytest.raises(ValueError, match=t9["name"].replace(".", r"\.") + ".*nothing was restored"):
            tr.load_state(path)
        os.truncate(path, a_off + a_len // 2)
        with pytest.raises(ValueError, match="truncated"):
            tr.load_state(path)
        with open(path, "r+b") as f:
            f.write(b"XXXXXXXX")
        with pytest.raises(ValueError, match="magic"):
            tr.load_state(path)
        assert tr.train_state().checksums() == before
    finally:
        for p in glob.glob(str(tmp_path / "*.cosa")):
            os.remove(p)
