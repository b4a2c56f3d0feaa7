"""Full-state checkpoints, the host side (cosa_amd/checkpoint.py): arena layout, checksums, file format, `--resume auto`,
pruning, the launcher's flags, and a host-device trainer that is saved, rebuilt with another seed, loaded and continued bit for bit."""
import os
import random

import numpy as np
import pytest
import torch

from cosa_amd import checkpoint as ck


def test_layout_is_aligned_deterministic_and_matches_the_library():
    rng = np.random.default_rng(0)
    nbytes = [0, 1, 3, 15, 16, 17, 255, 4096, 0, 65537] + [int(v) for v in rng.integers(0, 1 << 20, 50)]
    offs, total = ck.host_layout(nbytes)
    assert offs[0] == 0 and all(o % 16 == 0 for o in offs) and total % 16 == 0
    for i in range(len(nbytes) - 1):
        assert offs[i + 1] - offs[i] == (nbytes[i] + 15) // 16 * 16          # slots follow each other, each rounded up to 16
    assert total == offs[-1] + (nbytes[-1] + 15) // 16 * 16 and total >= sum(nbytes)
    assert ck.host_layout(nbytes) == (offs, total)
    from cosa_amd import _C
    assert os.path.exists(_C.LIB_PATH), "the library must be built: this test compares it with the host restatement"
    assert ck.state_layout(nbytes) == (offs, total)                          # cosa_state_layout (the built library) is the same definition
    assert ck.state_layout([]) == ([], 0) and ck.state_layout([0, 0]) == ([0, 0], 0)
    assert ck.state_layout([1 << 40])[1] == 1 << 40
    for bad in ([(1 << 40) + 1], [1] * 4097):
        with pytest.raises(ValueError):
            ck.state_layout(bad)
        with pytest.raises(ValueError):
            ck.host_layout(bad)


def test_checksums_follow_the_definition():
    rng = np.random.default_rng(1)
    b = rng.integers(0, 256, 48, dtype=np.uint8)
    w = [int.from_bytes(bytes(b[4 * i:4 * i + 4]), "little") for i in range(12)]
    assert ck.host_checksums(b) == (sum(w) % 2 ** 64, sum((i + 1) * v for i, v in enumerate(w)) % 2 ** 64)
    big = np.full(1 << 16, 0xFF, np.uint8)                                    # wraps mod 2^64 without complaint
    n = 1 << 14
    assert ck.host_checksums(big) == ((n * 0xFFFFFFFF) % 2 ** 64, (0xFFFFFFFF * n * (n + 1) // 2) % 2 ** 64)
    assert ck.host_checksums(np.zeros(0, np.uint8)) == (0, 0)


def test_header_and_rng_section_round_trip(tmp_path):
    ck_rng = ck.capture_rng(None)
    draws = (random.random(), float(np.random.rand()), float(np.random.randn()), torch.rand(3))
    extra = {"n_iter": 7, "best": -1, "loss_df": {"a": [0.1, float("nan"), 1e-300]}, "df": None, "blob": b"\x00\x01\xff",
             "arr": np.arange(6, dtype=np.int16).reshape(2, 3), "loader": {"rng": ck.pack_rng(None), "epoch": None, "consumed": 3}}
    blobs = list(ck_rng[1])
    header = {"rng": ck_rng[0], "n_rng_blobs": len(blobs), "tensors": [], "extra": ck._encode(extra, blobs)}
    arena = np.arange(32, dtype=np.uint8)
    p = str(tmp_path / "state_00000008.cosa")
    ck.write_file(p, header, blobs, arena)
    assert not os.path.exists(p + ".tmp")
    h, bl, a_off, a_len = ck.read_header(p)
    assert a_len == 32 and open(p, "rb").read()[a_off:] == arena.tobytes() and a_off + a_len == os.path.getsize(p)
    got = ck._decode(h["extra"], bl)
    assert got["n_iter"] == 7 and got["blob"] == b"\x00\x01\xff" and got["df"] is None and got["loader"]["consumed"] == 3
    assert np.array_equal(got["arr"], extra["arr"]) and got["arr"].dtype == np.int16
    assert got["loss_df"]["a"][0] == 0.1 and np.isnan(got["loss_df"]["a"][1]) and got["loss_df"]["a"][2] == 1e-300
    ck.restore_rng(h["rng"], bl[:h["n_rng_blobs"]])
    again = (random.random(), float(np.random.rand()), float(np.random.randn()), torch.rand(3))
    assert again[:3] == draws[:3] and torch.equal(again[3], draws[3])
    raw = open(p, "rb").read()
    assert b"pickle" not in raw and raw[:8] == ck.MAGIC
    # refusals that need no trainer: truncation and a bad magic
    open(p, "wb").write(raw[:-1])
    with pytest.raises(ValueError, match="truncated"):
        ck.read_header(p)
    open(p, "wb").write(raw[:10])
    with pytest.raises(ValueError, match="truncated"):
        ck.read_header(p)
    open(p, "wb").write(b"NOTACOSA" + raw[8:])
    with pytest.raises(ValueError, match="magic"):
        ck.read_header(p)


def _tiny_file(path):
    ck.write_file(str(path), {"tensors": []}, [], np.zeros(16, np.uint8))


def test_auto_takes_the_newest_complete_file_and_pruning_keeps_k(tmp_path):
    d = str(tmp_path)
    assert ck.newest_state(d) is None
    for it in (4, 8, 12, 100):
        _tiny_file(ck.state_path(d, it))
    open(ck.state_path(d, 200) + ".tmp", "wb").write(b"half written")              # a writer was cut off before its rename
    raw = open(ck.state_path(d, 100), "rb").read()
    open(ck.state_path(d, 150), "wb").write(raw[:-3])                               # a cut-off file under a final name
    open(os.path.join(d, "best_seg.pth"), "wb").write(b"x")
    assert ck.list_states(d) == [ck.state_path(d, it) for it in (4, 8, 12, 100)]
    assert ck.newest_state(d) == ck.state_path(d, 100)
    gone = ck.prune_states(d, 2)
    assert gone == [ck.state_path(d, 4), ck.state_path(d, 8)]
    assert ck.list_states(d) == [ck.state_path(d, 12), ck.state_path(d, 100)]
    assert os.path.exists(ck.state_path(d, 200) + ".tmp") and os.path.exists(os.path.join(d, "best_seg.pth"))
    assert ck.prune_states(d, 0) == [] and len(ck.list_states(d)) == 2              # keep 0: nothing is ever removed


def test_flag_defaults_leave_the_run_scripts_command_lines_unchanged():
    from cosa_amd.args import parse
    new = {"save_iters": 0, "keep_states": 2, "resume": None}
    for argv in (["EXP_VOC", "--work_dir", "/tmp/x", "--dataset", "VOC12", "--voc12_root", "/data/VOC2012", "--max_iters", "32000", "--aux_layer", "-4"],
                 ["EXP_COCO", "--work_dir", "/tmp/x", "--dataset", "COCO", "--coco_root", "/data/coco/"]):
        a, changed = parse(argv)
        assert {k: getattr(a, k) for k in new} == new and not set(new) & set(changed)
        b, changed_b = parse(argv + ["--save_iters", "500", "--resume", "auto", "--keep_states", "3"])
        assert (b.save_iters, b.resume, b.keep_states) == (500, "auto", 3)
        assert {k: v for k, v in vars(b).items() if k not in new} == {k: v for k, v in vars(a).items() if k not in new}
        assert {k: v for k, v in changed_b.items() if k not in new} == changed


# ---- a host-device trainer: the real CoSATrainer set-up, optimizer and EMA around a toy network ----------------------------------------
class _TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = torch.nn.Module()
        self.encoder.proj = torch.nn.Linear(5, 7)
        self.encoder.head = torch.nn.Linear(7, 3)                # frozen by the trainer
        self.norm = torch.nn.LayerNorm(7)
        self.decoder = torch.nn.Linear(7, 3)
        self.classifier = torch.nn.Conv2d(7, 2, 1, bias=False)
        self.register_buffer("seen", torch.zeros(3, dtype=torch.int64))

    def get_param_groups(self):
        return [list(self.encoder.proj.parameters()), list(self.norm.parameters()), list(self.decoder.parameters()),
                list(self.classifier.parameters())]

    def check_nograd_precision(self, mode):
        pass


def _host_trainer(monkeypatch, seed, **over):
    from cosa_amd import train_step
    monkeypatch.setattr(train_step, "build_model", lambda args: _TinyNet())
    args = train_step.default_args("VOC12", crop_size=64, batch_size=2, usegmm=True, max_iters=100, **over)
    return train_step.CoSATrainer(args, torch.device("cpu"), seed=seed)


def _host_step(tr, k):
    """the unfused branch of CoSATrainer.step with made-up gradients; draws from every host generator like a loader would"""
    from cosa_amd.utils import torch_helper
    g = torch.Generator().manual_seed(1000 + k)
    tr.optimizer.zero_grad(set_to_none=True)
    for grp in tr.optimizer.param_groups:
        for p in grp["params"]:
            p.grad = torch.randn(p.shape, generator=g)
    tr.optimizer.step()
    torch_helper.ema_update(tr._ema_pairs[0], tr._ema_pairs[1], tr.args.momentum)
    tr.student.seen += k
    tr.cam_queue.update(torch.rand(2, 16, generator=g))
    tr.ema_lowthre.update(torch.rand((), generator=g, dtype=torch.float64))
    tr.ema_highthre.update(torch.tensor(float("nan"), dtype=torch.float64) if k == 1 else torch.rand((), generator=g, dtype=torch.float64))
    return (random.random(), float(np.random.rand()), float(torch.rand(())))


def test_host_trainer_two_plus_two_steps_equal_four_straight(tmp_path, monkeypatch):
    a = _host_trainer(monkeypatch, seed=3)
    draws_a = [_host_step(a, k) for k in range(4)]
    b = _host_trainer(monkeypatch, seed=3)
    draws_b = [_host_step(b, k) for k in range(2)]
    path = str(tmp_path / "state_00000002.cosa")
    b.save_state(path, n_iter=1, note="x")
    b.wait_state()
    c = _host_trainer(monkeypatch, seed=99)                                   # another seed: other weights, queues and generator states
    assert c.train_state().checksums() != b.train_state().checksums()
    extra = c.load_state(path)
    assert extra["n_iter"] == 1 and extra["note"] == "x"
    draws_c = [_host_step(c, k) for k in range(2, 4)]
    assert draws_b + draws_c == draws_a
    assert c.train_state().checksums() == a.train_state().checksums()
    assert c.optimizer.global_step == a.optimizer.global_step == 4
    assert [g["lr"] for g in c.optimizer.param_groups] == [g["lr"] for g in a.optimizer.param_groups]
    assert all(float(c.optimizer.state[p]["step"]) == 4.0 for g in c.optimizer.param_groups for p in g["params"])
    assert c.cam_queue.ptr == a.cam_queue.ptr == 8 and c.camaux_queue.ptr == 0
    for n in ("ema_lowthre", "ema_highthre", "ema_auxlowthre", "ema_auxhighthre"):
        assert float(getattr(c, n).X) == float(getattr(a, n).X), n
    names = c.train_state().names
    assert "ON.buffer.seen" in names and "AN.encoder.head.weight" in names and "opt.norm.weight.exp_avg_sq" in names
    assert "gmm.cam_queue.queue" in names and "gmm.trackers.X" in names and not any("head" in n for n in names if n.startswith("opt."))


def test_host_trainer_refusals_name_the_field_and_leave_the_state_alone(tmp_path, monkeypatch):
    b = _host_trainer(monkeypatch, seed=3)
    _host_step(b, 0)
    path = str(tmp_path / "state_00000001.cosa")
    b.save_state(path, n_iter=0)
    b.wait_state()
    before = b.train_state().checksums()
    for field, value in (("backbone", "dino_base_patch8_224"), ("num_classes", 81), ("crop_size", 128), ("usegmm", False), ("dataset", "COCO"),
                         ("teacher_precision", "bf16"), ("max_iters", 101)):
        old = getattr(b.args, field)
        setattr(b.args, field, value)
        try:
            with pytest.raises(ValueError, match=field) as e:
                b.load_state(path)
            assert repr(old) in str(e.value) and repr(value) in str(e.value)
        finally:
            setattr(b.args, field, old)
    header, blobs, a_off, a_len = ck.read_header(path)
    arena = open(path, "rb").read()[a_off:]

    def variant(mutate, arena=arena):
        import copy
        h = copy.deepcopy(header)
        mutate(h)
        p = str(tmp_path / "variant.cosa")
        ck.write_file(p, h, blobs, arena)
        return p

    for mutate, word in ((lambda h: h.update(world_size=8), "world_size"),
                         (lambda h: h["tensors"].pop(3), h_name := header["tensors"][3]["name"]),
                         (lambda h: h["tensors"].append(dict(h["tensors"][0], name="ON.extra.weight")), "ON.extra.weight"),
                         (lambda h: h["tensors"][0].update(shape=[5, 7]), "shape")):
        with pytest.raises(ValueError, match=word):
            b.load_state(variant(mutate))
    flipped = bytearray(arena)
    t5 = header["tensors"][5]
    flipped[t5["offset"]] ^= 0x10
    with pytest.raises(ValueError, match=t5["name"].replace(".", r"\.") + ".*nothing was restored"):
        b.load_state(variant(lambda h: None, bytes(flipped)))
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:len(raw) // 2])
    with pytest.raises(ValueError, match="truncated"):
        b.load_state(path)
    open(path, "wb").write(b"XXXXXXXX" + raw[8:])
    with pytest.raises(ValueError, match="magic"):
        b.load_state(path)
    assert b.train_state().checksums() == before and b.optimizer.global_step == 1


def test_extra_refuses_what_it_cannot_store():
    import pathlib
    for bad in (pathlib.Path("/x"), {"a": [object()]}, {1, 2}):
        with pytest.raises(TypeError, match="cannot be stored"):
            ck._encode({"v": bad}, [])


# ---- the loader position: batch k+1 after resume is batch k+1 of the uninterrupted run, names and arrays -------------------------------
@pytest.mark.parametrize("workers", [0, 2])
def test_iter_from_k_yields_batch_k_plus_one_of_the_straight_iterator(tmp_path, make_voc_tree, monkeypatch, workers):
    from cosa_amd.dataloaders import train_loader as tl
    from cosa_amd.utils import torch_helper
    root, lists, names, labels = make_voc_tree(tmp_path, n=10)
    # the device half of the loader is replaced by a pass-through: what is compared is everything the host draws and decodes
    monkeypatch.setattr(tl, "DeviceAugmenter", lambda crop, device: (lambda images, params: (images, params, None)))
    ds = tl.VOC12ClsDatasetNew(root_dir=root, name_list_dir=lists, crop_size=64)
    loader = tl.DeviceTrainLoader(ds, 2, device="cpu", num_workers=workers, shuffle=True)

    def same(a, b):
        assert a[0] == b[0] and len(a[1]) == len(b[1]) == 2                   # names
        assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))          # decoded images
        assert repr(a[2]) == repr(b[2]) and torch.equal(a[3], b[3])           # augmentation draws, labels

    torch_helper.setup_seed(11)
    start = ck.pack_rng(None)                                                 # "just before new_iter()"
    straight = list(iter(loader))
    assert len(straight) == 5 and len({tuple(b[0]) for b in straight}) == 5
    for k in (1, 4):
        ck.unpack_rng(start)
        it = iter(loader)
        for _ in range(k):
            next(it)
        at_save = ck.pack_rng(None)                                           # the save point: k batches consumed
        torch_helper.setup_seed(999)                                          # a new process: other generator states
        ck.unpack_rng(start)
        resumed = loader.iter_from(k)
        ck.unpack_rng(at_save)
        rest = list(resumed)
        assert len(rest) == 5 - k
        for got, want in zip(rest, straight[k:]):
            same(got, want)


# ---- world size 2 over gloo: rank 0 writes the shared arena, every rank its sidecar ----------------------------------------------------
def _rank_step(tr, k, rank, acc):
    out = _host_step(tr, k)
    g = torch.Generator().manual_seed(7000 + 10 * k + rank)                   # per-rank data: the queues and trackers differ by rank
    tr.camaux_queue.update(torch.rand(2, 16, generator=g))
    tr.ema_auxlowthre.update(torch.rand((), generator=g, dtype=torch.float64))
    acc += k + rank
    return out + (random.random() + rank,)


def _resume_worker(rank, world, port, tmp, ret):
    import socket  # noqa: F401
    import torch.distributed as dist
    from cosa_amd import train_step
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        train_step.build_model = lambda args: _TinyNet()

        def trainer(seed):
            args = train_step.default_args("VOC12", crop_size=64, batch_size=2, usegmm=True, max_iters=100, keep_states=1)
            tr = train_step.CoSATrainer(args, torch.device("cpu"), seed=seed)
            tr.extra_state = {"launcher.acc": torch.zeros(3, dtype=torch.float64)}
            return tr

        a = trainer(3)
        random.seed(100 + rank)
        draws_a = [_rank_step(a, k, rank, a.extra_state["launcher.acc"]) for k in range(4)]
        b = trainer(3)
        random.seed(100 + rank)
        path1, path2 = ck.state_path(tmp, 1), ck.state_path(tmp, 2)
        draws_b = [_rank_step(b, 0, rank, b.extra_state["launcher.acc"])]
        b.save_state(path1, n_iter=0, who=rank)
        draws_b.append(_rank_step(b, 1, rank, b.extra_state["launcher.acc"]))
        b.save_state(path2, n_iter=1, who=rank)
        b.wait_state()                                                        # barrier, then rank 0 prunes to keep_states = 1
        assert ck.list_states(tmp) == [path2] and ck.newest_state(tmp) == path2
        assert sorted(os.listdir(tmp)) == [os.path.basename(f) for f in (path2, ck.sidecar_path(path2, 0), ck.sidecar_path(path2, 1))]
        c = trainer(50 + rank)
        extra = c.load_state(path2)
        assert extra["n_iter"] == 1 and extra["who"] == rank
        draws_c = [_rank_step(c, k, rank, c.extra_state["launcher.acc"]) for k in (2, 3)]
        assert draws_b + draws_c == draws_a
        for part in ("shared", "local"):
            assert ck._states(c)[part].checksums() == ck._states(a)[part].checksums(), part
        assert torch.equal(c.extra_state["launcher.acc"], a.extra_state["launcher.acc"]) and c.optimizer.global_step == 4
        assert c.camaux_queue.ptr == a.camaux_queue.ptr == 8
        dist.barrier()
        if rank == 1:                                                         # a state without one rank's sidecar is not complete
            os.remove(ck.sidecar_path(path2, 1))
        dist.barrier()
        assert ck.newest_state(tmp) is None
        with pytest.raises(ValueError, match="sidecar"):
            c.load_state(path2)
        ret[rank] = ck._states(a)["local"].checksums()["gmm.camaux_queue.queue"]
    finally:
        dist.destroy_process_group()


def test_world_size_2_gloo_sidecars_round_trip(tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ret = mp.Manager().dict()
    mp.spawn(_resume_worker, args=(2, port, str(tmp_path), ret), nprocs=2, join=True)
    assert len(ret) == 2 and ret[0] != ret[1]                                 # the two ranks really held different queues
