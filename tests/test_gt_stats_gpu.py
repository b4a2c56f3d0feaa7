"""--gt_stats on the GPU: cosa_augment_labels and cosa_gt_stats against the numpy yardstick (tests/gt_stats_ref.py)
-- every comparison of counters is exact integer equality --, the cross-check with cosa_label_stats, the loader's sixth element against
the Pillow pipeline, the trainer (the flag changes no bit of a step, the counters resume with the run) and the launcher end to end."""
import functools
import json
import os
import random
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import gt_stats_ref as R
import label_stats_ref as LR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, K, S, h): the LDS path twice (K = 21 is VOC's) and, at COCO's K = 81, global atomics
SHAPES = {"K6": (2, 6, 64, 4), "K21": (2, 21, 96, 6), "K81": (2, 81, 64, 4)}


def _oracle():
    from oracle import c_oracle
    c_oracle.build()
    return c_oracle


@functools.lru_cache(maxsize=None)
def _case(name):
    """two calls per shape -- boxes full / interior, then row / empty; the second call's image 0 has no ground truth at all; integer
    logits (h / S a power of two: exact ties) -> [(inputs, reference counters)], computed once and shared"""
    B, K, S, h = SHAPES[name]
    oc = _oracle()
    calls = []
    for i, (boxes, labels, gts) in enumerate(((("full", "interior"), ("some", "all"), ("mixed", "mixed")),
                                              (("row", "empty"), ("none", "some"), ("mixed", "mixed")),
                                              (("full", "interior"), ("some", "some"), ("all255", "mixed")))):
        d = R.draw(oc, B, K, S, h, seed=900 + 10 * len(name) + i, box_kinds=boxes, label_kinds=labels, integer_logits=True, gt_kinds=gts)
        d = {k: np.ascontiguousarray(v) for k, v in d.items()}
        calls.append((d, R.reference(oc, d["gt"], d["mask_main"], d["mask_aux"], d["seg"], d["cls"], d["boxes"])))
    return calls


def _dev(d):
    dev = torch.device("cuda", 0)
    return {k: torch.from_numpy(v).to(dev) for k, v in d.items()}


def _run(t, counters, aux=True):
    from cosa_amd.utils import seg_helper
    seg_helper.gt_stats(t["gt"], t["mask_main"], t["mask_aux"] if aux else None, t["seg"], t["cls"], t["boxes"], counters)


def test_gather_equals_the_numpy_gather():
    """six images at S = 64 through DeviceAugmenter(labels=...): one smaller than the crop, one whose box has no rows; then the entry
    point alone, writing between sentinels"""
    from cosa_amd import _C
    from cosa_amd.dataloaders.augment import DeviceAugmenter, draw_params, label_tables
    S, dev = 64, torch.device("cuda", 0)
    random.seed(21)
    np.random.seed(21)
    rng = np.random.default_rng(21)
    sizes = ((90, 120), (120, 70), (60, 97), (24, 30), (75, 75), (112, 150))             # (24, 30): smaller than the crop at any scale
    images, params, labels, want = [], [], [], []
    for i, (h, w) in enumerate(sizes):
        p = draw_params(h, w, crop_size=S)
        gt = R.random_map(rng, h, w)
        sy, sx = label_tables(p, S)
        if i == 4:                                                                       # an empty row range: every row outside the image
            sy = np.full(S, -1, np.int32)
        images.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
        params.append(p)
        labels.append((gt, sy, sx))
        want.append(R.gather(gt, sy, sx))
    assert params[3]["new_h"] < S and params[3]["new_w"] < S and (want[4] == 255).all()
    assert all(np.array_equal(want[i], R.pillow_crop(labels[i][0], params[i], S)) for i in (0, 1, 2, 3, 5))
    aug = DeviceAugmenter(S, dev)
    wimg, simg, box, gt_d = aug(images, params, labels=labels)
    w0, s0, b0 = aug(images, params)
    assert gt_d.dtype == torch.uint8 and gt_d.shape == (6, S, S) and np.array_equal(gt_d.cpu().numpy(), np.stack(want))
    assert torch.equal(wimg, w0) and torch.equal(simg, s0) and torch.equal(box, b0)      # the images do not notice
    out = aug(images, params, debug=True, labels=labels)
    assert len(out) == 5 and torch.equal(out[4], gt_d)
    # the entry point alone, `out` between sentinels
    B = 6
    raw, maps, off = [], np.zeros((B, 3), np.int64), 0
    for i, (gt, _, _) in enumerate(labels):
        maps[i] = (off, gt.shape[1], gt.shape[0])
        raw.append(gt.reshape(-1))
        off += gt.size
    tables = np.stack([np.stack([sy, sx]) for _, sy, sx in labels]).astype(np.int32)
    buf = torch.full((16 + B * S * S + 16,), 7, dtype=torch.uint8, device=dev)
    L = _C.lib()
    raw_d, maps_d, tables_d = (torch.from_numpy(a).to(dev) for a in (np.concatenate(raw), maps, tables))      # (named: alive through the call)
    rc = L.cosa_augment_labels(_C.ptr(raw_d), raw_d.numel(), _C.ptr(maps_d), _C.ptr(tables_d), B, S, _C.ptr(buf[16:]), _C.stream_ptr())
    assert rc == 0
    got = buf.cpu().numpy()
    assert (got[:16] == 7).all() and (got[-16:] == 7).all() and np.array_equal(got[16:-16].reshape(B, S, S), np.stack(want))
    # a map that does not lie inside raw is not read: its image comes out as 255
    bad = maps.copy()
    bad[2, 0] = raw_d.numel() - 5
    bad_d = torch.from_numpy(bad).to(dev)
    assert L.cosa_augment_labels(_C.ptr(raw_d), raw_d.numel(), _C.ptr(bad_d), _C.ptr(tables_d), B, S, _C.ptr(buf[16:]), _C.stream_ptr()) == 0
    cut = buf.cpu().numpy()[16:-16].reshape(B, S, S)
    assert (cut[2] == 255).all() and np.array_equal(np.delete(cut, 2, 0), np.delete(np.stack(want), 2, 0))
    buf[16:-16] = 9
    # outside the envelope: a status, and nothing is touched
    assert L.cosa_augment_labels(_C.ptr(raw_d), raw_d.numel(), None, _C.ptr(tables_d), B, S, _C.ptr(buf[16:]), _C.stream_ptr()) != 0
    assert L.cosa_augment_labels(_C.ptr(raw_d), raw_d.numel(), _C.ptr(maps_d), _C.ptr(tables_d), B, 0, _C.ptr(buf[16:]), _C.stream_ptr()) != 0
    assert L.cosa_augment_labels(_C.ptr(raw_d), 0, _C.ptr(maps_d), _C.ptr(tables_d), B, S, _C.ptr(buf[16:]), _C.stream_ptr()) != 0
    torch.cuda.synchronize()
    assert bool((buf[16:-16] == 9).all())
    with pytest.raises(ValueError):
        aug(images, params, labels=labels[:5])


@pytest.mark.parametrize("name", list(SHAPES))
def test_counters_equal_the_numpy_reference(name):
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    B, K, S, h = SHAPES[name]
    assert _C.lib().cosa_gt_stats_uses_lds(K) == (0 if name == "K81" else 1)
    off, n = R.layout(K)
    calls = _case(name)
    kinds = [tuple(b) for d, _ in calls for b in d["boxes"]]
    assert (0, S, 0, S) in kinds and any(b[1] == b[0] for b in kinds) and any(b[1] - b[0] == 1 for b in kinds)
    assert any((d["gt"][0] == 255).all() for d, _ in calls) and any((d["gt"] == 200).any() for d, _ in calls)
    assert LR.top_two_margin(LR.resized_logits(_oracle(), calls[0][0]["seg"], calls[0][0]["cls"], S)) == 0.0      # the ties are there
    counters = seg_helper.new_gt_stats(K, torch.device("cuda", 0))
    total = np.zeros(n, np.int64)
    for d, want in calls:                          # the calls accumulate: after each, the counters are exactly the sum of the references
        _run(_dev(d), counters)
        total += want
        got = counters.cpu().numpy()
        assert np.array_equal(got, total), np.nonzero(got != total)[0]
    assert total[off["steps"]] == 3 and total[off["gt_other"]] > 0 and 0 < total[off["valid"]] < total[off["pix"]]
    main = total[off["main"]:off["aux"]].reshape(K, K + 1)
    assert main[:, K].sum() > 0 and main[:, :K].sum() > 0 and total[off["student"]:].sum() == total[off["valid"]]
    # without the auxiliary map its block keeps its bytes
    d, _ = calls[0]
    want = R.reference(_oracle(), d["gt"], d["mask_main"], None, d["seg"], d["cls"], d["boxes"])
    counters = torch.full((n,), 7, dtype=torch.int64, device=torch.device("cuda", 0))
    _run(_dev(d), counters, aux=False)
    got = counters.cpu().numpy() - 7
    assert np.array_equal(got, want) and not got[off["aux"]:off["student"]].any()


@pytest.mark.parametrize("name", ["K21", "K81"])
def test_cross_check_with_label_stats(name):
    """gt := the main mask as uint8, the same inputs to both kernels: student[k][k] == inter[k] and the column sums == pred[k] of
    cosa_label_stats, whatever a reference says about ties"""
    from cosa_amd.utils import seg_helper
    B, K, S, h = SHAPES[name]
    d = dict(_case(name)[0][0])
    d["gt"] = d["mask_main"].astype(np.uint8)
    t = _dev(d)
    g = seg_helper.new_gt_stats(K, t["seg"].device)
    _run(t, g)
    ls = seg_helper.new_label_stats(K, t["seg"].device)
    seg_helper.label_stats(t["mask_main"], t["mask_aux"], t["seg"], t["cls"], t["boxes"], None, None, ls)
    off, _ = R.layout(K)
    loff, _ = LR.layout(K)
    student = g.cpu().numpy()[off["student"]:].reshape(K, K)
    ls = ls.cpu().numpy()
    assert np.array_equal(np.diag(student), ls[loff["inter"]:loff["inter"] + K]) and student.sum() > 0
    assert np.array_equal(student.sum(0), ls[loff["pred"]:loff["pred"] + K])
    main = g.cpu().numpy()[off["main"]:off["aux"]].reshape(K, K + 1)
    assert np.array_equal(np.diag(main[:, :K]), ls[loff["main"]:loff["main"] + K]) and main.sum() == np.trace(main[:, :K])


def test_determinism_accumulation_and_unaligned_views():
    from cosa_amd.utils import seg_helper
    for name in ("K21", "K81"):
        K = SHAPES[name][1]
        (d0, w0), (d1, w1) = _case(name)[:2]
        runs = []
        for _ in range(2):
            counters = seg_helper.new_gt_stats(K, torch.device("cuda", 0))
            _run(_dev(d0), counters)
            _run(_dev(d1), counters)
            runs.append(counters.cpu().numpy())
        assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], w0 + w1)
    # S % 4 == 0 but the masks are views one float, gt one byte, off their alignment: the scalar loads
    K = SHAPES["K6"][1]
    d, want = _case("K6")[0]
    t = _dev(d)
    for k in ("mask_main", "mask_aux", "gt"):
        flat = torch.empty(t[k].numel() + 1, device=t[k].device, dtype=t[k].dtype)
        flat[1:] = t[k].reshape(-1)
        t[k] = flat[1:].view(t[k].shape)
        assert t[k].is_contiguous() and t[k].data_ptr() % (16 if k != "gt" else 4) != 0
    counters = seg_helper.new_gt_stats(K, t["seg"].device)
    _run(t, counters)
    assert np.array_equal(counters.cpu().numpy(), want)


def test_outside_the_envelope_returns_a_status_and_touches_nothing():
    from cosa_amd import _C
    from cosa_amd.utils import seg_helper
    dev = torch.device("cuda", 0)
    L = _C.lib()

    def call(B, K, S, h, counters, ignore=255, gt=True):
        z = lambda *s: torch.zeros(*s, device=dev)
        g = torch.zeros(B, S, S, dtype=torch.uint8, device=dev)
        return L.cosa_gt_stats(_C.ptr(g) if gt else None, _C.ptr(z(B, S, S)), None, _C.ptr(z(B, K, h, h)), _C.ptr(z(B, K - 1)),
                               _C.ptr(torch.zeros(B, 4, dtype=torch.int32, device=dev)), B, K, S, h, h, ignore, _C.ptr(counters), _C.stream_ptr())

    for K, S, h, ignore, gt, word in ((129, 16, 2, 255, True, b"K must be"), (5, 16, 17, 255, True, b"envelope"), (5, 16, 2, 3, True, b"ignore_index"),
                                      (5, 16, 2, 255, False, b"null")):
        counters = torch.full((4 + 2 * K * (K + 1) + K * K,), 3, dtype=torch.int64, device=dev)
        rc = call(1, K, S, h, counters, ignore, gt)
        assert rc != 0 and word in L.cosa_last_error()
        torch.cuda.synchronize()
        assert bool((counters == 3).all())
    with pytest.raises(ValueError):
        seg_helper.new_gt_stats(129, dev)
    with pytest.raises(_C.CosaError):                               # host tensors raise as everywhere
        seg_helper.gt_stats(torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8), None, torch.zeros(1, 3, 2, 2), torch.zeros(1, 2),
                            [[0, 8, 0, 8]], torch.zeros(4 + 24 + 9, dtype=torch.int64))


# ---- the loader ---------------------------------------------------------------------------------------------------------------------------
def _tree(make_voc_tree, tmp_path, n=6):
    from PIL import Image
    root, lists, names, labels = make_voc_tree(tmp_path, n=n)
    os.makedirs(f"{root}/SegmentationClassAug")
    rng = np.random.default_rng(4)
    for name in names:
        w, h = Image.open(f"{root}/JPEGImages/{name}.jpg").size
        Image.fromarray(R.random_map(rng, h, w)).save(f"{root}/SegmentationClassAug/{name}.png")
    return root, lists, names


def test_loader_yields_the_ground_truth_crop_and_the_same_images(make_voc_tree, tmp_path):
    from types import SimpleNamespace
    from PIL import Image
    from cosa_amd.dataloaders.augment import draw_params
    from cosa_amd.dataloaders.train_loader import DeviceTrainLoader, build_train_datasetv2
    root, lists, names = _tree(make_voc_tree, tmp_path)
    dev = torch.device("cuda", 0)
    base = dict(dataset="VOC12", voc12_root=root, coco_root="", name_list_dir=lists, scales=(0.5, 2), crop_size=64, ignore_index=255, num_classes=21)
    batches = []
    for on in (False, True):
        loader = DeviceTrainLoader(build_train_datasetv2(SimpleNamespace(**base, gt_stats=on, gt_dir=None)), 2, device=dev, num_workers=0)
        random.seed(8)
        np.random.seed(8)
        batches.append(list(loader))
        if on:
            random.seed(8)
            np.random.seed(8)
            skipped = list(loader.iter_from(1))                                          # resumption: the first batch drawn and dropped
    plain, with_gt = batches
    assert len(plain) == len(with_gt) == 3 and all(len(b) == 5 for b in plain) and all(len(b) == 6 for b in with_gt)
    for a, b in zip(plain, with_gt):
        assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:5]))
    assert len(skipped) == 2 and all(s[0] == w[0] and torch.equal(s[5], w[5]) and torch.equal(s[1], w[1]) for s, w in zip(skipped, with_gt[1:]))
    # the Pillow pipeline on the same decode and draws
    random.seed(8)
    np.random.seed(8)
    for batch in with_gt:
        for i, name in enumerate(batch[0]):
            w, h = Image.open(f"{root}/JPEGImages/{name}.jpg").size
            p = draw_params(h, w, crop_size=64, scale_range=(0.5, 2))
            assert np.array_equal(p["img_box"], batch[4][i].numpy())
            gt = np.asarray(Image.open(f"{root}/SegmentationClassAug/{name}.png"))
            assert np.array_equal(batch[5][i].cpu().numpy(), R.pillow_crop(gt, p, 64)), name


# ---- the trainer --------------------------------------------------------------------------------------------------------------------------
import test_label_stats_gpu as LS          # its _trainer / _state / _assert_same_state helpers (a test module, imported not edited)


def _gt_of(k, dev):
    g = torch.Generator().manual_seed(700 + k)
    gt = torch.randint(0, 21, (2, 16, 16), generator=g).repeat_interleave(4, 1).repeat_interleave(4, 2).to(torch.uint8)
    gt[:, 5:9, 10:40] = 255
    return gt.to(dev)


def _step(tr, k, with_gt=True):
    from cosa_amd.train_step import synthetic_batch
    batch = synthetic_batch(2, 64, 20, tr.device, seed=500 + k)
    return tr.step(*batch, n_iter=tr.args.warmup_iters + k, **(dict(gt=_gt_of(k, tr.device)) if with_gt else {}))


@functools.lru_cache(maxsize=None)
def _counting_run(directory):
    """four steps past warm-up with the flag on, a state file after the second; every step's monitor inputs are recorded and scored by the
    torch partner -> dict"""
    from cosa_amd.utils import seg_helper
    tr = LS._trainer(gt_stats=True)
    seen, plain = [], tr.update_gt_stats
    tr.update_gt_stats = lambda *a: (seen.append([t.clone() if torch.is_tensor(t) else t for t in a]), plain(*a))[1]
    logs = [_step(tr, 1), _step(tr, 2)]
    out = dict(s2=LS._state(tr), c2=tr.gt_stats_state.cpu().numpy().copy(), losses=[{k: v.clone() for k, v in l.items() if k.endswith("loss")} for l in logs])
    out["path"] = os.path.join(directory, LS.STATE_FILE)
    tr.save_state(out["path"], n_iter=1)
    tr.wait_state()
    _step(tr, 3)
    _step(tr, 4)
    out["c4"], out["s4"] = tr.gt_stats_state.cpu().numpy().copy(), LS._state(tr)
    partner = seg_helper.new_gt_stats(21, tr.device)
    for a in seen[:2]:
        seg_helper.gt_stats_torch(*a, partner)
    out["partner2"] = partner.cpu().numpy()
    return out


@pytest.fixture(scope="module")
def counting_run(tmp_path_factory):
    return _counting_run(str(tmp_path_factory.mktemp("gt_stats")))


def test_the_flag_changes_no_bit_of_a_step_and_the_counters_are_the_partners(counting_run):
    r = counting_run
    tr = LS._trainer()
    assert tr.gt_stats_state is None and tr.gt_stats() is None
    logs = [_step(tr, 1, with_gt=False), _step(tr, 2, with_gt=True)]                     # (with the flag off a gt is ignored)
    LS._assert_same_state(LS._state(tr), r["s2"])
    for l, want in zip(logs, r["losses"]):
        assert want and all(torch.equal(l[k].reshape(-1).view(torch.uint8), want[k].reshape(-1).view(torch.uint8)) for k in want)
    off, _ = R.layout(21)
    c2 = r["c2"]
    print("gt_stats trainer counters vs torch partner: differing slots", int((c2 != r["partner2"]).sum()), "of", c2.size,
          "sum |diff|", int(np.abs(c2 - r["partner2"]).sum()))
    assert c2[off["steps"]] == 2 and 0 < c2[off["valid"]] < c2[off["pix"]] and c2[off["student"]:].sum() == c2[off["valid"]]
    assert np.array_equal(c2, r["partner2"]), np.nonzero(c2 != r["partner2"])[0]
    on = LS._trainer(gt_stats=True)
    with pytest.raises(ValueError):
        _step(on, 1, with_gt=False)


def test_the_counters_resume_with_the_run_and_state_files_reconcile(counting_run, capsys):
    from cosa_amd import monitors
    r = counting_run
    tr = LS._trainer(seed=77, gt_stats=True)                        # another seed: nothing of its own survives the load
    assert tr.load_state(r["path"])["n_iter"] == 1
    assert np.array_equal(tr.gt_stats_state.cpu().numpy(), r["c2"])
    _step(tr, 3)
    _step(tr, 4)
    assert np.array_equal(tr.gt_stats_state.cpu().numpy(), r["c4"]) and r["c4"][0] == 4
    LS._assert_same_state(LS._state(tr), r["s4"])
    notes = monitors.BY_NAME["gt_stats"].notes
    off_tr = LS._trainer(seed=5)
    capsys.readouterr()
    off_tr.load_state(r["path"])                                    # the entry into a run without the flag: ignored, with the note
    assert notes[0] in capsys.readouterr().out
    LS._assert_same_state(LS._state(off_tr), r["s2"])
    without = os.path.join(os.path.dirname(r["path"]), "state_00000009.cosa")
    off_tr.save_state(without, n_iter=1)
    off_tr.wait_state()
    tr.load_state(without)                                          # ... and the reverse: the counters start at zero
    assert notes[1] in capsys.readouterr().out and int(tr.gt_stats_state.abs().sum()) == 0
    LS._assert_same_state(LS._state(tr), r["s2"])


# ---- the launcher -------------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_launcher_logs_and_writes_gt_stats(tmp_path, make_voc_tree):
    import shutil
    root, lists, names = _tree(make_voc_tree, tmp_path)
    shutil.copy(f"{lists}/train_aug.txt", f"{lists}/val.txt")
    work = str(tmp_path / "work")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), "-m", "cosa_amd.main", "EXP_G", "--work_dir", work, "--dataset", "VOC12", "--voc12_root", root,
           "--name_list_dir", lists, "--max_iters", "4", "--warmup_iters", "1", "--eval_iters", "100", "--log_iters", "2", "--aux_layer", "-4",
           "--crop_size", "64", "--batch_size", "2", "--num_workers", "0", "--pretrained", "false", "--finalval", "false", "--gt_stats", "true"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "Iter: 2;" in r.stdout and "Iter: 4;" in r.stdout and r.stdout.count(" gt: main") == 2, r.stdout[-3000:]
    recs = [json.loads(l) for l in open(os.path.join(work, "EXP_G", "gt_stats.jsonl"))]
    assert [x["iters"] for x in recs] == [2, 4]
    for x in recs:
        assert 0.0 <= x["main"]["miou"] <= 1.0 and x["steps"] == 2 and 0 < x["valid_frac"] <= 1.0
