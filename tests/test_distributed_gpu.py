"""Multi-GPU readiness on the one-GPU box: the REAL trainer (CoSATrainer + DistributedDataParallel, bucket views, fused AdamW+EMA on the
reduced gradients, redundant teacher EMA) with two ranks in fresh child processes started by torch.distributed.run -- both ranks on card 0
over gloo (RCCL needs a card per rank; the driver's 8-GPU node runs it).  main.py:45-50,250-252."""
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(cmd, env=None):
    e = dict(os.environ)
    e.update(env or {})
    e.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("n_iter,all_losses", [(1, False), (10 ** 6, True)])
def test_two_rank_trainer_ranks_identical_and_match_single_process(tmp_path, n_iter, all_losses):
    """after 3 steps the student AND teacher parameters of the two ranks are bit-identical (same averaged gradients, same fused update,
    teacher EMA computed redundantly: no broadcast needed, SURVEY e-1).  In the warm-up phase (classification losses only: batch means,
    so the average of the per-rank gradients IS the gradient of the concatenated batch) the parameter update also equals the
    single-process run on the concatenated batch: ||delta_ddp - delta_single|| <= 0.1 ||delta_single||.  (Not tighter: AdamW's first
    steps move every weight by ~lr * sign(g), so the few per cent of components whose bf16 gradient is at noise level flip sign with the
    summation order; measured 5.5e-2.  A broken reduction -- sum instead of mean, one rank's gradients only -- gives O(1).)  With all five losses live the per-rank normalisers of seg_loss (pixel counts, utils/seg_helper.py:800-813) make
    DDP differ from a concatenated batch BY DESIGN (the reference behaves the same), so only rank identity is asserted there."""
    out = str(tmp_path)
    common = ["--out", out, "--steps", "3", "--crop", "64", "--batch", "2", "--n-iter", str(n_iter)]
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "ddp_check.py")] + common, env={"COSA_DIST_BACKEND": "gloo"})
    r0, r1 = torch.load(os.path.join(out, "rank0.pt")), torch.load(os.path.join(out, "rank1.pt"))
    assert r0["world"] == 2 and r1["world"] == 2
    for net in ("student", "teacher"):
        for k in r0[net]:
            assert torch.equal(r0[net][k], r1[net][k]), f"{net}.{k} differs between the ranks"
    if all_losses:
        return
    _run([sys.executable, os.path.join(ROOT, "tools", "ddp_check.py"), "--single"] + common)
    s = torch.load(os.path.join(out, "single.pt"))
    from cosa_amd.train_step import CoSATrainer, default_args
    torch.manual_seed(0)
    init = {k: v.detach().cpu() for k, v in CoSATrainer(default_args("VOC12", crop_size=64, batch_size=4, teacher_graph=False, lr=1e-3),
                                                        torch.device("cuda", 0), seed=0).student.named_parameters()}
    num = den = 0.0
    for k, p0 in init.items():
        d_ddp, d_one = r0["student"][k] - p0, s["student"][k] - p0
        num += float((d_ddp - d_one).double().pow(2).sum())
        den += float(d_one.double().pow(2).sum())
    assert den > 0 and (num / den) ** 0.5 <= 0.1, (num / den) ** 0.5


def test_two_rank_differing_seeds_shadows_follow_the_broadcast_masters(tmp_path):
    """ranks built from DIFFERENT seeds (the reference's --random_seed under DDP): the DDP wrap, which follows the teacher capture and so the
    construction of the 16-bit copies (CoSATrainer.prepare_ddp), broadcasts rank 0's masters over those of rank 1, and the student's
    WeightShadows is refreshed behind it.  After the first step every rank's 16-bit copy of every student parameter equals
    master.to(bf16) bit for bit -- the frozen ones too, which the fused AdamW + EMA kernel never rewrites -- and the masters of the two ranks
    are the same bits (gloo, both ranks on card 0)."""
    out = str(tmp_path)
    _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
          "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "ddp_check.py"), "--out", out, "--steps", "1", "--crop", "64",
          "--batch", "2", "--n-iter", str(10 ** 6), "--rank-seeds"], env={"COSA_DIST_BACKEND": "gloo"})
    r0, r1 = torch.load(os.path.join(out, "rank0.pt")), torch.load(os.path.join(out, "rank1.pt"))
    assert r0["world"] == 2 and r1["world"] == 2
    for r in (r0, r1):
        assert set(r["student16"]) == set(r["student"])
        for k, p in r["student"].items():
            assert torch.equal(r["student16"][k], p.to(torch.bfloat16)), f"student.{k}: the 16-bit copy is not the master's"
    for k in r0["student"]:
        assert torch.equal(r0["student"][k], r1["student"][k]), f"student.{k} differs between the ranks"


def test_two_rank_defer_groups_and_grid_policy_give_the_same_weights_and_overlap_the_buckets(tmp_path):
    """VERDICT r4 item 8 (no multi-GPU node: host logic only).  The knobs the first RCCL run will A/B -- the number of batched weight-gradient
    launches per backward pass (`defer_groups` 1 / 6) and the persistent-GEMM grid policy (0 / 1) -- must not change a single bit of the
    trained weights (the batched weight gradient writes every tile once, in the same token order, however the linears are grouped), and
    with 6 groups DDP's bucket hooks -- where the all-reduces start -- must fire while the backward pass is still running: at least one
    bucket is complete BEFORE the last DeferredWgrad node has run (with one group the encoder's gradients all arrive at the end)."""
    res = {}
    for groups, grid in ((1, 0), (6, 1)):          # (both knobs flipped at once: any difference would show; (6, 0) and (1, 1) were run once by hand)
        out = str(tmp_path / f"g{groups}p{grid}")
        _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "ddp_check.py"), "--out", out, "--steps", "3", "--crop", "64",
              "--batch", "2", "--n-iter", str(10 ** 6), "--defer-groups", str(groups), "--grid-policy", str(grid), "--log-hooks"],
             env={"COSA_DIST_BACKEND": "gloo"})
        r0, r1 = torch.load(os.path.join(out, "rank0.pt")), torch.load(os.path.join(out, "rank1.pt"))
        assert r0["defer_groups"] == groups
        for k in r0["student"]:
            assert torch.equal(r0["student"][k], r1["student"][k]), f"student.{k} differs between the ranks ({groups} groups, grid {grid})"
        res[(groups, grid)] = r0
    base = res[(1, 0)]
    for key, r in res.items():
        for net in ("student", "teacher"):
            for k in base[net]:
                assert torch.equal(base[net][k], r[net][k]), f"{net}.{k}: {key} differs from (1, 0)"
    n_early = {}
    for (groups, grid), r in res.items():
        ev, step_ev = r["events"], []
        for e in ev:
            if e[0] == "step":
                step_ev.append([])
            else:
                step_ev[-1].append(e)
        assert len(step_ev) == 3
        for evs in step_ev[1:]:          # (DDP's first iteration runs on its provisional bucket assignment -- one hook call -- and rebuilds the buckets after it)
            defers = [e for e in evs if e[0] == "defer"]
            buckets = [e for e in evs if e[0] == "bucket"]
            assert len(defers) == groups and sum(d[1] for d in defers) == 48 and len(buckets) >= 2, (groups, len(defers), len(buckets))
            n_early.setdefault((groups, grid), []).append(sum(1 for b in buckets if b[2] < defers[-1][2]))
    # (measured on the one-GPU box, gloo: with one group every bucket -- the first one holds the decoder, the heads AND the last blocks' weights --
    # completes after the single weight-gradient node, 0 early buckets; with six groups buckets 0-4 complete between the groups, 5 early)
    for a, b in zip(n_early[(6, 1)], n_early[(1, 0)]):
        assert a > b, (n_early, "six weight-gradient groups completed no more buckets before the end of the backward pass than one group")


def test_teacher_graph_is_captured_before_ddp_and_changes_no_bit(tmp_path):
    """under data parallelism the teacher's hipGraph is captured BEFORE DistributedDataParallel is constructed
    (CoSATrainer.prepare_ddp), tools/ddp_check.py fails when the capture did not succeed, and the trained weights of a 2-rank run with the
    captured side-stream teacher are the same bits as with the eager teacher (gloo, both ranks on card 0)."""
    res = {}
    for graph in (False, True):
        out = str(tmp_path / f"graph{int(graph)}")
        _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
              "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "ddp_check.py"), "--out", out, "--steps", "4", "--crop", "64",
              "--batch", "2", "--n-iter", str(10 ** 6)] + (["--teacher-graph"] if graph else []), env={"COSA_DIST_BACKEND": "gloo"})
        res[graph] = [torch.load(os.path.join(out, f"rank{r}.pt")) for r in (0, 1)]
        assert all(r["graph_captured"] == graph and r["world"] == 2 for r in res[graph])
    for net in ("student", "teacher"):
        for k in res[False][0][net]:
            assert torch.equal(res[False][0][net][k], res[True][0][net][k]) and torch.equal(res[True][0][net][k], res[True][1][net][k]), f"{net}.{k}"


def test_one_rank_over_rccl_with_the_captured_teacher(tmp_path):
    """the part of the multi-GPU path a one-GPU box CAN run on the real backend: `init_process_group("nccl", device_id=...)` (RCCL, its watchdog
    thread and comm stream), the teacher hipGraph captured under it and replayed on the side stream beside DDP's bucket all-reduces (a world
    of one: the collectives are RCCL's own single-rank path), six weight-gradient groups.  Finite loss, capture asserted by the tool, and the
    same weights as the run without a process group."""
    out = str(tmp_path)
    common = ["--out", out, "--steps", "4", "--crop", "64", "--batch", "2", "--n-iter", str(10 ** 6), "--teacher-graph", "--defer-groups", "6"]
    _run([sys.executable, os.path.join(ROOT, "tools", "ddp_check.py"), "--force-dist"] + common,
         env={"COSA_DIST_BACKEND": "nccl", "MASTER_PORT": str(_free_port()), "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"})
    r = torch.load(os.path.join(out, "rank0.pt"))
    assert r["backend"] == "nccl" and r["graph_captured"] and r["teacher_async"] and r["world"] == 1 and r["loss"] == r["loss"]
    _run([sys.executable, os.path.join(ROOT, "tools", "ddp_check.py"), "--single", "--ranks", "1"] + common)
    s = torch.load(os.path.join(out, "single.pt"))
    for net in ("student", "teacher"):
        for k in r[net]:
            assert torch.equal(r[net][k], s[net][k]), f"{net}.{k}: one rank over RCCL differs from the run without a process group"
