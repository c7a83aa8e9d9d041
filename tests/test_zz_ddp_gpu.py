"""Two data-parallel ranks on ONE GPU (gloo's CUDA-tensor collectives stand in for RCCL; everything above the transport is the product
path: bucketed overlapped all-reduce with finality regions, row-sparse word-embedding exchange, global loss normaliser): the two replicas
must stay identical and must follow the single-process run on the concatenated batch -- the reference's nn.DataParallel semantics."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = [pytest.mark.gpu, pytest.mark.transport]
SHAPES = (20, 100, 50, 12)
STEPS = 4


def _slice_batch(bd, lo, hi):
    out = {}
    for k, v in bd.items():
        if torch.is_tensor(v):
            out[k] = v[lo:hi].contiguous()
        elif isinstance(v, dict):
            out[k] = {kk: vv[lo:hi].contiguous() for kk, vv in v.items()}
        else:
            out[k] = v
    return out


def _global_batches():
    from sam_textvqa_amd.synthetic import make_batch
    out = []
    for i in range(2):
        bd = make_batch(8, *SHAPES, vocab=300, context=3, device="cpu", seed=70 + i)
        bd["question_indices"] = (bd["question_indices"] % 499 + 1) * bd["question_mask"]
        bd["train_loss_mask"][1, 6:] = 0          # unequal numbers of unmasked decoding steps on the two ranks
        bd["train_loss_mask"][5] = 0
        out.append(bd)
    return out


def _to_gpu(bd):
    return {k: (v.cuda() if torch.is_tensor(v) else {kk: vv.cuda() for kk, vv in v.items()} if isinstance(v, dict) else v) for k, v in bd.items()}


def _run(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      SAM_DIST_BACKEND="gloo", SAM_DIST_SHARE_GPU="1")
    from sam_textvqa_amd import parallel
    from sam_textvqa_amd.synthetic import clone_batch
    from sam_textvqa_amd.trainer import Trainer
    from tests.test_model_gpu import _small_full_model
    if world > 1:
        parallel.init_distributed()
    model, _ = _small_full_model(3, ("n", "s"), SHAPES)
    dense = os.environ.get("SAM_TEST_DENSE_REDUCER") == "1" and world > 1
    if dense:
        # a caller-built reducer WITHOUT the row-sparse table exchange and without overlap (what bench.py --no-overlap builds): the word table
        # is all-reduced densely, so the trainer must not walk it row-sparsely (rows touched only on the other rank would be skipped)
        from sam_textvqa_amd.params import prepare
        groups = model.get_optimizer_parameters(1e-3)
        flat = prepare(model, groups=[g["params"] for g in groups])
        tr = Trainer(model, base_lr=1e-3, seed=3, reducer=parallel.GradReducer(flat.grad, overlap=False))
        assert tr.sparse is None and not tr.reducer.overlap and tr.reducer.sparse_hi == tr.reducer.sparse_lo
    else:
        tr = Trainer(model, base_lr=1e-3, seed=3)
    assert (tr.reducer is not None) == (world > 1)
    if world > 1 and not dense:
        assert tr.sparse is not None
        assert tr.reducer.world_size == world and tr.reducer.overlap and tr.reducer.dense_lo > 0 and len(tr.reducer.regions) == 7
    losses = []
    per = 8 // world
    for step in range(STEPS):
        bd = _slice_batch(_global_batches()[step % 2], rank * per, (rank + 1) * per)
        losses.append(tr.step(_to_gpu(clone_batch(bd))).item())
    torch.cuda.synchronize()
    torch.save((rank, losses, tr.flat.flat.cpu(), tr.exp_avg_sq.cpu()), os.path.join(out_dir, "w%d_r%d.pt" % (world, rank)))
    if world > 1:
        parallel.dist.barrier()
        parallel.dist.destroy_process_group()


def _spawn(world, out_dir):
    """the ranks as spawned processes on a rendezvous port taken from the OS.  A start-up failure of the rendezvous (the port handed out again while a previous
    test's sockets are still closing: EADDRINUSE, seen once in round 6) is retried ONCE on another port; a second failure is the test's failure"""
    ctx = mp.get_context("spawn")
    for attempt in range(2):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        for r in range(world):
            f = os.path.join(str(out_dir), "w%d_r%d.pt" % (world, r))
            if os.path.exists(f):
                os.remove(f)
        procs = [ctx.Process(target=_run, args=(r, world, port, str(out_dir))) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(600)
        if all(p.exitcode == 0 for p in procs):
            break
        for p in procs:
            if p.is_alive():
                p.kill()
        assert attempt == 0, [p.exitcode for p in procs]
    return [torch.load(os.path.join(str(out_dir), "w%d_r%d.pt" % (world, r))) for r in range(world)]


def test_two_ranks_match_each_other_and_the_global_batch_run(tmp_path):
    (r0, l0, p0, v0), (r1, l1, p1, v1) = _spawn(2, tmp_path)
    (_, lg, pg, vg), = _spawn(1, tmp_path)
    # replicas: same reduced gradients (bit-identical out of the all-reduce), the row-sparse table summed in a fixed order from the same
    # gathered list, deterministic norm + optimizer -> the SAME parameters and optimizer state, bit for bit (nothing re-synchronises later)
    assert torch.equal(p0, p1) and torch.equal(v0, v1), ((p0 - p1).abs().max().item(), (v0 - v1).abs().max().item())
    # DataParallel semantics: sum of the ranks' (count-weighted) losses == loss of the concatenated batch, step by step
    for a, b, g in zip(l0, l1, lg):
        assert abs((a + b) - g) <= 2e-3 * abs(g), (l0, l1, lg)
    # ... and the same trajectory: total parameter update of rank 0 vs the single-process run
    from tests.test_model_gpu import _small_full_model
    from sam_textvqa_amd.trainer import Trainer
    init = None
    # reconstruct the common initial point: both runs start from _small_full_model(seed 0); use the single run's first-step-independent init
    model, _ = _small_full_model(3, ("n", "s"), SHAPES)
    tr = Trainer(model, base_lr=1e-3, seed=3)
    init = tr.flat.flat.cpu()
    u_dp, u_g = (p0 - init).double(), (pg - init).double()
    moved = u_g.abs() > 0
    cos = float(torch.dot(u_dp[moved], u_g[moved]) / (u_dp[moved].norm() * u_g[moved].norm()))
    rel = float((u_dp - u_g).norm() / u_g.norm())
    assert cos > 0.98 and rel < 0.2, (cos, rel)


def test_two_ranks_with_a_dense_reducer_keep_identical_replicas(tmp_path, monkeypatch):
    """a reducer that all-reduces the word-embedding table densely (no sparse_range, overlap off) with DIFFERENT question tokens
    on the two ranks.  The row-sparse Adam walk must switch itself off there: the replicas end bit-identical and follow the single-process run."""
    monkeypatch.setenv("SAM_TEST_DENSE_REDUCER", "1")
    (r0, l0, p0, v0), (r1, l1, p1, v1) = _spawn(2, tmp_path)
    monkeypatch.delenv("SAM_TEST_DENSE_REDUCER")
    (_, lg, pg, vg), = _spawn(1, tmp_path)
    assert torch.equal(p0, p1) and torch.equal(v0, v1), ((p0 - p1).abs().max().item(), (v0 - v1).abs().max().item())
    for a, b, g in zip(l0, l1, lg):
        assert abs((a + b) - g) <= 2e-3 * abs(g), (l0, l1, lg)
    # the optimizer state of the table rows: every row either rank touched has moved on BOTH ranks (second moments non-zero), exactly as in the global run
    from tests.test_model_gpu import _small_full_model
    from sam_textvqa_amd.trainer import Trainer
    model, _ = _small_full_model(3, ("n", "s"), SHAPES)
    tr = Trainer(model, base_lr=1e-3, seed=3)
    lo, hi, d, _ = tr.sparse
    live_dp = (v0[lo:hi].view(-1, d) != 0).any(1)
    live_g = (vg[lo:hi].view(-1, d) != 0).any(1)
    assert torch.equal(live_dp, live_g) and int(live_g.sum()) > 8


@pytest.mark.parametrize("payload", ["fp32", "bf16"])
def test_bench_under_torch_distributed_run_one_rank_with_reducer_check(payload):
    """the command the driver uses on a multi-GPU node -- `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N --steps K --warmup W` -- at N = 1 with the data-parallel machinery forced on (SAM_FORCE_DIST=1: RCCL
    communicator, bucketed all-reduce on the reducer stream, row-sparse table exchange, global loss count) and every bucket re-verified at
    finish() (SAM_REDUCER_CHECK=1).  The JSON line must carry the contract's fields and the exposed-communication figure."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def make(port):
        env = dict(os.environ, SAM_FORCE_DIST="1", SAM_REDUCER_CHECK="1", SAM_GRAD_PAYLOAD=payload, HSA_ENABLE_IPC_MODE_LEGACY="0")
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
        return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(port),
                os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--full", "--no-cpu-baseline", "--no-eager-baseline", "--no-roofline",
                "--no-secondary"], env
    r = _run_child_with_fresh_port(make, None, "bench_dist_run_one_rank_%s" % payload, timeout=900)
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in out, key
    assert out["n_gpus"] == 1 and out["steps"] == 4 and out["scaling"] == "weak" and out["value"] > 0
    assert "exposed_comm_ms" in out and out["exposed_comm_ms"] >= 0.0
    assert out.get("dp_transport") == "rccl-direct"
    # the JSON line is the LAST line of stdout (RCCL's version banner, buffered in C stdio since the communicator was built, is flushed in front of it)
    assert [l for l in r.stdout.splitlines() if l.strip()][-1].startswith("{"), r.stdout[-400:]


def test_bench_under_torch_distributed_run_two_ranks_on_one_gpu():
    """`bench.py --gpus N` with N > 1 must FINISH.  The driver's exact command at --nproc-per-node 2, both ranks on this box's one GPU
    (gloo's CUDA-tensor collectives stand in for RCCL, which refuses two ranks on one device; the step is therefore eager -- SAM_BENCH_EAGER_COMM_LEG=1 forces
    the exposed-communication leg that a captured step takes, the leg round 5 ran on rank 0 only).  The JSON line must appear, from rank 0, with n_gpus = 2,
    two ranks seen by the reducer's group, the global batch of both -- inside 300 s (a mismatched collective hangs for ever)."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def make(port):
        env = dict(os.environ, SAM_DIST_BACKEND="gloo", SAM_DIST_SHARE_GPU="1", SAM_BENCH_EAGER_COMM_LEG="1", HSA_ENABLE_IPC_MODE_LEGACY="0", SAM_DP_CU_RESERVE="32")
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SAM_FORCE_DIST", "SAM_REDUCER_CHECK"):
            env.pop(k, None)
        return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(port),
                os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2", "--full"], env
    r = _run_child_with_fresh_port(make, None, "bench_dist_run_two_ranks", timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines                      # rank 0 prints, rank 1 does not
    out = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in out, key
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["warmup"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    assert out["rccl_ranks_seen"] == 2 and out["config"]["global_batch"] == 128 and out["config"]["parallelism"] == "dp2"
    assert out["exposed_comm_ms"] >= 0.0 and "every rank" in out["exposed_comm_source"]
    assert out["dp_transport"] == "process-group" and out["step_mode"] == "eager launches"
    assert out["cu_reserved"] == 32          # SAM_DP_CU_RESERVE: under a reducer spanning > 1 rank the backward's persistent grids leave CUs to the collectives
    assert abs(out["value"] - 128 * 3 / (out["ms_per_step"] * 3e-3)) <= 0.02 * out["value"]


_GRAPH_DP_SCRIPT = r"""
import os, sys, torch
sys.path.insert(0, os.environ["SAM_REPO"])
from tests.test_model_gpu import _small_full_model
from sam_textvqa_amd import parallel
from sam_textvqa_amd.synthetic import clone_batch, make_batch
from sam_textvqa_amd.trainer import Trainer
os.environ["SAM_FORCE_DIST"] = "1"
parallel.init_distributed()                               # 1-rank RCCL group
res = []
for mode in ("dp_graph", "dp_eager", "plain_graph", "dp_graph_no_overlap"):
    os.environ["SAM_FORCE_DIST"] = "0" if mode == "plain_graph" else "1"
    model, _ = _small_full_model(3, ("n", "s"), (20, 100, 50, 12))
    tr = Trainer(model, base_lr=1e-3, seed=3, use_graph=mode != "dp_eager", overlap=mode != "dp_graph_no_overlap")
    assert (tr.reducer is not None) == (mode != "plain_graph")
    if mode != "plain_graph":
        assert tr.reducer.comm is not None            # collectives go straight to RCCL on the reducer's stream (no ProcessGroupNCCL Work objects)
    if mode.startswith("dp_graph"):
        assert tr._dp_capturable() and tr.reducer.overlap == (mode == "dp_graph")
    batch = make_batch(4, vocab=300, device="cuda", seed=21)
    batch["question_indices"] = batch["question_indices"] % 500
    losses = [tr.step(clone_batch(batch)).item() for _ in range(6)]
    if mode != "dp_eager":
        assert tr._graph is not None, "the step was not captured"
    if mode == "dp_graph":
        assert tr.reducer.late_buckets == 0 and all(tr.reducer.done)       # (state of the capture pass: every bucket left at a finality mark)
    tr.flush_update()                                                      # (captured steps leave their update pending)
    res.append((losses, tr.flat.flat.clone()))
torch.cuda.synchronize()
(lg, pg), (le, pe), (lp, pp), (ln, pn) = res
print("LOSSES", lg, le, lp, ln)
for other in (le, lp, ln):
    assert all(abs(a - b) <= 2e-3 * abs(b) for a, b in zip(lg, other)), (lg, other)
assert (pg - pe).abs().max().item() < 7e-3 and (pg - pp).abs().max().item() < 7e-3 and (pg - pn).abs().max().item() < 7e-3
print("GRAPH_DP_OK")
"""


def _run_child_with_fresh_port(make_cmd_env, marker, name, timeout=600, tries=3):
    """run_child with a rendezvous port taken from the OS; a port can be handed out twice in a row while a previous test's agent is still closing its sockets
    (EADDRINUSE at TCPStore creation, seen once in round 6): such a start-up failure is retried on another port, anything else fails as usual"""
    from tests.util import run_child
    last = None
    for _ in range(tries):
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        cmd, env = make_cmd_env(port)
        try:
            return run_child(cmd, env, marker, name, timeout=timeout)
        except AssertionError as e:
            last = e
            if "EADDRINUSE" not in str(e) and "address already in use" not in str(e):
                raise
    raise last


def test_data_parallel_step_is_captured_and_trains_like_the_plain_step():
    """ONE step for every N: with RCCL collectives the data-parallel step (count all-reduce, bucket all-reduces forked onto the reducer stream at
    their finality marks, row-sparse table exchange, join, clip, Adam) is captured into the same kind of hipGraph as the single-GPU step and
    replayed; it trains like the eager data-parallel step and like the plain captured step (1-rank group: the sums are identities)"""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def make(port):
        env = dict(os.environ, SAM_REPO=root, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.pop("SAM_REDUCER_CHECK", None)
        return [sys.executable, "-c", _GRAPH_DP_SCRIPT], env
    _run_child_with_fresh_port(make, "GRAPH_DP_OK", "graph_dp_step")
