"""GPU: the data-parallel step (distributed.apply_gradient_allreduce on the HIP TRUNet) with 2 ranks sharing the
single GPU of the test box over gloo (RCCL needs one GPU per rank; the collective semantics are the same)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _worker(rank, world, port, q, precision):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from oracle import network_ref as nr, weights as W
    from tinyrecurrentunet_amd import distributed as td, network as hn
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    # rank-dependent initial weights: the start-up broadcast must make them rank 0's
    sd = W.fill_state_dict(nr.TRUNet(input_size=4), seed=10 + rank).state_dict()
    net = hn.TRUNet(input_size=4, precision=precision)
    net.load_state_dict(sd)
    net.cuda().train()
    td.apply_gradient_allreduce(net)
    xs = [torch.tensor(np.random.default_rng(50 + r).standard_normal((40, 4, 257)) * 0.5, dtype=torch.float32).cuda()
          for r in range(world)]
    cot = torch.tensor(np.random.default_rng(60).standard_normal((40, 8, 257)), dtype=torch.float32).cuda()
    y = net(xs[rank])
    (y * cot).sum().backward()
    torch.cuda.synchronize()
    got = torch.cat([p.grad.reshape(-1) for n, p in net.named_parameters() if p.grad is not None]).cpu()
    tgru_none = all(p.grad is None for n, p in net.named_parameters() if n.startswith("TGRU"))
    # expected: mean over ranks of the local gradients from rank 0's weights (BatchNorm statistics stay per rank)
    exp = 0
    for r in range(world):
        ref = hn.TRUNet(input_size=4, precision=precision)
        ref.load_state_dict(W.fill_state_dict(nr.TRUNet(input_size=4), seed=10).state_dict())
        ref.cuda().train()
        yy = ref(xs[r])
        (yy * cot).sum().backward()
        exp = exp + torch.cat([p.grad.reshape(-1) for n, p in ref.named_parameters() if p.grad is not None]).cpu()
    exp = exp / world
    q.put((rank, float((got - exp).norm() / exp.norm()), got.numel(), tgru_none))
    dist.destroy_process_group()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_rank_dp_step_matches_mean_of_local_gradients(precision):
    """fp32, and the bf16 engine of BASELINE.json configs[2] (its parameter gradients are the same flat fp32 tensor, so the
    all-reduce path is shared; the step is deterministic, so the mean of the local gradients is reproduced exactly)"""
    import socket
    world = 2
    with socket.socket() as sk:            # a port that is free right now (a fixed one can be in TIME_WAIT)
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q, precision)) for r in range(world)]
    [p.start() for p in ps]
    try:
        res = [q.get(timeout=300) for _ in range(world)]
    finally:
        [p.join(60) for p in ps]
        codes = [p.exitcode for p in ps]
        [p.kill() for p in ps if p.is_alive()]
    assert all(c == 0 for c in codes), codes
    for rank, err, n, tgru_none in res:
        assert n == 298592 and tgru_none
        assert err < 1e-5, (rank, err)


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bench_two_ranks_complete_without_deadlock(dtype):
    """bench.py under torch.distributed.run with 2 ranks (both on cuda:0, gloo instead of RCCL: this box has one GPU).
    Guards the control flow of the multi-GPU benchmark: every rank must take part in every step that contains the
    gradient all-reduce, including the instrumented one after the timed region (--full)."""
    import json
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ, TRUNET_BENCH_ONE_DEVICE="1", TRUNET_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2",
           "--warmup", "1", "--batch", "4", "--seconds", "1", "--dtype", dtype, "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["n_gpus"] == 2 and res["config"]["global_batch"] == 8 and res["value"] > 0
    assert res["roofline"] is not None and res["cpu_baseline"] is None and res["dtype"] == dtype


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_bare_bench_gpus_2_starts_its_own_ranks(dtype):
    """`python bench.py --gpus 2` with NO launcher (how the driver calls the benchmark): the parent starts the two ranks
    itself (reference: distributed.py:150-176), relays one JSON line and reports what torch.distributed saw.  Both ranks
    share cuda:0 over gloo here (one GPU per box); on a node the same code path runs RCCL with one GPU per rank."""
    import json
    import subprocess
    env = dict(os.environ, TRUNET_BENCH_ONE_DEVICE="1", TRUNET_BENCH_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "4",
           "--seconds", "1", "--dtype", dtype, "--full"]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    res = json.loads(lines[0])
    assert res["n_gpus"] == 2 and res["config"]["global_batch"] == 8 and res["value"] > 0 and res["dtype"] == dtype
    d = res["dist"]
    assert d["world_size_seen"] == 2 and d["dist_backend"] == "gloo" and d["self_spawned"] is True
    assert d["ms_per_step_rank_min"] <= d["ms_per_step_rank_max"] and len(d["device_of_rank"]) == 2
    assert d["allreduce_ms"] is not None and d["allreduce_ms"] > 0 and d["allreduce_in_place"] is True
    assert d["allreduce_bytes"] == 4 * 298592
