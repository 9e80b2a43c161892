"""Multi-process DP tests on gloo (world_size 2, CPU) — the distributed
path must be correct by construction before it ever touches RCCL/xGMI."""
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.filterwarnings("ignore")


def _run_ddp_equivalence(rank, world, port, results):
    os.environ.update({
        "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
        "RANK": str(rank), "WORLD_SIZE": str(world),
    })
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(100 + rank)  # different init per rank: broadcast must fix
    from raft_amd import RAFT, RaftConfig
    from raft_amd.parallel.ddp import BucketedDDP
    from raft_amd.engine.trainer import sequence_loss

    model = RAFT(RaftConfig(small=True))
    ddp = BucketedDDP(model, bucket_cap_mb=0.5)   # force several buckets

    # deterministic shard: rank r sees sample r of a fixed global batch
    g = torch.Generator().manual_seed(42)
    x1 = torch.rand(world, 3, 64, 96, generator=g)
    x2 = torch.rand(world, 3, 64, 96, generator=g)
    gt = torch.randn(world, 2, 64, 96, generator=g)

    preds = ddp(x1[rank:rank + 1], x2[rank:rank + 1], iters=2,
                test_mode=False)
    loss = sequence_loss(preds, gt[rank:rank + 1])
    loss.backward()
    ddp.finish_gradient_sync()

    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    if rank == 0:
        # single-process reference on the full global batch
        torch.manual_seed(100)  # rank-0 init == broadcast init
        ref = RAFT(RaftConfig(small=True))
        ref_preds = ref(x1, x2, iters=2, test_mode=False)
        # mean over the global batch == average of per-rank means here
        ref_loss = sequence_loss(ref_preds, gt)
        ref_loss.backward()
        worst = 0.0
        for (n, p) in ref.named_parameters():
            d = (grads[n] - p.grad).abs().max().item()
            worst = max(worst, d)
        results[0] = worst
    dist.barrier()
    dist.destroy_process_group()


def test_ddp_grad_equivalence():
    """DP=2 averaged grads == single-process batch-2 grads (within fp tol)."""
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        results = mgr.dict()
        port = 29611
        procs = [ctx.Process(target=_run_ddp_equivalence,
                             args=(r, 2, port, results)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
        assert results[0] < 5e-5, f"grad mismatch {results[0]}"


def _run_bench_train(rank, world, port):
    os.environ.update({
        "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port),
        "RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
    })
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from raft_amd import RAFT, RaftConfig
    from raft_amd.engine.trainer import Trainer, TrainConfig

    cfg = TrainConfig(num_steps=2, iters=2, batch=1, height=64, width=96)
    tr = Trainer(RAFT(RaftConfig(small=True)), cfg)
    for _ in range(2):
        x1 = torch.rand(1, 3, 64, 96)
        x2 = torch.rand(1, 3, 64, 96)
        gt = torch.randn(1, 2, 64, 96)
        stats = tr.step(x1, x2, gt)
        assert all(v == v for v in stats.values())  # finite
    dist.barrier()
    dist.destroy_process_group()


def test_trainer_distributed_steps():
    """Two gloo ranks step the Trainer on CPU. The spawned ranks inherit
    an environment with no visible GPU: this is the CPU path's test, and
    two ranks must not both land on device 0 of a one-GPU machine."""
    ctx = mp.get_context("spawn")
    port = 29613
    procs = [ctx.Process(target=_run_bench_train, args=(r, 2, port))
             for r in range(2)]
    hide = ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES")
    saved = {k: os.environ.get(k) for k in hide}
    os.environ.update({k: "" for k in hide})
    try:
        for p in procs:
            p.start()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for p in procs:
        p.join(300)
        assert p.exitcode == 0


def _run_graceful_stop(rank, world, port, results):
    import signal
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from raft_amd.engine.trainer import GracefulStop
        g = GracefulStop()
        if rank == 1:                      # signal reaches ONE rank only
            os.kill(os.getpid(), signal.SIGTERM)
        # both ranks must agree to stop (MAX-reduced flag)
        results[rank] = g.should_stop(distributed=True)
        g.restore()
    finally:
        dist.destroy_process_group()


def test_graceful_stop_rank_consistent():
    """A preemption signal delivered to a single rank stops every rank
    on the same step (no hanging collectives)."""
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        results = mgr.dict()
        port = 29627
        procs = [ctx.Process(target=_run_graceful_stop,
                             args=(r, 2, port, results)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
        assert results[0] is True and results[1] is True


def _run_mixed_dtype_ddp(rank, world, port, results):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from raft_amd.parallel.ddp import BucketedDDP
        torch.manual_seed(7 + rank)
        m = torch.nn.Sequential(torch.nn.Linear(8, 8),
                                torch.nn.Linear(8, 4))
        m[1] = m[1].to(torch.bfloat16)          # mixed-dtype module
        ddp = BucketedDDP(m)
        x = torch.randn(4, 8)
        # forward manually (a cast between the mixed-dtype layers)
        h = ddp.module[0](x)
        y = ddp.module[1](h.to(torch.bfloat16)).float().sum()
        y.backward()
        ddp.finish_gradient_sync()
        # every param has a grad of its own dtype after sync
        ok = all(p.grad is not None and p.grad.dtype == p.dtype
                 for p in m.parameters())
        results[rank] = bool(ok)
    finally:
        dist.destroy_process_group()


def test_ddp_mixed_dtype_buckets():
    """Buckets are partitioned by dtype — a bf16 submodule must not have
    its gradients cast through an fp32 flat buffer (or vice versa)."""
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        results = mgr.dict()
        port = 29631
        procs = [ctx.Process(target=_run_mixed_dtype_ddp,
                             args=(r, 2, port, results)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
        assert results[0] and results[1]


def _run_no_sync_accum(rank, world, port, results):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from raft_amd.parallel.ddp import BucketedDDP
        torch.manual_seed(3 + rank)
        m = torch.nn.Linear(6, 3)
        ddp = BucketedDDP(m)
        xs = [torch.randn(4, 6, generator=torch.Generator().manual_seed(
            100 * rank + i)) for i in range(3)]
        # micro-batches 0,1 under no_sync; 2 synced
        with ddp.no_sync():
            for x in xs[:2]:
                ddp(x).sum().backward()
        ddp(xs[2]).sum().backward()
        ddp.finish_gradient_sync()
        g = m.weight.grad.clone()
        # reference: average over ranks of the summed 3-micro-batch grads
        m2 = torch.nn.Linear(6, 3)
        with torch.no_grad():
            m2.weight.copy_(m.weight)
            m2.bias.copy_(m.bias)
        for x in xs:
            m2(x).sum().backward()
        ref = m2.weight.grad.clone()
        dist.all_reduce(ref)
        ref /= world
        results[rank] = float((g - ref).abs().max())
    finally:
        dist.destroy_process_group()


def test_ddp_no_sync_accumulation():
    """Micro-batch accumulation under no_sync(): gradients from all
    micro-batches are summed locally and reduced once — equal to the
    rank-averaged full sum."""
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        results = mgr.dict()
        port = 29637
        procs = [ctx.Process(target=_run_no_sync_accum,
                             args=(r, 2, port, results)) for r in range(2)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
            assert p.exitcode == 0
        assert results[0] < 1e-6 and results[1] < 1e-6, dict(results)
