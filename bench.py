#!/usr/bin/env python3
"""Flagship benchmark — BASELINE.json headline config.

Measures frames/sec (whole node) for raft-things inference at 2x436x1024,
bf16, 32 iters (BASELINE config 2) on N GPUs of one node (weak scaling: one
frame-pair stream per rank, synthetic data, random-init weights).

  python bench.py --gpus N --steps K --warmup W
  # N>1 is launched by the driver via torch.distributed.run (one rank/GPU,
  # RCCL over xGMI); rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the result
line. --dump-outputs DIR also writes what the last timed step returned
(the flow field; loss/epe/lr for --train) as DIR/<name>.npy, so two builds
can be compared output for output: model weights and inputs are seeded and
identical from run to run. --full is where anything beyond the headline
figure belongs; nothing does at present.

Extra modes (not used by the driver contract): --train benches the DP
training step (config 3 shape), --small / --height/--width/--iters override
the model/config.
"""
import argparse
import json
import os
import sys
import time

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=16)
    p.add_argument("--warmup", type=int, default=4)
    p.add_argument("--batch", type=int, default=1, help="per-rank batch")
    p.add_argument("--height", type=int, default=436)
    p.add_argument("--width", type=int, default=1024)
    p.add_argument("--iters", type=int, default=32)
    p.add_argument("--small", action="store_true")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--train", action="store_true",
                   help="bench the training step (config 3) instead")
    p.add_argument("--no-graph", action="store_true",
                   help="disable hipGraph capture of the inference step")
    p.add_argument("--trace", default=None,
                   help="write a chrome trace of a few steps to this path")
    p.add_argument("--trace-table", action="store_true",
                   help="print a torch-profiler op table of 3 steps to "
                        "stderr (works for --train too)")
    p.add_argument("--dump-outputs", default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step returned as DIR/<name>.npy (rank 0)")
    p.add_argument("--full", action="store_true",
                   help="also run the benchmark's secondary sections; a "
                        "plain run only times the headline steps (there "
                        "are no secondary sections at present)")
    return p.parse_args()


DUMP_BUDGET_BYTES = 64 * 1000 * 1000


def _named_outputs(out, train):
    """The last timed step's return value as {name: float ndarray}."""
    import numpy as np
    if isinstance(out, torch.Tensor):
        out = {"loss" if train else "flow": out}
    elif isinstance(out, (list, tuple)):
        out = {f"out{i}": v for i, v in enumerate(out)}
    arrays = {}
    for name, v in out.items():
        if isinstance(v, torch.Tensor):
            v = v.detach()
            v = v.to("cpu", torch.float64 if v.dtype == torch.float64
                     else torch.float32).numpy()
        a = np.asarray(v)
        if a.dtype != np.float64:
            a = a.astype(np.float32)
        arrays[name] = a
    return arrays


def dump_outputs(out, path, train=False):
    """Write the step's outputs as <path>/<name>.npy (float32/float64),
    at most DUMP_BUDGET_BYTES in all: an array over its share of the
    budget is stored as a fixed seeded sample of its flattened elements
    (the same positions every run, in ascending order)."""
    import numpy as np
    arrays = _named_outputs(out, train)
    os.makedirs(path, exist_ok=True)
    share = DUMP_BUDGET_BYTES // max(1, len(arrays))
    for name, a in arrays.items():
        if a.nbytes > share:
            rng = np.random.default_rng(0)
            idx = np.sort(rng.integers(0, a.size, share // a.itemsize))
            a = a.reshape(-1)[idx]
        np.save(os.path.join(path, f"{name}.npy"), a)


def pad8(x):
    import torch.nn.functional as F
    h, w = x.shape[-2:]
    ph = (-h) % 8
    pw = (-w) % 8
    if ph or pw:
        x = F.pad(x, (0, pw, 0, ph))
    return x


def _self_spawn(args):
    """`python bench.py --gpus N` without torchrun: spawn the ranks
    ourselves via torch.distributed.run (one rank per GPU over RCCL).
    Previously --gpus was silently ignored outside torchrun (r1 verdict).
    A rendezvous-port collision (concurrent jobs) retries on a fresh
    port."""
    import subprocess
    for attempt in range(3):
        port = str(20000 + (os.getpid() * 7 + attempt * 1009 +
                            int(time.time())) % 20000)
        cmd = [sys.executable, "-m", "torch.distributed.run",
               "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", port,
               os.path.abspath(__file__)] + sys.argv[1:]
        rc = subprocess.call(cmd)
        if rc == 0:
            return 0
        print(f"bench.py: spawn attempt {attempt} rc={rc} (port {port})",
              file=sys.stderr)
    return rc


def main():
    args = parse_args()
    if args.steps < 1:
        raise SystemExit("bench.py: --steps must be >= 1")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus > 1 and world == 1:
        return _self_spawn(args)
    if world > 1 and args.gpus > 1 and args.gpus != world:
        print(f"bench.py: --gpus {args.gpus} != WORLD_SIZE {world}; "
              f"using WORLD_SIZE", file=sys.stderr)
    have_gpu = torch.cuda.is_available()
    n_dev = torch.cuda.device_count() if have_gpu else 0
    if have_gpu and world > n_dev:
        # RCCL-validation mode: more ranks than GPUs (e.g. world=2 on a
        # 1-GPU box) oversubscribes devices round-robin. Reported n_gpus
        # stays the world size; config carries the physical count.
        local_rank = local_rank % n_dev
    dist = None
    if world > 1:
        # N ranks share one node's cores: unbounded intra-op threads make
        # the per-rank CPU side (launches, dataflow) thrash at world=8
        torch.set_num_threads(max(1, (os.cpu_count() or world) // world))
        import torch.distributed as dist_mod
        dist = dist_mod
        dist.init_process_group(backend="nccl" if have_gpu else "gloo")
        if have_gpu:
            torch.cuda.set_device(local_rank)

    from raft_amd import RAFT, RaftConfig

    if not have_gpu:
        # CPU fallback: plumbing config (BASELINE config 1) so the script
        # terminates; the driver runs the real bench on an MI355X.
        args.small, args.height, args.width = True, 128, 256
        args.iters, args.dtype = 12, "fp32"

    dev = torch.device(f"cuda:{local_rank}" if have_gpu else "cpu")
    if have_gpu:
        torch.backends.cudnn.benchmark = True
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32

    torch.manual_seed(1234 + rank)
    model = RAFT(RaftConfig(small=args.small)).to(dev)
    if not args.train:
        model = model.eval().to(dtype)

    H, W = args.height, args.width
    x1 = pad8(torch.rand(args.batch, 3, H, W)).to(dev, dtype)
    x2 = pad8(torch.rand(args.batch, 3, H, W)).to(dev, dtype)

    if args.train:
        run_step, teardown = _make_train_step(model, args, dev, dist)
    else:
        run_step, teardown = _make_infer_step(model, x1, x2, args)

    def sync():
        if dist is not None:
            dist.barrier()
        if have_gpu:
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        run_step()
    sync()
    if (args.trace or args.trace_table) and rank == 0:
        from torch.profiler import profile, ProfilerActivity
        shapes = os.environ.get("RAFT_AMD_TRACE_SHAPES", "0") == "1"
        with profile(activities=[ProfilerActivity.CPU,
                                 ProfilerActivity.CUDA],
                     record_shapes=shapes) as prof:
            for _ in range(3):
                run_step()
            sync()
        if args.trace:
            prof.export_chrome_trace(args.trace)
            print(f"trace written to {args.trace}", file=sys.stderr)
        if args.trace_table:
            ka = prof.key_averages(group_by_input_shape=shapes)
            print(ka.table(sort_by="self_cuda_time_total",
                           row_limit=60, max_shapes_column_width=60),
                  file=sys.stderr)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = run_step()
    sync()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:
        dump_outputs(out, args.dump_outputs, train=args.train)

    if dist is not None:
        t = torch.tensor([elapsed], device=dev if have_gpu else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    frames = args.steps * args.batch * world
    fps = frames / elapsed
    if rank == 0:
        model_name = "raft-small" if args.small else "raft-things"
        mode = "training" if args.train else "inference"
        result = {
            "metric": f"frames/sec (whole node), {model_name} "
                      f"2x{args.height}x{args.width}, {args.iters} iters, "
                      f"{mode}",
            "value": fps,
            "unit": "frames/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": 1e3 * elapsed / args.steps,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,   # reference publishes no numbers
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "model": model_name,
                "global_batch": args.batch * world,
                "height": args.height,
                "width": args.width,
                "iters": args.iters,
                "parallelism": f"dp{world}",
                "device": "cpu-fallback" if not have_gpu else "mi355x",
            },
        }
        if have_gpu and world > n_dev:
            result["config"]["physical_gpus"] = n_dev
            result["config"]["oversubscribed"] = True
        print(json.dumps(result), flush=True)
    teardown()
    if dist is not None:
        dist.destroy_process_group()


def _make_infer_step(model, x1, x2, args):
    iters = args.iters
    if torch.cuda.is_available():
        from raft_amd.engine.inference import InferenceEngine
        engine = InferenceEngine(model, iters=iters, dtype=x1.dtype,
                                 use_graph=not args.no_graph,
                                 loop_graph=False if args.no_graph
                                 else None)   # None = env/auto policy

        def step():
            return engine(x1, x2)

        return step, lambda: None

    def step():
        with torch.no_grad():
            out = model(x1, x2, iters=iters)
        return out

    return step, lambda: None


def _make_train_step(model, args, dev, dist):
    """Config 3: training step via the Trainer (sequence loss, AdamW, AMP
    bf16 autocast, channels-last, DP bucketed all-reduce when world>1)."""
    from raft_amd.engine.trainer import Trainer, TrainConfig
    # config-3 defaults when the inference defaults were left untouched;
    # write the effective values back so the JSON line reports them
    H = args.height = args.height if args.height != 436 else 368
    W = args.width = args.width if args.width != 1024 else 768
    b = args.batch = args.batch if args.batch > 1 else 2
    iters = args.iters = args.iters if args.iters != 32 else 12
    cfg = TrainConfig(num_steps=args.steps + args.warmup + 2, iters=iters,
                      batch=b, height=H, width=W,
                      amp=args.dtype == "bf16")
    tr = Trainer(model, cfg, device=dev)
    x1 = torch.rand(b, 3, H, W, device=dev)
    x2 = torch.rand(b, 3, H, W, device=dev)
    gt = torch.randn(b, 2, H, W, device=dev)

    def step():
        return tr.step(x1, x2, gt)

    return step, lambda: None


if __name__ == "__main__":
    sys.exit(main())
