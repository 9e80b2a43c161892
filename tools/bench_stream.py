"""Streaming A/B on the GPU: what a video session costs per frame against
the pairwise call it replaces.

  e2e     per-frame time over a ring of frames at bf16, batch 1:
            pairwise   engine(prev, cur) (engine.bidirectional with
                       --bidirectional: flows + masks, as the session
                       returns)
            cold       session.push, warm=False — the encoder reuse alone
            warm       session.push, warm=True — plus one forward_project
                       call per direction (a memset and two kernels each)
          The pairwise baseline is timed twice per round so its own
          run-to-run spread is known before a difference is judged.
  kernel  ops.forward_project alone at the headline (55x128) and config-4
          (135x240) 1/8 grids.

Device-event timing, every variant warmed up, variants alternated in one
process (tools/bench_bidir.py's timed / alternate). Prints one JSON line
per measurement; needs a GPU (no fallback). Run each mode as its own
process.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_bidir import alternate, timed  # noqa: E402,F401


def mode_kernel(args):
    import torch
    import torch.nn.functional as F
    from raft_amd import ops
    torch.manual_seed(3)
    for name, (H, W) in (("headline", (55, 128)), ("config4", (135, 240))):
        flow = F.interpolate(torch.randn(1, 2, 4, 5) * 4.0, size=(H, W),
                             mode="bilinear", align_corners=True) \
            .contiguous().cuda()
        series = alternate(
            [("fw", lambda: ops.forward_project(flow, 1)),
             ("bw", lambda: ops.forward_project(flow, -1))],
            reps=200, rounds=args.rounds)
        holes = ops.forward_project(flow, 1)[1].float().mean().item()
        row = {"bench": "kernel", "shape": name, "grid": [H, W],
               "hole_share": round(holes, 4)}
        for k, v in series.items():
            row[k + "_us"] = round(statistics.median(v) * 1e3, 2)
            row[k + "_min_us"] = round(min(v) * 1e3, 2)
            row[k + "_max_us"] = round(max(v) * 1e3, 2)
        print(json.dumps(row), flush=True)


def mode_e2e(args):
    import torch
    from raft_amd import RAFT, RaftConfig
    from raft_amd.engine.inference import InferenceEngine
    torch.manual_seed(0)
    dev = torch.device("cuda")
    model = RAFT(RaftConfig(small=False)).to(dev).eval()
    eng = InferenceEngine(model, iters=args.iters, dtype=torch.bfloat16)
    H, W = args.size
    bidir = args.bidirectional
    ring = [torch.rand(1, 3, H, W, device=dev) for _ in range(4)]
    pos = {"pair": 0, "cold": 0, "warm": 0}

    def nxt(key):
        pos[key] = (pos[key] + 1) % len(ring)
        return ring[pos[key] - 1], ring[pos[key]]

    def pairwise():
        prev, cur = nxt("pair")
        if bidir:
            eng.bidirectional(prev, cur)
        else:
            eng(prev, cur)

    cold = eng.stream(warm=False, bidirectional=bidir)
    warm = eng.stream(warm=True, bidirectional=bidir)
    cold.push(ring[0])
    warm.push(ring[0])

    series = alternate(
        [("pairwise_a", pairwise),
         ("cold", lambda: cold.push(nxt("cold")[1])),
         ("warm", lambda: warm.push(nxt("warm")[1])),
         ("pairwise_b", pairwise)], reps=args.reps, rounds=args.rounds)
    med = {k: statistics.median(v) for k, v in series.items()}
    both = series["pairwise_a"] + series["pairwise_b"]
    base = statistics.median(both)
    per_round = [abs(a - b) for a, b in zip(series["pairwise_a"],
                                            series["pairwise_b"])]
    spread = max(abs(med["pairwise_a"] - med["pairwise_b"]),
                 statistics.median(per_round))
    row = {"bench": "e2e", "size": [H, W], "iters": args.iters,
           "dtype": "bf16", "batch": 1, "bidirectional": bidir,
           "rounds": args.rounds, "reps": args.reps,
           "pairwise_a_ms": round(med["pairwise_a"], 3),
           "pairwise_b_ms": round(med["pairwise_b"], 3),
           "pairwise_ms": round(base, 3),
           "pairwise_min_ms": round(min(both), 3),
           "pairwise_max_ms": round(max(both), 3),
           "baseline_spread_ms": round(spread, 3)}
    for k in ("cold", "warm"):
        row[k + "_ms"] = round(med[k], 3)
        row[k + "_min_ms"] = round(min(series[k]), 3)
        row[k + "_max_ms"] = round(max(series[k]), 3)
    row["cold_over_pairwise"] = round(med["cold"] / base, 4)
    row["cold_not_slower_beyond_spread"] = bool(
        med["cold"] - base <= spread)
    row["cold_faster_beyond_spread"] = bool(base - med["cold"] > spread)
    row["warm_minus_cold_ms"] = round(med["warm"] - med["cold"], 3)
    print(json.dumps(row), flush=True)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("mode", choices=["kernel", "e2e"])
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--iters", type=int, default=32)
    p.add_argument("--bidirectional", action="store_true")
    p.add_argument("--size", default="436x1024",
                   type=lambda s: tuple(int(v) for v in s.split("x")))
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream needs a GPU (no CPU fallback)")
    {"kernel": mode_kernel, "e2e": mode_e2e}[args.mode](args)


if __name__ == "__main__":
    main()
