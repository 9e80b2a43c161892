"""Convergence-gated refinement A/B on the GPU: what the gate costs and
what an early stop saves, against the fixed-count call.

  kernel  ops.flow_residual alone at the headline (55x128) and 1080p
          (135x240) 1/8 grids, planar and interleaved coords.
  gate    the worst case of gating: Convergence(tol=None) takes every
          check and never stops, so the call runs the whole budget plus
          budget/every checks (launch + copy + wait each). Against the
          fixed-count call of the same budget, every in {1, 4, 8}.
  stop    an early stop at equal n: Convergence(tol=1e9, every=4,
          min_iters=n-1) stops after n iterations; against the fixed
          iters=n call, eager loop and captured loop each against the
          same mode.

The fixed-count baseline is timed twice per round (fixed_a, fixed_b) so
its own run-to-run spread is known before a difference is judged.
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

from bench_bidir import alternate  # noqa: E402


def _stats(row, key, series, unit="ms", scale=1.0):
    row[f"{key}_{unit}"] = round(statistics.median(series) * scale, 3)
    row[f"{key}_min_{unit}"] = round(min(series) * scale, 3)
    row[f"{key}_max_{unit}"] = round(max(series) * scale, 3)


def _spread(a, b):
    """Baseline noise: the larger of the gap between the two series'
    medians and the median per-round gap."""
    per_round = [abs(x - y) for x, y in zip(a, b)]
    return max(abs(statistics.median(a) - statistics.median(b)),
               statistics.median(per_round))


def mode_kernel(args):
    import torch
    from raft_amd import ops
    torch.manual_seed(3)
    for name, (H, W) in (("headline", (55, 128)), ("1080p", (135, 240))):
        prev = (torch.rand(1, 2, H, W) * 20.0).cuda()
        nxt = prev + torch.randn(1, 2, H, W).cuda() * 0.3
        iprev, inxt = (t.permute(0, 2, 3, 1).contiguous()
                       .permute(0, 3, 1, 2) for t in (prev, nxt))
        series = alternate(
            [("planar", lambda: ops.flow_residual_raw(prev, nxt, 0.01)),
             ("interleaved",
              lambda: ops.flow_residual_raw(iprev, inxt, 0.01))],
            reps=200, rounds=args.rounds)
        row = {"bench": "kernel", "shape": name, "grid": [H, W]}
        for k, v in series.items():
            _stats(row, k, v, "us", 1e3)
        print(json.dumps(row), flush=True)


def _engine(args):
    import torch
    from raft_amd import RAFT, RaftConfig
    from raft_amd.engine.inference import InferenceEngine
    torch.manual_seed(0)
    dev = torch.device("cuda")
    model = RAFT(RaftConfig(small=False)).to(dev).eval()
    eng = InferenceEngine(model, dtype=torch.bfloat16)
    H, W = args.size
    x1, x2 = (torch.rand(1, 3, H, W, device=dev) for _ in range(2))
    return eng, x1, x2


def mode_gate(args):
    from raft_amd import Convergence
    eng, x1, x2 = _engine(args)
    N = args.budget
    eng.loop_graph = args.graph

    def fixed():
        eng(x1, x2, iters=N)

    variants = [("fixed_a", fixed)]
    for every in (1, 4, 8):
        conv = Convergence(tol=None, every=every)
        variants.append((f"every{every}",
                         lambda c=conv: eng(x1, x2, iters=N, converge=c)))
    variants.append(("fixed_b", fixed))
    series = alternate(variants, reps=args.reps, rounds=args.rounds)
    both = series["fixed_a"] + series["fixed_b"]
    base = statistics.median(both)
    row = {"bench": "gate", "size": list(args.size), "budget": N,
           "loop_graph": args.graph, "rounds": args.rounds,
           "reps": args.reps,
           "baseline_spread_ms": round(_spread(series["fixed_a"],
                                               series["fixed_b"]), 3)}
    _stats(row, "fixed", both)
    for every in (1, 4, 8):
        k = f"every{every}"
        checks = len([i for i in range(1, N) if i % every == 0])
        _stats(row, k, series[k])
        row[k + "_checks"] = checks
        row[k + "_us_per_check"] = round(
            (statistics.median(series[k]) - base) * 1e3 / max(checks, 1), 2)
    print(json.dumps(row), flush=True)


def mode_stop(args):
    from raft_amd import Convergence
    eng, x1, x2 = _engine(args)
    N = args.budget
    for n in args.stops:
        if not 2 <= n <= N or (n - 1) % 4:
            raise SystemExit(f"stop {n}: need n = 4k+1 within the budget")
        conv = Convergence(tol=1e9, every=4, min_iters=n - 1)

        def call(graph, gated):
            eng.loop_graph = graph
            if gated:
                eng(x1, x2, iters=N, converge=conv)
                assert eng.last_info.iters_run == n
            else:
                eng(x1, x2, iters=n)

        series = alternate(
            [("eager_fixed_a", lambda: call(False, False)),
             ("eager_gated", lambda: call(False, True)),
             ("graph_fixed_a", lambda: call(True, False)),
             ("graph_gated", lambda: call(True, True)),
             ("eager_fixed_b", lambda: call(False, False)),
             ("graph_fixed_b", lambda: call(True, False))],
            reps=args.reps, rounds=args.rounds)
        row = {"bench": "stop", "size": list(args.size), "budget": N,
               "n": n, "checks": 1,
               "rounds": args.rounds, "reps": args.reps}
        for mode in ("eager", "graph"):
            a, b = series[mode + "_fixed_a"], series[mode + "_fixed_b"]
            _stats(row, mode + "_fixed", a + b)
            row[mode + "_spread_ms"] = round(_spread(a, b), 3)
            _stats(row, mode + "_gated", series[mode + "_gated"])
            row[mode + "_gated_minus_fixed_ms"] = round(
                statistics.median(series[mode + "_gated"])
                - statistics.median(a + b), 3)
        row["gated_graph_minus_gated_eager_ms"] = round(
            statistics.median(series["graph_gated"])
            - statistics.median(series["eager_gated"]), 3)
        print(json.dumps(row), flush=True)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("mode", choices=["kernel", "gate", "stop"])
    p.add_argument("--rounds", type=int, default=7)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--budget", type=int, default=32)
    p.add_argument("--graph", action="store_true",
                   help="gate mode: force the captured loop (default: the "
                        "eager loop)")
    p.add_argument("--stops", default=[5, 9, 17],
                   type=lambda s: [int(v) for v in s.split(",")])
    p.add_argument("--size", default="436x1024",
                   type=lambda s: tuple(int(v) for v in s.split("x")))
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_adaptive needs a GPU (no CPU fallback)")
    {"kernel": mode_kernel, "gate": mode_gate,
     "stop": mode_stop}[args.mode](args)


if __name__ == "__main__":
    main()
