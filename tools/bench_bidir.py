"""Bidirectional A/B on the GPU: what the shared pass costs against two
unidirectional calls.

  kernel  corr_volume_nhwc_bidir vs two corr_volume_nhwc calls with swapped
          operands (and vs one call), at the headline (55x128 queries) and
          config-4 (135x240) volumes, C=256; reports bytes written / time.
  e2e     engine(im1, im2, bidirectional=True) vs engine(im1, im2) followed
          by engine(im2, im1) at 436x1024, bf16, 32 iters, batch 1. The
          two-call baseline is timed twice per round so its own run-to-run
          spread is known before the difference is judged.

Device-event timing, every timed shape warmed up, variants alternated in
one process. Prints one JSON line per measurement; needs a GPU (no
fallback). Run each mode as its own process.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    """Milliseconds per call between two device events."""
    import torch
    start = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(reps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / reps


def alternate(variants, reps, rounds, warmup=3):
    """variants: list of (name, fn). Returns {name: [ms per round]}."""
    for _, fn in variants:
        for _ in range(warmup):
            fn()
    series = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            series[name].append(timed(fn, reps))
    return series


def mode_kernel(args):
    import torch
    from raft_amd.ops import require_hip
    hip = require_hip()
    torch.manual_seed(3)
    for name, (B, H, W, C) in (("headline", (1, 55, 128, 256)),
                               ("config4", (1, 135, 240, 256))):
        f1 = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
        f2 = torch.randn(B, H, W, C, device="cuda").to(torch.bfloat16)
        M = H * W
        one_vol = B * M * M * 2            # bytes of one bf16 volume

        def two():
            hip.corr_volume_nhwc(f1, f2, True)
            hip.corr_volume_nhwc(f2, f1, True)

        series = alternate(
            [("bidir", lambda: hip.corr_volume_nhwc_bidir(f1, f2)),
             ("two_calls", two),
             ("one_call", lambda: hip.corr_volume_nhwc(f1, f2, True))],
            reps=30 if H < 100 else 8, rounds=args.rounds)
        # outputs must not change: same bits as the two-call path
        out = hip.corr_volume_nhwc_bidir(f1, f2)
        assert torch.equal(out[:B], hip.corr_volume_nhwc(f1, f2, True))
        assert torch.equal(out[B:].view(B, M, M),
                           out[:B].view(B, M, M).transpose(1, 2))
        del out
        row = {"bench": "kernel", "shape": name, "M": M, "C": C}
        for k, written in (("bidir", 2 * one_vol), ("two_calls", 2 * one_vol),
                           ("one_call", one_vol)):
            ms = statistics.median(series[k])
            row[k + "_ms"] = round(ms, 4)
            row[k + "_min_ms"] = round(min(series[k]), 4)
            row[k + "_max_ms"] = round(max(series[k]), 4)
            row[k + "_write_GBps"] = round(written / ms / 1e6, 1)
        row["bidir_over_two_calls"] = round(
            row["bidir_ms"] / row["two_calls_ms"], 4)
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
    im1 = torch.rand(1, 3, H, W, device=dev)
    im2 = torch.rand(1, 3, H, W, device=dev)

    def two():
        eng(im1, im2)
        eng(im2, im1)

    def bidir():
        eng(im1, im2, bidirectional=True)

    # the baseline appears twice per round: the gap between its two series
    # is the run-to-run spread the bidirectional gain has to beat
    series = alternate([("two_calls_a", two), ("bidir", bidir),
                        ("two_calls_b", two)], reps=args.reps,
                       rounds=args.rounds)
    med = {k: statistics.median(v) for k, v in series.items()}
    base = statistics.median(series["two_calls_a"] + series["two_calls_b"])
    per_round = [abs(a - b) for a, b in zip(series["two_calls_a"],
                                            series["two_calls_b"])]
    spread = max(abs(med["two_calls_a"] - med["two_calls_b"]),
                 statistics.median(per_round))
    row = {"bench": "e2e", "size": [H, W], "iters": args.iters,
           "dtype": "bf16", "batch": 1, "rounds": args.rounds,
           "reps": args.reps,
           "two_calls_a_ms": round(med["two_calls_a"], 3),
           "two_calls_b_ms": round(med["two_calls_b"], 3),
           "two_calls_ms": round(base, 3),
           "two_calls_min_ms": round(min(series["two_calls_a"]
                                         + series["two_calls_b"]), 3),
           "two_calls_max_ms": round(max(series["two_calls_a"]
                                         + series["two_calls_b"]), 3),
           "baseline_spread_ms": round(spread, 3),
           "bidir_ms": round(med["bidir"], 3),
           "bidir_min_ms": round(min(series["bidir"]), 3),
           "bidir_max_ms": round(max(series["bidir"]), 3),
           "bidir_over_two_calls": round(med["bidir"] / base, 4),
           "bidir_faster_beyond_spread": bool(base - med["bidir"] > spread)}
    print(json.dumps(row), flush=True)


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("mode", choices=["kernel", "e2e"])
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--iters", type=int, default=32)
    p.add_argument("--size", default="436x1024",
                   type=lambda s: tuple(int(v) for v in s.split("x")))
    args = p.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bidir needs a GPU (no CPU fallback)")
    {"kernel": mode_kernel, "e2e": mode_e2e}[args.mode](args)


if __name__ == "__main__":
    main()
