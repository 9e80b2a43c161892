"""Frame interpolation on the GPU: what an in-between frame costs.

  kernel  ops.interpolate_frame (memset + scatter + synthesis kernels)
          against torch_ref.interpolate_frame — the same definition as a
          composition of PyTorch ops — on the same GPU tensors, at
          436x1024, batch 1, 3 channels, t = 0.5. The outputs of the two
          are compared bit for bit before anything is timed. Reports the
          bytes the op has to move (computed from the shapes) over its
          time.
  e2e     engine.interpolate with 1 and with 3 in-between frames against
          engine.bidirectional alone at 436x1024, bf16, 32 iters, batch 1:
          the cost of one in-between frame as a fraction of the
          bidirectional pass. The bidirectional baseline is timed twice
          per round so its own run-to-run spread is known.

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


def alternate(variants, rounds, warmup=3):
    """variants: list of (name, fn, reps). Returns {name: [ms per round]}."""
    for _, fn, _ in variants:
        for _ in range(warmup):
            fn()
    series = {name: [] for name, _, _ in variants}
    for _ in range(rounds):
        for name, fn, reps in variants:
            series[name].append(timed(fn, reps))
    return series


def _stats(row, key, values):
    row[key + "_ms"] = round(statistics.median(values), 4)
    row[key + "_min_ms"] = round(min(values), 4)
    row[key + "_max_ms"] = round(max(values), 4)


def mode_kernel(args):
    import torch
    import torch.nn.functional as F
    from raft_amd import ops
    from raft_amd.ops import torch_ref
    torch.manual_seed(3)
    dev = torch.device("cuda")
    H, W = args.size
    B, C, t = 1, 3, 0.5
    im0 = torch.rand(B, C, H, W, device=dev)
    im1 = torch.rand(B, C, H, W, device=dev)
    # a smooth field of a few pixels with a rough backward partner: motion
    # of the size the model returns, with real occlusion decisions
    fw = F.interpolate(torch.randn(B, 2, 6, 12, device=dev) * 6.0,
                       size=(H, W), mode="bilinear",
                       align_corners=True).contiguous()
    bw = (-fw + torch.randn(B, 2, H, W, device=dev) * 0.4).contiguous()
    occ_fw, occ_bw = ops.fb_consistency(fw, bw)

    def hip():
        return ops.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw, t)

    def oracle():
        return torch_ref.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw,
                                           t)

    got, want = hip(), oracle()
    names = ("frame", "flow_t0", "flow_t1", "cover")
    same = {n: bool(torch.equal(a, b)) for n, a, b in zip(names, got, want)}
    cover = got[3]
    series = alternate([("hip", hip, args.reps * 5),
                        ("oracle", oracle, max(1, args.reps // 5))],
                       rounds=args.rounds)
    cells = B * H * W
    # per cell: both images and the frame (C floats each), four flow planes
    # in, four out, two mask bytes, one cover byte, and the two 64-bit keys
    # written by the memset and read by the synthesis (the atomics of the
    # scatter come on top and are not counted)
    moved = cells * (3 * C * 4 + 8 * 4 + 3 + 2 * 8 * 2)
    row = {"bench": "kernel", "size": [H, W], "batch": B, "channels": C,
           "t": t, "rounds": args.rounds, "bit_identical": same,
           "uncovered_share": round((cover == 0).float().mean().item(), 5),
           "occluded_share": round(
               (occ_fw | occ_bw).float().mean().item(), 5),
           "bytes_moved": moved}
    _stats(row, "hip", series["hip"])
    _stats(row, "oracle", series["oracle"])
    row["hip_GBps"] = round(moved / row["hip_ms"] / 1e6, 1)
    row["oracle_over_hip"] = round(row["oracle_ms"] / row["hip_ms"], 2)
    row["hip_faster"] = bool(max(series["hip"]) < min(series["oracle"]))
    print(json.dumps(row), flush=True)
    if not all(same.values()):
        raise SystemExit(f"kernel and oracle differ: {same}")


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

    def bidir():
        eng.bidirectional(im1, im2)

    def interp1():
        eng.interpolate(im1, im2, times=(0.5,))

    def interp3():
        eng.interpolate(im1, im2, times=(0.25, 0.5, 0.75))

    series = alternate([("bidir_a", bidir, args.reps),
                        ("interp1", interp1, args.reps),
                        ("interp3", interp3, args.reps),
                        ("bidir_b", bidir, args.reps)], rounds=args.rounds)
    med = {k: statistics.median(v) for k, v in series.items()}
    base = statistics.median(series["bidir_a"] + series["bidir_b"])
    per_round = [abs(a - b) for a, b in zip(series["bidir_a"],
                                            series["bidir_b"])]
    spread = max(abs(med["bidir_a"] - med["bidir_b"]),
                 statistics.median(per_round))
    # one in-between frame: the slope between 1 and 3 frames (the
    # baseline's spread cancels), and the first frame over the pass alone
    per_frame = (med["interp3"] - med["interp1"]) / 2.0
    row = {"bench": "e2e", "size": [H, W], "iters": args.iters,
           "dtype": "bf16", "batch": 1, "rounds": args.rounds,
           "reps": args.reps,
           "bidir_a_ms": round(med["bidir_a"], 3),
           "bidir_b_ms": round(med["bidir_b"], 3),
           "bidir_ms": round(base, 3),
           "baseline_spread_ms": round(spread, 3)}
    _stats(row, "interp1", series["interp1"])
    _stats(row, "interp3", series["interp3"])
    row["per_inbetween_ms"] = round(per_frame, 4)
    row["per_inbetween_over_bidir"] = round(per_frame / base, 5)
    row["first_inbetween_ms"] = round(med["interp1"] - base, 4)
    row["first_inbetween_beyond_spread"] = bool(
        med["interp1"] - base > spread)
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
        raise SystemExit("bench_interp needs a GPU (no CPU fallback)")
    {"kernel": mode_kernel, "e2e": mode_e2e}[args.mode](args)


if __name__ == "__main__":
    main()
