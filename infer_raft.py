#!/usr/bin/env python3
"""RAFT optical-flow CLI — same flag surface as the reference's
infer_raft.py (BASELINE.json API contract), with the modes the reference
left unimplemented (train / val / export / flops) working.

Modes:
  test    run flow on an image pair — or consecutive pairs of a --data
          directory (--warm warm-starts, --workers parallel decode) —
          and write the color-coded PNG (reference infer_raft.py:74-78;
          output file name kept); --bidirectional adds the backward flow
          and forward-backward occlusion masks from the same pass;
          --stream runs the directory as one video session (each frame
          encoded once; --warm is then RAFT's projected warm start);
          --interp N (implies --bidirectional) also writes N evenly
          spaced in-between frames of every pair
  train   train on synthetic pairs, or on a --data directory of flow
          triplets (Sintel dir/tree, KITTI devkit, FlyingChairs);
          preemption-safe (--resume, --save-every, SIGTERM), --accum
          gradient accumulation (the reference had no train body)
  val     EPE evaluation — synthetic exact-gt pairs, or --data triplets
          (.flo / KITTI 16-bit png with validity masking / .pfm)
  export  save weights as reference-layout .npz (+ state_dict .pt)
  flops   parameter/FLOP report (the reference's flops mode crashes on an
          arity bug, networks/RAFT.py:144 — this one works)

Flags mirror the reference (infer_raft.py:51-67): --gpu --data --load
-m/--mode --out --batch -o/--optimizer --im1 --im2 --small, plus the
rebuild's --iters/--size/--dtype/--steps/--warm/--bidirectional/--stream/
--interp/--tol/--check-every/--min-iters/--workers/--resume/--save-every/
--accum (iters was hard-coded 20 in the reference, networks/RAFT.py:33).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch


def parse_args(argv=None):
    import raft_amd
    p = argparse.ArgumentParser(description=__doc__)
    p.add_argument("--version", action="version",
                   version=f"raft_amd {raft_amd.__version__}")
    p.add_argument("--gpu", default=None,
                   help="comma separated list of GPU(s) to use")
    p.add_argument("--data", default=None, help="dataset path (training)")
    p.add_argument("--load", default=None,
                   help="checkpoint to load (.npz reference layout or .pt)")
    p.add_argument("-m", "--mode", default="test",
                   choices=["train", "val", "test", "export", "flops"])
    p.add_argument("--out", default="./log", help="output directory")
    p.add_argument("--batch", default=1, type=int, help="batch per GPU")
    p.add_argument("-o", "--optimizer", default="adamw",
                   choices=["adam", "adamw", "sgd", "sgd_cyclic",
                            "sgd_1cycle"])
    p.add_argument("--im1", default="frame_0010.png", help="left image path")
    p.add_argument("--im2", default="frame_0011.png", help="right image path")
    p.add_argument("--small", action="store_true")
    # rebuild extensions
    p.add_argument("--iters", type=int, default=None,
                   help="refinement iterations (default: 20, ref value)")
    p.add_argument("--size", default="432x1024",
                   help="HxW input resize for test mode; 'native' keeps "
                        "the file size (pad8'd)")
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--steps", type=int, default=100, help="training steps")
    p.add_argument("--no-graph", action="store_true",
                   help="disable HIP-graph capture in test mode")
    p.add_argument("--warm", action="store_true",
                   help="warm-start each sequence pair from the previous "
                        "flow (official-RAFT 2-view style)")
    p.add_argument("--bidirectional", action="store_true",
                   help="test mode: also compute the backward flow and "
                        "forward-backward occlusion masks in the same pass "
                        "(writes *_bw.flo/.png and raft_occ_*_{fw,bw}.png)")
    p.add_argument("--stream", action="store_true",
                   help="test mode with --data DIR: run the sorted frames "
                        "as one video session — every frame is encoded "
                        "once, and --warm starts each pair from the "
                        "previous low-resolution flow projected forward "
                        "(same output files as without the flag). Frames "
                        "are decoded one at a time as they are pushed: "
                        "needs --batch 1, and --workers has no effect")
    p.add_argument("--interp", type=int, default=0, metavar="N",
                   help="test mode: also write N evenly spaced in-between "
                        "frames of every pair (t = k/(N+1)) as "
                        "raft_interp_*_tK.png next to the flow output; "
                        "implies --bidirectional; with --stream they come "
                        "from the session (between)")
    p.add_argument("--tol", type=float, default=None, metavar="PX",
                   help="test mode: stop the refinement loop once its "
                        "update is within PX full-resolution pixels (one "
                        "final iteration follows); --iters is then the "
                        "budget. The executed count is printed per pair")
    p.add_argument("--check-every", type=int, default=4, metavar="K",
                   help="with --tol: measure the update every K iterations")
    p.add_argument("--min-iters", type=int, default=1, metavar="M",
                   help="with --tol: no check before iteration M")
    p.add_argument("--workers", type=int, default=0,
                   help="parallel decode workers for sequence/val modes")
    p.add_argument("--resume", action="store_true",
                   help="resume training from <out>/train_state.pt")
    p.add_argument("--save-every", type=int, default=50,
                   help="checkpoint train_state.pt every N steps")
    p.add_argument("--accum", type=int, default=1,
                   help="micro-batches accumulated per optimizer step")
    args = p.parse_args(argv)
    for name, lo in (("batch", 1), ("steps", 1), ("accum", 1),
                     ("workers", 0), ("save_every", 1), ("interp", 0)):
        if getattr(args, name) < lo:
            p.error(f"--{name.replace('_', '-')} must be >= {lo}")
    if args.stream and args.mode != "test":
        p.error("--stream applies to --mode test with --data DIR")
    if args.iters is not None and args.iters < 1:
        p.error("--iters must be >= 1")
    if args.interp:
        if args.mode != "test":
            p.error("--interp applies to --mode test")
        args.bidirectional = True
    args.converge = None
    if args.tol is not None:
        if args.mode != "test":
            p.error("--tol applies to --mode test")
        try:
            args.converge = raft_amd.Convergence(
                tol=args.tol, every=args.check_every,
                min_iters=args.min_iters)
        except ValueError as e:
            p.error(str(e))
    return args


def _select_device(args):
    if args.gpu is not None and torch.cuda.is_available():
        os.environ.setdefault("HIP_VISIBLE_DEVICES", args.gpu)
    return torch.device("cuda") if torch.cuda.is_available() \
        else torch.device("cpu")


def _build_model(args, device):
    from raft_amd import RAFT, RaftConfig
    model = RAFT(RaftConfig(small=args.small)).to(device).eval()
    if args.load:
        from raft_amd.utils import checkpoint as ckpt
        if args.load.endswith(".npz"):
            ckpt.load_npz(model, args.load)
        else:
            state = torch.load(args.load, map_location="cpu",
                               weights_only=True)
            model.load_state_dict(state.get("model", state))
        print(f"loaded {args.load}")
    return model


def mode_test(args, device):
    from raft_amd.data.dataflow import PairDataflow
    from raft_amd.engine.inference import InferenceEngine
    from raft_amd.data.imageio import write_png
    from raft_amd.utils.flow_viz import flow_to_color
    from raft_amd.utils.flow_io import write_flo

    model = _build_model(args, device)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    engine = InferenceEngine(model, iters=args.iters, dtype=dtype,
                             use_graph=not args.no_graph)
    try:
        size = None if args.size == "native" else \
            tuple(int(v) for v in args.size.split("x"))
        if size is not None and (len(size) != 2 or min(size) < 1):
            raise ValueError(size)
    except ValueError:
        raise SystemExit(f"--size must be HxW (e.g. 432x1024) or "
                         f"'native', got {args.size!r}")
    if args.data and os.path.isdir(args.data):
        # sequence mode: consecutive frame pairs from a directory
        # (the reference parsed --data but never used it, infer_raft.py:54)
        frames = sorted(
            os.path.join(args.data, f) for f in os.listdir(args.data)
            if f.lower().endswith((".png", ".jpg", ".jpeg",
                                   ".ppm")))
        pairs = list(zip(frames[:-1], frames[1:]))
        if not pairs:
            raise SystemExit(f"no consecutive image pairs in {args.data}")
    else:
        if args.stream:
            raise SystemExit("--stream needs sequence mode: pass --data "
                             "DIR with the frames of one video (it does "
                             "not apply to an --im1/--im2 pair)")
        pairs = [(args.im1, args.im2)]
    if args.stream and args.batch != 1:
        raise SystemExit("--stream runs one video, frame by frame: "
                         "use --batch 1")
    os.makedirs(args.out, exist_ok=True)
    variant = "raft-small" if args.small else "raft-things"
    prev_flow = None
    prev_bw = None

    def _warm(prev):
        import torch.nn.functional as Fn
        # the engine pads frames up to a multiple of 8, so the model's
        # coords grid is ceil(H/8) x ceil(W/8) — match that here or
        # 'coords1 + flow_init' shape-mismatches on e.g. 436-high frames
        h8 = -(-prev.shape[-2] // 8)
        w8 = -(-prev.shape[-1] // 8)
        return Fn.interpolate(prev, size=(h8, w8), mode="bilinear",
                              align_corners=False) / 8.0

    def _write(i, flow, bidir):
        # --batch > 1 decodes several pairs into one forward (the
        # reference's TODO 'check if batch_size could be free',
        # networks/RAFT.py:46) — write every sample's outputs
        for j in range(flow.shape[0]):
            idx = i * args.batch + j
            flow_np = flow[j].float().permute(1, 2, 0).cpu().numpy()
            color = flow_to_color(flow_np, convert_to_bgr=True)
            suffix = f"_{idx:04d}" if len(pairs) > 1 else ""
            out_path = os.path.join(args.out,
                                    f"raft_flow_{variant}{suffix}.png")
            write_png(out_path, color)
            write_flo(os.path.join(
                args.out, f"raft_flow_{variant}{suffix}.flo"), flow_np)
            print(f"wrote {out_path}")
            if bidir is not None:
                stem = os.path.join(args.out, f"raft_flow_{variant}{suffix}")
                bw_np = bidir.flow_bw[j].float().permute(1, 2, 0) \
                    .cpu().numpy()
                write_png(stem + "_bw.png",
                          flow_to_color(bw_np, convert_to_bgr=True))
                write_flo(stem + "_bw.flo", bw_np)
                occ = os.path.join(args.out, f"raft_occ_{variant}{suffix}")
                for tag, m in (("fw", bidir.occ_fw), ("bw", bidir.occ_bw)):
                    write_png(f"{occ}_{tag}.png",
                              m[j, 0].cpu().numpy().astype(np.uint8) * 255)
                print(f"wrote {stem}_bw.png and {occ}_fw.png / _bw.png")

    def _ran(n):
        # the executed count, for gated runs only (--tol): an ungated pair
        # line stays as it was
        return (f"{n} iters",) if args.converge is not None else ()

    times = [k / (args.interp + 1) for k in range(1, args.interp + 1)]

    def _write_interp(i, frames_t):
        # frames_t: [T,B,3,H,W] fp32 in the inputs' [0,1] BGR range
        u8 = (frames_t.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8) \
            .permute(0, 1, 3, 4, 2).cpu().numpy()
        for j in range(u8.shape[1]):
            idx = i * args.batch + j
            suffix = f"_{idx:04d}" if len(pairs) > 1 else ""
            for k in range(u8.shape[0]):
                path = os.path.join(
                    args.out, f"raft_interp_{variant}{suffix}_t{k + 1}.png")
                write_png(path, np.ascontiguousarray(u8[k, j]))
            print(f"wrote {u8.shape[0]} in-between frame(s) "
                  f"raft_interp_{variant}{suffix}_t*.png")

    if args.stream:
        # one session over the sorted frames: pair i is (frame i, frame i+1)
        from raft_amd.data.dataflow import load_image, resize_to
        if args.workers:
            print("--stream decodes frames as they are pushed: --workers "
                  "ignored")
        session = engine.stream(warm=args.warm,
                                bidirectional=args.bidirectional,
                                converge=args.converge)
        for k, path in enumerate(frames):
            img = load_image(path)
            if size is not None:
                img = resize_to(img, size)
            t0 = time.perf_counter()
            res = session.push(img.unsqueeze(0))
            if res is None:
                continue
            bidir = res if args.bidirectional else None
            flow = res.flow_fw if args.bidirectional else res
            if device.type == "cuda":
                torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(k - 1, tuple(flow.shape), f"{dt * 1e3:.1f} ms",
                  *_ran(session.last_iters))
            _write(k - 1, flow, bidir)
            if times:
                _write_interp(k - 1, session.between(times))
        return

    ds = PairDataflow(pairs, input_size=size, batch=args.batch,
                      workers=args.workers)
    for i, (im1, im2) in enumerate(ds):
        flow_init = None
        if args.warm and prev_flow is not None:
            flow_init = _warm(prev_flow)
            if args.bidirectional:
                # each direction warm-starts from its own previous flow
                flow_init = (flow_init, _warm(prev_bw))
        t0 = time.perf_counter()
        bidir = None
        if args.bidirectional:
            bidir = engine.bidirectional(im1, im2, flow_init=flow_init,
                                         converge=args.converge)
            flow = bidir.flow_fw
            prev_bw = bidir.flow_bw.float()
        else:
            flow = engine(im1, im2, flow_init=flow_init,
                          converge=args.converge)
        prev_flow = flow.float()
        if device.type == "cuda":
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(i, tuple(flow.shape), f"{dt * 1e3:.1f} ms",
              *_ran(engine.last_info.iters_run))
        _write(i, flow, bidir)
        if times:
            from raft_amd.engine.inference import interpolate_between
            _write_interp(i, interpolate_between(
                im1.to(engine.device, engine.dtype),
                im2.to(engine.device, engine.dtype), bidir, times))


def mode_val(args, device):
    from raft_amd.data.synthetic import synthetic_pair
    from raft_amd.engine.trainer import epe
    from raft_amd.engine.inference import InferenceEngine
    from raft_amd.parallel.ddp import init_distributed
    import torch.distributed as dist

    rank = init_distributed()  # DP eval: shard samples, all-reduce the metric
    world = dist.get_world_size() if dist.is_initialized() else 1
    model = _build_model(args, device)
    engine = InferenceEngine(
        model, iters=args.iters,
        dtype=torch.bfloat16 if args.dtype == "bf16" else torch.float32,
        use_graph=not args.no_graph)
    epes = []
    if args.data and os.path.isdir(args.data):
        # file-based EPE (Sintel-style): consecutive frame pairs with a
        # ground-truth <frame1>.flo next to each first frame (the reference
        # had no EPE evaluation at all — SURVEY.md §5.5)
        from raft_amd.data.dataflow import load_image
        from raft_amd.data.datasets import find_flow_triplets
        from raft_amd.utils.flow_io import load_flow_gt
        samples = find_flow_triplets(args.data)
        if not samples:
            raise SystemExit(f"no (frame, frame, .flo) triplets in "
                             f"{args.data}")
        for f1, f2, flo in samples[rank::world]:
            im1 = load_image(f1).unsqueeze(0)
            im2 = load_image(f2).unsqueeze(0)
            gt_np, valid = load_flow_gt(flo)
            gt = torch.from_numpy(
                gt_np.astype(np.float32)).permute(2, 0, 1)[None]
            flow = engine(im1, im2)
            err = torch.norm(flow.float().cpu() - gt, dim=1)[0]
            if valid is not None:
                m = torch.from_numpy(valid)
                err = err[m] if m.any() else err
            epes.append(float(err.mean()))
        data_desc = f"{args.data} ({len(samples)} pairs)"
    else:
        for seed in range(8)[rank::world]:
            im1, im2, gt = synthetic_pair(args.batch, 288, 512, seed=seed)
            flow = engine(im1, im2)
            epes.append(float(epe(flow.float().cpu(), gt)))
        data_desc = "synthetic-warp 288x512"
    if world > 1:
        t = torch.tensor([float(np.sum(epes)), float(len(epes))],
                         dtype=torch.float64, device=device)
        dist.all_reduce(t)   # per-rank metric reduction
        mean = float((t[0] / t[1]).item())
    else:
        mean = float(np.mean(epes))
    if rank == 0:
        result = {"epe_mean": mean, "epe_per_batch": epes, "world": world,
                  "data": data_desc, "iters": args.iters}
        print(json.dumps(result))


def mode_train(args, device):
    from raft_amd.data.synthetic import synthetic_pair
    from raft_amd.engine.trainer import GracefulStop, Trainer, TrainConfig
    from raft_amd.parallel.ddp import init_distributed
    from raft_amd.utils import checkpoint as ckpt

    rank = init_distributed()
    model = _build_model(args, device)
    model.train()
    cfg = TrainConfig(num_steps=args.steps, batch=args.batch)
    tr = Trainer(model, cfg, device=device)
    os.makedirs(args.out, exist_ok=True)
    state_path = os.path.join(args.out, "train_state.pt")
    if args.resume and os.path.exists(state_path):
        tr.load(state_path)
        if rank == 0:
            print(f"resumed from {state_path} at step {tr.step_count}")
    stopper = GracefulStop()
    preempted = False
    data_iter = None
    if args.data and os.path.isdir(args.data):
        # file-based training (Sintel-style triplets — the same layout
        # --mode val evaluates on); synthetic pairs otherwise
        from raft_amd.data.datasets import (FlowPairDataset,
                                            find_flow_triplets,
                                            infinite_batches)
        world = int(os.environ.get("WORLD_SIZE", "1"))
        trips = find_flow_triplets(args.data)
        if not trips:
            raise SystemExit(f"no (frame, frame, .flo) triplets under "
                             f"{args.data}")
        ds = FlowPairDataset(trips, crop=(288, 512), batch=args.batch,
                             rank=rank, world=world, with_valid=True)
        data_iter = infinite_batches(ds)
        if rank == 0:
            print(f"training on {args.data}: {len(trips)} triplets")
    for step in range(tr.step_count, args.steps):
        def _next(mb):
            if data_iter is not None:
                return next(data_iter)   # (im1, im2, gt, valid)
            return synthetic_pair(args.batch, 288, 512,
                                  seed=(step * args.accum + mb) * 131 + rank)
        if args.accum > 1:
            stats = tr.step_accum([_next(m) for m in range(args.accum)])
        else:
            mb = _next(0)
            im1, im2, gt = mb[0], mb[1], mb[2]
            valid = mb[3].to(device) if len(mb) == 4 else None
            stats = tr.step(im1.to(device), im2.to(device), gt.to(device),
                            valid)
        if rank == 0 and (step % 10 == 0 or step == args.steps - 1):
            print(f"step {step}: loss {stats['loss']:.4f} "
                  f"epe {stats['epe']:.3f} lr {stats['lr']:.2e}")
        if stopper.should_stop(tr.distributed):
            preempted = True
        if rank == 0 and (preempted or
                          (step + 1) % args.save_every == 0):
            tr.save(state_path)
        if preempted:
            if rank == 0:
                print(f"preempted at step {step}: saved {state_path} "
                      f"(resume with --resume)")
            break
    stopper.restore()
    if rank == 0 and not preempted:
        tr.save(state_path)
        out = os.path.join(args.out, "raft_trained.npz")
        ckpt.save_npz(model, out)
        print(f"saved {out}")


def mode_export(args, device):
    from raft_amd.utils import checkpoint as ckpt
    model = _build_model(args, device)
    os.makedirs(args.out, exist_ok=True)
    variant = "raft-small" if args.small else "raft-things"
    npz_path = os.path.join(args.out, f"{variant}.npz")
    pt_path = os.path.join(args.out, f"{variant}.pt")
    ckpt.save_npz(model, npz_path)
    torch.save({"model": model.state_dict()}, pt_path)
    print(f"exported {npz_path} and {pt_path}")


def mode_flops(args, device):
    from raft_amd import RAFT, RaftConfig
    from raft_amd.engine.profiler import count_model_flops
    model = RAFT(RaftConfig(small=args.small))
    report = count_model_flops(model, 256, 448,
                               iters=args.iters or model.cfg.iters)
    print(json.dumps(report, indent=2))
    print("note: FLOPs counted as 2*MACs (multiply+add separately), matching "
          "tf.profiler convention the reference documents "
          "(infer_raft.py:93-95)")


def main(argv=None):
    args = parse_args(argv)
    device = _select_device(args)
    try:
        {"test": mode_test, "val": mode_val, "train": mode_train,
         "export": mode_export, "flops": mode_flops}[args.mode](args, device)
    except FileNotFoundError as e:
        raise SystemExit(f"file not found: {e.filename or e}")
    except IsADirectoryError as e:
        raise SystemExit(f"expected a file, got a directory: "
                         f"{e.filename or e}")


if __name__ == "__main__":
    sys.exit(main())
