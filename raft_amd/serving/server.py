"""Optical-flow serving: FastAPI app around the InferenceEngine.

The reference had no serving story (single-shot CLI only); this is the
production-serving layer for the rebuild: HTTP endpoints for flow
estimation with per-request dynamic shapes (pad8 + HIP-graph shape
buckets), Prometheus metrics, and health checks.

Run:  python -m raft_amd.serving.server --load w.npz --port 8000
Test: tests/test_serving.py (CPU, starlette TestClient)
"""
from __future__ import annotations

import argparse
import asyncio
import os
import io
import struct
import threading
import time
from typing import Optional

import numpy as np
import torch

try:
    from fastapi import FastAPI, Request, Response
    from prometheus_client import (Counter, Histogram, CollectorRegistry,
                                   generate_latest, CONTENT_TYPE_LATEST)
    _HAVE_SERVING = True
except ImportError:  # pragma: no cover
    _HAVE_SERVING = False


def _decode_image_bytes(data: bytes) -> torch.Tensor:
    """PNG or JPEG bytes -> [1,3,H,W] float BGR in [0,1] (in-memory codec
    dispatch — the reference accepted either via cv2.imdecode)."""
    from raft_amd.data.imageio import decode_image
    img = decode_image(data)
    t = torch.from_numpy(img.astype(np.float32) / 255.0)
    return t.permute(2, 0, 1).unsqueeze(0)


def _flo_bytes(flow: np.ndarray) -> bytes:
    buf = io.BytesIO()
    buf.write(b"PIEH")
    buf.write(struct.pack("<ii", flow.shape[1], flow.shape[0]))
    buf.write(flow.astype(np.float32).tobytes())
    return buf.getvalue()


def warm_engine(engine, shapes) -> None:
    """Run dummy pairs through the engine before traffic arrives: MIOpen
    benchmark-mode find, allocator growth and HIP-graph bucket capture
    all happen here instead of inside the first requests."""
    for h, w in shapes:
        z = torch.zeros(1, 3, h, w)
        engine(z, z)


def parse_shapes(spec: str):
    """'432x1024,288x512' -> [(432, 1024), (288, 512)]"""
    shapes = []
    for part in spec.split(","):
        if not part:
            continue
        h, w = part.lower().split("x")
        shapes.append((int(h), int(w)))
    return shapes


def create_app(model=None, iters: Optional[int] = None,
               dtype: torch.dtype = torch.float32,
               warmup_shapes=None):
    """Build the FastAPI app. model defaults to random-init raft-things."""
    if not _HAVE_SERVING:
        raise RuntimeError("fastapi / prometheus_client not installed")
    from raft_amd import RAFT, RaftConfig
    from raft_amd.engine.inference import InferenceEngine

    if model is None:
        model = RAFT(RaftConfig(small=False))
    engine = InferenceEngine(model, iters=iters, dtype=dtype)
    if warmup_shapes:
        warm_engine(engine, warmup_shapes)
    # Handlers are async; the blocking work (decode + inference) runs in
    # executor threads so the event loop (and /healthz) stays responsive
    # under long requests.  Decode parallelizes across requests; the
    # engine itself is guarded by a lock (shared HIP-graph buckets /
    # captured buffers are not reentrant).
    infer_lock = threading.Lock()
    max_body = int(os.environ.get("RAFT_AMD_MAX_BODY_MB", "256")) * 1024 * 1024

    def _gate(tol, check_every, min_iters):
        """Query parameters -> Convergence or None; ValueError (-> 400)
        on bad values."""
        if tol is None:
            if check_every is not None or min_iters is not None:
                raise ValueError("check_every / min_iters need tol")
            return None
        from raft_amd import Convergence
        kw = {}
        if check_every is not None:
            kw["every"] = check_every
        if min_iters is not None:
            kw["min_iters"] = min_iters
        return Convergence(tol=tol, **kw)

    def _run_flow(body: bytes, iters_req: Optional[int], converge=None):
        (n1,) = struct.unpack_from("<I", body, 0)
        im1 = _decode_image_bytes(body[4:4 + n1])
        im2 = _decode_image_bytes(body[4 + n1:])
        if im1.shape != im2.shape:
            raise ValueError(
                f"frame shapes differ: {tuple(im1.shape[2:])} vs "
                f"{tuple(im2.shape[2:])}")
        with infer_lock:
            out = engine(im1, im2, iters=iters_req, converge=converge)
            ran = engine.last_info.iters_run
        return out[0].float().permute(1, 2, 0).cpu().numpy(), ran

    def _run_flow_batch(body: bytes, iters_req: Optional[int],
                        converge=None):
        from concurrent.futures import ThreadPoolExecutor
        from raft_amd.engine.inference import run_mixed_batch
        (n_pairs,) = struct.unpack_from("<I", body, 0)
        off = 4
        raw = []
        for _ in range(n_pairs):
            (n1,) = struct.unpack_from("<I", body, off)
            raw.append(bytes(body[off + 4:off + 4 + n1]))
            off += 4 + n1
            (n2,) = struct.unpack_from("<I", body, off)
            raw.append(bytes(body[off + 4:off + 4 + n2]))
            off += 4 + n2
        # decode in threads: the C codec loops release the GIL during
        # the ctypes calls, so a batch's images decode in parallel
        if len(raw) > 2:
            with ThreadPoolExecutor(min(8, len(raw))) as ex:
                imgs = list(ex.map(_decode_image_bytes, raw))
        else:
            imgs = [_decode_image_bytes(b) for b in raw]
        pairs = list(zip(imgs[0::2], imgs[1::2]))
        for i, (a, b) in enumerate(pairs):
            if a.shape != b.shape:
                raise ValueError(f"pair {i}: frame shapes differ")
        with infer_lock:
            flows, ran = run_mixed_batch(engine, pairs, iters=iters_req,
                                         converge=converge,
                                         return_iters=True)
        return b"".join(
            _flo_bytes(f[0].float().permute(1, 2, 0).cpu().numpy())
            for f in flows), ran

    app = FastAPI(title="raft_amd flow service")
    # per-app registry: repeated create_app() in one process (tests,
    # multi-model serving) must not collide in the global registry
    registry = CollectorRegistry()
    requests_total = Counter("raft_requests_total", "flow requests served",
                             registry=registry)
    request_errors = Counter("raft_request_errors_total", "failed requests",
                             registry=registry)
    latency = Histogram("raft_request_seconds", "end-to-end request latency",
                        registry=registry)
    iters_run = Histogram("raft_iters_run",
                          "refinement iterations executed per pair",
                          buckets=(1, 2, 3, 4, 6, 8, 12, 16, 20, 24, 32, 48,
                                   64),
                          registry=registry)

    @app.get("/healthz")
    def healthz():
        return {"status": "ok", "device": str(engine.device),
                "cuda": torch.cuda.is_available()}

    @app.get("/metrics")
    def metrics():
        return Response(generate_latest(registry),
                        media_type=CONTENT_TYPE_LATEST)

    @app.post("/flow")
    async def flow(request: Request, fmt: str = "flo",
                   iters: Optional[int] = None,
                   tol: Optional[float] = None,
                   check_every: Optional[int] = None,
                   min_iters: Optional[int] = None):
        """Body framing (no multipart dependency):
        [uint32-le len(img1)] [img1 bytes] [img2 bytes] (PNG or JPEG).
        tol (full-resolution pixels) gates the refinement loop, checked
        every check_every iterations from min_iters on; the executed count
        comes back in X-Raft-Iters."""
        t0 = time.perf_counter()
        if fmt not in ("flo", "color"):
            request_errors.inc()
            return Response(f"unknown fmt {fmt!r} (flo|color)",
                            status_code=400)
        try:
            body = await request.body()
            if len(body) > max_body:
                request_errors.inc()
                return Response("payload too large", status_code=413)
            converge = _gate(tol, check_every, min_iters)
            flow_np, ran = await asyncio.get_event_loop().run_in_executor(
                None, _run_flow, body, iters, converge)
            if fmt == "color":
                from raft_amd.utils.flow_viz import flow_to_color
                from raft_amd.data.imageio import encode_png
                color = flow_to_color(flow_np, convert_to_bgr=True)
                payload = encode_png(color)
                media = "image/png"
            else:
                payload = _flo_bytes(flow_np)
                media = "application/octet-stream"
            requests_total.inc()
            latency.observe(time.perf_counter() - t0)
            iters_run.observe(ran)
            return Response(payload, media_type=media,
                            headers={"X-Raft-Iters": str(ran)})
        except (ValueError, struct.error, IndexError) as e:
            request_errors.inc()   # malformed body/image: client error
            return Response(f"bad request: {e}", status_code=400)
        except Exception:
            request_errors.inc()
            raise

    @app.post("/flow_batch")
    async def flow_batch(request: Request, iters: Optional[int] = None,
                         tol: Optional[float] = None,
                         check_every: Optional[int] = None,
                         min_iters: Optional[int] = None):
        """Batched flow with per-pair dynamic shapes. Body framing:
        [uint32-le n_pairs] then per pair
        [uint32 len(png1)][png1][uint32 len(png2)][png2].
        Same-shape pairs are grouped into one engine call
        (run_mixed_batch — BASELINE config 5 semantics); the response is
        the concatenation of one .flo record per pair, input order.
        tol / check_every / min_iters gate each shape group on its own;
        X-Raft-Iters lists the executed count of every pair."""
        t0 = time.perf_counter()
        try:
            body = await request.body()
            if len(body) > max_body:
                request_errors.inc()
                return Response("payload too large", status_code=413)
            converge = _gate(tol, check_every, min_iters)
            payload, ran = await asyncio.get_event_loop().run_in_executor(
                None, _run_flow_batch, body, iters, converge)
            requests_total.inc()
            latency.observe(time.perf_counter() - t0)
            for n in ran:
                iters_run.observe(n)
            return Response(payload, media_type="application/octet-stream",
                            headers={"X-Raft-Iters":
                                     ",".join(str(n) for n in ran)})
        except (ValueError, struct.error, IndexError) as e:
            request_errors.inc()
            return Response(f"bad request: {e}", status_code=400)
        except Exception:
            request_errors.inc()
            raise

    return app


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--load", default=None)
    p.add_argument("--small", action="store_true")
    p.add_argument("--iters", type=int, default=None)
    p.add_argument("--dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--host", default="127.0.0.1")
    p.add_argument("--port", type=int, default=8000)
    p.add_argument("--warmup", default="",
                   help="comma-separated HxW shapes to pre-capture "
                        "before serving, e.g. 432x1024,288x512")
    args = p.parse_args(argv)
    if args.iters is not None and args.iters < 1:
        p.error("--iters must be >= 1")
    try:
        warmup_shapes = parse_shapes(args.warmup)
    except ValueError:
        p.error(f"--warmup must be comma-separated HxW, got "
                f"{args.warmup!r}")

    from raft_amd import RAFT, RaftConfig
    model = RAFT(RaftConfig(small=args.small))
    if args.load:
        if args.load.endswith(".npz"):
            from raft_amd.utils import checkpoint as ckpt
            ckpt.load_npz(model, args.load)
        else:   # torch state_dict (.pt) — same dual surface as the CLI
            state = torch.load(args.load, map_location="cpu",
                               weights_only=True)
            model.load_state_dict(state.get("model", state))
    if torch.cuda.is_available():
        model = model.to("cuda")
    app = create_app(model, iters=args.iters,
                     dtype=torch.bfloat16 if args.dtype == "bf16"
                     else torch.float32,
                     warmup_shapes=warmup_shapes)
    import uvicorn
    uvicorn.run(app, host=args.host, port=args.port)


if __name__ == "__main__":
    main()
