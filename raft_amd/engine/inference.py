"""Inference engine: arbitrary-size input handling + HIP-graph capture.

The reference hardwired a (1, 432, 1024, 3) placeholder graph
(infer_raft.py:69, networks/RAFT.py:45-51).  This engine accepts any batch /
H / W (BASELINE config 5): inputs are padded to a multiple of 8
(official-RAFT style, bottom/right) and the flow is cropped back; per-shape
HIP graphs (torch.cuda.CUDAGraph == hipGraph on ROCm) are captured lazily
and cached by (B, H, W) bucket, removing the ~1000-launch overhead of the
32-iteration update loop.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

from raft_amd.convergence import ConvergenceInfo


def pad8(x: torch.Tensor) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """Pad H, W up to multiples of 8 (bottom/right, replicate edges so the
    padded band is benign). Returns (padded, (orig_h, orig_w))."""
    h, w = x.shape[-2:]
    ph = (-h) % 8
    pw = (-w) % 8
    if ph or pw:
        x = F.pad(x, (0, pw, 0, ph), mode="replicate")
    return x, (h, w)


def unpad(flow: torch.Tensor, hw: Tuple[int, int]) -> torch.Tensor:
    h, w = hw
    return flow[..., :h, :w]


class BidirectionalFlow(NamedTuple):
    """Result of InferenceEngine.bidirectional: flows [B,2,H,W] and
    occlusion masks [B,1,H,W] bool (True = occluded)."""
    flow_fw: torch.Tensor
    flow_bw: torch.Tensor
    occ_fw: torch.Tensor
    occ_bw: torch.Tensor


def _check_times(times) -> Tuple[float, ...]:
    times = tuple(float(t) for t in times)
    for t in times:
        if not 0.0 <= t <= 1.0:
            raise ValueError(f"interpolation times must lie in [0, 1], "
                             f"got {t}")
    return times


def interpolate_between(image1: torch.Tensor, image2: torch.Tensor,
                        bidir: BidirectionalFlow, times) -> torch.Tensor:
    """In-between frames [T,B,C,H,W] fp32 of two unpadded frames from
    their BidirectionalFlow: one ops.interpolate_frame call per time."""
    from raft_amd import ops
    times = _check_times(times)
    fw = bidir.flow_fw.float().contiguous()
    bw = bidir.flow_bw.float().contiguous()
    frames = [ops.interpolate_frame(image1, image2, fw, bw, bidir.occ_fw,
                                    bidir.occ_bw, t)[0] for t in times]
    if not frames:
        return image1.new_zeros((0,) + tuple(image1.shape),
                                dtype=torch.float32)
    return torch.stack(frames, dim=0)


class InferenceEngine:
    """Wraps a RAFT model for serving-style inference.

    * dynamic shapes via pad8/unpad,
    * optional bf16 execution,
    * optional HIP-graph capture per shape bucket (GPU only; capture is
      skipped transparently on CPU or when disabled).
    """

    def __init__(self, model, iters: Optional[int] = None,
                 dtype: torch.dtype = torch.float32,
                 use_graph: bool = True, max_graphs: int = 8,
                 loop_graph: Optional[bool] = None):
        if loop_graph is None:
            # env override, else AUTO (None): the fused loop enables
            # capture when iters <= 16 — measured +13% on the config-5
            # mixed-batch at 12 iters, -1.6% on the 32-iter headline
            import os
            e = os.environ.get("RAFT_AMD_LOOP_GRAPH")
            loop_graph = None if e is None else e == "1"
        self.loop_graph = loop_graph
        self.model = model.eval()
        self.iters = iters
        self.dtype = dtype
        if dtype != torch.float32:
            self.model = self.model.to(dtype)
        self.device = next(model.parameters()).device
        if self.device.type == "cuda":
            # channels-last end to end: MIOpen runs NHWC natively (no
            # batched_transpose kernels) and the fused NHWC hot loop gets
            # zero-copy physical views.
            self.model = self.model.to(memory_format=torch.channels_last)
            # MIOpen's heuristic (immediate) mode sometimes picks
            # no-workspace CK fallback solvers (~200 us/conv on the
            # encoders); benchmark mode runs a real find with workspace
            # during warmup and caches the fast igemm solutions.
            torch.backends.cudnn.benchmark = True
        self.use_graph = use_graph and self.device.type == "cuda"
        self.max_graphs = max_graphs
        self._graphs: Dict[Tuple[int, int, int], tuple] = {}
        self.last_info = None   # ConvergenceInfo of the last call

    @torch.no_grad()
    def __call__(self, image1: torch.Tensor, image2: torch.Tensor,
                 iters: Optional[int] = None,
                 flow_init=None, bidirectional: bool = False,
                 converge=None):
        """flow_init: [B,2,H/8,W/8] warm-start at 1/8 resolution (official
        RAFT 2-view warm start; the BASELINE EPE anchor is quoted with it).
        bidirectional=True returns the unpadded pair (flow_fw, flow_bw)
        from one shared pass; flow_init is then None or a pair.
        converge: a raft_amd.Convergence turns ``iters`` into a budget (the
        loop stops once its update is within the tolerance); the call's
        ConvergenceInfo is kept in ``self.last_info``."""
        iters = iters if iters is not None else self.iters
        n_run = iters if iters is not None else self.model.cfg.iters
        self.last_info = ConvergenceInfo(iters_run=n_run)
        image1 = image1.to(self.device, self.dtype, non_blocking=True)
        image2 = image2.to(self.device, self.dtype, non_blocking=True)
        image1, hw = pad8(image1)
        image2, _ = pad8(image2)
        if self.device.type == "cuda":
            image1 = image1.contiguous(memory_format=torch.channels_last)
            image2 = image2.contiguous(memory_format=torch.channels_last)
        from raft_amd.models import fused
        fusable = fused.can_fuse(self.model, image1)
        if fusable:
            # fused path: loop_graph None = AUTO (the fused loop captures
            # at iters <= 16, runs eager above — replay serializes the
            # two-stream overlap that pays at long iteration counts)
            self.model._fused_use_graph = self.loop_graph
        if bidirectional:
            # off the fused path this skips whole-model graph capture, as
            # flow_init calls do
            fw, bw, self.last_info = self.model(
                image1, image2, iters=iters, flow_init=flow_init,
                bidirectional=True, converge=converge, return_info=True)
            return unpad(fw, hw), unpad(bw, hw)
        if converge is not None:
            # a gated call decides its length on the host: like flow_init
            # calls it bypasses the whole-call graph
            out, self.last_info = self.model(
                image1, image2, iters=iters, flow_init=flow_init,
                converge=converge, return_info=True)
            return unpad(out, hw)
        if fusable:
            return unpad(self.model(image1, image2, iters=iters,
                                    flow_init=flow_init), hw)
        if not self.use_graph or flow_init is not None:
            return unpad(self.model(image1, image2, iters=iters,
                                    flow_init=flow_init), hw)

        key = (image1.shape[0], image1.shape[2], image1.shape[3],
               iters if iters is not None else -1)
        entry = self._graphs.get(key)
        if entry is None:
            if len(self._graphs) >= self.max_graphs:
                # bucket cache full: run eagerly rather than evict (captured
                # graphs own their memory pools)
                return unpad(self.model(image1, image2, iters=iters), hw)
            entry = self._capture(image1, image2, iters)
            self._graphs[key] = entry
        graph, in1, in2, out = entry
        in1.copy_(image1)
        in2.copy_(image2)
        graph.replay()
        return unpad(out, hw)

    @torch.no_grad()
    def bidirectional(self, image1: torch.Tensor, image2: torch.Tensor,
                      iters: Optional[int] = None, flow_init=None,
                      alpha1: float = 0.01, alpha2: float = 0.5,
                      converge=None) -> BidirectionalFlow:
        """Both flows plus forward-backward occlusion masks. The masks are
        computed on the unpadded flows, so "leaves the frame" means the
        real frame, not the pad8 canvas."""
        from raft_amd import ops
        fw, bw = self(image1, image2, iters=iters, flow_init=flow_init,
                      bidirectional=True, converge=converge)
        occ_fw, occ_bw = ops.fb_consistency(fw.contiguous(), bw.contiguous(),
                                            alpha1, alpha2)
        return BidirectionalFlow(fw, bw, occ_fw, occ_bw)

    @torch.no_grad()
    def interpolate(self, image1: torch.Tensor, image2: torch.Tensor,
                    times=(0.5,), iters: Optional[int] = None,
                    alpha1: float = 0.01, alpha2: float = 0.5,
                    converge=None) -> torch.Tensor:
        """Frames between ``image1`` (t=0) and ``image2`` (t=1) at the
        given times in [0, 1]: one ``bidirectional`` pass, then one
        ops.interpolate_frame call per time. Returns [T,B,C,H,W] fp32 in
        the value range of the inputs (as the engine's dtype holds them).
        The op runs on the unpadded images and flows, so "inside the
        frame" means the real frame, not the pad8 canvas."""
        times = _check_times(times)
        image1 = image1.to(self.device, self.dtype, non_blocking=True)
        image2 = image2.to(self.device, self.dtype, non_blocking=True)
        bidir = self.bidirectional(image1, image2, iters=iters,
                                   alpha1=alpha1, alpha2=alpha2,
                                   converge=converge)
        return interpolate_between(image1, image2, bidir, times)

    def stream(self, warm: bool = True, bidirectional: bool = False,
               iters: Optional[int] = None, alpha1: float = 0.01,
               alpha2: float = 0.5, converge=None):
        """A VideoFlowSession over this engine: push frames one at a time,
        get the flow from the previous frame to each new one. Every frame
        is encoded once, and ``warm`` starts each pair from the previous
        low-resolution flow projected forward (ops.forward_project).
        alpha1/alpha2: occlusion constants of bidirectional sessions, as
        in ``bidirectional``. converge: a raft_amd.Convergence gating
        every pair of the session (``session.last_iters``)."""
        from raft_amd.engine.video import VideoFlowSession
        return VideoFlowSession(self, warm=warm, bidirectional=bidirectional,
                                iters=iters, alpha1=alpha1, alpha2=alpha2,
                                converge=converge)

    def _capture(self, image1, image2, iters):
        in1 = image1.clone()
        in2 = image2.clone()
        # warm up on a side stream (allocator + MIOpen find outside capture)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self.model(in1, in2, iters=iters)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = self.model(in1, in2, iters=iters)
        return graph, in1, in2, out


class Prefetcher:
    """Async host->device double-buffering on a dedicated HIP copy stream —
    the rebuild's equivalent of the reference's
    ``StagingInput(QueueInput(ds))`` (infer_raft.py:37): the next batch's
    H2D copy overlaps the current batch's compute.

    Wraps any iterable of (im1, im2) CPU tensor batches; yields device
    tensors. Pins host memory for true async copies.
    """

    def __init__(self, iterable, device: torch.device,
                 dtype: torch.dtype = torch.float32):
        self.source = iterable
        self.device = device
        self.dtype = dtype
        self.use_cuda = device.type == "cuda"
        self.copy_stream = torch.cuda.Stream() if self.use_cuda else None

    def __iter__(self):
        it = iter(self.source)
        if not self.use_cuda:
            for im1, im2 in it:
                yield im1.to(self.device, self.dtype), \
                    im2.to(self.device, self.dtype)
            return
        nxt = self._start_copy(it)
        while nxt is not None:
            torch.cuda.current_stream().wait_stream(self.copy_stream)
            cur = nxt[:2]
            # the tensors were produced on copy_stream; record them so the
            # allocator doesn't recycle while in use on the main stream
            for t in cur:
                t.record_stream(torch.cuda.current_stream())
            nxt = self._start_copy(it)
            yield cur

    def _start_copy(self, it):
        try:
            im1, im2 = next(it)
        except StopIteration:
            return None
        with torch.cuda.stream(self.copy_stream):
            d1 = im1.pin_memory().to(self.device, self.dtype,
                                     non_blocking=True)
            d2 = im2.pin_memory().to(self.device, self.dtype,
                                     non_blocking=True)
        return d1, d2


def run_mixed_batch(engine: InferenceEngine, pairs, iters=None,
                    converge=None, return_iters: bool = False):
    """Mixed-batch inference with per-sample dynamic H x W (BASELINE
    config 5): groups same-shape pairs into batches (one kernel-efficient
    call per shape group), preserves input order in the returned list.

    pairs: sequence of (im1, im2) tensors [3,H,W] or [1,3,H,W].
    converge: a raft_amd.Convergence; each shape group is gated on its
    own. return_iters=True also returns the executed iteration count of
    every pair (its group's), in input order.
    """
    norm = []
    for im1, im2 in pairs:
        if im1.dim() == 3:
            im1 = im1.unsqueeze(0)
            im2 = im2.unsqueeze(0)
        norm.append((im1, im2))
    groups = {}
    for idx, (im1, im2) in enumerate(norm):
        groups.setdefault(tuple(im1.shape[-2:]), []).append(idx)
    out = [None] * len(norm)
    ran = [None] * len(norm)
    for shape, idxs in groups.items():
        b1 = torch.cat([norm[i][0] for i in idxs], dim=0)
        b2 = torch.cat([norm[i][1] for i in idxs], dim=0)
        flows = engine(b1, b2, iters=iters, converge=converge)
        for j, i in enumerate(idxs):
            out[i] = flows[j:j + 1]
            ran[i] = engine.last_info.iters_run
    return (out, ran) if return_iters else out
