"""Streaming video flow: one encoder pass per frame and RAFT's projected
warm start.

A pairwise call encodes every interior frame of a video twice — as the
second image of one pair and the first of the next. A session keeps the
newest frame's feature map and context across calls (FusedRaft.encode /
run_pair), so each push encodes only the new frame, and it carries the
1/8-resolution flow forward: the next pair starts from that flow
projected along itself (ops.forward_project, RAFT's forward_interpolate),
the backward direction from its own flow projected against itself.

Off the fused path (CPU, fp32, RAFT_AMD_NO_FUSE) the session keeps the
previous padded frame and calls the model pairwise: same interface and
warm start, no reuse.
"""
from __future__ import annotations

from typing import Optional

import torch

from raft_amd.engine.inference import (BidirectionalFlow,
                                       interpolate_between, pad8, unpad)


class VideoFlowSession:
    """Flow over a frame stream; build with ``InferenceEngine.stream``.

    ``push(frame)`` returns None for the first frame, then the flow from
    the previous frame to the pushed one, unpadded, [B,2,H,W] — a
    BidirectionalFlow (flows + occlusion masks) for bidirectional
    sessions. Returned tensors stay valid after later pushes.

    ``converge`` (a raft_amd.Convergence) gates the refinement loop of every
    pair; ``last_iters`` is the number of iterations the last pair ran and
    ``last_info`` its ConvergenceInfo (set for ungated sessions too).

    ``between(times)`` of a bidirectional session returns the in-between
    frames of the last two pushed frames (ops.interpolate_frame).
    """

    def __init__(self, engine, warm: bool = True,
                 bidirectional: bool = False, iters: Optional[int] = None,
                 alpha1: float = 0.01, alpha2: float = 0.5, converge=None):
        self.engine = engine
        self.converge = converge
        self.warm = warm
        self.bidirectional = bidirectional
        self.iters = iters if iters is not None else engine.iters
        self.alpha1 = alpha1
        self.alpha2 = alpha2
        self.reset()

    def reset(self) -> None:
        """Drop all cached state: the next push starts a new sequence."""
        self._shape = None      # (B, padded H, padded W) of the cached frame
        self._runner = None     # FusedRaft the cache belongs to, or None
        self._prev = None       # fused: (fmap, context); fallback: frame
        self.last_low = None    # previous pair's 1/8 flow (fw) — warm seed
        self.last_low_bw = None
        self._frames = (None, None)   # last two unpadded frames (references)
        self._last_bidir = None       # their BidirectionalFlow
        self.last_iters = None        # iterations the last pair ran
        self.last_info = None         # its ConvergenceInfo

    # ------------------------------------------------------------------
    def _flow_init(self):
        """Warm start for the next pair, or None: (fw[, bw]) projections of
        the previous pair's low-resolution flows."""
        if not self.warm or self.last_low is None:
            return None
        from raft_amd import ops
        fw = ops.forward_project(self.last_low, 1)[0]
        if not self.bidirectional:
            return fw
        return fw, ops.forward_project(self.last_low_bw, -1)[0]

    @torch.no_grad()
    def push(self, frame: torch.Tensor):
        from raft_amd import ops
        from raft_amd.models import fused
        eng = self.engine
        model = eng.model
        frame = frame.to(eng.device, eng.dtype, non_blocking=True)
        raw = frame
        frame, hw = pad8(frame)
        if eng.device.type == "cuda":
            frame = frame.contiguous(memory_format=torch.channels_last)

        runner = None
        if fused.can_fuse(model, frame):
            model._fused_use_graph = eng.loop_graph
            # rebuilt when the weights changed: feature maps cached from
            # the old weights must not meet the new ones
            runner = fused.get_fused(model)
        if self._prev is not None and runner is not self._runner:
            self.reset()
        shape = (frame.shape[0], frame.shape[2], frame.shape[3])
        if self._shape is not None and shape != self._shape:
            raise ValueError(
                f"frame of batch {shape[0]}, padded size {shape[1]}x"
                f"{shape[2]} pushed into a session holding batch "
                f"{self._shape[0]}, padded size {self._shape[1]}x"
                f"{self._shape[2]}; call reset() to start a new sequence")

        iters = self.iters if self.iters is not None else model.cfg.iters
        init = self._flow_init()
        bidir = self.bidirectional
        if runner is not None:
            cur = runner.encode(frame, want_context=True)
            if self._prev is None:
                res = None
            else:
                if bidir and init is not None:
                    init = torch.cat(init, dim=0)
                res = runner.run_pair(
                    self._prev[0], cur[0], self._prev[1],
                    cur[1] if bidir else None, iters, init, bidir,
                    return_low=True, converge=self.converge,
                    return_info=True)
        else:
            cur = frame
            res = None if self._prev is None else model(
                self._prev, frame, iters=iters, flow_init=init,
                bidirectional=bidir, return_low=True,
                converge=self.converge, return_info=True)
        self._prev, self._runner, self._shape = cur, runner, shape
        self._frames = (self._frames[1], raw)
        if res is None:
            return None
        res, self.last_info = res[:-1], res[-1]
        self.last_iters = self.last_info.iters_run
        eng.last_info = self.last_info

        # clone: a captured loop hands out its static output buffers
        n = 2 if bidir else 1
        flows = [unpad(t, hw).clone(memory_format=torch.contiguous_format)
                 for t in res[:n]]
        lows = [t.float().clone(memory_format=torch.contiguous_format)
                for t in res[n:]]
        self.last_low = lows[0]
        if not bidir:
            return flows[0]
        self.last_low_bw = lows[1]
        # on the unpadded (contiguous) flows, as engine.bidirectional does
        occ_fw, occ_bw = ops.fb_consistency(flows[0], flows[1], self.alpha1,
                                            self.alpha2)
        self._last_bidir = BidirectionalFlow(flows[0], flows[1], occ_fw,
                                             occ_bw)
        return self._last_bidir

    @torch.no_grad()
    def between(self, times=(0.5,)) -> torch.Tensor:
        """Frames [T,B,C,H,W] fp32 between the last two pushed frames at
        the given times in [0, 1] (0 = the older frame), from the flows
        and masks the last push returned."""
        if not self.bidirectional:
            raise ValueError(
                "between() needs a bidirectional session (backward flow "
                "and occlusion masks): build it with "
                "stream(bidirectional=True)")
        if self._last_bidir is None:
            raise RuntimeError("between() needs two pushed frames: push a "
                               "second frame first")
        return interpolate_between(self._frames[0], self._frames[1],
                                   self._last_bidir, times)
