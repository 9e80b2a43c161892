"""The RAFT model — re-design of networks/RAFT.py as an NCHW PyTorch module.

Capabilities vs the reference:
  * forward() supports inference (final flow) AND training (per-iteration
    upsampled predictions for the sequence loss) — the reference's train
    path was an unimplemented TODO (infer_raft.py);
  * dynamic batch / H / W (the reference hardwired (1, 432, 1024, 3),
    infer_raft.py:69). forward() itself requires H and W divisible by 8;
    padding to a multiple of 8 + cropping back (official-RAFT style) lives
    in raft_amd.engine.inference.InferenceEngine.pad8;
  * iters is a call-time argument (hard-coded 20 in networks/RAFT.py:33).

Numerics contract with the reference graph (networks/RAFT.py:53-134):
BGR input in [0,1], preprocess 2x-1, shared fnet for both frames, corr
pyramid 4 levels with 1/sqrt(c), context split -> tanh/relu, coords detached
each iteration, convex upsample (things) / align-corners upflow8 without the
x8 value scale (small — a deliberate reference quirk, see
ops.torch_ref.upflow8).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from raft_amd import ops
from raft_amd.convergence import Convergence, ConvergenceInfo, Gate
from raft_amd.models.encoders import BasicEncoder, SmallEncoder
from raft_amd.models.layers import coords_grid
from raft_amd.models.update import BasicUpdateBlock, SmallUpdateBlock


@dataclass
class RaftConfig:
    """Model hyper-parameters (networks/RAFT.py:26-43)."""
    small: bool = False
    dropout: float = 0.0
    iters: int = 20                    # reference default (RAFT.py:33)
    corr_levels: int = 4
    # raft-things values; __post_init__ applies the small overrides
    corr_radius: int = 4
    hidden_dim: int = 128
    context_dim: int = 128
    fnet_dim: int = 256
    # Reference quirk: the small path upsamples flow WITHOUT the x8 value
    # scale (RAFT.py:104-105). True restores official-RAFT scaling.
    scale_small_upflow: bool = False

    def __post_init__(self):
        if self.small:
            self.corr_radius = 3       # RAFT.py:38-41
            self.hidden_dim = 96
            self.context_dim = 64
            self.fnet_dim = 128

    @property
    def corr_channels(self) -> int:
        return self.corr_levels * (2 * self.corr_radius + 1) ** 2


class RAFT(nn.Module):
    def __init__(self, cfg: Optional[RaftConfig] = None, **kwargs):
        super().__init__()
        if cfg is None:
            cfg = RaftConfig(**kwargs)
        self.cfg = cfg
        hd, cd = cfg.hidden_dim, cfg.context_dim
        if cfg.small:
            self.fnet = SmallEncoder(output_dim=128, norm_fn="instance",
                                     dropout=cfg.dropout)
            self.cnet = SmallEncoder(output_dim=hd + cd, norm_fn="none",
                                     dropout=cfg.dropout)
            self.update_block = SmallUpdateBlock(cfg.corr_channels, hd, cd)
        else:
            self.fnet = BasicEncoder(output_dim=256, norm_fn="instance",
                                     dropout=cfg.dropout)
            self.cnet = BasicEncoder(output_dim=hd + cd, norm_fn="batch",
                                     dropout=cfg.dropout)
            self.update_block = BasicUpdateBlock(cfg.corr_channels, hd, cd)

    # ------------------------------------------------------------------
    @staticmethod
    def preprocess(img: torch.Tensor) -> torch.Tensor:
        """[0,1] -> [-1,1] (networks/RAFT.py:53-59). Input is BGR — the
        converted weights expect BGR channel order (RAFT.py:13)."""
        return 2.0 * img - 1.0

    def initialize_flow(self, img: torch.Tensor):
        """Identity coords at 1/8 resolution (networks/RAFT.py:111-117)."""
        B, _, H, W = img.shape
        coords0 = coords_grid(B, H // 8, W // 8, device=img.device,
                              dtype=torch.float32)
        return coords0, coords0.clone()

    # ------------------------------------------------------------------
    def forward(self, image1: torch.Tensor, image2: torch.Tensor,
                iters: Optional[int] = None, flow_init: Optional[torch.Tensor] = None,
                test_mode: bool = True, bidirectional: bool = False,
                return_low: bool = False, converge=None,
                return_info: bool = False):
        """Run the recurrent refinement.

        image1/image2: [B, 3, H, W] BGR in [0,1] (H, W divisible by 8 —
        use raft_amd.engine.inference.pad8 for arbitrary sizes).
        Returns the final upsampled flow [B, 2, H, W] when test_mode, else
        the list of per-iteration upsampled flow predictions (for the
        sequence loss — designed from the RAFT paper; the reference has no
        training path).

        bidirectional=True (test_mode only) returns ``(flow_fw, flow_bw)``
        — image1->image2 and image2->image1 — from ONE shared pass: fnet
        already sees both frames, the backward correlation volume is the
        transpose of the forward one, and the loop runs both directions
        as one batch of 2B. flow_init is then None or ``(init_fw, init_bw)``.

        return_low=True (test_mode only) also returns the final
        1/8-resolution flow [B,2,H/8,W/8] fp32 — the quantity flow_init
        seeds, so a video session can project it into the next pair's
        warm start: ``(up, low)``, or ``(fw, bw, low_fw, low_bw)`` when
        bidirectional.

        converge=Convergence(...) (test_mode only) makes ``iters`` a
        budget: the loop measures its own update every few iterations
        (ops.flow_residual) and, once it is within the tolerance, runs one
        final iteration and stops — see raft_amd.convergence. The result
        equals the ungated call with ``iters`` set to the executed count,
        bit for bit. return_info=True (test_mode only) appends the
        ConvergenceInfo (iterations run, the checks taken) as the last
        returned element.
        """
        iters = iters if iters is not None else self.cfg.iters
        if iters < 1:
            raise ValueError(f"iters must be >= 1, got {iters}")
        if (converge is not None or return_info) and not test_mode:
            raise ValueError("converge / return_info need test_mode=True")
        if converge is not None and not isinstance(converge, Convergence):
            raise ValueError(f"converge must be a Convergence or None, got "
                             f"{type(converge).__name__}")
        if return_low and not test_mode:
            raise ValueError("return_low=True needs test_mode=True")
        if bidirectional:
            if not test_mode:
                raise ValueError("bidirectional=True needs test_mode=True "
                                 "(training is unidirectional)")
            if flow_init is not None:
                if not (isinstance(flow_init, (tuple, list))
                        and len(flow_init) == 2):
                    raise ValueError("bidirectional flow_init must be None "
                                     "or a pair (init_fw, init_bw)")
                flow_init = torch.cat([flow_init[0], flow_init[1]], dim=0)

        # MI355X fast path: whole refinement loop on the fused NHWC bf16
        # kernels (inference only; numerics-tested vs this eager path).
        if test_mode:
            from raft_amd.models import fused
            if fused.can_fuse(self, image1):
                return fused.get_fused(self).run(image1, image2, iters,
                                                 flow_init, bidirectional,
                                                 return_low, converge,
                                                 return_info)

        img1 = self.preprocess(image1)
        img2 = self.preprocess(image2)

        # shared-weight fnet on both frames in one batched call
        # (reference shares via tf.AUTO_REUSE, model_utils.py:69)
        fmaps = self.fnet(torch.cat([img1, img2], dim=0))
        fmap1, fmap2 = torch.chunk(fmaps, 2, dim=0)
        if bidirectional:
            # both directions as one batch of 2B: [fw | bw]
            fmap1, fmap2 = fmaps, torch.cat([fmap2, fmap1], dim=0)
            img1 = torch.cat([img1, img2], dim=0)

        pyramid = ops.corr_pyramid(fmap1, fmap2, self.cfg.corr_levels)

        cnet = self.cnet(img1)
        net, inp = torch.split(cnet, [self.cfg.hidden_dim,
                                      self.cfg.context_dim], dim=1)
        net = torch.tanh(net)
        inp = torch.relu(inp)
        if image1.is_cuda:
            # keep every loop tensor channels-last: a single NCHW straggler
            # makes each cat fall back to NCHW and every conv re-layout its
            # inputs (measured ~12 re-layout copies/iter in training)
            net = net.contiguous(memory_format=torch.channels_last)
            inp = inp.contiguous(memory_format=torch.channels_last)

        coords0, coords1 = self.initialize_flow(img1)
        if flow_init is not None:
            coords1 = coords1 + flow_init

        flow_predictions: List[torch.Tensor] = []
        up_mask = None
        if converge is not None:
            # the gated loop is a path of its own (test mode only): the
            # ungated loop below, training included, is not touched by it
            coords1, up_mask, info = self._gated_loop(
                pyramid, net, inp, coords0, coords1, iters, converge,
                image1.is_cuda)
            low = coords1 - coords0
            return self._pack(self._upsample(low, up_mask), low,
                              image1.shape[0], bidirectional, return_low,
                              info if return_info else None)

        for _ in range(iters):
            coords1 = coords1.detach()        # RAFT.py:93
            corr = ops.corr_lookup(pyramid,
                                   coords1.permute(0, 2, 3, 1).contiguous(),
                                   self.cfg.corr_radius)
            corr = corr.to(net.dtype)
            flow = (coords1 - coords0).to(net.dtype)
            if image1.is_cuda:
                flow = flow.contiguous(memory_format=torch.channels_last)
            net, up_mask, delta_flow = self.update_block(net, inp, corr, flow)
            coords1 = coords1 + delta_flow.float()
            if not test_mode:
                flow_predictions.append(
                    self._upsample(coords1 - coords0, up_mask))

        if not test_mode:
            return flow_predictions
        low = coords1 - coords0
        up = self._upsample(low, up_mask)
        return self._pack(up, low, image1.shape[0], bidirectional, return_low,
                          ConvergenceInfo(iters_run=iters) if return_info
                          else None)

    @staticmethod
    def _pack(up, low, B, bidirectional, return_low, info):
        """forward()'s test-mode return value: the flow(s), then the
        low-resolution flow(s) (return_low), then info (return_info)."""
        res = (up[:B], up[B:]) if bidirectional else (up,)
        if return_low:
            res += (low[:B], low[B:]) if bidirectional else (low,)
        if info is not None:
            res += (info,)
        return res if len(res) > 1 else res[0]

    def _gated_loop(self, pyramid, net, inp, coords0, coords1, budget,
                    converge, channels_last):
        """The test-mode refinement loop under a convergence gate
        (raft_amd.convergence): the iterations of forward()'s loop, with
        the coords update measured (ops.flow_residual on the planar
        coords) after the check iterations and one final iteration after
        convergence. Returns (coords1, up_mask, ConvergenceInfo)."""
        gate = Gate(converge, budget, coords1.shape[2] * coords1.shape[3])
        up_mask = None
        last = False                # converged: this iteration is the final
        for it in range(1, budget + 1):
            gate.info.iters_run = it
            prev = coords1 = coords1.detach()
            corr = ops.corr_lookup(pyramid,
                                   coords1.permute(0, 2, 3, 1).contiguous(),
                                   self.cfg.corr_radius)
            corr = corr.to(net.dtype)
            flow = (coords1 - coords0).to(net.dtype)
            if channels_last:
                flow = flow.contiguous(memory_format=torch.channels_last)
            net, up_mask, delta_flow = self.update_block(net, inp, corr, flow)
            coords1 = coords1 + delta_flow.float()
            if last:
                break
            if gate.wants(it):
                max_sq, above = ops.flow_residual(prev, coords1, gate.thr_sq)
                last = gate.record(it, max_sq.cpu().numpy(),
                                   above.cpu().numpy())
        return coords1, up_mask, gate.info

    def _upsample(self, flow: torch.Tensor, up_mask: Optional[torch.Tensor]):
        if self.cfg.small:
            up = ops.upflow8(flow)            # no x8 value scale: ref quirk
            if self.cfg.scale_small_upflow:
                up = 8.0 * up
            return up
        return ops.convex_upsample(flow.to(up_mask.dtype), up_mask)

    # FLOP reporting lives in raft_amd.engine.profiler.count_model_flops
    # (the reference's flops mode crashes on an arity bug, RAFT.py:144).
