"""Autograd-wrapped hot ops: HIP kernels on GPU, torch_ref elsewhere.

Each op dispatches on the input's device:
  * CUDA/HIP tensor  -> hand-written gfx950 kernel from the in-tree
    extension (required; loud failure if unbuilt — see raft_amd.ops).
  * CPU tensor       -> raft_amd.ops.torch_ref (plain PyTorch, autograd-native).

The HIP forward/backward pairs are wrapped in torch.autograd.Function so the
training path (config 3, DP=8) backprops through them.  Plain GEMM backward
passes go through torch.matmul (rocBLAS/hipBLASLt) — library GEMMs are the
sanctioned path for non-fused matmuls.
"""
from __future__ import annotations

import math
import os
from typing import List

import torch

from raft_amd.ops import torch_ref


def _use_hip(t: torch.Tensor) -> bool:
    if not t.is_cuda:
        return False
    if os.environ.get("RAFT_AMD_FORCE_TORCH", "0") == "1":
        return False
    from raft_amd.ops import require_hip
    require_hip()  # loud failure if the extension is missing on GPU
    return True


class _CorrVolume(torch.autograd.Function):
    """C = F1·F2ᵀ/sqrt(c): HIP MFMA forward, torch.matmul backward.

    bf16 inputs (the autocast training path) run the bf16 NHWC NT-GEMM
    kernel — fp32 accumulate, fp32 volume out — and a bf16 matmul
    backward; the f32-exact MFMA kernel serves fp32 inputs (r2: the f32
    kernel was 2.85 ms/call at the config-3 shape vs ~0.4 ms bf16, and
    training numerics are autocast-bf16 anyway)."""

    @staticmethod
    def forward(ctx, fmap1, fmap2):
        from raft_amd.ops import require_hip
        hip = require_hip()
        C = fmap1.shape[1]
        if fmap1.dtype == torch.bfloat16 and C % 64 == 0:
            # channels-last tensors make this permute+contiguous a no-op.
            # bf16 volume out (r2): halves the pyramid, the lookup reads
            # AND the 12-iteration gradient-accumulation traffic
            f1p = fmap1.permute(0, 2, 3, 1).contiguous()
            f2p = fmap2.permute(0, 2, 3, 1).contiguous()
            corr = hip.corr_volume_nhwc(f1p, f2p, True)
        else:
            corr = hip.corr_volume(fmap1.contiguous(), fmap2.contiguous())
        ctx.save_for_backward(fmap1, fmap2)
        return corr

    @staticmethod
    def backward(ctx, grad_corr):
        fmap1, fmap2 = ctx.saved_tensors
        B, C, H, W = fmap1.shape
        scale = 1.0 / math.sqrt(C)
        bf = fmap1.dtype == torch.bfloat16
        g = grad_corr.reshape(B, H * W, H * W)
        g = (g.to(torch.bfloat16) if bf else g.float()) * scale
        f1 = fmap1.reshape(B, C, H * W)
        f2 = fmap2.reshape(B, C, H * W)
        f1 = f1 if bf else f1.float()
        f2 = f2 if bf else f2.float()
        # dF1 = dC · F2 ; dF2 = dCᵀ · F1   (both [B, HW, C] -> back to NCHW)
        g1 = torch.matmul(g, f2.transpose(1, 2))       # [B, HW, C]
        g2 = torch.matmul(g.transpose(1, 2), f1.transpose(1, 2))
        g1 = g1.transpose(1, 2).reshape(B, C, H, W).to(fmap1.dtype)
        g2 = g2.transpose(1, 2).reshape(B, C, H, W).to(fmap2.dtype)
        return g1, g2


def corr_volume(fmap1: torch.Tensor, fmap2: torch.Tensor) -> torch.Tensor:
    if _use_hip(fmap1):
        return _CorrVolume.apply(fmap1, fmap2)
    return torch_ref.corr_volume(fmap1, fmap2)


class _CorrPool2x(torch.autograd.Function):
    """2x2/2 avg-pool (TF VALID) over the target dims of the volume."""

    @staticmethod
    def forward(ctx, corr):
        from raft_amd.ops import require_hip
        ctx.in_shape = corr.shape
        if corr.dtype == torch.bfloat16:
            return require_hip().corr_pool2x_bf16(corr.contiguous())
        return require_hip().corr_pool2x(corr.contiguous())

    @staticmethod
    def backward(ctx, grad_out):
        B, HW, H2, W2 = ctx.in_shape
        g = grad_out * 0.25
        g = g.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)
        if g.shape[-2] < H2 or g.shape[-1] < W2:  # VALID drops odd tails
            pad_h = H2 - g.shape[-2]
            pad_w = W2 - g.shape[-1]
            g = torch.nn.functional.pad(g, (0, pad_w, 0, pad_h))
        return g


def corr_pyramid(fmap1: torch.Tensor, fmap2: torch.Tensor,
                 num_levels: int = 4) -> List[torch.Tensor]:
    """Build volume + pooled pyramid (model_utils.py:199-221)."""
    corr = corr_volume(fmap1, fmap2)
    if _use_hip(corr):
        levels = [corr]
        for _ in range(num_levels - 1):
            last = levels[-1]
            if last.shape[-2] < 2 or last.shape[-1] < 2:
                levels.append(last)
            else:
                levels.append(_CorrPool2x.apply(last))
        return levels
    return torch_ref.corr_pyramid_pool(corr, num_levels)


class _CorrLookup(torch.autograd.Function):
    """(2r+1)^2-tap x L-level bilinear window gather (K3)."""

    @staticmethod
    def forward(ctx, coords, radius, *levels):
        from raft_amd.ops import require_hip
        out = require_hip().corr_lookup(list(levels), coords.contiguous(),
                                        radius)
        ctx.save_for_backward(coords)
        ctx.radius = radius
        ctx.level_shapes = [tuple(l.shape) for l in levels]
        ctx.level_dtypes = [l.dtype for l in levels]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from raft_amd.ops import require_hip
        (coords,) = ctx.saved_tensors
        grads = require_hip().corr_lookup_backward(
            grad_out.contiguous(), coords.contiguous(), ctx.radius,
            [list(s) for s in ctx.level_shapes])
        grads = [g.to(dt) for g, dt in zip(grads, ctx.level_dtypes)]
        # coords are detached in the RAFT loop (RAFT.py:93) — no coord grad.
        return (None, None, *grads)


class _CorrLookupNHWC(torch.autograd.Function):
    """Training-path lookup (r2): the NHWC kernel with bf16 tap output.

    The fp32 NCHW forward cost 650 us/call at the config-3 shape AND its
    output was immediately cast to bf16 (12 big aten::copy_ per step);
    the NHWC output permutes to a channels-last NCHW view for free, and
    the wave backward consumes the NHWC bf16 grad without the re-layout
    copy."""

    @staticmethod
    def forward(ctx, coords, radius, *levels):
        from raft_amd.ops import require_hip
        C = len(levels) * (2 * radius + 1) ** 2
        out = require_hip().corr_lookup_nhwc(
            list(levels), coords.contiguous(), radius, C, True, None,
            None, 0)
        ctx.save_for_backward(coords)
        ctx.radius = radius
        ctx.level_shapes = [tuple(l.shape) for l in levels]
        ctx.level_dtypes = [l.dtype for l in levels]
        return out                       # [B, H, W, C] bf16

    @staticmethod
    def backward(ctx, grad_out):
        from raft_amd.ops import require_hip
        (coords,) = ctx.saved_tensors
        bf = ctx.level_dtypes[0] == torch.bfloat16
        grads = require_hip().corr_lookup_backward(
            grad_out.permute(0, 3, 1, 2), coords.contiguous(), ctx.radius,
            [list(s) for s in ctx.level_shapes], bf)
        grads = [g.to(dt) for g, dt in zip(grads, ctx.level_dtypes)]
        return (None, None, *grads)


def corr_lookup(pyramid: List[torch.Tensor], coords: torch.Tensor,
                radius: int) -> torch.Tensor:
    if _use_hip(coords):
        # NHWC kernel path: required for bf16 pyramids (the NCHW family is
        # fp32-exact only) and preferred for training (bf16 taps,
        # channels-last output view, NHWC wave backward)
        training = torch.is_grad_enabled() and \
            any(p.requires_grad for p in pyramid)
        if radius <= 4 and (pyramid[0].dtype == torch.bfloat16 or training):
            out = _CorrLookupNHWC.apply(coords, radius, *pyramid)
            return out.permute(0, 3, 1, 2)   # channels-last NCHW view
        return _CorrLookup.apply(coords, radius, *pyramid)
    return torch_ref.corr_lookup(pyramid, coords, radius)


class _GruGates(torch.autograd.Function):
    """Fused pointwise h' = (1-σ(z))h + σ(z)tanh(q) with analytic backward."""

    @staticmethod
    def forward(ctx, h, z_act, q_act):
        from raft_amd.ops import require_hip
        # layouts are resolved in the binding (identical dense strides run
        # as-is, incl. channels-last — no re-layout copies in the loop)
        out = require_hip().gru_gates_fwd(h, z_act, q_act)
        ctx.save_for_backward(h, z_act, q_act)
        return out

    @staticmethod
    def backward(ctx, grad_h_new):
        from raft_amd.ops import require_hip
        h, z_act, q_act = ctx.saved_tensors
        gh, gz, gq = require_hip().gru_gates_bwd(grad_h_new, h, z_act, q_act)
        return gh, gz, gq


def gru_gates(h: torch.Tensor, z_act: torch.Tensor,
              q_act: torch.Tensor) -> torch.Tensor:
    if _use_hip(h):
        return _GruGates.apply(h, z_act, q_act)
    return torch_ref.gru_gates(h, z_act, q_act)


class _ConvexUpsample(torch.autograd.Function):
    """8x convex upsample (K5): softmax over 9 taps fused into the kernel."""

    @staticmethod
    def forward(ctx, flow, mask):
        from raft_amd.ops import require_hip
        # layout dispatch lives in the binding (channels-last fast path)
        out = require_hip().convex_upsample(flow, mask)
        ctx.save_for_backward(flow, mask)
        return out

    @staticmethod
    def backward(ctx, grad_up):
        from raft_amd.ops import require_hip
        flow, mask = ctx.saved_tensors
        gf, gm = require_hip().convex_upsample_backward(
            grad_up.contiguous(), flow, mask)
        return gf, gm


def convex_upsample(flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    if _use_hip(flow):
        return _ConvexUpsample.apply(flow, mask)
    return torch_ref.convex_upsample(flow, mask)


def upflow8(flow: torch.Tensor) -> torch.Tensor:
    return torch_ref.upflow8(flow)


def fb_consistency(flow_fw: torch.Tensor, flow_bw: torch.Tensor,
                   alpha1: float = 0.01, alpha2: float = 0.5):
    """Forward-backward occlusion masks ``(occ_fw, occ_bw)``, each
    [B,1,H,W] bool (see torch_ref.fb_consistency). On GPU one kernel
    launch computes both directions; no autograd."""
    if _use_hip(flow_fw):
        from raft_amd.ops import require_hip
        fw, bw = flow_fw.detach(), flow_bw.detach()
        if fw.dtype != bw.dtype or fw.dtype not in (torch.float32,
                                                    torch.bfloat16):
            fw, bw = fw.float(), bw.float()
        (occ,) = require_hip().fb_consistency(fw.contiguous(),
                                              bw.contiguous(), alpha1,
                                              alpha2, False)
        B = fw.shape[0]
        occ = occ.bool()
        return occ[:B], occ[B:]
    return (torch_ref.fb_consistency(flow_fw, flow_bw, alpha1, alpha2),
            torch_ref.fb_consistency(flow_bw, flow_fw, alpha1, alpha2))


def forward_project(flow: torch.Tensor, direction: int = 1):
    """Forward projection of a flow field along itself (``direction=+1``)
    or against itself (``-1``): ``(projected [B,2,H,W] fp32, holes
    [B,1,H,W] bool)``. See torch_ref.forward_project for the definition;
    the GPU kernels match it bit for bit, are stream-ordered (no host
    sync) and graph-capturable. No autograd. As with every op here, a
    CUDA tensor without the built extension is an error, not a fall-back
    to the oracle; ``RAFT_AMD_FORCE_TORCH=1`` selects the oracle
    explicitly."""
    if direction not in (1, -1):
        raise ValueError(f"direction must be +1 or -1, got {direction}")
    if _use_hip(flow):
        from raft_amd.ops import require_hip
        if flow.dim() != 4 or flow.shape[1] != 2:
            raise ValueError(f"flow must be [B,2,H,W], got "
                             f"{tuple(flow.shape)}")
        out, holes = require_hip().forward_project(
            flow.detach().float().contiguous(), direction)
        return out, holes
    return torch_ref.forward_project(flow.detach(), direction)


def flow_residual_raw(prev: torch.Tensor, nxt: torch.Tensor, thr_sq: float,
                      out=None) -> torch.Tensor:
    """The HIP op behind ``flow_residual`` without the unpacking: a [B,2]
    int32 device tensor, column 0 the fp32 bits of max_sq, column 1 the
    count of cells above ``thr_sq``. prev/nxt are logical [B,2,H,W] fp32
    views — planar, or the permuted view of interleaved [B,H,W,2] coords —
    read in place. One memset and one kernel on the current stream, so a
    loop can launch it between iterations and read the result later.
    ``out`` reuses a result tensor."""
    from raft_amd.ops import require_hip
    return require_hip().flow_residual(prev.detach(), nxt.detach(),
                                       float(thr_sq), out)


def flow_residual(prev: torch.Tensor, nxt: torch.Tensor, thr_sq: float):
    """Per-sample size of a coords update: ``(max_sq [B] fp32, above [B]
    int64)`` — the largest squared displacement between ``prev`` and
    ``nxt`` ([B,2,H,W] fp32) and the number of cells whose squared
    displacement is not ``<= thr_sq``. See torch_ref.flow_residual for the
    definition; the GPU kernel matches it bit for bit, is stream-ordered
    (no host sync) and graph-capturable. No autograd. A CUDA tensor without
    the built extension is an error, not a fall-back to the oracle;
    ``RAFT_AMD_FORCE_TORCH=1`` selects the oracle explicitly."""
    if _use_hip(prev):
        if prev.dim() != 4 or prev.shape[1] != 2 or prev.shape != nxt.shape:
            raise ValueError(f"prev and nxt must both be [B,2,H,W], got "
                             f"{tuple(prev.shape)} and {tuple(nxt.shape)}")
        if prev.dtype != torch.float32 or nxt.dtype != torch.float32:
            prev, nxt = prev.float(), nxt.float()
        res = flow_residual_raw(prev, nxt, thr_sq)
        return (res[:, 0].contiguous().view(torch.float32),
                res[:, 1].to(torch.int64))
    return torch_ref.flow_residual(prev, nxt, thr_sq)


def interpolate_frame(im0: torch.Tensor, im1: torch.Tensor,
                      flow_fw: torch.Tensor, flow_bw: torch.Tensor,
                      occ_fw: torch.Tensor, occ_bw: torch.Tensor, t: float):
    """The frame at time ``t`` in [0, 1] between ``im0`` and ``im1`` from
    their bidirectional flows and occlusion masks (what
    ``InferenceEngine.bidirectional`` returns): ``(frame [B,C,H,W] fp32,
    flow_t0, flow_t1 [B,2,H,W] fp32, cover [B,1,H,W] uint8)``. See
    torch_ref.interpolate_frame for the definition; the GPU kernels match
    it bit for bit, are stream-ordered (no host sync) and
    graph-capturable. Images may be bf16 or fp32 (computed in fp32), masks
    bool. No autograd. A CUDA tensor without the built extension is an
    error, not a fall-back to the oracle; ``RAFT_AMD_FORCE_TORCH=1``
    selects the oracle explicitly."""
    t = torch_ref._check_interp_args(im0, im1, flow_fw, flow_bw, occ_fw,
                                     occ_bw, t)
    args = [a.detach() for a in (im0, im1, flow_fw, flow_bw)]
    if _use_hip(im0):
        from raft_amd.ops import require_hip
        im0, im1, fw, bw = (a.float().contiguous() for a in args)
        # a bool mask is one 0/1 byte per cell: reinterpret, no copy
        masks = [(m.contiguous().view(torch.uint8) if m.dtype == torch.bool
                  else (m != 0).view(torch.uint8)).detach()
                 for m in (occ_fw, occ_bw)]
        frame, ft0, ft1, cover = require_hip().interpolate_frame(
            im0, im1, fw, bw, masks[0], masks[1], t)
        return frame, ft0, ft1, cover
    return torch_ref.interpolate_frame(*args, occ_fw.detach(),
                                       occ_bw.detach(), t)
