"""Fused NHWC bf16 inference path (MI355X-native hot loop).

Runs the whole RAFT refinement loop on the hand-written gfx950 kernels
(raft_amd/ops/csrc/{corr_nhwc,fconv}.hip), operating on *physical NHWC*
tensors throughout:

  encoders (PyTorch/MIOpen, channels-last)  ->  bf16 NT-GEMM corr volume
  -> bf16 pooled pyramid -> per iteration: NHWC lookup fused with the
  motion encoder's first corr conv (the taps never leave LDS) -> rest of
  the motion encoder (4 fconvs, the flow branch on a second stream from
  the start of the iteration, writing into the reusable GRU input buffer)
  -> fused SepConvGRU (2 fconv pairs per direction with the gate math in
  the epilogue) -> fused flow head + mask head -> coords update, which
  also writes the next iteration's flow input -> final convex upsample.

This path is inference-only (no autograd) and numerics-matched to the
eager model (tests/test_fused.py compares against the fp32 golden path).
Training keeps the autograd ops.

Weight packing: conv weights [N, Cin, kh, kw] -> [kh*kw, N, Cin_pad] bf16
(c-contiguous = the MFMA B-fragment order); the mask head's x0.25 scale
(model_utils.py:183) is folded into its packed weights and bias.
"""
from __future__ import annotations

from typing import Optional

import torch

from raft_amd.convergence import ConvergenceInfo, Gate

ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = 0, 1, 2, 3


def _pad8(c: int) -> int:
    return (c + 7) // 8 * 8


def pack_conv(conv: torch.nn.Conv2d, pad_cin: Optional[int] = None,
              scale: float = 1.0):
    """[N, Cin, kh, kw] -> ([taps, N, Cin_pad] bf16 contiguous, bias fp32)."""
    w = conv.weight.detach().float()
    N, Cin, kh, kw = w.shape
    cp = pad_cin if pad_cin is not None else Cin
    wp = w.new_zeros(N, cp, kh, kw)
    wp[:, :Cin] = w * scale
    wp = wp.permute(2, 3, 0, 1).reshape(kh * kw, N, cp)
    wp = wp.contiguous().to(device=conv.weight.device, dtype=torch.bfloat16)
    if conv.bias is not None:
        bias = (conv.bias.detach().float() * scale).contiguous()
    else:
        bias = torch.zeros(N, device=conv.weight.device)
    return wp, bias, kh, kw


def pack_zr(convz: torch.nn.Conv2d, convr: torch.nn.Conv2d):
    """Stack [Wz; Wr] along N for the fused z/r gate kernel."""
    wz, bz, kh, kw = pack_conv(convz)
    wr, br, _, _ = pack_conv(convr)
    return torch.cat([wz, wr], dim=1).contiguous(), \
        torch.cat([bz, br]).contiguous(), kh, kw


class _FC:
    """A packed conv ready for fconv_plain."""

    def __init__(self, conv, pad_cin=None, scale=1.0):
        self.wp, self.bias, self.kh, self.kw = pack_conv(conv, pad_cin, scale)

    def __call__(self, hip, in1, in2=None, act=ACT_RELU, out=None, n_off=0,
                 in1_off=0, in1_len=0, stride=1, res=None):
        return hip.fconv_plain(in1, in2, self.wp, self.bias, self.kh,
                               self.kw, act, out, n_off, in1_off, in1_len,
                               -1, -1, stride, res)


class _GruDir:
    """One GRU direction: z/r gate conv pair + candidate conv over [h | x].

    ctx > 0 hoists the context channels out of the loop. x = [inp(ctx) |
    rest] and inp is the same in every iteration, so the packed columns
    [W_h | W_inp | W_rest] of each conv are split: ``precompute`` runs the
    W_inp part of z, r and q once per pair as one stacked conv (fp32 out,
    biases folded in), and the per-iteration convs read only [h | rest] —
    the rest slice of x in place — starting from their slice of that
    term."""

    def __init__(self, convz, convr, convq, ctx: int = 0):
        self.zr_w, self.zr_b, self.kh, self.kw = pack_zr(convz, convr)
        self.q_w, self.q_b, _, _ = pack_conv(convq)
        self.ctx = ctx
        self.hd = hd = self.q_w.shape[1]
        if ctx:
            full = torch.cat([self.zr_w, self.q_w], dim=1)  # rows z, r, q
            self.pre_w = full[..., hd:hd + ctx].contiguous()
            self.pre_b = torch.cat([self.zr_b, self.q_b]).contiguous()
            loop = torch.cat([full[..., :hd], full[..., hd + ctx:]], dim=-1)
            self.zr_w = loop[:, :2 * hd].contiguous()
            self.q_w = loop[:, 2 * hd:].contiguous()
            self.zr_b = self.q_b = None          # live in pre

    def precompute(self, hip, x):
        """[B,H,W,3*hd] fp32: channels [0, 2hd) for zr, [2hd, 3hd) for q."""
        return hip.fconv_plain_f32(x, self.pre_w, self.pre_b, self.kh,
                                   self.kw, 0, self.ctx)

    def __call__(self, hip, h, x, pre=None):
        if not self.ctx:
            z, rh = hip.fconv_gru_zr(h, x, self.zr_w, self.zr_b, self.kh,
                                     self.kw)
            return hip.fconv_gru_q(rh, x, self.q_w, self.q_b, self.kh,
                                   self.kw, z, h)
        ctx, rest = self.ctx, x.shape[-1] - self.ctx
        z, rh = hip.fconv_gru_zr_pre(h, x, self.zr_w, self.kh, self.kw, pre,
                                     0, ctx, rest)
        return hip.fconv_gru_q_pre(rh, x, self.q_w, self.kh, self.kw, z, h,
                                   pre, 2 * self.hd, ctx, rest)


def _pack_fp8(wp_bf16, dev):
    """[taps, N, C] bf16 packed weights -> (uint8 e4m3, amax float)."""
    w = wp_bf16.float()
    aw = float(w.abs().max().clamp_min(1e-12))
    w8 = (w * (448.0 / aw)).to(torch.float8_e4m3fn).view(torch.uint8)
    return w8.contiguous().to(dev), aw


class _GruDirFP8:
    """fp8 e4m3 SepConvGRU direction (RAFT_AMD_FP8_GRU=1, r2 study):
    MX-scaled MFMA K=128 convs; inputs share the per-iteration x amax
    scale (h/rh are gate-bounded <= 1 <= ax). Requires hidden and input
    dims that are multiples of 128 (raft-things: 128 + 256)."""

    def __init__(self, convz, convr, convq):
        zr_w, self.zr_b, self.kh, self.kw = pack_zr(convz, convr)
        q_w, self.q_b, _, _ = pack_conv(convq)
        dev = self.zr_b.device
        self.zr_w8, self.zr_aw = _pack_fp8(zr_w, dev)
        self.q_w8, self.q_aw = _pack_fp8(q_w, dev)

    def __call__(self, hip, h, x8, ax, h8):
        z, rh8 = hip.fconv_fp8_gru_zr(h8, x8, h, self.zr_w8, self.zr_b, ax,
                                      self.zr_aw, self.kh, self.kw)
        return hip.fconv_fp8_gru_q(rh8, x8, self.q_w8, self.q_b, ax,
                                   self.q_aw, self.kh, self.kw, z, h)


def pack_smallc(wp: torch.Tensor) -> torch.Tensor:
    """[taps, N, C] packed weights -> the [N, 128] image fconv_smallc_packed
    reads its B fragments from: k = tap*C + c, zero tail."""
    taps, N, C = wp.shape
    img = wp.new_zeros(N, 128)
    img[:, :taps * C] = wp.permute(1, 0, 2).reshape(N, taps * C)
    return img.contiguous()


class _MotionFront:
    """The front of the motion encoder shared by both update blocks: the
    corr branch (lookup -> convc1 [-> convc2]) and the flow branch (convf1
    -> convf2), independent until ``conv`` and each latency-bound, so they
    run on two streams.

    early_fork: the flow channels of x_buf are written by the delta-flow
    kernel of the previous iteration (by ops.flow_slice at loop entry), so
    both branches depend on coords1 alone and the fork comes first; off,
    the lookup writes them and the flow branch follows it.
    f1_packed: convf1 on fconv_smallc_packed (weights packed once, here)."""

    def _init_front(self, enc, early_fork: bool, f1_packed: bool):
        self.f1 = _FC(enc.convf1)                    # Cin=2: small-K direct
        self.f2 = _FC(enc.convf2)
        self.early_fork = early_fork
        taps, N, C = self.f1.wp.shape
        self.f1_pk = None
        if (f1_packed and C <= 4 and taps * C <= 128 and N % 16 == 0
                and N <= 128 and self.f1.kh <= 9 and self.f1.kw <= 9):
            self.f1_pk = pack_smallc(self.f1.wp)
        self.side_stream = None                      # set by FusedRaft.run
        self._ev_fork = torch.cuda.Event()
        self._ev_join = torch.cuda.Event()

    def _flow_branch(self, hip, x_buf, off):
        f1 = self.f1
        if self.f1_pk is not None:
            flo1 = hip.fconv_smallc_packed(x_buf, self.f1_pk, f1.bias, f1.kh,
                                           f1.kw, ACT_RELU, off, 2)
        else:
            flo1 = hip.fconv_smallk(x_buf, f1.wp, f1.bias, f1.kh, f1.kw,
                                    ACT_RELU, off, 2, 1)
        return self.f2(hip, flo1)

    def _front(self, hip, x_buf, off, corr_pad, lookup):
        """(cor, flo) of one iteration. lookup: None (corr_pad is the
        lookup's output and x_buf holds the flow) or a callable launching
        the lookup part, returning (tensor, whether convc1 is applied)."""
        def head():
            return lookup() if lookup is not None else (corr_pad, False)

        def tail(t, is_c1):
            c = t if is_c1 else self.c1(hip, t)
            c2 = getattr(self, "c2", None)
            return c2(hip, c) if c2 is not None else c

        side = self.side_stream
        if side is None or torch.cuda.is_current_stream_capturing():
            cor = tail(*head())
            return cor, self._flow_branch(hip, x_buf, off)
        early = self.early_fork and lookup is not None
        cur = torch.cuda.current_stream()
        t = None if early else head()
        self._ev_fork.record(cur)
        side.wait_event(self._ev_fork)
        with torch.cuda.stream(side):
            flo = self._flow_branch(hip, x_buf, off)
            self._ev_join.record(side)
        cor = tail(*(head() if early else t))
        cur.wait_event(self._ev_join)
        flo.record_stream(cur)
        return cor, flo

    def _dflow(self, hip, h1, coords1, x_buf, off):
        """coords1 + delta-flow; with the early fork also the flow slice
        of x_buf the next iteration reads."""
        if self.early_fork:
            return hip.fconv_dflow_coords(h1, self.fh2.wp, self.fh2.bias,
                                          coords1, 3, 3, x_buf, off)
        return hip.fconv_dflow_coords(h1, self.fh2.wp, self.fh2.bias,
                                      coords1, 3, 3)


class FusedBasicUpdate(_MotionFront):
    """Packed raft-things update block (motion enc + SepConvGRU + heads)."""

    def __init__(self, ub, corr_cpad: int, ctx_dim: int, hoist: bool = False,
                 early_fork: bool = False, f1_packed: bool = False):
        enc = ub.encoder
        self.c1 = _FC(enc.convc1, pad_cin=corr_cpad)
        self.c2 = _FC(enc.convc2)
        self._init_front(enc, early_fork, f1_packed)
        self.cv = _FC(enc.conv)                      # in: [cor(192)|flo(64)]
        import os as _os
        hd = ub.gru.convz1.weight.shape[0]
        cat_dim = ub.gru.convz1.weight.shape[1]
        self.fp8_gru = (_os.environ.get("RAFT_AMD_FP8_GRU", "0") == "1"
                        and hd % 128 == 0 and (cat_dim - hd) % 128 == 0)
        if self.fp8_gru:
            self.gru1 = _GruDirFP8(ub.gru.convz1, ub.gru.convr1,
                                   ub.gru.convq1)
            self.gru2 = _GruDirFP8(ub.gru.convz2, ub.gru.convr2,
                                   ub.gru.convq2)
        else:
            hc = ctx_dim if hoist else 0
            self.gru1 = _GruDir(ub.gru.convz1, ub.gru.convr1, ub.gru.convq1,
                                hc)
            self.gru2 = _GruDir(ub.gru.convz2, ub.gru.convr2, ub.gru.convq2,
                                hc)
        # the fp8 GRU quantizes the whole x: it keeps the full-K convs
        self.hoist = hoist and not self.fp8_gru
        # flow_head.conv1 and mask[0] are both 3x3(128->256) on net: run as
        # ONE N=512 conv; their consumers read strided slices of the result
        self.fh1 = _FC(ub.flow_head.conv1)
        self.m0 = _FC(ub.mask[0])
        self.heads_w = torch.cat([self.fh1.wp, self.m0.wp], dim=1) \
            .contiguous()
        self.heads_b = torch.cat([self.fh1.bias, self.m0.bias]).contiguous()
        self.fh2 = _FC(ub.flow_head.conv2)
        self.m2 = _FC(ub.mask[2], scale=0.25)        # fold the 0.25 scale
        self.ctx_dim = ctx_dim

    def precompute(self, hip, x_buf):
        """The loop-invariant context terms of the GRU convs (one fp32
        tensor per direction), or None without the hoist."""
        if not self.hoist:
            return None
        return (self.gru1.precompute(hip, x_buf),
                self.gru2.precompute(hip, x_buf))

    def __call__(self, hip, net, x_buf, corr_pad, coords1, final=True,
                 pre=None, lookup=None):
        # motion encoder (model_utils.py:110-119): corr branch (c1->c2) and
        # flow branch (f1->f2) on two streams, joined before cv — see
        # _MotionFront
        ctx = self.ctx_dim
        cor, flo = self._front(hip, x_buf, ctx + 126, corr_pad, lookup)
        self.cv(hip, cor, flo, ACT_RELU, out=x_buf, n_off=ctx)   # 126 ch
        # SepConvGRU (model_utils.py:138-156)
        if self.fp8_gru:
            # one dynamic input scale per iteration (x_buf is complete
            # here); h/rh are gate-bounded <= 1 <= ax so they share it
            ax = x_buf.abs().amax().to(torch.float32).clamp_(min=1.0) \
                .contiguous()
            x8 = hip.quant_fp8(x_buf, ax)
            net = self.gru1(hip, net, x8, ax, hip.quant_fp8(net, ax))
            net = self.gru2(hip, net, x8, ax, hip.quant_fp8(net, ax))
        elif self.hoist:
            net = self.gru1(hip, net, x_buf, pre[0])
            net = self.gru2(hip, net, x_buf, pre[1])
        else:
            net = self.gru1(hip, net, x_buf)
            net = self.gru2(hip, net, x_buf)
        if not final:
            # intermediate iterations: the mask head is dead in test mode
            # (only the FINAL flow is upsampled — exactly the pruning TF
            # performs on the reference's fetched graph), so run the
            # flow-head 3x3 alone instead of the merged N=512 conv
            h1 = self.fh1(hip, net)
            coords_new = self._dflow(hip, h1, coords1, x_buf, ctx + 126)
            return net, None, coords_new
        # final iteration — heads: one merged 3x3 conv (flow_head.conv1 +
        # mask[0] stacked along N); mask from a strided slice; the
        # delta-flow final conv also applies coords1 += dflow in-kernel
        hbuf = hip.fconv_plain(net, None, self.heads_w, self.heads_b, 3, 3,
                               ACT_RELU, None, 0, 0, 0, -1, -1, 1, None)
        coords_new = self._dflow(hip, hbuf, coords1, x_buf, ctx + 126)
        mask = self.m2(hip, hbuf, act=ACT_NONE, in1_off=256, in1_len=256)
        return net, mask, coords_new


class FusedSmallUpdate(_MotionFront):
    """Packed raft-small update block (motion enc + ConvGRU, no mask)."""

    def __init__(self, ub, corr_cpad: int, ctx_dim: int, hoist: bool = False,
                 early_fork: bool = False, f1_packed: bool = False):
        enc = ub.encoder
        self.c1 = _FC(enc.convc1, pad_cin=corr_cpad)
        self._init_front(enc, early_fork, f1_packed)
        self.cv = _FC(enc.conv)                      # in: [cor(96)|flo(32)]
        self.hoist = hoist
        self.gru = _GruDir(ub.gru.convz, ub.gru.convr, ub.gru.convq,
                           ctx_dim if hoist else 0)
        self.fh1 = _FC(ub.flow_head.conv1)
        self.fh2 = _FC(ub.flow_head.conv2)
        self.ctx_dim = ctx_dim
        # x = [inp(ctx) | motion(80) | flow(2)]; motion encoder out = 80

    def precompute(self, hip, x_buf):
        return self.gru.precompute(hip, x_buf) if self.hoist else None

    def __call__(self, hip, net, x_buf, corr_pad, coords1, final=True,
                 pre=None, lookup=None):
        ctx = self.ctx_dim
        cor, flo = self._front(hip, x_buf, ctx + 80, corr_pad, lookup)
        self.cv(hip, cor, flo, ACT_RELU, out=x_buf, n_off=ctx)   # 80 ch
        net = self.gru(hip, net, x_buf, pre)
        h1 = self.fh1(hip, net)
        coords_new = self._dflow(hip, h1, coords1, x_buf, ctx + 80)
        return net, None, coords_new


def pack_raw(w: torch.Tensor, bias, pad_cin: Optional[int] = None):
    """Pack raw [N, Cin, kh, kw] fp32 weights -> ([taps, N, Cin_pad] bf16,
    bias fp32)."""
    N, Cin, kh, kw = w.shape
    cp = pad_cin if pad_cin is not None else Cin
    wp = w.new_zeros(N, cp, kh, kw)
    wp[:, :Cin] = w
    wp = wp.permute(2, 3, 0, 1).reshape(kh * kw, N, cp)
    wp = wp.contiguous().to(torch.bfloat16)
    if bias is None:
        bias = torch.zeros(N, device=w.device)
    return wp, bias.contiguous().float(), kh, kw


def fold_norm(conv: torch.nn.Conv2d, norm) -> tuple:
    """Fold an eval-mode BatchNorm (or Identity) into conv weights/bias —
    cnet norms use running stats at inference (model_utils.py:11)."""
    w = conv.weight.detach().float()
    b = conv.bias.detach().float() if conv.bias is not None \
        else torch.zeros(w.shape[0], device=w.device)
    if isinstance(norm, torch.nn.BatchNorm2d):
        scale = norm.weight.detach().float() / torch.sqrt(
            norm.running_var.detach().float() + norm.eps)
        w = w * scale.view(-1, 1, 1, 1)
        b = (b - norm.running_mean.detach().float()) * scale + \
            norm.bias.detach().float()
    return w, b


class _PC:
    """Packed conv (optionally norm-folded) with stride/residual support."""

    def __init__(self, conv, norm=None, pad_cin=None, stride=1):
        w, b = fold_norm(conv, norm) if norm is not None else (
            conv.weight.detach().float(),
            conv.bias.detach().float() if conv.bias is not None
            else torch.zeros(conv.weight.shape[0],
                             device=conv.weight.device))
        self.wp, self.bias, self.kh, self.kw = pack_raw(w, b, pad_cin)
        self.stride = stride

    def __call__(self, hip, x, act=ACT_NONE, res=None):
        return hip.fconv_plain(x, None, self.wp, self.bias, self.kh,
                               self.kw, act, None, 0, 0, 0, -1, -1,
                               self.stride, res)


class _FusedResBlock:
    """ResidualBlock (model_utils.py:19-35) on fconv/inorm kernels.
    instance norms need the stats kernels; batch/none norms are folded."""

    def __init__(self, blk, norm_fn: str, bottleneck: bool):
        self.instance = norm_fn == "instance"
        self.bottleneck = bottleneck
        nf = (lambda m: None) if self.instance else (lambda m: m)
        self.c1 = _PC(blk.conv1, nf(blk.norm1),
                      stride=1 if bottleneck else blk.conv1.stride[0])
        self.c2 = _PC(blk.conv2, nf(blk.norm2), stride=blk.conv2.stride[0])
        if bottleneck:
            self.c3 = _PC(blk.conv3, nf(blk.norm3))
        self.down = None
        if blk.downsample is not None:
            self.down = _PC(blk.downsample[0], nf(blk.downsample[1]),
                            stride=blk.downsample[0].stride[0])
            self.down_instance = self.instance

    def _norm_relu(self, hip, x, mode=1, res=None):
        m, r = hip.inorm_stats(x)
        return hip.inorm_apply(x, m, r, res, mode)

    def __call__(self, hip, x):
        if self.down is not None:
            d = self.down(hip, x, ACT_NONE)
            res = self._norm_relu(hip, d, 0) if self.instance else d
        else:
            res = x
        if self.instance:
            t = self._norm_relu(hip, self.c1(hip, x))
            if self.bottleneck:
                t = self._norm_relu(hip, self.c2(hip, t))
                y = self.c3(hip, t)
            else:
                y = self.c2(hip, t)
            # relu(res + relu(norm(y))): apply mode 2
            return self._norm_relu(hip, y, 2, res)
        # batch (folded) / none
        t = self.c1(hip, x, ACT_RELU)
        if self.bottleneck:
            t = self.c2(hip, t, ACT_RELU)
            return self.c3(hip, t, ACT_NONE, res=res)   # relu(res+relu(v))
        return self.c2(hip, t, ACT_NONE, res=res)


class FusedEncoder:
    """Basic/SmallEncoder (model_utils.py:61-105) on the NHWC kernel set.
    Input: physical-NHWC bf16 images padded to 8 channels."""

    def __init__(self, enc, norm_fn: str):
        from raft_amd.models.encoders import SmallEncoder
        bottleneck = isinstance(enc, SmallEncoder)
        self.instance = norm_fn == "instance"
        # stem 7x7/2: MFMA fconv with Cin padded 3->8 (A/B measured 300 us
        # vs 860 us for the small-K direct kernel at 440x1024 — the
        # grid-stride group loop serializes at this cell count)
        self.conv1 = _PC(enc.conv1,
                         None if self.instance else enc.norm1,
                         pad_cin=8, stride=2)
        self.blocks = []
        for layer in (enc.layer1, enc.layer2, enc.layer3):
            for blk in layer:
                self.blocks.append(_FusedResBlock(blk, norm_fn, bottleneck))
        self.proj = _PC(enc.conv2)

    def __call__(self, hip, x8):
        h = self.conv1(hip, x8, ACT_NONE if self.instance else ACT_RELU)
        if self.instance:
            m, r = hip.inorm_stats(h)
            h = hip.inorm_apply(h, m, r, None, 1)
        for blk in self.blocks:
            h = blk(hip, h)
        return self.proj(hip, h, ACT_NONE)


_warned_bidir_fp8 = False


class FusedRaft:
    """Caches packed weights for a RAFT model; call run() for inference."""

    def __init__(self, model):
        from raft_amd.ops import require_hip
        self.hip = require_hip()
        self.model = model
        cfg = model.cfg
        K = 2 * cfg.corr_radius + 1
        self.corr_c = cfg.corr_levels * K * K
        self.corr_cpad = _pad8(self.corr_c)
        import os
        # RAFT_AMD_GRU_HOIST (default 1): compute the context part of the
        # GRU convs once per pair instead of in every iteration; 0 = the
        # full-K convs. Read here, so one process can hold both variants.
        # The in-place slice read needs a 16-byte aligned context width.
        hoist = (os.environ.get("RAFT_AMD_GRU_HOIST", "1") != "0"
                 and cfg.context_dim % 8 == 0)
        # The motion-encoder front (profiles/motion_front.md), each default
        # 1, 0 = the earlier path, read here like the hoist:
        # RAFT_AMD_EARLY_FORK: the delta-flow kernel writes the next
        #   iteration's flow slice, so the flow branch forks before the
        #   lookup instead of after it;
        # RAFT_AMD_LOOKUP_CONV: lookup and convc1 as one kernel
        #   (ops.corr_lookup_conv1x1), no lookup buffer;
        # RAFT_AMD_CONVF1_PACKED: convf1 on ops.fconv_smallc_packed
        #   (weights packed once, one block per position tile). Only with
        #   RAFT_AMD_SMALLC_MFMA at its default: 0 there selects the
        #   direct kernels behind ops.fconv_smallk.
        def switch(name):
            return os.environ.get(name, "1") != "0"
        early = switch("RAFT_AMD_EARLY_FORK")
        f1pk = (switch("RAFT_AMD_CONVF1_PACKED")
                and switch("RAFT_AMD_SMALLC_MFMA"))
        if cfg.small:
            self.update = FusedSmallUpdate(model.update_block, self.corr_cpad,
                                           cfg.context_dim, hoist, early,
                                           f1pk)
            self.x_dim = cfg.context_dim + 82
        else:
            self.update = FusedBasicUpdate(model.update_block, self.corr_cpad,
                                           cfg.context_dim, hoist, early,
                                           f1pk)
            self.x_dim = cfg.context_dim + 128
        self.early_fork = early
        self.convf1_packed = self.update.f1_pk is not None
        self.lookup_conv = (switch("RAFT_AMD_LOOKUP_CONV")
                            and self.hip.lookup_conv_serves(
                                1, self.corr_c, self.corr_cpad,
                                self.update.c1.wp.shape[1]))
        self.gru_hoist = self.update.hoist
        self.fuse_enc = os.environ.get("RAFT_AMD_EAGER_ENC", "0") != "1"
        if self.fuse_enc:
            fnorm = "instance"
            cnorm = "none" if cfg.small else "batch"
            self.fnet_f = FusedEncoder(model.fnet, fnorm)
            self.cnet_f = FusedEncoder(model.cnet, cnorm)
        self._version = self._weights_version()
        self._graphs = {}
        self._res_host = {}     # pinned [B,2] landing buffers of _check
        self.last_info = None

    def _weights_version(self) -> int:
        return sum(p._version for p in self.model.parameters())

    def stale(self) -> bool:
        return self._version != self._weights_version()

    @torch.no_grad()
    def _loop(self, levels, net, x_buf, coords0, coords1, iters):
        """The refinement loop + final upsample — entirely in-repo kernels,
        so it is hipGraph-capturable (BASELINE config 5) without MIOpen's
        capture-time workspace fallbacks. Returns (upsampled flow, the
        1/8-resolution flow coords1 - coords0 as [B,H8,W8,2] fp32)."""
        hip = self.hip
        corr_buf = self._corr_buf(net)
        mask = None
        # the context channels of x_buf never change inside the loop: their
        # share of the GRU pre-activations is computed once, here, so it is
        # part of a captured loop and reads the graph's static x_buf
        pre = self.update.precompute(hip, x_buf)
        self._enter(x_buf, coords1)
        for it in range(iters):
            net, mask, coords1 = self._iteration(
                levels, net, x_buf, corr_buf, coords1, pre,
                final=(it == iters - 1))
        return self._upsample(coords0, coords1, mask)

    def _corr_buf(self, net):
        """The lookup's output buffer (pad channels zero), or None where
        the fused lookup -> convc1 kernel makes it unnecessary."""
        if self.lookup_conv:
            return None
        B, H8, W8, _ = net.shape
        return torch.zeros(B, H8, W8, self.corr_cpad, device=net.device,
                           dtype=torch.bfloat16)

    def _enter(self, x_buf, coords1):
        """Loop entry: with the early fork no kernel of the first
        iteration writes the flow slice of x_buf, so it is written here
        from the starting coords1 (warm start included)."""
        if self.early_fork:
            self.hip.flow_slice(coords1, x_buf, self.x_dim - 2)

    def _iteration(self, levels, net, x_buf, corr_buf, coords1, pre, final):
        """One refinement iteration: (net, mask or None, new coords1)."""
        hip, upd = self.hip, self.update
        radius = self.model.cfg.corr_radius
        off = self.x_dim - 2
        vs = getattr(self, "_vol_scale", None)
        early = self.early_fork

        def lookup():
            if corr_buf is None:
                # lookup -> convc1 in one kernel; it writes no flow
                if not early:
                    hip.flow_slice(coords1, x_buf, off)
                return hip.corr_lookup_conv1x1(
                    list(levels), coords1, radius, upd.c1.wp, upd.c1.bias,
                    ACT_RELU, vs), True
            # without the early fork the lookup also writes flow =
            # coords1 - grid into the GRU input buffer's flow slice
            return hip.corr_lookup_nhwc(
                list(levels), coords1, radius, self.corr_cpad, True,
                corr_buf, None if early else x_buf, off, vs), False

        return upd(hip, net, x_buf, None, coords1, final=final, pre=pre,
                   lookup=lookup)

    def _upsample(self, coords0, coords1, mask):
        cfg = self.model.cfg
        hip = self.hip
        flow = coords1 - coords0                         # [B,H,W,2] fp32
        if cfg.small:
            from raft_amd.ops import torch_ref
            up = torch_ref.upflow8(flow.permute(0, 3, 1, 2))
            if cfg.scale_small_upflow:
                up = 8.0 * up
            return up, flow
        flow_nchw = flow.permute(0, 3, 1, 2).contiguous()
        mask_nchw = mask.permute(0, 3, 1, 2).contiguous()
        return hip.convex_upsample(flow_nchw, mask_nchw), flow

    def _side(self):
        side = getattr(self, "_side_stream", None)
        if side is None:
            side = torch.cuda.Stream()
            self._side_stream = side
        self.update.side_stream = side   # motion-encoder branch overlap
        return side

    @torch.no_grad()
    def encode(self, image, want_context=True):
        """Encoder stage for one frame batch [N,3,H,W]: preprocess,
        8-channel NHWC staging, fnet on the current stream and
        (``want_context``) cnet on the side stream. Returns (fmap
        [N,H8,W8,C], context [N,H8,W8,hidden+context] or None), both
        physical NHWC. The context is still in flight on the side stream:
        run_pair joins it before reading. The results carry over to later
        calls — a video session feeds each frame's maps to two consecutive
        pairs."""
        return self._encode([image], want_context, None)

    def _encode(self, images, want_context, context_batch):
        """encode() on several image tensors as one batch; cnet sees the
        first ``context_batch`` rows (None: all). run() needs both: each
        image preprocessed on its own and the context of frame 1 alone
        keep it on the bits it has always returned."""
        model = self.model
        hip = self.hip
        imgs = [model.preprocess(im) for im in images]
        N = sum(im.shape[0] for im in imgs)
        nc = N if context_batch is None else context_batch
        side = self._side()
        cur = torch.cuda.current_stream()
        ctx = None

        if self.fuse_enc:
            # in-repo encoders: images -> physical NHWC padded to 8 ch
            # (Cin=3 would hit the scalar staging seam in every load)
            _, _, Hi, Wi = imgs[0].shape
            x8 = torch.zeros(N, Hi, Wi, 8, device=imgs[0].device,
                             dtype=torch.bfloat16)
            r = 0
            for im in imgs:
                x8[r:r + im.shape[0], ..., :3] = im.permute(0, 2, 3, 1)
                r += im.shape[0]
            if want_context:
                side.wait_stream(cur)
                # x8 may be released before the side stream has read it
                x8.record_stream(side)
                with torch.cuda.stream(side):
                    ctx = self.cnet_f(hip, x8 if nc == N
                                      else x8[:nc].contiguous())
            return self.fnet_f(hip, x8), ctx

        x = imgs[0] if len(imgs) == 1 else torch.cat(imgs, dim=0)
        fmaps = model.fnet(x).permute(0, 2, 3, 1).contiguous()
        if want_context:
            side.wait_stream(cur)
            x.record_stream(side)
            with torch.cuda.stream(side):
                ctx = model.cnet(x if nc == N else x[:nc]) \
                    .permute(0, 2, 3, 1)
        return fmaps, ctx

    @torch.no_grad()
    def run(self, image1, image2, iters, flow_init=None,
            bidirectional=False, return_low=False, converge=None,
            return_info=False):
        """bidirectional: both directions share one pass — cnet sees both
        frames, the volume kernel stores each tile twice (forward and
        transposed) and the loop runs at batch 2B ([fw | bw]); flow_init
        is then already the [2B,2,H8,W8] concatenation. Returns the pair
        (flow_fw, flow_bw). return_low appends the 1/8-resolution flow(s),
        converge / return_info gate the loop, see run_pair."""
        B0 = image1.shape[0]
        fmaps, ctx = self._encode([image1, image2], True,
                                  None if bidirectional else B0)
        return self.run_pair(fmaps[:B0].contiguous(),
                             fmaps[B0:].contiguous(), ctx, None, iters,
                             flow_init, bidirectional, return_low, converge,
                             return_info)

    @torch.no_grad()
    def run_pair(self, f1p, f2p, ctx1, ctx2=None, iters=None,
                 flow_init=None, bidirectional=False, return_low=False,
                 converge=None, return_info=False):
        """Pair stage: everything from the correlation volume on, fed with
        encode() results. f1p/f2p: [B,H8,W8,C] feature maps of the two
        frames; ctx1: context of frame 1 — bidirectional runs also need
        frame 2's, either as ctx2 or already stacked under ctx1 ([2B]
        rows, frame 1 first). Returns the upsampled flow, or (flow_fw,
        flow_bw); with return_low followed by the 1/8-resolution flow
        [B,2,H8,W8] fp32 (one per direction) — the quantity flow_init
        seeds. Under graph replay the results live in static buffers that
        the next replay of the same shape overwrites: clone to keep.

        converge: a raft_amd.Convergence makes ``iters`` a budget — the
        loop checks its coords update (ops.flow_residual on the
        interleaved coords) and after convergence runs the final
        iteration and stops; the result equals the ungated call with
        iters = the executed count bit for bit. return_info appends the
        ConvergenceInfo, also kept as ``self.last_info``."""
        model = self.model
        cfg = model.cfg
        hip = self.hip
        side = self._side()
        iters = iters if iters is not None else cfg.iters
        B, H8, W8, C = f1p.shape

        import os as _os
        fp8_mode = _os.environ.get("RAFT_AMD_FP8_CORR", "0")
        if C % 128 != 0:
            fp8_mode = "0"
        self._vol_scale = None
        if bidirectional:
            if fp8_mode != "0":
                global _warned_bidir_fp8
                if not _warned_bidir_fp8:
                    _warned_bidir_fp8 = True
                    import warnings
                    warnings.warn("RAFT_AMD_FP8_CORR is ignored for "
                                  "bidirectional runs: using the bf16 "
                                  "correlation volume")
            # [2B, HW, H8, W8]: forward volume, then its exact transpose
            # (= the volume of (f2, f1)) from the same accumulators
            vol = hip.corr_volume_nhwc_bidir(f1p, f2p)
            pool = hip.corr_pool2x_bf16
            B = 2 * B
        elif fp8_mode == "2":
            # r2 roadmap #4: e4m3 GEMM AND e4m3 volume storage — halves
            # the volume write/read streams; lookup dequantizes by the
            # device-scalar vol_scale
            vol, self._vol_scale = hip.corr_volume_nhwc_fp8s(f1p, f2p)
            pool = hip.corr_pool2x_fp8
        elif fp8_mode == "1":
            # e4m3 GEMM at the MX MFMA rate, bf16 volume
            vol = hip.corr_volume_nhwc_fp8(f1p, f2p, True)
            pool = hip.corr_pool2x_bf16
        else:
            vol = hip.corr_volume_nhwc(f1p, f2p, True)   # bf16 volume
            pool = hip.corr_pool2x_bf16
        levels = [vol]
        for _ in range(cfg.corr_levels - 1):
            last = levels[-1]
            if last.shape[-2] < 2 or last.shape[-1] < 2:
                levels.append(last)               # degenerate tiny level
            else:
                levels.append(pool(last))

        # join the context encoder(s): every cnet launched so far sits on
        # the side stream, a cached one from an earlier call included
        torch.cuda.current_stream().wait_stream(side)
        for c in (ctx1, ctx2):
            if c is not None:
                c.record_stream(torch.cuda.current_stream())
        ctx = ctx1 if ctx2 is None else torch.cat([ctx1, ctx2], dim=0)
        if ctx.shape[0] != B:
            raise ValueError(f"context has {ctx.shape[0]} rows, the loop "
                             f"batch is {B}" + (" (bidirectional runs need "
                                                "both frames' context)"
                                                if bidirectional else ""))
        net = torch.tanh(ctx[..., :cfg.hidden_dim]).contiguous()
        inp = torch.relu(ctx[..., cfg.hidden_dim:]).contiguous()

        ys, xs = torch.meshgrid(
            torch.arange(H8, device=net.device, dtype=torch.float32),
            torch.arange(W8, device=net.device, dtype=torch.float32),
            indexing="ij")
        coords0 = torch.stack([xs, ys], dim=-1)[None].expand(B, -1, -1, -1) \
            .contiguous()                                # [B,H,W,2] (x,y)
        coords1 = coords0.clone()
        if flow_init is not None:                        # [B,2,H,W] logical
            coords1 = coords1 + flow_init.permute(0, 2, 3, 1).float()

        # loop-graph policy (r2, measured): replay wins where the loop is
        # launch-bound — config-5 mixed-batch at 12 iters 333 -> 377 fps —
        # and loses slightly at the 32-iter headline (replay serializes
        # the cross-stream motion-encoder overlap; see
        # profiles/r02_optimization_pass.md). AUTO = capture when
        # iters <= 16; explicit True/False (RAFT_AMD_LOOP_GRAPH) overrides.
        use_graph = getattr(model, "_fused_use_graph", None)
        if use_graph is None:
            use_graph = iters <= 16
        # a gated call (converge) runs the same iterations one at a time
        # and measures the coords update at its check iterations; the same
        # graph policy applies to its budget
        gate = None
        info = ConvergenceInfo(iters_run=iters)
        if converge is not None:
            gate = Gate(converge, iters, H8 * W8)
            info = gate.info
        self.last_info = info

        def eager():
            x_buf = torch.empty(B, H8, W8, self.x_dim, device=net.device,
                                dtype=torch.bfloat16)
            x_buf[..., :cfg.context_dim] = inp
            if gate is None:
                return self._loop(levels, net, x_buf, coords0, coords1,
                                  iters)
            return self._loop_gated(levels, net, x_buf, coords0, coords1,
                                    gate)

        if not use_graph:
            out, low = eager()
            return self._result(out, low, bidirectional, return_low,
                                info if return_info else None)

        # a bidirectional run shares the captured loop of a unidirectional
        # batch-2B run (identical kernels) — except under RAFT_AMD_FP8_CORR,
        # where that graph may hold fp8 level buffers. One (step, tail)
        # graph pair serves every budget and Convergence of a shape.
        key = (B, H8, W8, iters if gate is None else "gated")
        if bidirectional and fp8_mode != "0":
            key += ("bf16",)
        entry = self._graphs.get(key)
        if entry is None:
            if len(self._graphs) >= 4:     # shape-bucket cap
                out, low = eager()
                return self._result(out, low, bidirectional, return_low,
                                    info if return_info else None)
            if gate is None:
                entry = self._capture(levels, net, inp, coords0, coords1,
                                      iters)
            else:
                entry = self._capture_gated(levels, net, inp, coords0,
                                            coords1)
            self._graphs[key] = entry
        graph, st = entry
        for dst, src in zip(st["levels"], levels):
            dst.copy_(src)
        st["net"].copy_(net)
        st["x_buf"][..., :cfg.context_dim].copy_(inp)
        st["coords1"].copy_(coords1)
        if st.get("vol_scale") is not None:   # fp8-storage dequant scalar
            st["vol_scale"].copy_(self._vol_scale)
        if gate is None:
            graph.replay()
        else:
            self._replay_gated(graph, st, gate)
        return self._result(st["out"], st["low"], bidirectional, return_low,
                            info if return_info else None)

    @staticmethod
    def _result(out, low, bidirectional, return_low, info=None):
        """Shape run_pair's return value: out [B,2,H,W], low the loop's
        [B,H8,W8,2] flow (returned as its logical [B,2,H8,W8] view), info
        the ConvergenceInfo to append (return_info)."""
        h = out.shape[0] // 2
        res = (out[:h], out[h:]) if bidirectional else (out,)
        if return_low:
            low = low.permute(0, 3, 1, 2)
            res += (low[:h], low[h:]) if bidirectional else (low,)
        if info is not None:
            res += (info,)
        return res if len(res) > 1 else res[0]

    # ------------------------------------------------------ gated loop
    def _check(self, gate, it, prev, nxt):
        """Measure the coords update prev -> nxt (interleaved [B,H8,W8,2])
        of iteration ``it`` and tell whether the loop has converged: one
        memset + one kernel, one device-to-host copy of the [B,2] result
        and one wait — the only synchronisation of a gated call."""
        raw = self.hip.flow_residual(prev.permute(0, 3, 1, 2),
                                     nxt.permute(0, 3, 1, 2), gate.thr_sq,
                                     None)
        B = raw.shape[0]
        host = self._res_host.get(B)
        if host is None:
            host = torch.empty(B, 2, dtype=torch.int32).pin_memory()
            self._res_host[B] = host
        host.copy_(raw, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        return gate.record_raw(it, host.numpy())

    @torch.no_grad()
    def _loop_gated(self, levels, net, x_buf, coords0, coords1, gate):
        """_loop under a convergence gate: non-final iterations up to the
        decision, then the final one (merged heads + mask) and the
        upsample — the kernel sequence of _loop with iters = the executed
        count."""
        corr_buf = self._corr_buf(net)
        pre = self.update.precompute(self.hip, x_buf)
        self._enter(x_buf, coords1)
        last = False
        for it in range(1, gate.budget + 1):
            final = last or it == gate.budget
            prev = coords1
            net, mask, coords1 = self._iteration(levels, net, x_buf,
                                                 corr_buf, coords1, pre,
                                                 final=final)
            if final:
                break
            if gate.wants(it):
                last = self._check(gate, it, prev, coords1)
        gate.info.iters_run = it
        return self._upsample(coords0, coords1, mask)

    def _step(self, st):
        """One non-final iteration on the static buffers (a step graph's
        body): coords_prev <- coords1, then net and coords1 advance."""
        st["coords_prev"].copy_(st["coords1"])
        net, _, coords1 = self._iteration(
            st["levels"], st["net"], st["x_buf"], st["corr_buf"],
            st["coords1"], st["pre"], final=False)
        st["net"].copy_(net)
        st["coords1"].copy_(coords1)

    def _tail(self, st):
        """The final iteration and the upsample on the static buffers."""
        _, mask, coords1 = self._iteration(
            st["levels"], st["net"], st["x_buf"], st["corr_buf"],
            st["coords1"], st["pre"], final=True)
        return self._upsample(st["coords0"], coords1, mask)

    def _set_pre(self, st):
        """The hoisted context terms of this call into the static buffers
        the two graphs read (eager: the graphs serve every pair)."""
        pre = self.update.precompute(self.hip, st["x_buf"])
        if pre is None:
            return
        if isinstance(pre, tuple):
            for dst, src in zip(st["pre"], pre):
                dst.copy_(src)
        else:
            st["pre"].copy_(pre)

    def _replay_gated(self, graphs, st, gate):
        step, tail = graphs
        self._set_pre(st)
        self._enter(st["x_buf"], st["coords1"])
        last = False
        for it in range(1, gate.budget + 1):
            if last or it == gate.budget:
                tail.replay()
                break
            step.replay()
            if gate.wants(it):
                last = self._check(gate, it, st["coords_prev"],
                                   st["coords1"])
        gate.info.iters_run = it

    def _static(self, levels, net, inp, coords0, coords1):
        cfg = self.model.cfg
        st = {
            "levels": [l.clone() for l in levels],
            "net": net.clone(),
            "x_buf": torch.empty(net.shape[0], net.shape[1], net.shape[2],
                                 self.x_dim, device=net.device,
                                 dtype=torch.bfloat16),
            "coords0": coords0.clone(),
            "coords1": coords1.clone(),
            "vol_scale": None,
        }
        if getattr(self, "_vol_scale", None) is not None:
            # fp8-storage mode: the graph must read a STABLE scale buffer
            # that replays refresh (the per-run tensor is a new allocation)
            st["vol_scale"] = self._vol_scale.clone()
            self._vol_scale = st["vol_scale"]
        st["x_buf"][..., :cfg.context_dim] = inp
        return st

    def _capture_gated(self, levels, net, inp, coords0, coords1):
        """Two graphs for a shape: a step graph (one non-final iteration,
        static net / coords_prev / coords1 in and out) and a tail graph
        (final iteration + upsample)."""
        st = self._static(levels, net, inp, coords0, coords1)
        st["coords_prev"] = coords1.clone()
        st["corr_buf"] = self._corr_buf(net)
        st["pre"] = self.update.precompute(self.hip, st["x_buf"])
        self._enter(st["x_buf"], st["coords1"])
        # warm up on a side stream (allocator steady-state before capture)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._step(st)
                self._tail(st)
        torch.cuda.current_stream().wait_stream(s)
        step = torch.cuda.CUDAGraph()
        with torch.cuda.graph(step):
            self._step(st)
        tail = torch.cuda.CUDAGraph()
        with torch.cuda.graph(tail):
            st["out"], st["low"] = self._tail(st)
        return (step, tail), st

    def _capture(self, levels, net, inp, coords0, coords1, iters):
        st = self._static(levels, net, inp, coords0, coords1)
        # warm up on a side stream (allocator steady-state before capture)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self._loop(st["levels"], st["net"], st["x_buf"],
                           st["coords0"], st["coords1"], iters)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            st["out"], st["low"] = self._loop(
                st["levels"], st["net"], st["x_buf"], st["coords0"],
                st["coords1"], iters)
        return graph, st


def get_fused(model) -> Optional[FusedRaft]:
    """Return (building if needed) the packed fused runner for this model.
    Rebuilds automatically when the underlying weights changed."""
    f = getattr(model, "_fused_cache", None)
    if f is None or f.stale():
        f = FusedRaft(model)
        model._fused_cache = f
    return f


def can_fuse(model, image1: torch.Tensor) -> bool:
    import os

    import raft_amd.ops as O
    if os.environ.get("RAFT_AMD_NO_FUSE", "0") == "1":
        return False
    try:
        p = next(model.update_block.parameters())
    except StopIteration:
        return False
    cfg = model.cfg
    return (image1.is_cuda and not torch.is_grad_enabled()
            and p.dtype == torch.bfloat16 and O.hip_available()
            and cfg.corr_levels <= 4 and cfg.fnet_dim % 64 == 0)
