"""Pure-PyTorch golden implementations of the RAFT hot ops.

These mirror the reference TF graph *exactly* (file:line citations below) and
are the numerics oracle for the HIP kernels (tests compare HIP output against
these in fp32).  They also serve as the CPU execution path.

Conventions: NCHW activations; coords are ``[B, H, W, 2]`` float with last
dim (x, y); correlation volume level i is ``[B, H1*W1, H2/2^i, W2/2^i]``.
"""
from __future__ import annotations

import math
from typing import List

import torch
import torch.nn.functional as F


def corr_volume(fmap1: torch.Tensor, fmap2: torch.Tensor) -> torch.Tensor:
    """All-pairs correlation ``C = F1·F2ᵀ / sqrt(c)``.

    Mirrors networks/model_utils.py:199-215 (reshape + matmul + 1/sqrt(c)).
    fmap*: [B, C, H, W] -> returns [B, H*W, H, W] in fp32 (accumulation is
    always fp32 regardless of input dtype — SURVEY.md §7 hard part (e)).
    """
    B, C, H, W = fmap1.shape
    f1 = fmap1.reshape(B, C, H * W).transpose(1, 2).float()  # [B, HW, C]
    f2 = fmap2.reshape(B, C, H * W).float()                  # [B, C, HW]
    corr = torch.matmul(f1, f2) / math.sqrt(C)
    return corr.reshape(B, H * W, H, W)


def corr_pyramid_pool(corr: torch.Tensor, num_levels: int = 4) -> List[torch.Tensor]:
    """2x2/2 average-pool pyramid over the *target* dims, TF VALID semantics
    (floor division) — model_utils.py:215-219.

    corr: [B, H1*W1, H2, W2]; returns [level0, ..., level{num_levels-1}].
    """
    pyramid = [corr]
    for _ in range(num_levels - 1):
        if corr.shape[-2] < 2 or corr.shape[-1] < 2:
            # degenerate level (tiny input): keep the last level so the
            # channel count contract (L*KK) holds; lookup clamps anyway
            pyramid.append(corr)
            continue
        corr = F.avg_pool2d(corr, 2, stride=2)  # default floor, matches VALID
        pyramid.append(corr)
    return pyramid


def bilinear_sample_volume(corr: torch.Tensor, x: torch.Tensor,
                           y: torch.Tensor) -> torch.Tensor:
    """Edge-clamp bilinear gather from [N, H2, W2] at per-sample (x, y).

    Replicates networks/utils.py:39-99 (tf_grid_sample) exactly:
      * corner ints by *truncation toward zero* (tf.cast, utils.py:54-57),
        not floor — differs for negative coords;
      * both corners clamped to the image, weights computed from the
        CLAMPED x1/y1 via qx = x1 - x (utils.py:60-89) — the edge-clamp
        boundary (vs zeros-pad in official PyTorch grid_sample);
      * weights wa=qx*qy, wb=qx*(1-qy), wc=(1-qx)*qy, wd=(1-qx)(1-qy).

    x, y: [N, K] sample coordinates into each of the N slices.
    Returns [N, K].
    """
    N, H2, W2 = corr.shape
    xt = torch.trunc(x)
    yt = torch.trunc(y)
    x0 = torch.clamp(xt.long(), 0, W2 - 1)
    x1 = torch.clamp(xt.long() + 1, 0, W2 - 1)
    y0 = torch.clamp(yt.long(), 0, H2 - 1)
    y1 = torch.clamp(yt.long() + 1, 0, H2 - 1)

    n = torch.arange(N, device=corr.device).unsqueeze(1)  # [N,1]
    Ia = corr[n, y0, x0]
    Ib = corr[n, y1, x0]
    Ic = corr[n, y0, x1]
    Id = corr[n, y1, x1]

    qx = x1.to(x.dtype) - x
    qy = y1.to(y.dtype) - y
    wa = qx * qy
    wb = qx * (1.0 - qy)
    wc = (1.0 - qx) * qy
    wd = (1.0 - qx) * (1.0 - qy)
    return wa * Ia + wb * Ib + wc * Ic + wd * Id


def corr_lookup(pyramid: List[torch.Tensor], coords: torch.Tensor,
                radius: int) -> torch.Tensor:
    """Multi-scale (2r+1)^2-tap window lookup — model_utils.py:224-249.

    Window order: reference builds delta = stack(meshgrid(dy, dx)[::-1]) so
    tap index k ↔ offset (dx = k // (2r+1) - r, dy = k % (2r+1) - r)
    (model_utils.py:235-237): the x offset varies along the *slow* window
    axis. Channel layout of the output: [lvl0 k0..k_{K-1}, lvl1 ..., ...].

    pyramid: list of [B, H1*W1, H2_i, W2_i]; coords: [B, H, W, 2] (x, y).
    Returns [B, L*(2r+1)^2, H, W] (NCHW, ready for the motion encoder).
    """
    B, H, W, _ = coords.shape
    K = 2 * radius + 1
    dev = coords.device
    dt = coords.dtype
    r = float(radius)
    # offsets along tap index k: off_x slow, off_y fast (see docstring)
    off = torch.linspace(-r, r, K, device=dev, dtype=dt)
    off_x = off.repeat_interleave(K)  # [K*K]
    off_y = off.repeat(K)             # [K*K]

    cf = coords.reshape(B * H * W, 2)
    out_levels = []
    for i, corr in enumerate(pyramid):
        Bc, HW, H2, W2 = corr.shape
        c = corr.reshape(B * H * W, H2, W2)
        cx = cf[:, 0:1] / (2 ** i) + off_x.unsqueeze(0)  # [N, K*K]
        cy = cf[:, 1:2] / (2 ** i) + off_y.unsqueeze(0)
        sampled = bilinear_sample_volume(c, cx, cy)      # [N, K*K]
        out_levels.append(sampled.reshape(B, H, W, K * K))
    out = torch.cat(out_levels, dim=-1)                  # [B, H, W, L*K*K]
    return out.permute(0, 3, 1, 2).contiguous()


def gru_gates(h: torch.Tensor, z_act: torch.Tensor,
              q_act: torch.Tensor) -> torch.Tensor:
    """Pointwise GRU state update ``h' = (1-σ(z))·h + σ(z)·tanh(q)``.

    The gate math of model_utils.py:146,154,168 with the conv activations
    already applied by the caller's convs (z_act/q_act are pre-activation).
    """
    z = torch.sigmoid(z_act)
    q = torch.tanh(q_act)
    return (1.0 - z) * h + z * q


def convex_upsample(flow: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """8x convex upsample with a learned 9-way mask — networks/RAFT.py:119-134.

    flow: [B, 2, H, W]; mask: [B, 576, H, W] with channel c = k*64 + dy*8 + dx
    (reference reshapes NHWC 576 -> (9, 1, 8, 8), RAFT.py:125).  Softmax over
    the 9 taps; taps are the 3x3 zero-padded neighborhood of 8*flow
    (tf.extract_image_patches SAME, RAFT.py:128).  Output [B, 2, 8H, 8W];
    out(8y+dy, 8x+dx) = Σ_k m[k,dy,dx,y,x] · 8·flow[nbr_k(y,x)].
    """
    B, _, H, W = flow.shape
    m = mask.reshape(B, 9, 8, 8, H, W)
    m = torch.softmax(m, dim=1)
    # F.unfold channel order is (c, ky, kx) with c slowest; view separates it.
    patches = F.unfold(8.0 * flow, 3, padding=1).reshape(B, 2, 9, 1, 1, H, W)
    up = (m.unsqueeze(1) * patches).sum(dim=2)           # [B, 2, 8, 8, H, W]
    up = up.permute(0, 1, 4, 2, 5, 3)                    # [B, 2, H, 8, W, 8]
    return up.reshape(B, 2, 8 * H, 8 * W)


def upflow8(flow: torch.Tensor) -> torch.Tensor:
    """Bilinear x8 upsample, align_corners=True — networks/utils.py:105-111.

    NOTE (deliberate reference quirk): the reference does *not* multiply the
    flow values by 8 on this path (RAFT.py:104-105), unlike official RAFT.
    Callers that want physically-scaled flow pass the result through
    ``8 * upflow8(flow)`` themselves (see RaftConfig.scale_small_upflow).
    """
    B, C, H, W = flow.shape
    return F.interpolate(flow, size=(8 * H, 8 * W), mode="bilinear",
                         align_corners=True)


def fb_consistency(flow_fw: torch.Tensor, flow_bw: torch.Tensor,
                   alpha1: float = 0.01, alpha2: float = 0.5,
                   return_terms: bool = False):
    """Forward-backward consistency occlusion mask (UnFlow, Meister et al.
    2018, with its published constants).

    Per pixel (x, y) of ``flow_fw`` with f = flow_fw[:, :, y, x]:
      p = (x, y) + f (one fp32 add per axis); ``inb`` = p inside
      [0, W-1] x [0, H-1]; w = standard bilinear sample of ``flow_bw`` at p
      (corners floor(p) and +1, both clamped to the frame, weights clamped
      to [0, 1] — NOT the trunc/clamped-weight quirk of the correlation
      lookup); res = |f + w|^2; bound = alpha1 * (|f|^2 + |w|^2) + alpha2;
      occluded = (not inb) or res > bound.

    Returns occ [B,1,H,W] bool (and res, bound [B,1,H,W] fp32 with
    ``return_terms``). The backward mask is the same call with the
    arguments swapped.
    """
    fw = flow_fw.float()
    bw = flow_bw.float()
    B, _, H, W = fw.shape
    xs = torch.arange(W, device=fw.device, dtype=torch.float32)
    ys = torch.arange(H, device=fw.device, dtype=torch.float32)
    fx, fy = fw[:, 0], fw[:, 1]                          # [B, H, W]
    px = xs.view(1, 1, W) + fx
    py = ys.view(1, H, 1) + fy
    inb = (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)

    # NaN -> corner 0 (the pixel is out of frame either way)
    x0f = torch.nan_to_num(px.floor(), nan=0.0).clamp(0, W - 1)
    y0f = torch.nan_to_num(py.floor(), nan=0.0).clamp(0, H - 1)
    x0, y0 = x0f.long(), y0f.long()
    x1 = (x0 + 1).clamp(max=W - 1)
    y1 = (y0 + 1).clamp(max=H - 1)
    ax = torch.nan_to_num(px - x0f, nan=0.0).clamp(0, 1)
    ay = torch.nan_to_num(py - y0f, nan=0.0).clamp(0, 1)
    w00 = (1 - ax) * (1 - ay)
    w01 = ax * (1 - ay)
    w10 = (1 - ax) * ay
    w11 = ax * ay

    flat = bw.reshape(B, 2, H * W)

    def tap(yi, xi):
        idx = (yi * W + xi).reshape(B, 1, H * W).expand(B, 2, H * W)
        return flat.gather(2, idx).reshape(B, 2, H, W)

    w = (w00.unsqueeze(1) * tap(y0, x0) + w01.unsqueeze(1) * tap(y0, x1)
         + w10.unsqueeze(1) * tap(y1, x0) + w11.unsqueeze(1) * tap(y1, x1))
    wx, wy = w[:, 0], w[:, 1]
    sx, sy = fx + wx, fy + wy
    res = sx * sx + sy * sy
    bound = alpha1 * ((fx * fx + fy * fy) + (wx * wx + wy * wy)) + alpha2
    occ = (~inb | (res > bound)).unsqueeze(1)
    if return_terms:
        return occ, res.unsqueeze(1), bound.unsqueeze(1)
    return occ


def forward_project(flow: torch.Tensor, direction: int = 1):
    """Deterministic forward projection of a flow field — RAFT's warm start
    (``forward_interpolate``) as a nearest-source splat. This definition is
    the contract: the HIP kernel (csrc/flow_project.hip) matches it bit for
    bit.

    flow: [B,2,H,W] fp32. Returns (projected [B,2,H,W] fp32, holes
    [B,1,H,W] bool, taken before filling).

    Scatter: source cell (x, y), linear index i = y*W + x, value f, targets
    t = (x + fx, y + fy) for ``direction=+1`` and (x - fx, y - fy) for
    ``direction=-1`` (one fp32 add / subtract per coordinate). It is valid
    iff 0 <= tx <= W-1 and 0 <= ty <= H-1 (NaN / Inf are dropped) and is
    then a candidate for the in-grid cells of {floor(tx), floor(tx)+1} x
    {floor(ty), floor(ty)+1} at distance d2 = dx*dx + dy*dy (products and
    sum rounded separately, no FMA).
    Winner: each cell takes the value f (never negated) of the candidate
    with the smallest d2, exact ties to the lowest i — the minimum of the
    64-bit key (float_bits(d2) << 32) | i, independent of execution order.
    Holes: a cell without candidate takes the mean of the nearest covered
    cells to its left, right, above and below — added in that order from
    0.0, divided by their count (correctly rounded) — or 0 when its row
    and column hold none (utils.flow_tools._fill_holes_nearest4).

    ``direction=+1`` is the constant-velocity warm start of the forward
    flow; ``direction=-1`` the same assumption for the backward flow of
    the next pair (a point at x in frame t+1 with backward flow b sits at
    x - b in frame t+2 and keeps b).
    """
    if direction not in (1, -1):
        raise ValueError(f"direction must be +1 or -1, got {direction}")
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError(f"flow must be [B,2,H,W], got {tuple(flow.shape)}")
    f = flow.float().contiguous()
    B, _, H, W = f.shape
    dev = f.device
    HW = H * W
    if B * HW == 0:
        return f.clone(), torch.zeros(B, 1, H, W, dtype=torch.bool,
                                      device=dev)
    xs = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    ys = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    fx, fy = f[:, 0], f[:, 1]                            # [B, H, W]
    tx = xs + fx if direction > 0 else xs - fx
    ty = ys + fy if direction > 0 else ys - fy
    valid = (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
    x0 = torch.where(valid, tx, torch.zeros_like(tx)).floor()
    y0 = torch.where(valid, ty, torch.zeros_like(ty)).floor()

    empty = torch.iinfo(torch.int64).max
    keys = torch.full((B * HW,), empty, dtype=torch.int64, device=dev)
    src = torch.arange(HW, device=dev, dtype=torch.int64).view(1, H, W)
    base = (torch.arange(B, device=dev, dtype=torch.int64) * HW) \
        .view(B, 1, 1)
    for dy in (0.0, 1.0):
        for dx in (0.0, 1.0):
            qx, qy = x0 + dx, y0 + dy
            ok = valid & (qx <= W - 1) & (qy <= H - 1)
            ddx, ddy = tx - qx, ty - qy
            d2 = (ddx * ddx + ddy * ddy).contiguous()
            key = (d2.view(torch.int32).to(torch.int64) << 32) | src
            cell = base + (qy * W + qx).long()
            keys.scatter_reduce_(0, cell[ok], key[ok], reduce="amin")

    cov = (keys != empty).view(B, H, W)
    winner = (keys & 0xFFFFFFFF).view(B, 1, HW).expand(B, 2, HW)
    winner = torch.where(cov.view(B, 1, HW), winner,
                         torch.zeros_like(winner))
    val = f.view(B, 2, HW).gather(2, winner).view(B, 2, H, W)
    val = torch.where(cov.unsqueeze(1), val, torch.zeros_like(val))

    def nearest(dim: int, reverse: bool):
        """Value and presence of the nearest covered cell strictly before
        (or after, ``reverse``) each cell along ``dim`` of [B,H,W]."""
        n = cov.shape[dim]
        c, v = cov, val
        if reverse:
            c, v = c.flip(dim), v.flip(dim + 1)
        shape = [1, 1, 1]
        shape[dim] = n
        pos = torch.arange(n, device=dev).view(shape)
        last = torch.where(c, pos, torch.full_like(pos, -1)) \
            .cummax(dim).values
        # strictly before: shift by one along dim
        last = torch.cat([torch.full_like(last.narrow(dim, 0, 1), -1),
                          last.narrow(dim, 0, n - 1)], dim=dim)
        has = last >= 0
        idx = last.clamp(min=0).unsqueeze(1).expand(B, 2, H, W)
        got = v.gather(dim + 1, idx)
        if reverse:
            has, got = has.flip(dim), got.flip(dim + 1)
        return got, has

    total = torch.zeros_like(val)
    count = torch.zeros(B, H, W, dtype=torch.float32, device=dev)
    for dim, reverse in ((2, False), (2, True), (1, False), (1, True)):
        got, has = nearest(dim, reverse)
        total = total + torch.where(has.unsqueeze(1), got,
                                    torch.zeros_like(got))
        count = count + has.float()
    fill = torch.where((count > 0).unsqueeze(1),
                       total / count.clamp(min=1.0).unsqueeze(1),
                       torch.zeros_like(total))
    out = torch.where(cov.unsqueeze(1), val, fill)
    return out, ~cov.unsqueeze(1)
