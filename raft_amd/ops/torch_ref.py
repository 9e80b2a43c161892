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


def _splat_keys(tx: torch.Tensor, ty: torch.Tensor):
    """Nearest-source splat of the targets (tx, ty), each [B,H,W] fp32, of
    the source cells of a [B,H,W] grid: per cell the minimum 64-bit key
    (float_bits(d2) << 32) | source_index over the valid targets whose
    {floor, floor+1}^2 neighbourhood holds the cell (see forward_project).
    Returns (keys [B*H*W] int64, the value of a cell without candidate)."""
    B, H, W = tx.shape
    HW = H * W
    dev = tx.device
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
    return keys, empty


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
    keys, empty = _splat_keys(tx, ty)

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


def flow_residual(prev: torch.Tensor, nxt: torch.Tensor, thr_sq: float):
    """Size of one refinement update — what the convergence gate measures.
    This definition is the contract: the HIP kernel
    (csrc/flow_residual.hip) matches it bit for bit.

    prev, nxt: [B,2,H,W] fp32, the 1/8-grid coordinates before and after
    one iteration. Returns ``(max_sq [B] fp32, above [B] int64)``.

    Per cell dx = nxt.x - prev.x, dy = nxt.y - prev.y and d2 = dx*dx +
    dy*dy, all fp32, each operation rounded on its own (no FMA).
    ``max_sq[b]`` is the maximum of d2 over the cells of sample b: NaN (any
    payload) if any cell is NaN, +inf orders normally. ``above[b]`` counts
    the cells with ``not (d2 <= thr_sq)`` (thr_sq rounded to fp32): a cell
    at exactly thr_sq is not above, a NaN cell is.
    """
    if prev.dim() != 4 or prev.shape[1] != 2 or prev.shape != nxt.shape:
        raise ValueError(f"prev and nxt must both be [B,2,H,W], got "
                         f"{tuple(prev.shape)} and {tuple(nxt.shape)}")
    B = prev.shape[0]
    d = nxt.detach().float() - prev.detach().float()
    dx, dy = d[:, 0], d[:, 1]
    xx = dx * dx
    yy = dy * dy
    d2 = (xx + yy).reshape(B, -1)
    thr = torch.tensor(thr_sq, dtype=torch.float32, device=d2.device)
    above = (~(d2 <= thr)).sum(dim=1)
    if d2.shape[1] == 0:
        return d2.new_zeros(B), above
    return d2.max(dim=1).values, above       # torch's max propagates NaN


def _check_interp_args(im0, im1, flow_fw, flow_bw, occ_fw, occ_bw, t):
    """Argument contract of interpolate_frame; returns t as a float."""
    try:
        t = float(t)
    except (TypeError, ValueError):
        raise ValueError(f"t must be a number in [0, 1], got {t!r}")
    if not 0.0 <= t <= 1.0:           # NaN fails both comparisons
        raise ValueError(f"t must lie in [0, 1], got {t}")
    if im0.dim() != 4 or im0.shape[1] < 1 or im0.shape != im1.shape:
        raise ValueError(f"images must both be [B,C,H,W] with C >= 1, got "
                         f"{tuple(im0.shape)} and {tuple(im1.shape)}")
    B, _, H, W = im0.shape
    for name, f in (("flow_fw", flow_fw), ("flow_bw", flow_bw)):
        if f.dim() != 4 or tuple(f.shape) != (B, 2, H, W):
            raise ValueError(f"{name} must be [B,2,H,W] = {(B, 2, H, W)}, "
                             f"got {tuple(f.shape)}")
    for name, m in (("occ_fw", occ_fw), ("occ_bw", occ_bw)):
        if m.dim() != 4 or tuple(m.shape) != (B, 1, H, W):
            raise ValueError(f"{name} must be [B,1,H,W] = {(B, 1, H, W)}, "
                             f"got {tuple(m.shape)}")
    return t


def interpolate_frame(im0: torch.Tensor, im1: torch.Tensor,
                      flow_fw: torch.Tensor, flow_bw: torch.Tensor,
                      occ_fw: torch.Tensor, occ_bw: torch.Tensor, t: float):
    """The frame at time t in [0, 1] between ``im0`` (t=0) and ``im1``
    (t=1), from their bidirectional flows and occlusion masks. This
    definition is the contract: the HIP kernels (csrc/frame_interp.hip)
    match it bit for bit.

    im0, im1: [B,C,H,W] (computed in fp32); flow_fw (0->1), flow_bw (1->0):
    [B,2,H,W] fp32; occ_fw, occ_bw: [B,1,H,W] bool as fb_consistency
    returns them. Returns (frame [B,C,H,W] fp32, flow_t0, flow_t1
    [B,2,H,W] fp32, cover [B,1,H,W] uint8: bit 0 = splat A, bit 1 =
    splat B).

    With tf = float32(t), u = 1 - tf, every product and sum a separately
    rounded fp32 operation (no FMA), divisions correctly rounded:

    1. Splats (the scatter rules of forward_project): source p of frame 0
       targets p + tf*flow_fw[p] (A), source p of frame 1 targets
       p + u*flow_bw[p] (B). Per cell q: coverA, gA = flow_fw[winnerA],
       coverB, gB = flow_bw[winnerB].
    2. Ft0 = (-tf)*gA if coverA, else tf*gB if coverB; Ft1 = (-u)*gB if
       coverB, else u*gA if coverA; with neither, the linear approximation
       Ft0 = (-(u*tf))*fw[q] + (tf*tf)*bw[q],
       Ft1 = (u*u)*fw[q] + (-(tf*u))*bw[q].
    3. x0 = q + Ft0, x1 = q + Ft1; in0 / in1 = inside the frame (NaN is
       outside); o0 = occ_fw at the cell nearest x0, o1 = occ_bw at the
       cell nearest x1 (round half to even, clamped, NaN -> 0);
       v0 = in0 and not o1, v1 = in1 and not o0; (w0, w1) = (u if v0 else
       0, tf if v1 else 0), and (u, tf) when that sum is 0.
    4. S0 / S1 = bilinear samples of im0 at x0 / im1 at x1 in the
       convention of fb_consistency (clamped corners, weights clamped to
       [0,1], NaN -> corner 0 and weight 0, summed as
       ((w00*a + w01*b) + w10*c) + w11*d);
       frame = (w0*S0 + w1*S1) / (w0 + w1).

    t=0 returns im0 and t=1 returns im1 bit for bit (for finite flows);
    swapping the frames, the flows and the masks and replacing t by 1-t
    gives the same frame with flow_t0 / flow_t1 exchanged.
    """
    t = _check_interp_args(im0, im1, flow_fw, flow_bw, occ_fw, occ_bw, t)
    a0 = im0.float().contiguous()
    a1 = im1.float().contiguous()
    fw = flow_fw.float().contiguous()
    bw = flow_bw.float().contiguous()
    B, C, H, W = a0.shape
    dev = a0.device
    HW = H * W
    if B * HW == 0:
        return (a0.clone(), fw.clone(), bw.clone(),
                torch.zeros(B, 1, H, W, dtype=torch.uint8, device=dev))

    # the scalars, rounded to fp32 one operation at a time on the host
    c = torch.tensor([t], dtype=torch.float32)
    tf = c.item()
    u = (1.0 - c).item()
    ut = ((1.0 - c) * c).item()
    tt = (c * c).item()
    uu = ((1.0 - c) * (1.0 - c)).item()

    xs = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    ys = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)

    def splat(f, s):
        keys, empty = _splat_keys(xs + s * f[:, 0], ys + s * f[:, 1])
        cov = (keys != empty).view(B, 1, H, W)
        winner = (keys & 0xFFFFFFFF).view(B, 1, HW).expand(B, 2, HW)
        winner = torch.where(cov.view(B, 1, HW), winner,
                             torch.zeros_like(winner))
        return cov, f.view(B, 2, HW).gather(2, winner).view(B, 2, H, W)

    cov_a, g_a = splat(fw, tf)
    cov_b, g_b = splat(bw, u)
    ft0 = torch.where(cov_a, (-tf) * g_a, torch.where(
        cov_b, tf * g_b, (-ut) * fw + tt * bw))
    ft1 = torch.where(cov_b, (-u) * g_b, torch.where(
        cov_a, u * g_a, uu * fw + (-ut) * bw))
    cover = cov_a.to(torch.uint8) | (cov_b.to(torch.uint8) << 1)

    def inside(px, py):
        return (px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)

    def nearest(mask, px, py):
        xr = torch.nan_to_num(px.round(), nan=0.0).clamp(0, W - 1).long()
        yr = torch.nan_to_num(py.round(), nan=0.0).clamp(0, H - 1).long()
        idx = (yr * W + xr).view(B, 1, HW)
        return mask.reshape(B, 1, HW).gather(2, idx).view(B, H, W) != 0

    def sample(img, px, py):
        x0f = torch.nan_to_num(px.floor(), nan=0.0).clamp(0, W - 1)
        y0f = torch.nan_to_num(py.floor(), nan=0.0).clamp(0, H - 1)
        x0, y0 = x0f.long(), y0f.long()
        x1 = (x0 + 1).clamp(max=W - 1)
        y1 = (y0 + 1).clamp(max=H - 1)
        ax = torch.nan_to_num(px - x0f, nan=0.0).clamp(0, 1)
        ay = torch.nan_to_num(py - y0f, nan=0.0).clamp(0, 1)
        w00 = ((1 - ax) * (1 - ay)).unsqueeze(1)
        w01 = (ax * (1 - ay)).unsqueeze(1)
        w10 = ((1 - ax) * ay).unsqueeze(1)
        w11 = (ax * ay).unsqueeze(1)
        flat = img.view(B, C, HW)

        def tap(yi, xi):
            idx = (yi * W + xi).view(B, 1, HW).expand(B, C, HW)
            return flat.gather(2, idx).view(B, C, H, W)

        return ((w00 * tap(y0, x0) + w01 * tap(y0, x1))
                + w10 * tap(y1, x0)) + w11 * tap(y1, x1)

    p0x, p0y = xs + ft0[:, 0], ys + ft0[:, 1]
    p1x, p1y = xs + ft1[:, 0], ys + ft1[:, 1]
    o0 = nearest(occ_fw, p0x, p0y)
    o1 = nearest(occ_bw, p1x, p1y)
    v0 = inside(p0x, p0y) & ~o1
    v1 = inside(p1x, p1y) & ~o0
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    w0 = torch.where(v0, zero + u, zero)
    w1 = torch.where(v1, zero + tf, zero)
    none = (w0 + w1) == 0
    w0 = torch.where(none, zero + u, w0).unsqueeze(1)
    w1 = torch.where(none, zero + tf, w1).unsqueeze(1)
    frame = (w0 * sample(a0, p0x, p0y) + w1 * sample(a1, p1x, p1y)) \
        / (w0 + w1)
    return frame, ft0, ft1, cover
