"""The shortened motion-encoder front, on hardware.

Three kernels, each against the kernels it replaces on the same inputs,
bit for bit (``torch.equal``):

  * ``corr_lookup_conv1x1`` against ``corr_lookup_nhwc`` (bf16 out) ->
    ``fconv_plain`` 1x1: the tap arithmetic is one shared device function,
    the GEMM runs the same 32-wide chunks in the same order from a zero
    accumulator, bias then activation in the epilogue;
  * ``fconv_smallc_packed`` against ``fconv_smallk``: same k order, same
    chunks;
  * ``fconv_dflow_coords`` with ``flow_buf``: coords as without it, and
    the flow slice ``corr_lookup_nhwc`` writes for those coords.

Then the loop entry routes of the fused model (gated, captured,
bidirectional, warm start) with the three switches on against off.

Buffers a kernel reads are views into zero-tailed allocations (the
``_padded`` pattern of tests/test_gru_hoist_gpu.py). Shapes: (16, 24) has
four real pyramid levels, (9, 17) = 306 positions is a multiple of no tile
and ends in a 1x2 level, built as run_pair builds it; B=2, H=11, W in
(40, 300) give the conv kernels right-edge partial tiles and both row
borders.
"""
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
ACT_RELU = 1


def _hip():
    from raft_amd.ops import require_hip
    return require_hip()


def _padded(shape, dtype, fill):
    """A tensor of ``shape`` that is a view into a longer zero-tailed flat
    buffer: whatever a kernel reads just past its end is defined."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.zeros(n + 4096, device=DEV, dtype=dtype)
    t = flat[:n].view(*shape)
    t.copy_(fill)
    return t


def _pack(w, pad_cin=None):
    n, cin, kh, kw = w.shape
    cp = pad_cin or cin
    wp = w.new_zeros(n, cp, kh, kw)
    wp[:, :cin] = w
    return wp.permute(2, 3, 0, 1).reshape(kh * kw, n, cp).contiguous() \
        .to(torch.bfloat16)


# ------------------------------------------------- fused lookup -> conv1x1
def _levels(vol, fp8):
    """The pyramid of a [B, HW, H8, W8] fp32 volume as run_pair builds it
    (a level below 2 rows or columns repeats the last), as bf16 or e4m3."""
    lv = [vol]
    for _ in range(3):
        last = lv[-1]
        if last.shape[-2] < 2 or last.shape[-1] < 2:
            lv.append(last)
        else:
            lv.append(F.avg_pool2d(last, 2, 2))
    if fp8:
        return [_padded(l.shape, torch.uint8,
                        l.to(torch.float8_e4m3fn).view(torch.uint8))
                for l in lv]
    return [_padded(l.shape, torch.bfloat16, l) for l in lv]


def _coords(B, H8, W8, g):
    """The pixel grid plus noise of several pixels; a part at exact
    integers; positions driven far outside the frame on every side."""
    ys, xs = torch.meshgrid(
        torch.arange(H8, device=DEV, dtype=torch.float32),
        torch.arange(W8, device=DEV, dtype=torch.float32), indexing="ij")
    grid = torch.stack([xs, ys], dim=-1)[None].expand(B, -1, -1, -1)
    c = grid + torch.randn(B, H8, W8, 2, device=DEV, generator=g) * 3.0
    sel = torch.rand(B, H8, W8, 1, device=DEV, generator=g)
    c = torch.where(sel < 0.2, c.round(), c)          # exact integers
    c = c.contiguous()
    far = 1000.0
    c[:, 0, 0::4, 0] -= far                           # left
    c[:, 1, 1::4, 0] += far                           # right
    c[:, 2, 2::4, 1] -= far                           # above
    c[:, 3, 3::4, 1] += far                           # below
    c[:, 4, 0::3] -= far                              # above left
    c[:, 5, 1::3] += far                              # below right
    return _padded(c.shape, torch.float32, c)


@functools.lru_cache(maxsize=None)
def _lookup_case(H8, W8, radius, N, fp8):
    """Inputs and both paths' outputs of one case: computed once, shared,
    never modified."""
    hip = _hip()
    B = 2
    g = torch.Generator(device=DEV).manual_seed(97 * H8 + 13 * radius + N)
    vol = torch.randn(B, H8 * W8, H8, W8, device=DEV, generator=g) * 2.0
    lv = _levels(vol, fp8)
    coords = _coords(B, H8, W8, g)
    C = 4 * (2 * radius + 1) ** 2
    cpad = (C + 7) // 8 * 8
    w = torch.randn(N, C, 1, 1, device=DEV, generator=g) * 0.1
    bias = torch.randn(N, device=DEV, generator=g)
    wp = _padded((1, N, cpad), torch.bfloat16, _pack(w, cpad))
    vs = torch.full((1,), 0.37, device=DEV) if fp8 else None
    corr_buf = _padded((B, H8, W8, cpad), torch.bfloat16,
                       torch.zeros(B, H8, W8, cpad, device=DEV))
    taps = hip.corr_lookup_nhwc(list(lv), coords, radius, cpad, True,
                                corr_buf, None, 0, vs)
    pair = hip.fconv_plain(taps, None, wp, bias, 1, 1, ACT_RELU, None, 0, 0,
                           0, -1, -1, 1, None)
    fused = hip.corr_lookup_conv1x1(list(lv), coords, radius, wp, bias,
                                    ACT_RELU, vs)
    torch.cuda.synchronize()
    return dict(lv=lv, coords=coords, w=w, bias=bias, pair=pair, fused=fused,
                C=C, radius=radius)


LOOKUP_CASES = [(16, 24, 4, 256, False), (16, 24, 3, 96, False),
                (9, 17, 4, 256, False), (9, 17, 3, 96, False),
                (9, 17, 4, 256, True)]


@pytest.mark.gpu
@pytest.mark.parametrize(
    "H8,W8,radius,N,fp8", LOOKUP_CASES,
    ids=[f"{h}x{w}-r{r}-N{n}-{'e4m3' if f else 'bf16'}"
         for h, w, r, n, f in LOOKUP_CASES])
def test_lookup_conv_is_the_unfused_pair(H8, W8, radius, N, fp8):
    c = _lookup_case(H8, W8, radius, N, fp8)
    a, b = c["fused"], c["pair"]
    assert a.shape == b.shape == (2, H8, W8, N) and a.dtype == torch.bfloat16
    assert torch.isfinite(b.float()).all()
    assert float(b.float().abs().max()) > 0
    d = (a.float() - b.float()).abs()
    print(f"{H8}x{W8} r{radius} N{N} fp8={fp8}: {int((d > 0).sum())} of "
          f"{d.numel()} differ, max {d.max().item():.3e}")
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_lookup_conv_matches_fp32_composition():
    """Against relu(conv1x1(lookup)) of raft_amd/ops/torch_ref.py in fp32
    on the bf16 volume and bf16-rounded weights, at the fconv tolerance of
    tests/test_fused.py (0.05 * max|ref| + 0.05): ties the composition
    itself to the reference."""
    from raft_amd.ops import torch_ref as R
    c = _lookup_case(16, 24, 4, 256, False)
    pyr = [l.float() for l in c["lv"]]
    taps = R.corr_lookup(pyr, c["coords"], c["radius"])      # [B,C,H,W]
    ref = F.relu(F.conv2d(taps, c["w"].to(torch.bfloat16).float(),
                          c["bias"])).permute(0, 2, 3, 1)
    err = (c["fused"].float() - ref).abs().max().item()
    tol = 0.05 * ref.abs().max().item() + 0.05
    print(f"fused vs fp32 composition: err {err:.4f} tol {tol:.4f}")
    assert err < tol, (err, tol)


@pytest.mark.gpu
def test_lookup_conv_refuses_what_it_does_not_serve():
    hip = _hip()
    assert hip.lookup_conv_serves(7040, 324, 328, 256)
    assert hip.lookup_conv_serves(7040, 196, 200, 96)
    assert not hip.lookup_conv_serves(7040, 324, 328, 100)   # N % 16
    assert not hip.lookup_conv_serves(7040, 324, 324, 256)   # Cs % 8
    c = _lookup_case(9, 17, 3, 96, False)
    lv32 = [l.float() for l in c["lv"]]
    wp = _pack(c["w"], 200)
    with pytest.raises(RuntimeError, match="no kernel"):
        hip.corr_lookup_conv1x1(lv32, c["coords"], 3, wp, c["bias"], 1, None)
    torch.cuda.synchronize()


# ------------------------------------------------------------------ convf1
@pytest.mark.gpu
@pytest.mark.parametrize("W", (40, 300))
@pytest.mark.parametrize("kh,C,N,total,off",
                         [(7, 2, 128, 24, 14), (7, 2, 64, 24, 14),
                          (3, 4, 64, 4, 0)],
                         ids=["7x7-C2-N128", "7x7-C2-N64", "3x3-C4-N64"])
def test_convf1_packed_is_fconv_smallk(W, kh, C, N, total, off):
    from raft_amd.models.fused import pack_smallc
    hip = _hip()
    B, H = 2, 11
    g = torch.Generator(device=DEV).manual_seed(W + 10 * kh + N)
    x = _padded((B, H, W, total), torch.bfloat16,
                torch.randn(B, H, W, total, device=DEV, generator=g))
    w = torch.randn(N, C, kh, kh, device=DEV, generator=g) * 0.1
    bias = torch.randn(N, device=DEV, generator=g)
    wp = _pack(w)
    wpk = _padded((N, 128), torch.bfloat16, pack_smallc(wp))
    old = hip.fconv_smallk(x, wp, bias, kh, kh, ACT_RELU, off, C, 1)
    new = hip.fconv_smallc_packed(x, wpk, bias, kh, kh, ACT_RELU, off, C)
    torch.cuda.synchronize()
    ref = F.relu(F.conv2d(x[..., off:off + C].float().permute(0, 3, 1, 2),
                          w.to(torch.bfloat16).float(), bias,
                          padding=kh // 2)).permute(0, 2, 3, 1)
    err = (old.float() - ref).abs().max().item()
    d = (new.float() - old.float()).abs()
    print(f"{kh}x{kh} C{C} N{N} W{W}: smallk vs conv2d {err:.4f}; "
          f"{int((d > 0).sum())} of {d.numel()} differ")
    assert err < 0.05 * ref.abs().max().item() + 0.05
    assert torch.equal(new, old)


# --------------------------------------------------- delta-flow + flow_out
def run_dflow():
    """Body of the child process (one RAFT_AMD_TINYN2 setting). Returns
    the list of failures."""
    sys.path.insert(0, ROOT)
    hip = _hip()
    bad = []
    B, H, Cin, TOT, OFF = 2, 11, 72, 24, 14
    for W in (40, 300):
        g = torch.Generator(device=DEV).manual_seed(W)
        h1 = _padded((B, H, W, Cin), torch.bfloat16,
                     torch.randn(B, H, W, Cin, device=DEV, generator=g))
        wp = _padded((9, 2, Cin), torch.bfloat16,
                     torch.randn(9, 2, Cin, device=DEV, generator=g) * 0.1)
        bias = torch.randn(2, device=DEV, generator=g)
        coords = _coords(B, H, W, g)
        before = torch.randn(B, H, W, TOT, device=DEV, generator=g) \
            .to(torch.bfloat16)
        xbuf = _padded((B, H, W, TOT), torch.bfloat16, before)
        plain = hip.fconv_dflow_coords(h1, wp, bias, coords, 3, 3)
        new = hip.fconv_dflow_coords(h1, wp, bias, coords, 3, 3, xbuf, OFF)
        # what the lookup kernel writes as the flow of those coords
        lv = [_padded((B, H * W, 2, 2), torch.bfloat16,
                      torch.randn(B, H * W, 2, 2, device=DEV, generator=g))]
        want = torch.zeros(B, H, W, TOT, device=DEV, dtype=torch.bfloat16)
        hip.corr_lookup_nhwc(lv, plain, 1, 16, True, None, want, OFF)
        torch.cuda.synchronize()
        ref = coords + F.conv2d(
            h1.float().permute(0, 3, 1, 2),
            wp.float().reshape(3, 3, 2, Cin).permute(2, 3, 0, 1), bias,
            padding=1).permute(0, 2, 3, 1)
        err = (plain - ref).abs().max().item()
        print(f"W={W}: coords vs conv2d {err:.2e}", flush=True)
        if not err < 1e-2:
            bad.append(f"W={W}: coords off the conv2d reference by {err}")
        if not torch.equal(new, plain):
            bad.append(f"W={W}: coords_out changed by flow_buf")
        if not torch.equal(xbuf[..., OFF:OFF + 2], want[..., OFF:OFF + 2]):
            bad.append(f"W={W}: flow slice differs from the lookup's")
        if not (torch.equal(xbuf[..., :OFF], before[..., :OFF]) and
                torch.equal(xbuf[..., OFF + 2:], before[..., OFF + 2:])):
            bad.append(f"W={W}: neighbouring channels were written")
        # the loop-entry kernel writes the same slice
        ent = _padded((B, H, W, TOT), torch.bfloat16, before)
        hip.flow_slice(plain, ent, OFF)
        torch.cuda.synchronize()
        if not torch.equal(ent, xbuf):
            bad.append(f"W={W}: flow_slice differs from the delta-flow write")
    return bad


@pytest.mark.gpu
@pytest.mark.parametrize("tinyn2", (0, 1))
def test_dflow_writes_the_next_flow_slice(tinyn2):
    env = dict(os.environ, RAFT_AMD_TINYN2=str(tinyn2))
    argv = [sys.executable]
    if sys.flags.no_user_site:
        argv.append("-s")
    argv += [os.path.abspath(__file__), "dflow"]
    # one child, no retry: a fault, abort or hang fails the case as it is
    r = subprocess.run(argv, env=env, capture_output=True, text=True,
                       timeout=180)
    print(r.stdout[-2000:])
    assert r.returncode == 0, \
        f"child exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"


# ------------------------------------------------------- loop entry routes
SWITCHES = ("RAFT_AMD_EARLY_FORK", "RAFT_AMD_LOOKUP_CONV",
            "RAFT_AMD_CONVF1_PACKED")


@functools.lru_cache(maxsize=None)
def _models(small):
    """(on, off): the same weights with the three switches at their
    defaults and at 0 (read when the fused runner is built)."""
    from raft_amd import RAFT, RaftConfig
    from raft_amd.models.fused import get_fused
    torch.manual_seed(23)
    out = []
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        ref = None
        for val in (None, "0"):
            for k in SWITCHES:
                if val is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = val
            m = RAFT(RaftConfig(small=small)).to(DEV).to(torch.bfloat16) \
                .eval()
            if ref is None:
                ref = m
            else:
                m.load_state_dict(ref.state_dict())
            f = get_fused(m)
            on = val is None
            assert f.early_fork == on and f.lookup_conv == on and \
                f.convf1_packed == on
            out.append(m)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return tuple(out)


def _images():
    g = torch.Generator(device=DEV).manual_seed(5)
    return [torch.rand(1, 3, 64, 96, device=DEV, generator=g)
            .to(torch.bfloat16) for _ in range(2)]


ROUTES = ("eager", "captured", "gated", "gated-captured", "bidirectional",
          "warm-start")


@pytest.mark.gpu
@pytest.mark.parametrize("small", (False, True), ids=("things", "small"))
@pytest.mark.parametrize("route", ROUTES)
def test_route_matches_switches_off(route, small):
    from raft_amd import Convergence
    on, off = _models(small)
    x1, x2 = _images()
    kw, graph, iters = {}, False, 4
    if route == "captured":
        graph = None                      # auto: iters <= 16 captures
    elif route == "gated":
        kw = dict(converge=Convergence(tol=1e-6, every=2))
        iters = 6
    elif route == "gated-captured":
        kw = dict(converge=Convergence(tol=1e-6, every=2))
        graph, iters = None, 6
    elif route == "bidirectional":
        kw = dict(bidirectional=True)
    elif route == "warm-start":
        g = torch.Generator(device=DEV).manual_seed(9)
        kw = dict(flow_init=torch.randn(1, 2, 8, 12, device=DEV,
                                        generator=g) * 2.0)
    outs = []
    with torch.no_grad():
        for m in (on, off):
            m._fused_use_graph = graph
            o = m(x1, x2, iters=iters, **kw)
            o = o if isinstance(o, tuple) else (o,)
            outs.append([t.float().clone() for t in o])
            torch.cuda.synchronize()
            if graph is None:
                assert len(m._fused_cache._graphs) >= 1
    for a, b in zip(*outs):
        assert torch.isfinite(a).all()
        assert float(a.abs().max()) > 0
        assert torch.equal(a, b), (a - b).abs().max().item()


if __name__ == "__main__":
    assert sys.argv[1] == "dflow"
    failures = run_dflow()
    for line in failures:
        print("FAIL", line)
    sys.exit(1 if failures else 0)
