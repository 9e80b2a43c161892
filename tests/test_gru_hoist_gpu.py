"""The GRU context hoist, on hardware.

x = [inp | rest] feeds every GRU conv together with h, and inp (the
context features) is the same in all refinement iterations. The hoisted
path computes conv(inp) once as an fp32 tensor (``fconv_plain_f32``, the
EP_PLAIN_F32 epilogue, bias folded in) and lets the per-iteration convs
read [h | rest] — rest as an in-place slice of x — and add that term
(``fconv_gru_zr_pre`` / ``fconv_gru_q_pre``).

Shapes follow tests/test_fconv_variants.py, the smallest that reach every
staging branch: B=2, H=11, W in (40, 300), hd=32, x of 76 channels split
as inp = the first 40 (a multiple of 8) and rest = 36 (no multiple of 8
or 32), kernel shapes 1x5, 5x1 and 3x3.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

B, H, HD, XD, CTX = 2, 11, 32, 76, 40
REST = XD - CTX
WIDTHS = (40, 300)
SHAPES = ((1, 5), (5, 1), (3, 3))
DEV = "cuda:0"


def _hip():
    from raft_amd.ops import require_hip
    return require_hip()


def _pack(w):
    n, cin, kh, kw = w.shape
    return w.permute(2, 3, 0, 1).reshape(kh * kw, n, cin).contiguous() \
        .to(torch.bfloat16)


def _conv(x_nhwc, w, bias, kh, kw, dtype=torch.float32):
    """SAME conv of an NHWC tensor with bf16-rounded weights, in dtype."""
    y = F.conv2d(x_nhwc.to(dtype).permute(0, 3, 1, 2),
                 w.to(torch.bfloat16).to(dtype),
                 None if bias is None else bias.to(dtype),
                 padding=(kh // 2, kw // 2))
    return y.permute(0, 2, 3, 1)


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


@functools.lru_cache(maxsize=None)
def _case(W, kh, kw):
    """Inputs, weights, both kernel paths' outputs and the references of one
    (width, kernel shape) — computed once, shared by the tests, never
    modified."""
    hip = _hip()
    g = torch.Generator(device=DEV).manual_seed(1000 * W + 10 * kh + kw)

    def rn(*s, scale=1.0):
        return torch.randn(*s, device=DEV, generator=g) * scale

    h = rn(B, H, W, HD, scale=0.5).to(torch.bfloat16)
    x = _padded((B, H, W, XD), torch.bfloat16, rn(B, H, W, XD, scale=0.5))
    wzr, bzr = rn(2 * HD, HD + XD, kh, kw, scale=0.1), rn(2 * HD)
    wq, bq = rn(HD, HD + XD, kh, kw, scale=0.1), rn(HD)
    c = dict(h=h, x=x, wzr=wzr, bzr=bzr, wq=wq, bq=bq)

    # split the columns [W_h | W_inp | W_rest]
    def loop_w(w):
        return _pack(torch.cat([w[:, :HD], w[:, HD + CTX:]], dim=1))

    w_all = torch.cat([wzr, wq], dim=0)                  # rows z, r, q
    c["pre_w4"] = w_all[:, HD:HD + CTX]                  # [3hd, ctx, kh, kw]
    c["pre_b"] = torch.cat([bzr, bq]).contiguous()
    c["pre"] = hip.fconv_plain_f32(x, _pack(c["pre_w4"]), c["pre_b"], kh, kw,
                                   0, CTX)
    # present kernels: full x, with bias
    c["z0"], c["rh0"] = hip.fconv_gru_zr(h, x, _pack(wzr), bzr, kh, kw)
    c["hn0"] = hip.fconv_gru_q(c["rh0"], x, _pack(wq), bq, kh, kw, c["z0"], h)
    # hoisted: rest slice of x in place, plus pre, no bias. The candidate
    # stage runs on the present kernels' rh and z, so that both candidate
    # convs see the same inputs.
    c["z1"], c["rh1"] = hip.fconv_gru_zr_pre(h, x, loop_w(wzr), kh, kw,
                                             c["pre"], 0, CTX, REST)
    c["hn1"] = hip.fconv_gru_q_pre(c["rh0"], x, loop_w(wq), kh, kw, c["z0"],
                                   h, c["pre"], 2 * HD, CTX, REST)
    torch.cuda.synchronize()
    return c


CASES = [(W, kh, kw) for W in WIDTHS for kh, kw in SHAPES]
IDS = [f"W{W}-{kh}x{kw}" for W, kh, kw in CASES]


@pytest.mark.parametrize("W,kh,kw", CASES, ids=IDS)
def test_precompute_fp32_output(W, kh, kw):
    """EP_PLAIN_F32 against an fp64 conv of the same bf16 values. The only
    error is the fp32 summation of K = taps*ctx exact products, bounded by
    K * 2^-23 * (sum of |products| + |bias|)."""
    c = _case(W, kh, kw)
    inp = c["x"][..., :CTX]
    ref = _conv(inp, c["pre_w4"], c["pre_b"], kh, kw, torch.float64)
    mag = _conv(inp.abs(), c["pre_w4"].abs(), c["pre_b"].abs(), kh, kw,
                torch.float64)
    K = kh * kw * CTX
    tol = K * 2.0 ** -23 * mag.max().item()
    assert c["pre"].dtype == torch.float32
    assert c["pre"].shape == (B, H, W, 3 * HD)
    err = (c["pre"].double() - ref).abs().max().item()
    print(f"pre {kh}x{kw} W={W}: err {err:.3e} tol {tol:.3e}")
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("W,kh,kw", CASES, ids=IDS)
def test_hoisted_matches_present_kernels(W, kh, kw):
    """Both paths round the same pre-activation, summed in another order,
    to bf16: at most one bf16 ulp apart."""
    c = _case(W, kh, kw)
    for tag, a, b in (("z", c["z1"], c["z0"]), ("rh", c["rh1"], c["rh0"]),
                      ("h'", c["hn1"], c["hn0"])):
        a, b = a.float(), b.float()
        d = (a - b).abs()
        bound = 2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 1e-6
        print(f"{tag} {kh}x{kw} W={W}: max |a-b| {d.max().item():.3e}, "
              f"{int((d > 0).sum())} of {d.numel()} differ, worst "
              f"excess {(d - bound).max().item():.3e}")
        assert bool((d <= bound).all()), tag


@pytest.mark.parametrize("W,kh,kw", CASES, ids=IDS)
def test_hoisted_matches_conv2d(W, kh, kw):
    """Hoisted outputs against F.conv2d, tolerance of
    test_fconv_gru_pair_matches_eager."""
    c = _case(W, kh, kw)
    h, x = c["h"], c["x"]
    zr = torch.sigmoid(_conv(torch.cat([h, x], dim=-1), c["wzr"], c["bzr"],
                             kh, kw))
    q = torch.tanh(_conv(torch.cat([c["rh0"], x], dim=-1), c["wq"], c["bq"],
                         kh, kw))
    z0 = c["z0"].float()
    for tag, got, ref in (
            ("z", c["z1"], zr[..., :HD]),
            ("rh", c["rh1"], zr[..., HD:] * h.float()),
            ("h'", c["hn1"], (1.0 - z0) * h.float() + z0 * q)):
        err = (got.float() - ref).abs().max().item()
        print(f"{tag} {kh}x{kw} W={W}: err {err:.4f}")
        assert err < 0.08, (tag, err)


@pytest.mark.parametrize("W", WIDTHS)
@pytest.mark.parametrize("kh,kw", SHAPES)
@pytest.mark.parametrize("width,off,total", [(76, 40, 116), (82, 64, 146)],
                         ids=["76at40of116", "82at64of146"])
def test_in_place_slice_is_bit_identical(W, kh, kw, width, off, total):
    """in2 as a slice of a wider buffer against a contiguous copy of the
    slice. 82 at 64 of 146 is raft-small's layout: the slice ends inside a
    k-step (k-tail) and its rows are not 16-byte aligned."""
    hip = _hip()
    g = torch.Generator(device=DEV).manual_seed(width + W + kh)

    def rn(*s, scale=1.0):
        return torch.randn(*s, device=DEV, generator=g) * scale

    wide = _padded((B, H, W, total), torch.bfloat16,
                   rn(B, H, W, total, scale=0.5))
    tight = _padded((B, H, W, width), torch.bfloat16,
                    wide[..., off:off + width])
    h = rn(B, H, W, HD, scale=0.5).to(torch.bfloat16)
    z = torch.rand(B, H, W, HD, device=DEV, generator=g).to(torch.bfloat16)
    pre = rn(B, H, W, 3 * HD)
    wzr = _pack(rn(2 * HD, HD + width, kh, kw, scale=0.1))
    wq = _pack(rn(HD, HD + width, kh, kw, scale=0.1))
    za, rha = hip.fconv_gru_zr_pre(h, wide, wzr, kh, kw, pre, 0, off, width)
    zb, rhb = hip.fconv_gru_zr_pre(h, tight, wzr, kh, kw, pre, 0, 0, width)
    qa = hip.fconv_gru_q_pre(h, wide, wq, kh, kw, z, h, pre, 2 * HD, off,
                             width)
    qb = hip.fconv_gru_q_pre(h, tight, wq, kh, kw, z, h, pre, 2 * HD, 0,
                             width)
    assert torch.isfinite(za.float()).all() and torch.isfinite(qa.float()).all()
    assert torch.equal(za, zb)
    assert torch.equal(rha, rhb)
    assert torch.equal(qa, qb)


@pytest.mark.parametrize("small", [False, True], ids=["things", "small"])
def test_model_hoist_on_and_off_match_eager(small, monkeypatch):
    """As test_fused_model_matches_eager_bf16, with the switch at 0 and at
    1 on the same weights; then the captured loop against the uncaptured
    one with the hoist on, as test_loop_graph_auto_policy."""
    from raft_amd import RAFT, RaftConfig
    import raft_amd.models.fused as fused
    torch.manual_seed(11)
    m = RAFT(RaftConfig(small=small)).to(DEV).to(torch.bfloat16).eval()
    x1 = torch.rand(1, 3, 64, 96, device=DEV, dtype=torch.bfloat16)
    x2 = torch.rand(1, 3, 64, 96, device=DEV, dtype=torch.bfloat16)
    with torch.no_grad():
        monkeypatch.setenv("RAFT_AMD_NO_FUSE", "1")
        ref = m(x1, x2, iters=4)
        monkeypatch.delenv("RAFT_AMD_NO_FUSE")
        assert fused.can_fuse(m, x1)
        outs, errs = {}, {}
        for hoist, graph in (("0", False), ("1", False), ("1", True)):
            mh = RAFT(RaftConfig(small=small)).to(DEV).to(torch.bfloat16) \
                .eval()
            mh.load_state_dict(m.state_dict())
            mh._fused_use_graph = graph
            monkeypatch.setenv("RAFT_AMD_GRU_HOIST", hoist)
            out = mh(x1, x2, iters=4)
            f = mh._fused_cache
            assert f.gru_hoist == (hoist == "1")
            assert len(f._graphs) == (1 if graph else 0)
            assert out.shape == ref.shape
            outs[hoist, graph] = out.float().clone()
            errs[hoist, graph] = (out.float() - ref.float()).abs().max() \
                .item()
            del mh._fused_cache          # releases a captured graph's pool
            torch.cuda.synchronize()
    print(f"small={small}: err vs eager  hoist off {errs['0', False]:.5f}  "
          f"hoist on {errs['1', False]:.5f}")
    assert errs["1", False] < 0.05, errs
    assert errs["0", False] < 0.05, errs
    d = (outs["1", True] - outs["1", False]).abs().max().item()
    print(f"small={small}: captured vs uncaptured, hoist on: {d:.2e}")
    assert torch.allclose(outs["1", True], outs["1", False], atol=1e-3), d


def test_binding_checks_raise():
    hip = _hip()
    W, kh, kw = 40, 1, 5
    h = torch.zeros(B, H, W, HD, device=DEV, dtype=torch.bfloat16)
    x = torch.zeros(B, H, W, XD, device=DEV, dtype=torch.bfloat16)
    wzr = torch.zeros(kh * kw, 2 * HD, HD + REST, device=DEV,
                      dtype=torch.bfloat16)
    wq = torch.zeros(kh * kw, HD, HD + REST, device=DEV,
                     dtype=torch.bfloat16)
    pre = torch.zeros(B, H, W, 3 * HD, device=DEV)
    # the well-formed calls pass
    hip.fconv_gru_zr_pre(h, x, wzr, kh, kw, pre, 0, CTX, REST)
    hip.fconv_gru_q_pre(h, x, wq, kh, kw, h, h, pre, 2 * HD, CTX, REST)
    # in2 offset no multiple of 8 (slice still inside x, weights matching)
    w35 = torch.zeros(kh * kw, 2 * HD, HD + 35, device=DEV,
                      dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        hip.fconv_gru_zr_pre(h, x, w35, kh, kw, pre, 0, CTX + 1, 35)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        hip.fconv_gru_q_pre(h, x, wq, kh, kw, h, h, pre, 2 * HD, 4, REST)
    # slice past the end of x
    with pytest.raises(RuntimeError, match="exceeds"):
        hip.fconv_gru_zr_pre(h, x, wzr, kh, kw, pre, 0, CTX + 8, REST)
    # pre of the wrong dtype
    with pytest.raises(RuntimeError, match="fp32"):
        hip.fconv_gru_zr_pre(h, x, wzr, kh, kw, pre.to(torch.bfloat16), 0,
                             CTX, REST)
    with pytest.raises(RuntimeError, match="fp32"):
        hip.fconv_gru_q_pre(h, x, wq, kh, kw, h, h, pre.double(), 2 * HD,
                            CTX, REST)
    # pre not contiguous
    with pytest.raises(RuntimeError, match="contiguous"):
        hip.fconv_gru_zr_pre(h, x, wzr, kh, kw,
                             torch.zeros(B, H, W, 6 * HD, device=DEV)[..., ::2],
                             0, CTX, REST)
    # pre_off + N > pre_stride
    with pytest.raises(RuntimeError, match="exceeds pre"):
        hip.fconv_gru_zr_pre(h, x, wzr, kh, kw, pre, HD + 1, CTX, REST)
    with pytest.raises(RuntimeError, match="exceeds pre"):
        hip.fconv_gru_q_pre(h, x, wq, kh, kw, h, h, pre, 2 * HD + 1, CTX,
                            REST)
    torch.cuda.synchronize()
