"""GPU tests for frame interpolation: the frame_interp kernels against the
oracle (bit for bit), bf16 images, determinism and graph capture, and the
engine / session on the fused bf16 path."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from raft_amd.ops import torch_ref as R

TIMES = (0.0, 0.3, 0.5, 1.0)

# (B, C, H, W, amp, seed): batch stride and odd sizes; one ragged block; a
# multiple of the block with an even channel count; more cells per row
# than a block next to an odd channel count. amp scales the smooth flow so
# that its slope exceeds 2 px per cell somewhere (see _inputs).
SHAPES = [(2, 3, 37, 53, 24.0, 0), (1, 1, 5, 7, 3.0, 1),
          (1, 4, 64, 96, 40.0, 2), (1, 3, 8, 300, 40.0, 3)]


def _hip():
    from raft_amd.ops import require_hip
    return require_hip()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _inputs(B, C, H, W, amp, seed):
    """_fb_inputs-style smooth fields (test_bidirectional_gpu), scaled up:
    a splat to t = 0.5 leaves a cell uncovered only where neighbouring
    targets are more than 2 cells apart, i.e. where the flow's slope
    exceeds 2 px per cell, and collides where the slope is below -1."""
    g = torch.Generator().manual_seed(seed)
    gh, gw = min(5, H), min(7, W)
    fw = F.interpolate(torch.randn(B, 2, gh, gw, generator=g) * amp,
                       size=(H, W), mode="bilinear", align_corners=True)
    bw = -fw + torch.randn(B, 2, H, W, generator=g) * 0.4
    im0 = torch.rand(B, C, H, W, generator=g)
    im1 = torch.rand(B, C, H, W, generator=g)
    occ_fw = torch.rand(B, 1, H, W, generator=g) < 0.35
    occ_bw = torch.rand(B, 1, H, W, generator=g) < 0.35
    return im0, im1, fw.contiguous(), bw.contiguous(), occ_fw, occ_bw


_REF = {}


def _reference(case, t):
    """Inputs and CPU oracle outputs, computed once per (case, t) and
    shared (never modified) by the tests below."""
    key = (case, t)
    if key not in _REF:
        args = _inputs(*case)
        _REF[key] = (args, R.interpolate_frame(*args, t))
    return _REF[key]


def _situations(fw, t):
    """(share of targets that leave the frame, number of valid sources
    that win no cell at all, i.e. lost every collision) of splat A."""
    B, _, H, W = fw.shape
    xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
    ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
    tx, ty = xs + t * fw[:, 0], ys + t * fw[:, 1]
    valid = (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
    keys, empty = R._splat_keys(tx, ty)
    keys = keys.view(B, H * W)
    lost = 0
    for b in range(B):
        winners = (keys[b][keys[b] != empty] & 0xFFFFFFFF).unique()
        lost += int(valid[b].sum().item()) - winners.numel()
    return 1.0 - valid.float().mean().item(), lost


def _same(got, want):
    """torch.equal, with NaN equal to NaN (the payload bits of a NaN that
    an arithmetic operation produces are the hardware's, not the
    definition's)."""
    got, want = got.cpu(), want.cpu()
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if not got.is_floating_point():
        return torch.equal(got, want)
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and \
        torch.equal(got[~nan], want[~nan])


# ------------------------------------------------------------------ kernel
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "x".join(
    str(v) for v in c[:4]))
def test_inputs_hold_all_three_situations(case):
    """Targets that leave the frame, collisions and cells that neither
    splat reaches all occur in every case's inputs (at t = 0.5)."""
    (im0, im1, fw, bw, occ_fw, occ_bw), ref = _reference(case, 0.5)
    for flow in (fw, bw):
        out, lost = _situations(flow, 0.5)
        assert 0.0 < out < 1.0
        assert lost > 0
    cover = ref[3]
    assert (cover == 0).any() and (cover == 3).any()
    assert (occ_fw & occ_bw).any()


@pytest.mark.parametrize("t", TIMES)
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "x".join(
    str(v) for v in c[:4]))
def test_interpolate_frame_matches_oracle_exactly(dev, case, t):
    from raft_amd import ops
    args, ref = _reference(case, t)
    im0, im1, fw, bw, occ_fw, occ_bw = (a.to(dev) for a in args)
    out = _hip().interpolate_frame(im0, im1, fw, bw,
                                   occ_fw.view(torch.uint8),
                                   occ_bw.view(torch.uint8), t)
    assert len(out) == 4
    for got, want, name in zip(out, ref, ("frame", "flow_t0", "flow_t1",
                                          "cover")):
        assert got.dtype == want.dtype and got.shape == want.shape, name
        assert torch.equal(got.cpu(), want), name
    pub = ops.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw, t)
    for got, want in zip(pub, out):
        assert torch.equal(got, want)
    if t == 0.0:
        assert torch.equal(out[0], im0)
    if t == 1.0:
        assert torch.equal(out[0], im1)
    # the oracle computes the same on the device's own tensors
    if t == 0.3:
        dev_ref = R.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw, t)
        for got, want in zip(out, dev_ref):
            assert torch.equal(got, want)


@pytest.mark.parametrize("t", TIMES)
def test_nan_and_inf_flows(dev, t):
    from raft_amd import ops
    im0, im1, fw, bw, occ_fw, occ_bw = _inputs(2, 3, 37, 53, 24.0, 4)
    fw, bw = fw.clone(), bw.clone()
    g = torch.Generator().manual_seed(9)
    for flow in (fw, bw):
        flat = flow.view(-1)
        idx = torch.randperm(flat.numel(), generator=g)[:90]
        flat[idx[:30]] = float("nan")
        flat[idx[30:60]] = float("inf")
        flat[idx[60:]] = float("-inf")
    ref = R.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw, t)
    out = ops.interpolate_frame(*(a.to(dev) for a in (im0, im1, fw, bw,
                                                      occ_fw, occ_bw)), t)
    # an uncovered cell with a non-finite flow of its own keeps a
    # non-finite intermediate flow; the frame never does
    if t == 0.5:
        assert ref[1].isnan().any() and ref[1].isinf().any()
    assert torch.isfinite(ref[0]).all()
    for got, want, name in zip(out, ref, ("frame", "flow_t0", "flow_t1",
                                          "cover")):
        assert _same(got, want), name
    assert torch.equal(out[0].cpu(), ref[0])
    assert torch.equal(out[3].cpu(), ref[3])


def test_bf16_images_equal_their_fp32_upcast(dev):
    from raft_amd import ops
    args, _ = _reference(SHAPES[0], 0.3)
    im0, im1, fw, bw, occ_fw, occ_bw = (a.to(dev) for a in args)
    h0, h1 = im0.to(torch.bfloat16), im1.to(torch.bfloat16)
    got = ops.interpolate_frame(h0, h1, fw, bw, occ_fw, occ_bw, 0.3)
    want = ops.interpolate_frame(h0.float(), h1.float(), fw, bw, occ_fw,
                                 occ_bw, 0.3)
    assert got[0].dtype == torch.float32
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    ref = R.interpolate_frame(h0.cpu(), h1.cpu(), args[2], args[3], args[4],
                              args[5], 0.3)
    assert torch.equal(got[0].cpu(), ref[0])


def test_binding_rejects_bad_arguments(dev):
    args, _ = _reference(SHAPES[1], 0.5)
    im0, im1, fw, bw, occ_fw, occ_bw = (a.to(dev) for a in args)
    o0, o1 = occ_fw.view(torch.uint8), occ_bw.view(torch.uint8)
    hip = _hip()
    with pytest.raises(RuntimeError):
        hip.interpolate_frame(im0, im1, fw, bw, o0, o1, 1.5)
    with pytest.raises(RuntimeError):
        hip.interpolate_frame(im0, im1, fw, bw, occ_fw, o1, 0.5)   # bool
    with pytest.raises(RuntimeError):
        hip.interpolate_frame(im0.cpu(), im1, fw, bw, o0, o1, 0.5)
    with pytest.raises(RuntimeError):
        hip.interpolate_frame(im0, im1, fw[:, :1].contiguous(), bw, o0, o1,
                              0.5)
    with pytest.raises(RuntimeError):
        hip.interpolate_frame(im0, im1, fw.transpose(2, 3), bw, o0, o1, 0.5)
    with pytest.raises(RuntimeError):
        hip.interpolate_frame(im0.half(), im1.half(), fw, bw, o0, o1, 0.5)


def test_determinism_and_graph_capture(dev):
    from raft_amd import ops
    case = SHAPES[0]
    args, _ = _reference(case, 0.3)
    bufs = [a.to(dev).clone() for a in args]
    a = ops.interpolate_frame(*bufs, 0.3)
    b = ops.interpolate_frame(*bufs, 0.3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.interpolate_frame(*bufs, 0.3)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = ops.interpolate_frame(*bufs, 0.3)
    for seed in (5, 6):
        fresh = [x.to(dev) for x in _inputs(*case[:5], seed)]
        for buf, new in zip(bufs, fresh):
            buf.copy_(new)
        g.replay()
        want = ops.interpolate_frame(*fresh, 0.3)
        for x, y in zip(out, want):
            assert torch.equal(x, y)
        assert not torch.equal(out[0], a[0])
    del g
    torch.cuda.synchronize()


# ------------------------------------------------------- engine and session
def _release(m):
    del m._fused_cache
    torch.cuda.synchronize()


def test_engine_interpolate_gpu_bf16(dev):
    from raft_amd import RAFT, RaftConfig
    from raft_amd.engine.inference import InferenceEngine
    torch.manual_seed(11)
    m = RAFT(RaftConfig(small=False)).to(dev)
    eng = InferenceEngine(m, iters=4, dtype=torch.bfloat16)
    x1 = torch.rand(1, 3, 44, 60)
    x2 = torch.rand(1, 3, 44, 60)
    out = eng.interpolate(x1, x2, times=(0.25, 0.5))
    assert out.shape == (2, 1, 3, 44, 60) and out.is_cuda
    assert out.dtype == torch.float32 and torch.isfinite(out).all()
    assert out.min() >= 0.0 and out.max() <= 1.0
    assert not torch.equal(out[0], out[1])
    ends = eng.interpolate(x1, x2, times=(0.0, 1.0))
    assert torch.equal(ends[0].cpu(), x1.to(torch.bfloat16).float())
    assert torch.equal(ends[1].cpu(), x2.to(torch.bfloat16).float())
    _release(m)


def test_session_between_gpu_bf16(dev):
    from raft_amd import RAFT, RaftConfig, ops
    from raft_amd.engine.inference import InferenceEngine
    torch.manual_seed(12)
    m = RAFT(RaftConfig(small=False)).to(dev)
    eng = InferenceEngine(m, iters=4, dtype=torch.bfloat16, loop_graph=False)
    frames = [torch.rand(1, 3, 44, 60).to(dev, torch.bfloat16)
              for _ in range(3)]
    s = eng.stream(warm=True, bidirectional=True)
    assert s.push(frames[0]) is None
    with pytest.raises(RuntimeError):
        s.between((0.5,))
    for i in (1, 2):
        res = s.push(frames[i])
        got = s.between((0.5,))
        assert got.shape == (1, 1, 3, 44, 60) and got.dtype == torch.float32
        want = ops.interpolate_frame(frames[i - 1], frames[i], res.flow_fw,
                                     res.flow_bw, res.occ_fw, res.occ_bw,
                                     0.5)[0]
        assert torch.equal(got[0], want)
        assert torch.isfinite(got).all()
    with pytest.raises(ValueError, match="bidirectional"):
        eng.stream().between((0.5,))
    _release(m)
