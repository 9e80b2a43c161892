"""Frame interpolation at time t (ops.interpolate_frame): the oracle's
definition against its stated consequences and hand-built scenes, the
argument contract, engine.interpolate, session.between and the CLI flag —
all on the CPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from raft_amd import ops
from raft_amd.ops import torch_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "images")


def _smooth(B, H, W, amp):
    return F.interpolate(torch.randn(B, 2, 4, 5) * amp, size=(H, W),
                         mode="bilinear", align_corners=True).contiguous()


def _scene(seed, B=2, C=3, H=17, W=23, amp=6.0):
    """Random images, smooth flows large enough to leave the frame, and
    random masks dense enough that both are set at many cells."""
    torch.manual_seed(seed)
    im0, im1 = torch.rand(B, C, H, W), torch.rand(B, C, H, W)
    fw = _smooth(B, H, W, amp)
    bw = -fw + torch.randn(B, 2, H, W) * 0.4
    occ_fw = torch.rand(B, 1, H, W) < 0.4
    occ_bw = torch.rand(B, 1, H, W) < 0.4
    return im0, im1, fw, bw.contiguous(), occ_fw, occ_bw


def _leaves_frame(flow):
    _, _, H, W = flow.shape
    px = torch.arange(W, dtype=torch.float32).view(1, 1, W) + flow[:, 0]
    py = torch.arange(H, dtype=torch.float32).view(1, H, 1) + flow[:, 1]
    return ~((px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1))


# -------------------------------------------------------------- consequences
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_endpoints_return_the_inputs(seed):
    im0, im1, fw, bw, occ_fw, occ_bw = _scene(seed)
    assert _leaves_frame(fw).any() and _leaves_frame(bw).any()
    assert (occ_fw & occ_bw).any()
    out0 = ops.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw, 0.0)
    out1 = ops.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw, 1.0)
    assert torch.equal(out0[0], im0)
    assert torch.equal(out1[0], im1)
    # with the masks that hit both samples at once
    full = torch.ones_like(occ_fw)
    assert torch.equal(
        ops.interpolate_frame(im0, im1, fw, bw, full, full, 0.0)[0], im0)
    assert torch.equal(
        ops.interpolate_frame(im0, im1, fw, bw, full, full, 1.0)[0], im1)
    for out in (out0, out1):
        frame, ft0, ft1, cover = out
        assert frame.dtype == ft0.dtype == ft1.dtype == torch.float32
        assert ft0.shape == ft1.shape == fw.shape
        assert cover.dtype == torch.uint8
        assert cover.shape == occ_fw.shape


@pytest.mark.parametrize("t", [0.25, 0.5, 0.75])
@pytest.mark.parametrize("seed", [0, 3])
def test_swap_symmetry(seed, t):
    im0, im1, fw, bw, occ_fw, occ_bw = _scene(seed)
    a = ops.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw, t)
    b = ops.interpolate_frame(im1, im0, bw, fw, occ_bw, occ_fw, 1.0 - t)
    assert torch.equal(a[0], b[0])
    assert torch.equal(a[1], b[2]) and torch.equal(a[2], b[1])
    # cover bits are exchanged with the splats
    assert torch.equal(a[3], ((b[3] & 1) << 1) | (b[3] >> 1))
    # all four cover states occur: the symmetry is not vacuous
    assert set(a[3].unique().tolist()) == {0, 1, 2, 3}


def test_pure_translation():
    torch.manual_seed(4)
    H, W, dx, dy = 24, 30, 4, -2
    im0 = torch.rand(1, 3, H, W)
    im1 = torch.roll(im0, shifts=(dy, dx), dims=(2, 3))   # im1(x) = im0(x-d)
    fw = torch.empty(1, 2, H, W)
    fw[:, 0], fw[:, 1] = float(dx), float(dy)
    occ = torch.zeros(1, 1, H, W, dtype=torch.bool)
    frame, ft0, ft1, cover = ops.interpolate_frame(im0, im1, fw, -fw, occ,
                                                   occ, 0.5)
    want = torch.roll(im0, shifts=(dy // 2, dx // 2), dims=(2, 3))
    m = 5                                     # >= |d| = 4.47
    inner = (slice(None), slice(None), slice(m, H - m), slice(m, W - m))
    assert torch.equal(frame[inner], want[inner])
    assert (cover[inner] == 3).all()
    assert torch.equal(ft0[inner], (-0.5 * fw)[inner])
    assert torch.equal(ft1[inner], (0.5 * fw)[inner])


def test_occlusion_strips_take_the_visible_frame():
    """A 12x12 square moving by (8, 0) over a static textured background:
    at t = 0.5 it sits 4 px along. The 4 columns it has already left are
    background seen in frame 1 only (frame 0 still shows the square
    there); the 4 columns it has not reached yet are background seen in
    frame 0 only."""
    torch.manual_seed(5)
    H, W, S, X, Y, D = 32, 48, 12, 10, 10, 8
    bg = torch.rand(1, 3, H, W)
    sq = torch.rand(1, 3, S, S) + 2.0            # unlike any background
    im0, im1 = bg.clone(), bg.clone()
    im0[:, :, Y:Y + S, X:X + S] = sq
    im1[:, :, Y:Y + S, X + D:X + D + S] = sq
    fw = torch.zeros(1, 2, H, W)
    bw = torch.zeros(1, 2, H, W)
    fw[:, 0, Y:Y + S, X:X + S] = float(D)
    bw[:, 0, Y:Y + S, X + D:X + D + S] = -float(D)
    occ_fw = torch.zeros(1, 1, H, W, dtype=torch.bool)
    occ_bw = torch.zeros(1, 1, H, W, dtype=torch.bool)
    # frame-0 background the square covers in frame 1, and frame-1
    # background the square covered in frame 0
    occ_fw[:, :, Y:Y + S, X + S:X + S + D] = True
    occ_bw[:, :, Y:Y + S, X:X + D] = True
    frame = ops.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw, 0.5)[0]
    left = (slice(None), slice(None), slice(Y, Y + S),
            slice(X, X + D // 2))
    lead = (slice(None), slice(None), slice(Y, Y + S),
            slice(X + S + D // 2, X + S + D))
    assert torch.equal(frame[left], im1[left])
    assert torch.equal(frame[left], bg[left])
    assert not torch.equal(im0[left], im1[left])
    assert torch.equal(frame[lead], im0[lead])
    assert torch.equal(frame[lead], bg[lead])
    assert not torch.equal(im0[lead], im1[lead])


@pytest.mark.parametrize("t,a,b", [(0.5, 0.5, 0.5), (0.25, 1.0, 1.0 / 3)])
def test_fallback_where_neither_splat_covers(t, a, b):
    """flow_fw = a (x - c) and flow_bw = b (x - c) with t*a = (1-t)*b =
    0.25: both splats spread their sources 1.25 cells apart and drop the
    outermost ones (12 cells, c = 5.5: x = 9 lands on 9.875, x = 10 would
    land on 11.125), so the border cells are reached by neither splat and
    take the linear approximation."""
    H = W = 12
    c = 5.5
    xs = torch.arange(W, dtype=torch.float32).view(1, W).expand(H, W)
    ys = torch.arange(H, dtype=torch.float32).view(H, 1).expand(H, W)
    field = torch.stack([xs - c, ys - c])[None]
    fw = (a * field).contiguous()
    torch.manual_seed(6)
    bw = (b * field + torch.randn(1, 2, H, W) * 0.01).contiguous()
    im0, im1 = torch.rand(1, 2, H, W), torch.rand(1, 2, H, W)
    occ = torch.zeros(1, 1, H, W, dtype=torch.bool)
    _, ft0, ft1, cover = ops.interpolate_frame(im0, im1, fw, bw, occ, occ, t)
    hole = (cover == 0).expand(1, 2, H, W)
    assert hole.any() and not hole.all()
    tf = torch.tensor(t, dtype=torch.float32)
    u = 1.0 - tf
    want0 = (-(u * tf)) * fw + (tf * tf) * bw
    want1 = (u * u) * fw + (-(tf * u)) * bw
    assert torch.equal(ft0[hole], want0[hole])
    assert torch.equal(ft1[hole], want1[hole])
    # and only there: a covered cell carries a splatted flow
    assert not torch.equal(ft0[~hole], want0[~hole])


def test_exact_tie_goes_to_the_lowest_source_index():
    H, W = 5, 7
    fw = torch.full((1, 2, H, W), 100.0)      # every other source leaves
    fw[0, :, 2, 1] = torch.tensor([2.0, 0.0])     # (1,2) -> (3,2), index 15
    fw[0, :, 2, 5] = torch.tensor([-2.0, 0.0])    # (5,2) -> (3,2), index 19
    bw = torch.zeros(1, 2, H, W)
    im = torch.rand(1, 1, H, W)
    occ = torch.zeros(1, 1, H, W, dtype=torch.bool)
    _, ft0, _, cover = ops.interpolate_frame(im, im, fw, bw, occ, occ, 1.0)
    assert cover[0, 0, 2, 3] & 1
    assert ft0[0, :, 2, 3].tolist() == [-2.0, 0.0]     # -tf * flow of 15
    # one more candidate at the same distance but a lower index takes over
    fw[0, :, 0, 3] = torch.tensor([0.0, 2.0])     # (3,0) -> (3,2), index 3
    _, ft0, _, _ = ops.interpolate_frame(im, im, fw, bw, occ, occ, 1.0)
    assert ft0[0, :, 2, 3].tolist() == [0.0, -2.0]
    # a nearer candidate beats a lower index: (4,2) -> (3.25, 2) is nearer
    # to cell (4,2) than (1,2) -> (3,2) is
    fw[0, :, 2, 4] = torch.tensor([-0.75, 0.0])
    _, ft0, _, _ = ops.interpolate_frame(im, im, fw, bw, occ, occ, 1.0)
    assert ft0[0, :, 2, 4].tolist() == [0.75, 0.0]
    assert ft0[0, :, 2, 3].tolist() == [0.0, -2.0]     # d2 = 0 still wins


def test_half_integer_target_feeds_four_cells():
    H, W = 5, 7
    fw = torch.full((1, 2, H, W), 100.0)
    fw[0, :, 1, 1] = 1.0                          # (1,1) -> (1.5, 1.5)
    bw = torch.full((1, 2, H, W), 100.0)
    im = torch.rand(1, 1, H, W)
    occ = torch.zeros(1, 1, H, W, dtype=torch.bool)
    _, ft0, ft1, cover = ops.interpolate_frame(im, im, fw, bw, occ, occ,
                                               0.5)
    want = torch.zeros(H, W, dtype=torch.uint8)
    want[1:3, 1:3] = 1
    assert torch.equal(cover[0, 0], want)
    assert (ft0[0, :, 1:3, 1:3] == -0.5).all()
    assert (ft1[0, :, 1:3, 1:3] == 0.5).all()


def test_nan_and_inf_flows_are_dropped():
    im0, im1, fw, bw, occ_fw, occ_bw = _scene(7, B=1)
    fw[0, 0, 3, 4] = float("nan")
    fw[0, 1, 8, 9] = float("inf")
    bw[0, 0, 5, 5] = float("-inf")
    frame, _, _, cover = ops.interpolate_frame(im0, im1, fw, bw, occ_fw,
                                               occ_bw, 0.5)
    assert torch.isfinite(frame).all()
    assert frame.min() >= 0.0 and frame.max() <= 1.0
    assert set(cover.unique().tolist()) <= {0, 1, 2, 3}


# ------------------------------------------------------------------ errors
def test_argument_errors():
    im0, im1, fw, bw, occ_fw, occ_bw = _scene(0)
    for t in (-0.01, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ops.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw, t)
        with pytest.raises(ValueError):
            R.interpolate_frame(im0, im1, fw, bw, occ_fw, occ_bw, t)
    with pytest.raises(ValueError):           # images disagree
        ops.interpolate_frame(im0, im1[:, :, :-1], fw, bw, occ_fw, occ_bw,
                              0.5)
    with pytest.raises(ValueError):           # flow of another size
        ops.interpolate_frame(im0, im1, fw[:, :, :, :-1].contiguous(), bw,
                              occ_fw, occ_bw, 0.5)
    with pytest.raises(ValueError):           # not [B,2,H,W]
        ops.interpolate_frame(im0, im1, im0, bw, occ_fw, occ_bw, 0.5)
    with pytest.raises(ValueError):
        ops.interpolate_frame(im0, im1, fw, bw[0], occ_fw, occ_bw, 0.5)
    with pytest.raises(ValueError):           # mask of another shape
        ops.interpolate_frame(im0, im1, fw, bw, occ_fw[:1], occ_bw, 0.5)
    with pytest.raises(ValueError):
        ops.interpolate_frame(im0, im1, fw, bw, occ_fw, fw > 0, 0.5)


# -------------------------------------------------------- engine and session
H0, W0, ITERS = 44, 60, 2


@pytest.fixture(scope="module")
def rig():
    from raft_amd import RAFT, RaftConfig
    from raft_amd.data.synthetic import synthetic_pair
    from raft_amd.engine import InferenceEngine
    torch.manual_seed(5)
    m = RAFT(RaftConfig(small=True)).eval()
    eng = InferenceEngine(m, iters=ITERS)
    a, b, _ = synthetic_pair(1, H0, W0, seed=0)
    return dict(eng=eng, a=a, b=b, bidir=eng.bidirectional(a, b))


def test_engine_interpolate_cpu(rig):
    eng, a, b, bi = rig["eng"], rig["a"], rig["b"], rig["bidir"]
    out = eng.interpolate(a, b, times=(0.25, 0.5, 0.75))
    assert out.shape == (3, 1, 3, H0, W0) and out.dtype == torch.float32
    assert torch.isfinite(out).all()
    lo, hi = min(a.min(), b.min()), max(a.max(), b.max())
    assert out.min() >= lo - 1e-5 and out.max() <= hi + 1e-5
    for k, t in enumerate((0.25, 0.5, 0.75)):
        want = ops.interpolate_frame(a, b, bi.flow_fw, bi.flow_bw,
                                     bi.occ_fw, bi.occ_bw, t)[0]
        assert torch.equal(out[k], want)
    ends = eng.interpolate(a, b, times=(0.0, 1.0))
    assert torch.equal(ends[0], a) and torch.equal(ends[1], b)
    assert eng.interpolate(a, b).shape == (1, 1, 3, H0, W0)
    with pytest.raises(ValueError):
        eng.interpolate(a, b, times=(0.5, 1.25))


def test_session_between(rig):
    eng, a, b = rig["eng"], rig["a"], rig["b"]
    s = eng.stream(warm=False, bidirectional=True)
    with pytest.raises(RuntimeError):
        s.between((0.5,))
    assert s.push(a) is None
    with pytest.raises(RuntimeError):
        s.between((0.5,))
    out = s.push(b)
    got = s.between((0.25, 0.5))
    assert got.shape == (2, 1, 3, H0, W0) and got.dtype == torch.float32
    for k, t in enumerate((0.25, 0.5)):
        want = ops.interpolate_frame(a, b, out.flow_fw, out.flow_bw,
                                     out.occ_fw, out.occ_bw, t)[0]
        assert torch.equal(got[k], want)
    assert torch.equal(got, eng.interpolate(a, b, times=(0.25, 0.5)))
    # the next push moves the window: now between b and a
    out = s.push(a)
    want = ops.interpolate_frame(b, a, out.flow_fw, out.flow_bw, out.occ_fw,
                                 out.occ_bw, 0.5)[0]
    assert torch.equal(s.between((0.5,))[0], want)
    s.reset()
    with pytest.raises(RuntimeError):
        s.between((0.5,))


def test_session_between_needs_bidirectional(rig):
    s = rig["eng"].stream(warm=False)
    s.push(rig["a"])
    s.push(rig["b"])
    with pytest.raises(ValueError, match="bidirectional"):
        s.between((0.5,))


# --------------------------------------------------------------------- CLI
def test_cli_interp_pair_mode(tmp_path, monkeypatch):
    import infer_raft
    from raft_amd.data.imageio import read_png
    monkeypatch.setattr(infer_raft, "_select_device",
                        lambda args: torch.device("cpu"))
    torch.manual_seed(7)
    out = tmp_path / "out"
    infer_raft.main(["--mode", "test", "--small", "--im1",
                     os.path.join(GOLDEN, "flower.jpg"), "--im2",
                     os.path.join(GOLDEN, "china.jpg"), "--out", str(out),
                     "--size", "40x56", "--iters", "2", "--interp", "2"])
    names = sorted(p.name for p in out.iterdir())
    interp = [n for n in names if n.startswith("raft_interp_")]
    assert interp == ["raft_interp_raft-small_t1.png",
                      "raft_interp_raft-small_t2.png"]
    # --interp implies --bidirectional
    assert "raft_flow_raft-small_bw.flo" in names
    imgs = [read_png(str(out / n)) for n in interp]
    for img in imgs:
        assert img.shape == (40, 56, 3) and img.dtype == np.uint8
    assert not np.array_equal(imgs[0], imgs[1])


def test_cli_interp_stream_mode(tmp_path, monkeypatch):
    import infer_raft
    from raft_amd.data.imageio import read_png, write_png
    monkeypatch.setattr(infer_raft, "_select_device",
                        lambda args: torch.device("cpu"))
    rng = np.random.default_rng(0)
    seq = tmp_path / "seq"
    seq.mkdir()
    for i in range(3):
        write_png(str(seq / f"frame_{i:02d}.png"),
                  (rng.random((40, 56, 3)) * 255).astype(np.uint8))
    outs = {}
    for tag, extra in (("pair", []), ("stream", ["--stream"])):
        torch.manual_seed(7)
        out = tmp_path / tag
        infer_raft.main(["--mode", "test", "--small", "--data", str(seq),
                         "--out", str(out), "--size", "40x56", "--iters",
                         "2", "--interp", "1", *extra])
        outs[tag] = sorted(p.name for p in out.iterdir()
                           if p.name.startswith("raft_interp_"))
    assert outs["pair"] == outs["stream"] == [
        "raft_interp_raft-small_0000_t1.png",
        "raft_interp_raft-small_0001_t1.png"]
    for n in outs["pair"]:
        a = read_png(str(tmp_path / "pair" / n))
        assert a.shape == (40, 56, 3)
        assert np.array_equal(a, read_png(str(tmp_path / "stream" / n)))


def test_cli_interp_needs_test_mode():
    import infer_raft
    with pytest.raises(SystemExit):
        infer_raft.main(["--mode", "flops", "--interp", "2"])
    with pytest.raises(SystemExit):
        infer_raft.main(["--mode", "test", "--interp", "-1"])
