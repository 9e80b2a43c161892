"""Streaming video flow without a GPU: the forward-projection oracle
(properties + an independent scalar re-implementation), the video session
on the eager model, and the --stream CLI."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from raft_amd.ops import torch_ref as R


def smooth_flow(B, H, W, amp):
    """The construction test_bidirectional's fb_inputs uses: a coarse random
    grid, bilinearly stretched."""
    return F.interpolate(torch.randn(B, 2, 4, 5) * amp, size=(H, W),
                         mode="bilinear", align_corners=True).contiguous()


# (B, H, W, amp, seed) of the smooth inputs shared with the GPU tests
SMOOTH = [(2, 12, 16, 2.0, 0), (1, 9, 13, 3.0, 1), (1, 17, 64, 6.0, 2)]


# ------------------------------------------------------------------ oracle
def test_uniform_integer_shift():
    """A uniform shift (3,-2) projects onto itself: covered cells gather
    the flow, and the vacated band is refilled with the exact value (the
    mean of 1..3 equal neighbours must be that value: division, not a
    reciprocal multiply — 9 * (1/3) != 3). Every cell is pinned.

    What the definition implies here, cell by cell: the sources land on
    integer targets, so next to the floor cell (d2 = 0) each is also a
    candidate for the floor+1 cells at distance exactly 1. On the side the
    content moves away from, the vacated band is therefore one cell
    narrower than the shift (those cells are covered, at d2 = 1, with the
    same value); on the side it moves towards, the band is the full shift.
    Where the two bands cross, a cell has no covered cell on its row or
    its column, and the definition gives it exactly 0."""
    H, W = 12, 16
    u = torch.zeros(1, 2, H, W)
    u[:, 0] = 3.0
    u[:, 1] = -2.0
    xs = torch.arange(W).view(1, W).expand(H, W)
    ys = torch.arange(H).view(H, 1).expand(H, W)
    # direction=+1 moves content right 3 / up 2, direction=-1 left 3 / down 2
    for d, band_x, band_y in ((1, xs < 3, ys >= H - 2 + 1),
                              (-1, xs >= W - 3 + 1, ys < 2)):
        out, holes = R.forward_project(u, d)
        assert out.dtype == torch.float32 and holes.dtype == torch.bool
        assert out.shape == (1, 2, H, W) and holes.shape == (1, 1, H, W)
        assert torch.equal(holes[0, 0], band_x | band_y)
        dead = band_x & band_y            # no covered cell on row or column
        assert dead.any()
        want = torch.where(dead, torch.zeros_like(u), u)
        assert torch.equal(out, want)


def test_zero_flow_is_identity():
    z = torch.zeros(2, 2, 7, 9)
    for d in (1, -1):
        out, holes = R.forward_project(z, d)
        assert torch.equal(out, z) and not holes.any()


def test_everything_leaves_the_frame():
    f = torch.full((1, 2, 6, 8), 100.0)
    for d in (1, -1):
        out, holes = R.forward_project(f, d)
        assert holes.all() and torch.equal(out, torch.zeros_like(f))


def test_nan_source_is_dropped():
    torch.manual_seed(3)
    f = smooth_flow(1, 12, 16, 2.0)
    bad = f.clone()
    bad[0, 0, 5, 7] = float("nan")
    gone = f.clone()
    gone[0, :, 5, 7] = 100.0            # leaves the frame: dropped as well
    for d in (1, -1):
        out, holes = R.forward_project(bad, d)
        assert torch.isfinite(out).all()
        ref, ref_holes = R.forward_project(gone, d)
        assert torch.equal(out, ref) and torch.equal(holes, ref_holes)
    inf = f.clone()
    inf[0, 1, 5, 7] = float("inf")
    out, _ = R.forward_project(inf, 1)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("B,H,W,amp,seed", SMOOTH)
def test_direction_symmetry(B, H, W, amp, seed):
    torch.manual_seed(seed)
    f = smooth_flow(B, H, W, amp)
    a, ha = R.forward_project(f, -1)
    b, hb = R.forward_project(-f, 1)
    assert torch.equal(a, -b) and torch.equal(ha, hb)


def _row(values, W=8):
    """One-row flow: every source leaves the frame except the given
    {x: fx} ones."""
    f = torch.zeros(1, 2, 1, W)
    f[0, 0] = 100.0
    for x, fx in values.items():
        f[0, 0, 0, x] = fx
    return f


def test_collision_nearer_source_wins():
    # x=2 lands at 3.25 (0.25 from cell 3, 0.75 from cell 4),
    # x=5 lands at 3.5  (0.5 from both)
    out, holes = R.forward_project(_row({2: 1.25, 5: -1.5}), 1)
    assert out[0, 0, 0, 3].item() == 1.25
    assert out[0, 0, 0, 4].item() == -1.5
    assert holes[0, 0, 0].tolist() == [True, True, True, False, False,
                                       True, True, True]
    # holes take the mean of the nearest covered cells of their row
    assert out[0, 0, 0, 0].item() == 1.25 and out[0, 0, 0, 7].item() == -1.5


def test_exact_tie_goes_to_lowest_source_index():
    # both land at 3.5: d2 = 0.25 to cells 3 and 4 from either source
    out, _ = R.forward_project(_row({2: 1.5, 5: -1.5}), 1)
    assert out[0, 0, 0, 3].item() == 1.5 and out[0, 0, 0, 4].item() == 1.5
    # direction=-1 swaps the signs: now the low index carries -1.5
    out, _ = R.forward_project(_row({2: -1.5, 5: 1.5}), -1)
    assert out[0, 0, 0, 3].item() == -1.5 and out[0, 0, 0, 4].item() == -1.5
    # same along a column
    f = _row({2: 1.5, 5: -1.5}).flip(1).transpose(2, 3).contiguous()
    out, _ = R.forward_project(f, 1)
    assert out[0, 1, 3, 0].item() == 1.5 and out[0, 1, 4, 0].item() == 1.5


def _scalar_forward_project(flow, direction):
    """Independent per-pixel double loop over the definition, in numpy
    fp32 scalars (each operation rounds on its own)."""
    f32 = np.float32
    fl = flow.numpy()
    B, _, H, W = fl.shape
    out = np.zeros((B, 2, H, W), np.float32)
    holes = np.ones((B, 1, H, W), bool)
    for b in range(B):
        best = {}
        for y in range(H):
            for x in range(W):
                fx, fy = fl[b, 0, y, x], fl[b, 1, y, x]
                tx = f32(x) + fx if direction > 0 else f32(x) - fx
                ty = f32(y) + fy if direction > 0 else f32(y) - fy
                if not (0 <= tx <= W - 1 and 0 <= ty <= H - 1):
                    continue
                x0, y0 = math.floor(tx), math.floor(ty)
                for qy in (y0, y0 + 1):
                    for qx in (x0, x0 + 1):
                        if qx > W - 1 or qy > H - 1:
                            continue
                        dx, dy = tx - f32(qx), ty - f32(qy)
                        d2 = f32(dx * dx) + f32(dy * dy)
                        cand = (float(d2), y * W + x)
                        if (qy, qx) not in best or cand < best[(qy, qx)]:
                            best[(qy, qx)] = cand
        for (qy, qx), (_, src) in best.items():
            out[b, :, qy, qx] = fl[b, :, src // W, src % W]
            holes[b, 0, qy, qx] = False
        cov = ~holes[b, 0]
        for y in range(H):
            for x in range(W):
                if cov[y, x]:
                    continue
                s = np.zeros(2, np.float32)
                n = 0
                for sy, sx in ((0, -1), (0, 1), (-1, 0), (1, 0)):
                    yy, xx = y + sy, x + sx
                    while 0 <= yy < H and 0 <= xx < W and not cov[yy, xx]:
                        yy, xx = yy + sy, xx + sx
                    if 0 <= yy < H and 0 <= xx < W:
                        s = s + out[b, :, yy, xx]
                        n += 1
                if n:
                    out[b, :, y, x] = s / f32(n)
    return torch.from_numpy(out), torch.from_numpy(holes)


@pytest.mark.parametrize("B,H,W,amp,seed", SMOOTH)
def test_oracle_matches_scalar_loop(B, H, W, amp, seed):
    torch.manual_seed(seed)
    f = smooth_flow(B, H, W, amp)
    for d in (1, -1):
        out, holes = R.forward_project(f, d)
        ref, ref_holes = _scalar_forward_project(f, d)
        share = holes.float().mean().item()
        print(f"{B}x{H}x{W} amp {amp} dir {d:+d}: holes {share:.3f}")
        assert 0.0 < share < 0.5          # both branches run
        assert torch.equal(holes, ref_holes)
        assert torch.equal(out, ref)
    # the public op is the oracle on CPU
    from raft_amd import ops
    o, h = ops.forward_project(f, -1)
    assert torch.equal(o, out) and torch.equal(h, holes)


def test_against_scipy_nearest_griddata():
    """Set up as RAFT's forward_interpolate: scatter the sources that land
    strictly inside the frame, nearest-neighbour interpolate onto the
    grid."""
    pytest.importorskip("scipy")
    from scipy.interpolate import griddata
    torch.manual_seed(4)
    H, W = 55, 128
    fl = smooth_flow(1, H, W, 4.0)
    out, _ = R.forward_project(fl, 1)
    f = fl[0].numpy()
    x0, y0 = np.meshgrid(np.arange(W), np.arange(H))
    x1, y1 = x0 + f[0], y0 + f[1]
    v = (x1 > 0) & (x1 < W) & (y1 > 0) & (y1 < H)
    g = np.stack([griddata((x1[v], y1[v]), f[c][v], (x0, y0),
                           method="nearest", fill_value=0) for c in (0, 1)])
    g = torch.from_numpy(g.astype(np.float32))
    ours = (out[0] - g).abs().mean().item()
    unprojected = (fl[0] - g).abs().mean().item()
    print(f"mean |proj - griddata| {ours:.4f}, unprojected {unprojected:.4f}")
    assert ours < 0.25 * unprojected


# ----------------------------------------------------------------- session
H0, W0, ITERS = 44, 60, 2


@pytest.fixture(scope="module")
def rig():
    """raft-small fp32 engine, four 44x60 frames (pad8 -> 48x64) and the
    pairwise references, computed once."""
    from raft_amd import RAFT, RaftConfig
    from raft_amd.data.synthetic import synthetic_pair
    from raft_amd.engine import InferenceEngine
    from raft_amd.engine.inference import pad8
    torch.manual_seed(5)
    m = RAFT(RaftConfig(small=True)).eval()
    eng = InferenceEngine(m, iters=ITERS)
    a, b, _ = synthetic_pair(1, H0, W0, seed=0)
    c, d, _ = synthetic_pair(1, H0, W0, seed=1)
    frames = [a, b, c, d]
    pairs = list(zip(frames[:-1], frames[1:]))
    cold = [eng(p, q) for p, q in pairs]
    cold_bi = [eng(p, q, bidirectional=True) for p, q in pairs]

    def lows(p, q, init, bidir):
        with torch.no_grad():
            return m(pad8(p)[0], pad8(q)[0], iters=ITERS, flow_init=init,
                     bidirectional=bidir, return_low=True)
    return dict(m=m, eng=eng, frames=frames, pairs=pairs, cold=cold,
                cold_bi=cold_bi, lows=lows)


def test_model_return_low(rig):
    m, (p, q) = rig["m"], rig["pairs"][0]
    from raft_amd.engine.inference import pad8
    p, q = pad8(p)[0], pad8(q)[0]
    with torch.no_grad():
        up, low = m(p, q, iters=ITERS, return_low=True)
        assert low.shape == (1, 2, 6, 8) and low.dtype == torch.float32
        assert torch.equal(up, m(p, q, iters=ITERS))
        fw, bw, lf, lb = m(p, q, iters=ITERS, bidirectional=True,
                           return_low=True)
        assert lf.shape == lb.shape == (1, 2, 6, 8)
        assert torch.allclose(lf, low, atol=1e-5)
        assert not torch.allclose(lf, lb, atol=1e-3)
        with pytest.raises(ValueError):
            m(p, q, iters=ITERS, test_mode=False, return_low=True)


def test_session_cold_equals_pairwise(rig):
    from raft_amd.engine import VideoFlowSession
    s = rig["eng"].stream(warm=False)
    assert isinstance(s, VideoFlowSession)
    assert s.push(rig["frames"][0]) is None
    for frame, ref in zip(rig["frames"][1:], rig["cold"]):
        out = s.push(frame)
        assert out.shape == (1, 2, H0, W0)
        assert torch.equal(out, ref)


def test_session_warm_is_projected_warm_start(rig):
    eng, lows = rig["eng"], rig["lows"]
    s = eng.stream(warm=True)
    assert s.push(rig["frames"][0]) is None
    init = None
    outs = []
    for i, (p, q) in enumerate(rig["pairs"]):
        out = s.push(q)
        outs.append(out)
        assert torch.equal(out, eng(p, q, flow_init=init))
        _, low = lows(p, q, init, False)
        init = R.forward_project(low, 1)[0]
        if i > 0:
            # the warm start is not a no-op
            assert not torch.equal(out, rig["cold"][i])
    # outputs of push 2 are unchanged after push 4
    assert torch.equal(outs[0], rig["cold"][0])


def test_session_bidirectional(rig):
    eng, lows = rig["eng"], rig["lows"]
    cold = eng.stream(warm=False, bidirectional=True)
    warm = eng.stream(warm=True, bidirectional=True)
    assert cold.push(rig["frames"][0]) is None
    assert warm.push(rig["frames"][0]) is None
    init = None
    for i, (p, q) in enumerate(rig["pairs"]):
        out = cold.push(q)
        assert torch.equal(out.flow_fw, rig["cold_bi"][i][0])
        assert torch.equal(out.flow_bw, rig["cold_bi"][i][1])
        ref = eng.bidirectional(p, q)
        assert torch.equal(out.occ_fw, ref.occ_fw)
        assert torch.equal(out.occ_bw, ref.occ_bw)
        assert out.occ_fw.shape == (1, 1, H0, W0)

        out = warm.push(q)
        ref = eng.bidirectional(p, q, flow_init=init)
        for got, want in zip(out, ref):
            assert torch.equal(got, want)
        _, _, lf, lb = lows(p, q, init, True)
        init = (R.forward_project(lf, 1)[0], R.forward_project(lb, -1)[0])


def test_session_reset_and_shape_change(rig):
    s = rig["eng"].stream(warm=True)
    f = rig["frames"]
    assert s.push(f[0]) is None
    first = s.push(f[1])
    keep = first.clone()
    s.push(f[2])
    s.push(f[3])
    assert torch.equal(first, keep)       # survives later pushes
    with pytest.raises(ValueError) as e:
        s.push(torch.rand(1, 3, 52, 60))
    assert "56x64" in str(e.value) and "48x64" in str(e.value)
    with pytest.raises(ValueError):
        s.push(torch.rand(2, 3, H0, W0))
    # the session is still usable, and reset() starts a new sequence
    assert s.push(f[0]) is not None
    s.reset()
    assert s.push(torch.rand(1, 3, 52, 60)) is None
    s.reset()
    assert s.push(f[0]) is None
    assert torch.equal(s.push(f[1]), rig["cold"][0])


def test_session_iters_override(rig):
    (p, q) = rig["pairs"][0]
    s = rig["eng"].stream(warm=False, iters=3)
    s.push(p)
    assert torch.equal(s.push(q), rig["eng"](p, q, iters=3))


# --------------------------------------------------------------------- CLI
def _write_seq(tmp_path, n=4, H=40, W=56):
    from raft_amd.data.imageio import write_png
    rng = np.random.default_rng(0)
    seq = tmp_path / "seq"
    seq.mkdir()
    for i in range(n):
        write_png(str(seq / f"frame_{i:02d}.png"),
                  (rng.random((H, W, 3)) * 255).astype(np.uint8))
    return seq


def _cli(monkeypatch, seq, out, *extra):
    import infer_raft
    # these are CPU tests on every machine: where a GPU is visible the
    # fp32 CLI would run the eager model on MIOpen, whose solver choice
    # differs between the captured pairwise call and the session's plain
    # one (low-order bits) — byte identity is a statement about the CPU
    monkeypatch.setattr(infer_raft, "_select_device",
                        lambda args: torch.device("cpu"))
    torch.manual_seed(7)         # the CLI builds a randomly initialised model
    infer_raft.main(["--mode", "test", "--small", "--data", str(seq),
                     "--out", str(out), "--size", "40x56", "--iters", "2",
                     *extra])
    return sorted(p.name for p in out.iterdir())


def test_cli_stream_matches_pairwise_files(tmp_path, monkeypatch):
    seq = _write_seq(tmp_path)
    plain = _cli(monkeypatch, seq, tmp_path / "plain")
    stream = _cli(monkeypatch, seq, tmp_path / "stream", "--stream")
    assert stream == plain and len(plain) == 6
    for name in plain:
        if name.endswith(".flo"):
            assert (tmp_path / "plain" / name).read_bytes() == \
                (tmp_path / "stream" / name).read_bytes(), name


def test_cli_stream_warm_bidirectional(tmp_path, monkeypatch):
    from raft_amd.data.imageio import read_png
    seq = _write_seq(tmp_path)
    plain = _cli(monkeypatch, seq, tmp_path / "plain", "--warm",
                 "--bidirectional")
    stream = _cli(monkeypatch, seq, tmp_path / "stream", "--stream",
                  "--warm", "--bidirectional")
    assert stream == plain and len(stream) == 18
    occ = read_png(str(tmp_path / "stream" / "raft_occ_raft-small_0002_bw.png"))
    assert occ.shape[:2] == (40, 56)
    assert set(np.unique(occ).tolist()) <= {0, 255}
    # pair 0 has no warm start yet: both runs compute the same flow
    name = "raft_flow_raft-small_0000_bw.flo"
    assert (tmp_path / "plain" / name).read_bytes() == \
        (tmp_path / "stream" / name).read_bytes()


def test_cli_stream_needs_a_sequence(tmp_path):
    import infer_raft
    with pytest.raises(SystemExit) as e:
        infer_raft.main(["--mode", "test", "--small", "--stream", "--im1",
                         "a.png", "--im2", "b.png", "--out",
                         str(tmp_path / "o")])
    assert "--stream needs sequence mode" in str(e.value)
    with pytest.raises(SystemExit):
        infer_raft.main(["--mode", "flops", "--stream"])
