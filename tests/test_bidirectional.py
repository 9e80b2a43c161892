"""Bidirectional flow + forward-backward occlusion: oracle properties, the
eager model path, the engine and the CLI (no GPU needed)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from raft_amd.ops import torch_ref as R


def fb_inputs(B=2, H=37, W=53):
    """Smooth forward flow + a noisy near-inverse backward flow (shared
    with the GPU test): ~35 % occluded, ~7 % leaving the frame."""
    fw = F.interpolate(torch.randn(B, 2, 5, 7) * 2.0, size=(H, W),
                       mode="bilinear", align_corners=True)
    bw = -fw + torch.randn(B, 2, H, W) * 0.4
    return fw.contiguous(), bw.contiguous()


def check_masks(occ, occ_ref, res, bound):
    """Masks must agree wherever the decision is not within rounding of
    the threshold; that excluded band may hold at most 1 % of pixels."""
    clear = (res - bound).abs() > 1e-3 * (1 + bound)
    assert (~clear).float().mean().item() <= 0.01
    assert torch.equal(occ[clear], occ_ref[clear])


def _scalar_fb(fw, bw, alpha1, alpha2):
    """Independent pure-Python double loop over the definition."""
    B, _, H, W = fw.shape
    f32 = np.float32
    fwn, bwn = fw.numpy(), bw.numpy()
    res = np.zeros((B, 1, H, W), np.float32)
    bound = np.zeros((B, 1, H, W), np.float32)
    inb = np.zeros((B, 1, H, W), bool)
    for b in range(B):
        for y in range(H):
            for x in range(W):
                fx, fy = fwn[b, 0, y, x], fwn[b, 1, y, x]
                px = f32(x) + fx
                py = f32(y) + fy
                inb[b, 0, y, x] = (0 <= px <= W - 1) and (0 <= py <= H - 1)
                x0 = int(min(max(math.floor(px), 0), W - 1))
                y0 = int(min(max(math.floor(py), 0), H - 1))
                x1, y1 = min(x0 + 1, W - 1), min(y0 + 1, H - 1)
                ax = min(max(float(px) - x0, 0.0), 1.0)
                ay = min(max(float(py) - y0, 0.0), 1.0)
                w = [0.0, 0.0]
                for c in range(2):
                    p = bwn[b, c]
                    w[c] = ((1 - ax) * (1 - ay) * float(p[y0, x0])
                            + ax * (1 - ay) * float(p[y0, x1])
                            + (1 - ax) * ay * float(p[y1, x0])
                            + ax * ay * float(p[y1, x1]))
                fx, fy = float(fx), float(fy)
                res[b, 0, y, x] = (fx + w[0]) ** 2 + (fy + w[1]) ** 2
                bound[b, 0, y, x] = alpha1 * (fx * fx + fy * fy + w[0] ** 2
                                              + w[1] ** 2) + alpha2
    occ = ~inb | (res > bound)
    return (torch.from_numpy(occ), torch.from_numpy(res),
            torch.from_numpy(bound), torch.from_numpy(inb))


def test_fb_oracle_constant_translation():
    H, W = 16, 24
    fw = torch.zeros(1, 2, H, W)
    fw[:, 0] = 2.0
    occ = R.fb_consistency(fw, -fw)
    assert occ.shape == (1, 1, H, W) and occ.dtype == torch.bool
    per_col = occ[0, 0].sum(dim=0).tolist()
    assert per_col == [0] * (W - 2) + [H, H]


def test_fb_oracle_matches_scalar_loop():
    fw, bw = fb_inputs()
    occ, res, bound = R.fb_consistency(fw, bw, return_terms=True)
    occ_s, res_s, bound_s, inb_s = _scalar_fb(fw, bw, 0.01, 0.5)
    assert res.dtype == torch.float32 and bound.dtype == torch.float32
    assert torch.allclose(res, res_s, rtol=1e-5, atol=1e-6)
    assert torch.allclose(bound, bound_s, rtol=1e-5, atol=1e-6)
    check_masks(occ, occ_s, res_s, bound_s)
    # every pixel that leaves the frame is occluded, and both branches of
    # the criterion are exercised
    assert occ[~inb_s].all()
    assert (~inb_s).float().mean().item() > 0.02
    assert (occ & inb_s).float().mean().item() > 0.05
    assert (~occ).float().mean().item() > 0.2
    # swapped arguments give the backward mask of the public op
    from raft_amd import ops
    o_fw, o_bw = ops.fb_consistency(fw, bw)
    assert torch.equal(o_fw, occ)
    assert torch.equal(o_bw, R.fb_consistency(bw, fw))


@pytest.mark.parametrize("small", [False, True])
def test_model_bidirectional_cpu(small):
    from raft_amd import RAFT, RaftConfig
    dev = torch.device("cpu")
    m = RAFT(RaftConfig(small=small)).to(dev).eval()
    x1 = torch.rand(1, 3, 32, 48)
    x2 = torch.rand(1, 3, 32, 48)
    with torch.no_grad():
        fw, bw = m(x1, x2, iters=3, bidirectional=True)
        ref_fw = m(x1, x2, iters=3)
        ref_bw = m(x2, x1, iters=3)
        assert fw.shape == ref_fw.shape and bw.shape == ref_bw.shape
        assert torch.allclose(fw, ref_fw, atol=1e-5)
        assert torch.allclose(bw, ref_bw, atol=1e-5)
        assert not torch.allclose(fw, bw, atol=1e-3)
        with pytest.raises(ValueError):
            m(x1, x2, iters=3, bidirectional=True, test_mode=False)
        z = torch.zeros(1, 2, 4, 6)
        fw0, bw0 = m(x1, x2, iters=3, bidirectional=True, flow_init=(z, z))
        assert torch.equal(fw0, fw) and torch.equal(bw0, bw)
        o = torch.ones(1, 2, 4, 6)
        fw1, bw1 = m(x1, x2, iters=3, bidirectional=True, flow_init=(o, o))
        assert not torch.allclose(fw1, fw, atol=1e-3)
        assert not torch.allclose(bw1, bw, atol=1e-3)


def test_engine_bidirectional_cpu_unpadded():
    from raft_amd import RAFT, RaftConfig
    from raft_amd.engine.inference import InferenceEngine
    m = RAFT(RaftConfig(small=True)).to(torch.device("cpu")).eval()
    eng = InferenceEngine(m, iters=2)
    x1 = torch.rand(1, 3, 30, 45)
    x2 = torch.rand(1, 3, 30, 45)
    out = eng.bidirectional(x1, x2)
    assert out.flow_fw.shape == (1, 2, 30, 45)
    assert out.flow_bw.shape == (1, 2, 30, 45)
    assert out.occ_fw.shape == (1, 1, 30, 45)
    assert out.occ_bw.shape == (1, 1, 30, 45)
    assert out.occ_fw.dtype == torch.bool and out.occ_bw.dtype == torch.bool
    fw, bw = eng(x1, x2, bidirectional=True)
    assert torch.equal(fw, out.flow_fw) and torch.equal(bw, out.flow_bw)


def _write_seq(tmp_path, n=3, H=40, W=56):
    from raft_amd.data.imageio import write_png
    rng = np.random.default_rng(0)
    seq = tmp_path / "seq"
    seq.mkdir()
    for i in range(n):
        write_png(str(seq / f"frame_{i:02d}.png"),
                  (rng.random((H, W, 3)) * 255).astype(np.uint8))
    return seq


NEW_FILES = ["raft_flow_raft-small_{i:04d}_bw.flo",
             "raft_flow_raft-small_{i:04d}_bw.png",
             "raft_occ_raft-small_{i:04d}_fw.png",
             "raft_occ_raft-small_{i:04d}_bw.png"]
OLD_FILES = ["raft_flow_raft-small_{i:04d}.flo",
             "raft_flow_raft-small_{i:04d}.png"]


def test_cli_bidirectional_sequence_warm(tmp_path):
    import infer_raft
    from raft_amd.data.imageio import read_png
    from raft_amd.utils.flow_io import read_flo
    seq = _write_seq(tmp_path)
    out = tmp_path / "out"
    infer_raft.main(["--mode", "test", "--small", "--data", str(seq),
                     "--out", str(out), "--size", "40x56", "--iters", "2",
                     "--bidirectional", "--warm"])
    for i in range(2):
        for name in OLD_FILES + NEW_FILES:
            assert (out / name.format(i=i)).exists(), name.format(i=i)
    assert len(list(out.iterdir())) == 12
    bw = read_flo(str(out / "raft_flow_raft-small_0001_bw.flo"))
    assert bw.shape == (40, 56, 2)
    occ = read_png(str(out / "raft_occ_raft-small_0000_fw.png"))
    assert occ.shape[:2] == (40, 56)
    assert set(np.unique(occ).tolist()) <= {0, 255}


def test_cli_without_flag_writes_no_new_files(tmp_path):
    import infer_raft
    seq = _write_seq(tmp_path)
    out = tmp_path / "out"
    infer_raft.main(["--mode", "test", "--small", "--data", str(seq),
                     "--out", str(out), "--size", "40x56", "--iters", "2",
                     "--warm"])
    names = sorted(p.name for p in out.iterdir())
    assert names == sorted(n.format(i=i) for i in range(2)
                           for n in OLD_FILES)
