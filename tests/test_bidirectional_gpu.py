"""GPU tests for the shared-pass bidirectional path: the dual-store
correlation volume, the forward-backward consistency kernel, the fused
model and the engine."""
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from raft_amd.ops import torch_ref as R


def _hip():
    from raft_amd.ops import require_hip
    return require_hip()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _fb_inputs(B=2, H=37, W=53):
    fw = F.interpolate(torch.randn(B, 2, 5, 7) * 2.0, size=(H, W),
                       mode="bilinear", align_corners=True)
    bw = -fw + torch.randn(B, 2, H, W) * 0.4
    return fw.contiguous(), bw.contiguous()


def _check_masks(occ, occ_ref, res, bound):
    clear = (res - bound).abs() > 1e-3 * (1 + bound)
    assert (~clear).float().mean().item() <= 0.01
    assert torch.equal(occ[clear], occ_ref[clear])


def _inb(flow):
    """In-frame decision of the oracle's definition (one fp32 add)."""
    _, _, H, W = flow.shape
    px = torch.arange(W, dtype=torch.float32).view(1, 1, W) + flow[:, 0]
    py = torch.arange(H, dtype=torch.float32).view(1, H, 1) + flow[:, 1]
    return ((px >= 0) & (px <= W - 1) & (py >= 0) & (py <= H - 1)) \
        .unsqueeze(1)


# (2,12,12): M=144, interior + edge tiles, batch stride; (1,12,15): M=180,
# M % 8 != 0 -> scalar reverse store next to an interior tile; (1,16,16):
# M=256, all interior, vector path only; (1,5,7): M=35, one edge tile.
@pytest.mark.parametrize("B,H,W", [(2, 12, 12), (1, 12, 15), (1, 16, 16),
                                   (1, 5, 7)])
def test_corr_volume_bidir_exact(dev, B, H, W):
    C, M = 128, H * W
    f1 = torch.randn(B, H, W, C, device=dev).to(torch.bfloat16).contiguous()
    f2 = torch.randn(B, H, W, C, device=dev).to(torch.bfloat16).contiguous()
    out = _hip().corr_volume_nhwc_bidir(f1, f2)
    assert out.shape == (2 * B, M, H, W) and out.dtype == torch.bfloat16
    fwd = _hip().corr_volume_nhwc(f1, f2, True)
    assert torch.equal(out[:B], fwd)
    assert torch.equal(out[B:].view(B, M, M),
                       out[:B].view(B, M, M).transpose(1, 2))
    ref = R.corr_volume(f2.float().permute(0, 3, 1, 2),
                        f1.float().permute(0, 3, 1, 2))
    err = (out[B:].float() - ref).abs().max().item()
    assert err < 0.02 * ref.abs().max().item() + 0.05, err


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fb_consistency_matches_oracle(dev, dtype):
    fw, bw = _fb_inputs()
    fw, bw = fw.to(dtype), bw.to(dtype)
    B = fw.shape[0]
    occ, res, bound = _hip().fb_consistency(fw.to(dev), bw.to(dev), 0.01,
                                            0.5, True)
    assert occ.shape == (2 * B, 1, 37, 53) and occ.dtype == torch.uint8
    occ, res, bound = occ.cpu().bool(), res.cpu(), bound.cpu()
    # oracle on the same (possibly bf16-rounded) values, both directions
    for sl, a, b in ((slice(0, B), fw, bw), (slice(B, 2 * B), bw, fw)):
        o_ref, r_ref, b_ref = R.fb_consistency(a.float(), b.float(),
                                               return_terms=True)
        assert torch.allclose(res[sl], r_ref, rtol=1e-4, atol=1e-5)
        assert torch.allclose(bound[sl], b_ref, rtol=1e-4, atol=1e-5)
        # in-frame decisions are identical: every leaving pixel is flagged
        # whatever its residual, and the rest follow the threshold
        out_of_frame = ~_inb(a.float())
        assert out_of_frame.any()
        assert occ[sl][out_of_frame].all()
        _check_masks(occ[sl], o_ref, r_ref, b_ref)
    # the public op returns the same masks as bool halves
    from raft_amd import ops
    o_fw, o_bw = ops.fb_consistency(fw.to(dev), bw.to(dev))
    assert o_fw.dtype == torch.bool
    assert torch.equal(o_fw.cpu(), occ[:B]) and torch.equal(o_bw.cpu(),
                                                            occ[B:])


def _eager_refs(m, x1, x2, iters):
    """Eager bf16 references for both directions. An InferenceEngine made
    earlier in the session leaves cudnn.benchmark on, and a MIOpen find
    per new conv shape would cost each case ~15 s: the references only
    need to be right, so they run in immediate mode."""
    os.environ["RAFT_AMD_NO_FUSE"] = "1"
    bench = torch.backends.cudnn.benchmark
    torch.backends.cudnn.benchmark = False
    try:
        return m(x1, x2, iters=iters), m(x2, x1, iters=iters)
    finally:
        torch.backends.cudnn.benchmark = bench
        os.environ.pop("RAFT_AMD_NO_FUSE")


def _fused_vs_eager(dev, small, H, W, iters, min_diff=None):
    from raft_amd import RAFT, RaftConfig
    import raft_amd.models.fused as fused
    torch.manual_seed(11)
    m = RAFT(RaftConfig(small=small)).to(dev).to(torch.bfloat16).eval()
    x1 = torch.rand(1, 3, H, W, device=dev, dtype=torch.bfloat16)
    x2 = torch.rand(1, 3, H, W, device=dev, dtype=torch.bfloat16)
    with torch.no_grad():
        ref_fw, ref_bw = _eager_refs(m, x1, x2, iters)
        assert fused.can_fuse(m, x1)
        fw, bw = m(x1, x2, iters=iters, bidirectional=True)
    assert getattr(m, "_fused_cache", None) is not None
    assert fw.shape == ref_fw.shape and bw.shape == ref_bw.shape
    e_fw = (fw.float() - ref_fw.float()).abs().max().item()
    e_bw = (bw.float() - ref_bw.float()).abs().max().item()
    sep = (ref_fw.float() - ref_bw.float()).abs().max().item()
    print(f"small={small} {H}x{W} iters={iters}: err fw {e_fw:.4g} "
          f"bw {e_bw:.4g}, refs differ by {sep:.4g}")
    if min_diff is not None:
        # the two directions must be far enough apart for the comparison
        # to tell a swapped pair
        assert sep > min_diff, (small, sep)
    assert e_fw < 0.05, (small, e_fw)
    assert e_bw < 0.05, (small, e_bw)
    del m._fused_cache
    torch.cuda.synchronize()


@pytest.mark.parametrize("small", [False, True])
def test_fused_bidirectional_matches_eager_bf16(dev, small):
    _fused_vs_eager(dev, small, 64, 96, 6, min_diff=0.1)


@pytest.mark.parametrize("H,W", [(40, 56), (96, 120), (64, 64)])
@pytest.mark.parametrize("small", [False, True])
def test_fused_bidirectional_shape_sweep(dev, small, H, W):
    _fused_vs_eager(dev, small, H, W, 3)


def test_bidirectional_graph_and_determinism(dev):
    from raft_amd import RAFT, RaftConfig
    from raft_amd.models import fused
    m = RAFT(RaftConfig(small=True)).to(dev).to(torch.bfloat16).eval()
    x1 = torch.rand(1, 3, 64, 96, device=dev, dtype=torch.bfloat16)
    x2 = torch.rand(1, 3, 64, 96, device=dev, dtype=torch.bfloat16)
    with torch.no_grad():
        fw, bw = m(x1, x2, iters=8, bidirectional=True)     # captured
        f = fused.get_fused(m)
        assert len(f._graphs) == 1
        fw, bw = fw.clone(), bw.clone()     # replays reuse the out buffer
        fw2, bw2 = m(x1, x2, iters=8, bidirectional=True)   # replay
        assert len(f._graphs) == 1
    assert torch.equal(fw, fw2) and torch.equal(bw, bw2)
    m2 = RAFT(RaftConfig(small=True)).to(dev).to(torch.bfloat16).eval()
    m2.load_state_dict(m.state_dict())
    m2._fused_use_graph = False
    with torch.no_grad():
        fw_e, bw_e = m2(x1, x2, iters=8, bidirectional=True)
    assert torch.allclose(fw.float(), fw_e.float(), atol=1e-3), \
        (fw.float() - fw_e.float()).abs().max().item()
    assert torch.allclose(bw.float(), bw_e.float(), atol=1e-3), \
        (bw.float() - bw_e.float()).abs().max().item()
    # release the captured graph + its pool before later capture tests
    del m._fused_cache
    torch.cuda.synchronize()


def test_bidirectional_ignores_fp8_corr_with_warning(dev):
    """fp8 volumes are unidirectional only: a bidirectional run under
    RAFT_AMD_FP8_CORR warns once and computes exactly what it computes
    without the switch."""
    import warnings

    from raft_amd import RAFT, RaftConfig
    from raft_amd.models import fused
    m = RAFT(RaftConfig(small=True)).to(dev).to(torch.bfloat16).eval()
    m._fused_use_graph = False
    x1 = torch.rand(1, 3, 64, 96, device=dev, dtype=torch.bfloat16)
    x2 = torch.rand(1, 3, 64, 96, device=dev, dtype=torch.bfloat16)
    with torch.no_grad():
        fw, bw = m(x1, x2, iters=2, bidirectional=True)
        fused._warned_bidir_fp8 = False
        os.environ["RAFT_AMD_FP8_CORR"] = "2"
        try:
            with pytest.warns(UserWarning, match="RAFT_AMD_FP8_CORR"):
                fw8, bw8 = m(x1, x2, iters=2, bidirectional=True)
            with warnings.catch_warnings():
                # warned once: a second call must stay silent
                warnings.filterwarnings("error",
                                        message=".*RAFT_AMD_FP8_CORR.*")
                m(x1, x2, iters=2, bidirectional=True)
        finally:
            os.environ.pop("RAFT_AMD_FP8_CORR")
    assert torch.equal(fw, fw8) and torch.equal(bw, bw8)
    del m._fused_cache
    torch.cuda.synchronize()


def test_engine_bidirectional_gpu_bf16(dev):
    from raft_amd import RAFT, RaftConfig
    from raft_amd.engine.inference import InferenceEngine
    m = RAFT(RaftConfig(small=False)).to(dev)
    eng = InferenceEngine(m, iters=4, dtype=torch.bfloat16)
    x1 = torch.rand(1, 3, 44, 60)
    x2 = torch.rand(1, 3, 44, 60)
    out = eng.bidirectional(x1, x2)
    for flow in (out.flow_fw, out.flow_bw):
        assert flow.shape == (1, 2, 44, 60) and flow.is_cuda
        assert flow.dtype == torch.float32 and torch.isfinite(flow).all()
    for occ in (out.occ_fw, out.occ_bw):
        assert occ.shape == (1, 1, 44, 60) and occ.dtype == torch.bool
    fw, bw = out.flow_fw.cpu(), out.flow_bw.cpu()
    for occ, a, b in ((out.occ_fw, fw, bw), (out.occ_bw, bw, fw)):
        o_ref, r_ref, b_ref = R.fb_consistency(a, b, return_terms=True)
        _check_masks(occ.cpu(), o_ref, r_ref, b_ref)
    del m._fused_cache
    torch.cuda.synchronize()
