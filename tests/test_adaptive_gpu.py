"""GPU tests for convergence-gated refinement: the flow_residual kernel
against the oracle (bit for bit, both memory layouts, captured), and the
fused loop's gate — every gated result equals the ungated fused iters=n
call bit for bit, with the loop graph on AUTO, forced on and forced off."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from raft_amd import RAFT, Convergence, ConvergenceInfo, RaftConfig
from raft_amd.ops import torch_ref as R


def _hip():
    from raft_amd.ops import require_hip
    return require_hip()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


# ------------------------------------------------------------------ kernel
def residual_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    prev = torch.rand(B, 2, H, W, generator=g) * 20.0
    nxt = prev + torch.randn(B, 2, H, W, generator=g) * 0.3
    return prev, nxt


def _layout(t, dev, interleaved):
    """The logical [B,2,H,W] tensor on the device: planar, or the view of
    an interleaved [B,H,W,2] buffer (the fused loop's coords)."""
    t = t.to(dev)
    if not interleaved:
        return t.contiguous()
    v = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert v.stride(1) == 1 or v.shape[1] == 1
    return v


def _unpack(raw):
    raw = raw.cpu()
    return raw[:, 0].contiguous().view(torch.float32), raw[:, 1].long()


def _assert_same(got, ref):
    (max_sq, above), (ref_max, ref_above) = got, ref
    max_sq, above = max_sq.cpu(), above.cpu()
    assert max_sq.dtype == torch.float32 and above.dtype == torch.int64
    nan = torch.isnan(ref_max)
    assert torch.equal(torch.isnan(max_sq), nan)
    assert torch.equal(max_sq[~nan].view(torch.int32),
                       ref_max[~nan].view(torch.int32))
    assert torch.equal(above, ref_above)


# a single cell; one partial wave; batch stride, one wave plus a tail;
# several blocks per sample with a ragged tail; the headline 1/8 grid
SHAPES = [(1, 1, 1), (1, 5, 7), (2, 9, 13), (3, 17, 64), (1, 55, 128)]


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_flow_residual_matches_oracle_exactly(dev, B, H, W):
    from raft_amd import ops
    prev, nxt = residual_inputs(B, H, W, B * 1000 + H * W)
    d = nxt - prev
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).flatten()
    thresholds = [0.0, float(d2[d2.numel() // 3]), float(d2.median()),
                  math.inf]
    # special inputs: the all-zero update; a NaN cell in the first sample
    # and a +inf cell in the last (the same sample when B == 1, where NaN
    # must win), every other sample clean
    bad = nxt.clone()
    bad[0, 0, H // 2, W // 2] = float("nan")
    bad[B - 1, 1, H - 1, W - 1] = float("inf")
    inputs = [(prev, nxt), (prev, prev.clone()), (prev, bad)]
    for interleaved in (False, True):
        for p, n in inputs:
            pd, nd = _layout(p, dev, interleaved), _layout(n, dev,
                                                           interleaved)
            for thr in thresholds:
                ref = R.flow_residual(p, n, thr)
                raw = _hip().flow_residual(pd, nd, thr, None)
                assert raw.shape == (B, 2) and raw.dtype == torch.int32
                _assert_same(_unpack(raw), ref)
                _assert_same(ops.flow_residual(pd, nd, thr), ref)
    ref = R.flow_residual(prev, bad, thresholds[2])
    assert math.isnan(ref[0][0])
    if B > 1:
        assert math.isinf(ref[0][B - 1])
    # the equality cell is not above
    k = d2.numel() // 3
    ref = R.flow_residual(prev, nxt, thresholds[1])
    assert int(ref[1].sum()) == int((d2 > d2[k]).sum())


def _check_against_oracle(prev, nxt, pd, nd, thr=0.01):
    _assert_same(_unpack(_hip().flow_residual(pd, nd, thr, None)),
                 R.flow_residual(prev, nxt, thr))


# the listed shapes, then single columns and rows (the stride of a size-1
# dim is meaningless, so the cell stride must come from the other one)
@pytest.mark.parametrize("B,H,W", SHAPES + [(2, 7, 1), (2, 1, 9), (1, 300, 1)])
def test_flow_residual_reads_both_layouts_in_place(dev, B, H, W):
    """Planar and interleaved coords run without a copy; a view whose cells
    do not sit at one stride, or a pair of unlike layouts, is copied — and
    every case still matches the oracle."""
    prev, nxt = residual_inputs(B, H, W, 11)
    in_place = _hip().flow_residual_in_place
    for interleaved in (False, True):
        p, n = _layout(prev, dev, interleaved), _layout(nxt, dev,
                                                        interleaved)
        assert in_place(p, n)
        _check_against_oracle(prev, nxt, p, n)
    # a size-1 dim with a nonsense stride changes nothing
    if W == 1 or H == 1:
        dim = 3 if W == 1 else 2
        strides = list(_layout(prev, dev, False).stride())
        strides[dim] = 12345
        p, n = (torch.as_strided(_layout(t, dev, False), t.shape, strides)
                for t in (prev, nxt))
        assert in_place(p, n)
        _check_against_oracle(prev, nxt, p, n)
    # the fused loop's coords: [B,H8,W8,2] buffers seen as [B,2,H8,W8]
    buf_p = prev.permute(0, 2, 3, 1).contiguous().to(dev)
    buf_n = nxt.permute(0, 2, 3, 1).contiguous().to(dev)
    assert in_place(buf_p.permute(0, 3, 1, 2), buf_n.permute(0, 3, 1, 2))
    if H > 1 and W > 1:
        # the left half of a wider field: rows are 2W cells apart, so the
        # cells do not sit at one stride and the op has to copy
        wide_p, wide_n = residual_inputs(B, H, 2 * W, 12)
        vp, vn = wide_p.to(dev)[..., :W], wide_n.to(dev)[..., :W]
        assert not in_place(vp, vn)
        _check_against_oracle(wide_p[..., :W], wide_n[..., :W], vp, vn)
        # unlike layouts
        p, n = _layout(prev, dev, False), _layout(nxt, dev, True)
        assert not in_place(p, n)
        _check_against_oracle(prev, nxt, p, n)


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_flow_residual_clears_its_result(dev, B, H, W):
    """Two calls into the same result tensor: the memset is part of the op
    (the atomics would otherwise fold into the earlier, larger result)."""
    prev, nxt = residual_inputs(B, H, W, 7)
    big = prev + 5.0
    for interleaved in (False, True):
        p, n, b = (_layout(t, dev, interleaved) for t in (prev, nxt, big))
        out = _hip().flow_residual(p, b, 0.0, None)
        first = out.clone()
        again = _hip().flow_residual(p, n, 0.01, out)
        assert again.data_ptr() == out.data_ptr()
        fresh = _hip().flow_residual(p, n, 0.01, None)
        assert torch.equal(out, fresh) and not torch.equal(out, first)
        _hip().flow_residual(p, n, 0.01, out)
        assert torch.equal(out, fresh)
        _assert_same(_unpack(out), R.flow_residual(prev, nxt, 0.01))


@pytest.mark.parametrize("B,H,W", SHAPES)
def test_flow_residual_graph_capture(dev, B, H, W):
    prev, nxt = residual_inputs(B, H, W, 8)
    for interleaved in (False, True):
        p, n = _layout(prev, dev, interleaved), _layout(nxt, dev,
                                                        interleaved)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _hip().flow_residual(p, n, 0.01, None)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = _hip().flow_residual(p, n, 0.01, None)
        for seed in (9, 10):
            p2, n2 = residual_inputs(B, H, W, seed)
            if seed == 10:
                n2[0, 1, 0, 0] = float("nan")
            p.copy_(p2)
            n.copy_(n2)
            g.replay()
            _assert_same(_unpack(out), R.flow_residual(p2, n2, 0.01))
        del g
        torch.cuda.synchronize()


# -------------------------------------------------------------- fused loop
BUDGET = 8
SEED = 3
MODES = [None, True, False]          # loop graph: AUTO (on at 8), on, off


def expected_stop(trace, tol, every, min_iters, budget):
    for i, max_px, _ in trace:
        if i % every == 0 and i >= min_iters and i < budget \
                and max_px <= tol:
            return i + 1
    return budget


def trace_tolerances(trace):
    v = sorted(t[1] for t in trace)
    return [(a + b) / 2 for a, b in zip(v, v[1:]) if b - a >= 1e-3 * b]


class Case:
    """One bf16 model and frame pair on the fused path; ungated references
    are computed once per iteration count (eager loop) and shared."""

    def __init__(self, small, H, W, zero_head=False):
        dev = torch.device("cuda:0")
        torch.manual_seed(SEED)
        m = RAFT(RaftConfig(small=small))
        if zero_head:
            with torch.no_grad():
                m.update_block.flow_head.conv2.weight.zero_()
                m.update_block.flow_head.conv2.bias.zero_()
        self.model = m.to(dev).to(torch.bfloat16).eval()
        g = torch.Generator().manual_seed(SEED + 1)
        self.x1, self.x2 = (
            torch.rand(1, 3, H, W, generator=g).to(dev, torch.bfloat16)
            .contiguous(memory_format=torch.channels_last) for _ in range(2))
        self.H, self.W = H, W
        self._ungated = {}
        from raft_amd.models import fused
        with torch.no_grad():
            assert fused.can_fuse(self.model, self.x1)

    def ungated(self, n, **kw):
        key = (n,) + tuple(sorted(kw))
        if key not in self._ungated:
            self.model._fused_use_graph = False
            with torch.no_grad():
                res = self.model(self.x1, self.x2, iters=n, **kw)
            self._ungated[key] = res
        return self._ungated[key]

    def gated(self, conv, mode, budget=BUDGET, **kw):
        self.model._fused_use_graph = mode
        with torch.no_grad():
            res = self.model(self.x1, self.x2, iters=budget, converge=conv,
                             return_info=True, **kw)
        # a captured loop hands out its static buffers: keep copies
        return tuple(t.clone() if torch.is_tensor(t) else t for t in res)

    def release(self):
        self.model.__dict__.pop("_fused_cache", None)
        torch.cuda.synchronize()


# 64x96: an 8x12 grid, one block per sample; 136x200: a 17x25 grid (425
# cells, two blocks per sample with a ragged tail)
@pytest.fixture(scope="module",
                params=[(False, 64, 96), (True, 64, 96),
                        (False, 136, 200), (True, 136, 200)],
                ids=["things-64x96", "small-64x96", "things-136x200",
                     "small-136x200"])
def case(request):
    c = Case(*request.param)
    yield c
    c.release()


@pytest.fixture(scope="module")
def trace(case):
    out, info = case.gated(Convergence(tol=None, every=1), False)
    assert info.iters_run == BUDGET
    assert [c[0] for c in info.checks] == list(range(1, BUDGET))
    assert torch.equal(out, case.ungated(BUDGET))
    return info.checks


def _all_modes(case, conv, n, budget=BUDGET, checks=None):
    infos = []
    for mode in MODES:
        out, info = case.gated(conv, mode, budget)
        assert info.iters_run == n, (mode, info)
        assert torch.equal(out, case.ungated(n)), mode
        if checks is not None:
            assert [c[0] for c in info.checks] == checks, mode
        infos.append(info)
    assert infos[0] == infos[1] == infos[2]
    return infos[0]


def test_fused_stops_where_the_trace_says(case, trace):
    tols = trace_tolerances(trace)
    assert len(tols) >= 2, trace            # else: change SEED
    for tol in tols:
        for every, min_iters in ((1, 1), (1, 3), (2, 1)):
            n = expected_stop(trace, tol, every, min_iters, BUDGET)
            info = _all_modes(case, Convergence(tol=tol, every=every,
                                                min_iters=min_iters), n)
            want = [c for c in trace
                    if c[0] % every == 0 and min_iters <= c[0] < n]
            # (iteration, max_px) are the trace's; frac_above depends on tol
            assert [c[:2] for c in info.checks] == [c[:2] for c in want]


@pytest.mark.parametrize("kw,n,checks", [
    (dict(tol=1e9, every=2, min_iters=3), 5, [4]),
    (dict(tol=1e9, every=3), 4, [3]),
    (dict(tol=1e9, every=8), 8, []),
    (dict(tol=0.0, every=3), 8, [3, 6]),
])
def test_fused_forced_stops(case, trace, kw, n, checks):
    _all_modes(case, Convergence(**kw), n, checks=checks)


def test_fused_one_graph_pair_per_shape(case, trace):
    """Every budget and Convergence of a shape replays one (step, tail)
    pair, held as one shape bucket."""
    from raft_amd.models import fused
    f = fused.get_fused(case.model)
    for conv, budget, n in ((Convergence(tol=1e9, every=2), 8, 3),
                            (Convergence(tol=1e9, every=4), 12, 5),
                            (Convergence(tol=None, every=1), 6, 6)):
        out, info = case.gated(conv, True, budget)
        assert info.iters_run == n
        assert torch.equal(out, case.ungated(n))
    keys = [k for k in f._graphs if k[0] == 1 and "gated" in k]
    assert len(keys) == 1 and len(f._graphs) <= 4


def test_fused_gated_calls_repeat_exactly(case, trace):
    conv = Convergence(tol=trace_tolerances(trace)[0], every=1, min_iters=2)
    for mode in MODES:
        a, ia = case.gated(conv, mode)
        b, ib = case.gated(conv, mode)
        assert torch.equal(a, b) and ia == ib and len(ia.checks) >= 1


def test_fused_bidirectional_and_return_order(case, trace):
    g = torch.Generator().manual_seed(6)
    dev = case.x1.device
    init = tuple(torch.randn(1, 2, case.H // 8, case.W // 8, generator=g)
                 .to(dev) for _ in range(2))
    conv = Convergence(tol=1e9, every=2, min_iters=3)
    ref = case.ungated(5, bidirectional=True, return_low=True)
    refw = None
    for mode in MODES:
        res = case.gated(conv, mode, bidirectional=True, return_low=True)
        assert len(res) == 5 and res[4].iters_run == 5
        assert [c[0] for c in res[4].checks] == [4]
        for a, b in zip(res[:4], ref):
            assert torch.equal(a, b)
        warm = case.gated(conv, mode, bidirectional=True, flow_init=init)
        assert warm[2].iters_run == 5
        if refw is None:
            case.model._fused_use_graph = False
            with torch.no_grad():
                refw = case.model(case.x1, case.x2, iters=5,
                                  bidirectional=True, flow_init=init)
            assert not torch.equal(refw[0], ref[0])
        assert torch.equal(warm[0], refw[0])
        assert torch.equal(warm[1], refw[1])


@pytest.mark.parametrize("small", [False, True], ids=["things", "small"])
@pytest.mark.parametrize("H,W", [(64, 96), (136, 200)])
def test_fused_zeroed_flow_head_converges_at_once(small, H, W):
    case = Case(small, H, W, zero_head=True)
    conv = Convergence(tol=0.0, every=2)
    for mode in MODES:
        out, info = case.gated(conv, mode)
        assert info == ConvergenceInfo(iters_run=3, checks=[(2, 0.0, 0.0)])
        assert torch.equal(out, case.ungated(3))
    case.release()


@pytest.mark.parametrize("small", [False, True], ids=["things", "small"])
@pytest.mark.parametrize("loop_graph", MODES)
def test_fused_warm_session(small, loop_graph):
    """Four frames through a warm gated session: each pair stops where the
    rule says and equals the ungated session at that count."""
    from raft_amd.engine import InferenceEngine
    dev = torch.device("cuda:0")
    torch.manual_seed(SEED)
    m = RAFT(RaftConfig(small=small)).to(dev).eval()
    eng = InferenceEngine(m, iters=BUDGET, dtype=torch.bfloat16,
                          loop_graph=loop_graph)
    g = torch.Generator().manual_seed(12)
    frames = [torch.rand(1, 3, 64, 96, generator=g).to(dev, torch.bfloat16)
              for _ in range(4)]
    conv = Convergence(tol=1e9, every=2, min_iters=3)
    gated = eng.stream(warm=True, converge=conv)
    assert gated.push(frames[0]) is None and gated.last_iters is None
    outs = []
    for x in frames[1:]:
        outs.append(gated.push(x))
        assert gated.last_iters == 5 and eng.last_info.iters_run == 5
        assert [c[0] for c in gated.last_info.checks] == [4]
    eng.loop_graph = False
    fixed = eng.stream(warm=True, iters=5)
    plain = eng.stream(warm=True)
    fixed.push(frames[0])
    plain.push(frames[0])
    for x, out in zip(frames[1:], outs):
        assert torch.equal(out, fixed.push(x))
        assert fixed.last_iters == 5
        plain.push(x)
        assert plain.last_iters == BUDGET and plain.last_info.checks == []
    # the engine's own entry points
    eng.loop_graph = loop_graph
    out = eng(frames[0], frames[1], converge=conv).clone()
    assert eng.last_info.iters_run == 5
    eng.loop_graph = False
    assert torch.equal(out, eng(frames[0], frames[1], iters=5))
    m.__dict__.pop("_fused_cache", None)
    torch.cuda.synchronize()
