"""Convergence-gated refinement on the CPU: the flow_residual oracle against
a scalar loop, the stopping rule of the eager loop (a gated call that ran n
iterations equals the ungated iters=n call bit for bit), and the layers
above it — engine, video session, serving, CLI."""
import math

import numpy as np
import pytest
import torch

from raft_amd import RAFT, Convergence, ConvergenceInfo, RaftConfig
from raft_amd.ops import torch_ref as R


# ------------------------------------------------------------------ oracle
def scalar_residual(prev, nxt, thr_sq):
    """flow_residual as a scalar fp32 loop: every operation rounded on its
    own, NaN handled by hand."""
    p, n = prev.numpy(), nxt.numpy()
    thr = np.float32(thr_sq)
    B, _, H, W = p.shape
    max_sq, above = [], []
    with np.errstate(all="ignore"):
        for b in range(B):
            m, nan, cnt = np.float32(0.0), False, 0
            for y in range(H):
                for x in range(W):
                    dx = np.float32(n[b, 0, y, x] - p[b, 0, y, x])
                    dy = np.float32(n[b, 1, y, x] - p[b, 1, y, x])
                    d2 = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
                    if not d2 <= thr:
                        cnt += 1
                    if np.isnan(d2):
                        nan = True
                    elif d2 > m:
                        m = d2
            max_sq.append(np.float32("nan") if nan else m)
            above.append(cnt)
    return np.array(max_sq, np.float32), np.array(above, np.int64)


def _same(max_sq, above, ref_max, ref_above):
    assert max_sq.dtype == torch.float32 and above.dtype == torch.int64
    got = max_sq.numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref_max))
    ok = ~np.isnan(ref_max)
    assert np.array_equal(got[ok].view(np.int32), ref_max[ok].view(np.int32))
    assert np.array_equal(above.numpy(), ref_above)


def residual_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    prev = torch.rand(B, 2, H, W, generator=g) * 20.0
    nxt = prev + torch.randn(B, 2, H, W, generator=g) * 0.3
    return prev, nxt


def test_flow_residual_matches_scalar_loop():
    prev, nxt = residual_inputs(3, 5, 7, 0)
    nxt[0, 0, 2, 3] = float("nan")        # sample 0: a NaN cell
    nxt[1, 1, 0, 0] = float("inf")        # sample 1: a +inf cell
    d = nxt - prev                        # sample 2 stays clean
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    clean = d2[2].flatten()
    eq = float(clean[11])                 # one cell's exact d2
    for thr in (0.0, eq, float(clean.median()), math.inf):
        max_sq, above = R.flow_residual(prev, nxt, thr)
        _same(max_sq, above, *scalar_residual(prev, nxt, thr))
    max_sq, above = R.flow_residual(prev, nxt, eq)
    assert math.isnan(max_sq[0]) and math.isinf(max_sq[1])
    assert float(max_sq[2]) == float(clean.max())      # nothing leaks over
    # the equality cell is not above: only strictly larger cells count
    assert int(above[2]) == int((clean > eq).sum()) < clean.numel()
    assert int(above[2]) == int((clean >= eq).sum()) - 1
    # NaN counts as above even against +inf, +inf does not
    _, above = R.flow_residual(prev, nxt, math.inf)
    assert above.tolist() == [1, 0, 0]
    # the all-zero update
    max_sq, above = R.flow_residual(prev, prev.clone(), 0.0)
    assert max_sq.tolist() == [0.0] * 3 and above.tolist() == [0] * 3


def test_ops_flow_residual_dispatches_to_oracle_on_cpu():
    from raft_amd import ops
    prev, nxt = residual_inputs(2, 4, 6, 1)
    a = ops.flow_residual(prev, nxt, 0.01)
    b = R.flow_residual(prev, nxt, 0.01)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with pytest.raises(ValueError):
        ops.flow_residual(prev, nxt[:, :1], 0.01)


# ------------------------------------------------------------ dataclass
def test_convergence_fields():
    c = Convergence(tol=0.5)
    assert (c.every, c.min_iters, c.frac) == (4, 1, 0.0)
    t = np.float32(0.5) / np.float32(8)
    assert c.thr_sq == float(np.float32(t * t))
    assert Convergence(tol=None).thr_sq == math.inf
    for kw in (dict(tol=-1.0), dict(tol=float("nan")),
               dict(tol=1.0, every=0), dict(tol=1.0, min_iters=0),
               dict(tol=1.0, frac=1.0), dict(tol=1.0, frac=-0.1)):
        with pytest.raises(ValueError):
            Convergence(**kw)
    # check iterations: i % every == 0, i >= min_iters, i < N
    c = Convergence(tol=1.0, every=2, min_iters=3)
    assert [i for i in range(1, 9) if c.checks_after(i, 8)] == [4, 6]


# ----------------------------------------------------------- eager loop
HH, WW, BUDGET = 64, 96, 8
SEED = 3


def expected_stop(trace, tol, every, min_iters, budget):
    """The stop the rule prescribes, read off an every=1 trace: the first
    check iteration whose max_px is within tol, plus the final one."""
    for i, max_px, _ in trace:
        if i % every == 0 and i >= min_iters and i < budget \
                and max_px <= tol:
            return i + 1
    return budget


def trace_tolerances(trace):
    """Midpoints between adjacent sorted trace values at least 0.1 % apart:
    tolerances at which the decision has a margin."""
    v = sorted(t[1] for t in trace)
    return [(a + b) / 2 for a, b in zip(v, v[1:]) if b - a >= 1e-3 * b]


class Case:
    def __init__(self, small):
        torch.manual_seed(SEED)
        self.model = RAFT(RaftConfig(small=small)).eval()
        g = torch.Generator().manual_seed(SEED + 1)
        self.x1 = torch.rand(1, 3, HH, WW, generator=g)
        self.x2 = torch.rand(1, 3, HH, WW, generator=g)
        self._ungated = {}
        with torch.no_grad():
            self.traced, self.trace = self.model(
                self.x1, self.x2, iters=BUDGET,
                converge=Convergence(tol=None, every=1), return_info=True)

    def ungated(self, n):
        if n not in self._ungated:
            with torch.no_grad():
                self._ungated[n] = self.model(self.x1, self.x2, iters=n)
        return self._ungated[n]

    def gated(self, conv, budget=BUDGET):
        with torch.no_grad():
            return self.model(self.x1, self.x2, iters=budget, converge=conv,
                              return_info=True)


@pytest.fixture(scope="module", params=[False, True],
                ids=["things", "small"])
def case(request):
    return Case(request.param)


def test_trace_only_runs_the_whole_budget(case):
    info = case.trace
    assert isinstance(info, ConvergenceInfo)
    assert info.iters_run == BUDGET
    assert [c[0] for c in info.checks] == list(range(1, BUDGET))
    assert all(c[1] > 0 and c[2] == 0.0 for c in info.checks)
    assert torch.equal(case.traced, case.ungated(BUDGET))


def test_stops_where_the_trace_says(case):
    tols = trace_tolerances(case.trace.checks)
    assert len(tols) >= 2, case.trace.checks   # else: change SEED
    stops = set()
    for tol in tols:
        for every, min_iters in ((1, 1), (1, 3), (2, 1)):
            n = expected_stop(case.trace.checks, tol, every, min_iters,
                              BUDGET)
            out, info = case.gated(Convergence(tol=tol, every=every,
                                               min_iters=min_iters))
            assert info.iters_run == n, (tol, every, min_iters)
            assert torch.equal(out, case.ungated(n)), (tol, every, min_iters)
            # the checks taken are the trace's, up to the stop
            want = [c for c in case.trace.checks
                    if c[0] % every == 0 and min_iters <= c[0] < n]
            assert [c[:2] for c in info.checks] == [c[:2] for c in want]
            stops.add(n)
    print("stops exercised:", sorted(stops))


@pytest.mark.parametrize("kw,budget,n,checks", [
    (dict(tol=1e9, every=2, min_iters=3), BUDGET, 5, [4]),
    (dict(tol=1e9, every=3), BUDGET, 4, [3]),
    (dict(tol=1e9, every=8), BUDGET, 8, []),
    (dict(tol=1e9, every=1), 1, 1, []),
    (dict(tol=0.0, every=3), BUDGET, 8, [3, 6]),      # never converges
])
def test_forced_stops(case, kw, budget, n, checks):
    out, info = case.gated(Convergence(**kw), budget)
    assert info.iters_run == n
    assert [c[0] for c in info.checks] == checks
    assert torch.equal(out, case.ungated(n))


def test_frac_lets_a_share_of_cells_move(case):
    """At a tolerance that k of the cells exceed at the first check, the
    loop stops there iff floor(frac * cells) >= k."""
    tol = case.trace.checks[1][1] / 2          # half of iteration 2's max
    _, info = case.gated(Convergence(tol=tol, every=2))
    assert info.iters_run == BUDGET            # frac=0: the max decides
    cells = (HH // 8) * (WW // 8)
    # frac_above is the largest per-sample share of cells still moving
    k = round(info.checks[0][2] * cells)
    print(f"{k} of {cells} cells above {tol:.4g} px")
    assert 1 < k < cells
    out, info = case.gated(Convergence(tol=tol, every=2,
                                       frac=(k + 0.5) / cells))
    assert info.iters_run == 3 and len(info.checks) == 1
    assert torch.equal(out, case.ungated(3))
    _, info = case.gated(Convergence(tol=tol, every=2, min_iters=2,
                                     frac=(k - 0.5) / cells))
    assert info.checks[0][:1] == (2,) and info.iters_run > 3


@pytest.mark.parametrize("small", [False, True], ids=["things", "small"])
def test_zeroed_flow_head_converges_at_once(small):
    torch.manual_seed(SEED)
    m = RAFT(RaftConfig(small=small)).eval()
    with torch.no_grad():
        m.update_block.flow_head.conv2.weight.zero_()
        m.update_block.flow_head.conv2.bias.zero_()
        g = torch.Generator().manual_seed(5)
        x1 = torch.rand(1, 3, HH, WW, generator=g)
        x2 = torch.rand(1, 3, HH, WW, generator=g)
        out, info = m(x1, x2, iters=BUDGET,
                      converge=Convergence(tol=0.0, every=2),
                      return_info=True)
        assert info.iters_run == 3
        assert info.checks == [(2, 0.0, 0.0)]
        assert torch.equal(out, m(x1, x2, iters=3))


def test_bidirectional_warm_and_return_order(case):
    m = case.model
    g = torch.Generator().manual_seed(6)
    init = (torch.randn(1, 2, HH // 8, WW // 8, generator=g),
            torch.randn(1, 2, HH // 8, WW // 8, generator=g))
    conv = Convergence(tol=1e9, every=2, min_iters=3)
    with torch.no_grad():
        res = m(case.x1, case.x2, iters=BUDGET, flow_init=init,
                bidirectional=True, return_low=True, converge=conv,
                return_info=True)
        ref = m(case.x1, case.x2, iters=5, flow_init=init,
                bidirectional=True, return_low=True)
        cold = m(case.x1, case.x2, iters=5, bidirectional=True)
    assert len(res) == 5 and len(ref) == 4
    fw, bw, low_fw, low_bw, info = res
    assert isinstance(info, ConvergenceInfo) and info.iters_run == 5
    assert fw.shape == (1, 2, HH, WW)
    assert low_fw.shape == (1, 2, HH // 8, WW // 8)
    for a, b in zip(res[:4], ref):
        assert torch.equal(a, b)
    assert not torch.equal(fw, cold[0])           # the seed is not a no-op
    # unidirectional: (up, low, info); without a gate info reports the count
    with torch.no_grad():
        up, low, info = m(case.x1, case.x2, iters=2, return_low=True,
                          return_info=True)
    assert info == ConvergenceInfo(iters_run=2, checks=[])
    assert torch.equal(up, case.ungated(2))
    assert low.shape == (1, 2, HH // 8, WW // 8)


def test_argument_errors(case):
    m = case.model
    conv = Convergence(tol=1.0)
    with pytest.raises(ValueError):
        m(case.x1, case.x2, iters=2, test_mode=False, converge=conv)
    with pytest.raises(ValueError):
        m(case.x1, case.x2, iters=2, test_mode=False, return_info=True)
    with pytest.raises(ValueError):
        m(case.x1, case.x2, iters=2, converge=0.5)


# ------------------------------------------------- engine, session, serving
def _frames(n):
    g = torch.Generator().manual_seed(7)
    return [torch.rand(1, 3, 40, 56, generator=g) for _ in range(n)]


@pytest.fixture(scope="module")
def engine():
    from raft_amd.engine import InferenceEngine
    torch.manual_seed(SEED)
    return InferenceEngine(RAFT(RaftConfig(small=True)), iters=6)


def test_engine_calls_carry_the_gate(engine):
    from raft_amd.engine.inference import run_mixed_batch
    a, b, c = _frames(3)
    conv = Convergence(tol=1e9, every=2, min_iters=3)
    out = engine(a, b, converge=conv)
    assert engine.last_info.iters_run == 5
    assert [k[0] for k in engine.last_info.checks] == [4]
    assert torch.equal(out, engine(a, b, iters=5))
    assert engine.last_info == ConvergenceInfo(iters_run=5)
    engine(a, b)
    assert engine.last_info.iters_run == 6
    bi = engine.bidirectional(a, b, converge=conv)
    assert engine.last_info.iters_run == 5
    ref = engine.bidirectional(a, b, iters=5)
    assert torch.equal(bi.flow_fw, ref.flow_fw)
    assert torch.equal(bi.occ_bw, ref.occ_bw)
    mid = engine.interpolate(a, b, times=(0.5,), converge=conv)
    assert engine.last_info.iters_run == 5
    assert torch.equal(mid, engine.interpolate(a, b, times=(0.5,), iters=5))
    # each shape group of a mixed batch is gated on its own
    small = torch.rand(1, 3, 32, 48)
    pairs = [(a, b), (small, small), (b, c)]
    flows, ran = run_mixed_batch(engine, pairs, converge=conv,
                                 return_iters=True)
    assert ran == [5, 5, 5]
    ref = run_mixed_batch(engine, pairs, iters=5)
    for f, r in zip(flows, ref):
        assert torch.equal(f, r)
    flows, ran = run_mixed_batch(engine, pairs, return_iters=True)
    assert ran == [6, 6, 6]


def test_session_reports_iterations(engine):
    frames = _frames(4)
    conv = Convergence(tol=1e9, every=2, min_iters=3)
    gated = engine.stream(warm=True, converge=conv)
    fixed = engine.stream(warm=True, iters=5)
    plain = engine.stream(warm=True)
    assert gated.push(frames[0]) is None and gated.last_iters is None
    fixed.push(frames[0])
    plain.push(frames[0])
    for x in frames[1:]:
        out = gated.push(x)
        assert gated.last_iters == 5
        assert [k[0] for k in gated.last_info.checks] == [4]
        assert torch.equal(out, fixed.push(x))
        assert fixed.last_iters == 5
        plain.push(x)
        assert plain.last_iters == 6 and plain.last_info.checks == []
    # a session without a gate is the session it has always been
    cold = engine.stream(warm=False)
    cold.push(frames[0])
    assert torch.equal(cold.push(frames[1]), engine(frames[0], frames[1]))
    gated.reset()
    assert gated.last_iters is None


def test_cli_flags():
    import infer_raft
    args = infer_raft.parse_args(["--tol", "0.5", "--check-every", "2",
                                  "--min-iters", "3"])
    assert args.converge == Convergence(tol=0.5, every=2, min_iters=3)
    assert infer_raft.parse_args([]).converge is None
    for bad in (["--tol", "-1"], ["--tol", "1", "--check-every", "0"],
                ["--tol", "1", "-m", "val"]):
        with pytest.raises(SystemExit):
            infer_raft.parse_args(bad)


def test_cli_prints_the_executed_count(tmp_path, capsys):
    import infer_raft
    from raft_amd.data.imageio import write_png
    rng = np.random.RandomState(0)
    for name in ("a.png", "b.png"):
        write_png(str(tmp_path / name),
                  (rng.rand(32, 48, 3) * 255).astype(np.uint8))
    infer_raft.main(["--small", "--iters", "6", "--size", "native",
                     "--im1", str(tmp_path / "a.png"),
                     "--im2", str(tmp_path / "b.png"),
                     "--out", str(tmp_path / "out"), "--tol", "1e9",
                     "--check-every", "2", "--min-iters", "3"])
    assert "5 iters" in capsys.readouterr().out


# ----------------------------------------------------------------- serving
@pytest.fixture(scope="module")
def client():
    pytest.importorskip("fastapi")      # the guard of tests/test_serving.py
    from starlette.testclient import TestClient

    from raft_amd.serving.server import create_app
    torch.manual_seed(SEED)
    return TestClient(create_app(RAFT(RaftConfig(small=True)).eval(),
                                 iters=6))


def _png(h=32, w=48, seed=0):
    from raft_amd.data.imageio import encode_png
    rng = np.random.RandomState(seed)
    return encode_png((rng.rand(h, w, 3) * 255).astype(np.uint8))


def _body(b1, b2):
    import struct
    return struct.pack("<I", len(b1)) + b1 + b2


def _hist_count(client):
    for line in client.get("/metrics").text.splitlines():
        if line.startswith("raft_iters_run_count"):
            return float(line.split()[-1])
    raise AssertionError("raft_iters_run histogram missing")


def test_serving_reports_iterations(client):
    import struct
    body = _body(_png(seed=1), _png(seed=2))
    before = _hist_count(client)
    r = client.post("/flow", content=body)
    assert r.status_code == 200 and r.headers["X-Raft-Iters"] == "6"
    plain = r.content
    r = client.post("/flow?tol=1e9&check_every=2&min_iters=3", content=body)
    assert r.status_code == 200 and r.headers["X-Raft-Iters"] == "5"
    gated = r.content
    r = client.post("/flow?iters=5", content=body)
    assert r.headers["X-Raft-Iters"] == "5" and r.content == gated
    assert gated != plain
    assert _hist_count(client) == before + 3
    # batch: one value per pair, input order, each shape group on its own
    p1, p2, q = _png(seed=3), _png(seed=4), _png(24, 40, seed=5)
    batch = struct.pack("<I", 3)
    for a, b in ((p1, p2), (q, q), (p2, p1)):
        batch += struct.pack("<I", len(a)) + a + struct.pack("<I", len(b)) + b
    r = client.post("/flow_batch?tol=1e9&check_every=1", content=batch)
    assert r.status_code == 200 and r.headers["X-Raft-Iters"] == "2,2,2"
    r = client.post("/flow_batch", content=batch)
    assert r.headers["X-Raft-Iters"] == "6,6,6"
    assert _hist_count(client) == before + 9


def test_serving_rejects_bad_gate_values(client):
    body = _body(_png(seed=1), _png(seed=2))
    for q in ("tol=-1", "tol=1&check_every=0", "tol=1&min_iters=0",
              "check_every=2"):
        assert client.post(f"/flow?{q}", content=body).status_code == 400, q
        r = client.post(f"/flow_batch?{q}", content=b"\x00\x00\x00\x00")
        assert r.status_code == 400, q
