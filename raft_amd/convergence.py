"""Convergence-gated refinement: the rule that lets the GRU loop stop when
its own update has settled.

Iterations are numbered 1..N (N = the ``iters`` budget). After iteration i
a check is taken when ``i % every == 0``, ``i >= min_iters`` and ``i < N``;
it measures the coords update of iteration i (ops.flow_residual). The loop
batch has converged when every sample has at most ``floor(frac * cells)``
cells whose update exceeds ``tol`` — with ``frac=0``: when the largest
update of every sample is within ``tol``. The loop then runs exactly one
more iteration, the final one, and stops: n = i + 1. A gated call that ran
n iterations therefore executes the kernel sequence of an ungated call with
``iters=n`` and returns the same bits.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np


@dataclass(frozen=True)
class Convergence:
    """tol: update magnitude in full-resolution pixels below which a cell
    counts as settled; None = trace-only (every check is evaluated and
    recorded, the loop never stops early). every: check period in
    iterations. min_iters: first iteration a check may follow. frac: share
    of cells per sample that may still move more than tol."""
    tol: Optional[float]
    every: int = 4
    min_iters: int = 1
    frac: float = 0.0

    def __post_init__(self):
        if self.tol is not None and not float(self.tol) >= 0.0:
            raise ValueError(f"tol must be >= 0 or None, got {self.tol}")
        if int(self.every) != self.every or self.every < 1:
            raise ValueError(f"every must be an integer >= 1, got "
                             f"{self.every}")
        if int(self.min_iters) != self.min_iters or self.min_iters < 1:
            raise ValueError(f"min_iters must be an integer >= 1, got "
                             f"{self.min_iters}")
        if not 0.0 <= float(self.frac) < 1.0:
            raise ValueError(f"frac must lie in [0, 1), got {self.frac}")

    @property
    def thr_sq(self) -> float:
        """Squared threshold on the 1/8 grid, computed in fp32:
        (float32(tol) / 8)^2. Trace-only mode compares against +inf, so
        only NaN cells count as above."""
        if self.tol is None:
            return math.inf
        with np.errstate(over="ignore"):
            t = np.float32(self.tol) / np.float32(8)
            return float(np.float32(t * t))

    def checks_after(self, i: int, budget: int) -> bool:
        return i % self.every == 0 and i >= self.min_iters and i < budget


@dataclass
class ConvergenceInfo:
    """iters_run: iterations executed, the final one included. checks: one
    ``(iteration, max_px, frac_above)`` per check taken — max_px the
    largest update of that iteration in full-resolution pixels,
    8 * sqrt(max over samples of max_sq); frac_above the largest per-sample
    share of cells above the threshold."""
    iters_run: int = 0
    checks: List[Tuple[int, float, float]] = field(default_factory=list)


class Gate:
    """Host side of one gated loop: which iterations are checked, what a
    check's result means, and the ConvergenceInfo it leaves behind."""

    def __init__(self, conv: Convergence, budget: int, cells: int):
        self.conv = conv
        self.budget = budget
        self.cells = cells
        self.thr_sq = conv.thr_sq
        self.allowed = int(math.floor(float(conv.frac) * cells))
        self.info = ConvergenceInfo()

    def wants(self, i: int) -> bool:
        return self.conv.checks_after(i, self.budget)

    def record(self, i: int, max_sq, above) -> bool:
        """max_sq [B] fp32 and above [B] integers (array-likes on the
        host) of iteration i. Returns True when the loop has converged."""
        max_sq = np.asarray(max_sq, dtype=np.float32).reshape(-1)
        above = np.asarray(above).reshape(-1)
        if np.isnan(max_sq).any():
            max_px = math.nan
        else:
            max_px = 8.0 * math.sqrt(float(max_sq.max()))
        self.info.checks.append(
            (i, max_px, float(above.max()) / max(self.cells, 1)))
        return self.conv.tol is not None and \
            bool((above <= self.allowed).all())

    def record_raw(self, i: int, raw) -> bool:
        """raw: the [B,2] int32 result of ops.flow_residual_raw, on the
        host."""
        raw = np.ascontiguousarray(np.asarray(raw, dtype=np.int32))
        return self.record(i, raw[:, 0].copy().view(np.float32), raw[:, 1])
