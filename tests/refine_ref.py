"""numpy restatement of solve_dtype="refine" (csrc/row_solve.hip: k_row_refine, refine_row) on
the rows of a `row_auto_ref.Batch`: the fp32 factor of the row's primal system, the first solve in fp32, steps of
iterative refinement with the residual F^T (rho - F x) - lambda x in fp64 from the ratings and the correction from the
fp32 factor, and the kernel's stopping rule.  tests/test_refine_ref_cpu.py pins what it does on the fixtures without a
device; tests/test_gpu_row_refine.py holds the kernel to the same conditions.

It is a restatement of the arithmetic, not of the kernel's summation order: the fp32 Gram is numpy's float32 product
(for the f16x2 Gram with an extra relative perturbation of 2^-21 for the operand split), the factor numpy's float32
Cholesky, the substitutions float32 row by row."""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from tests import row_auto_ref as R

MAX_STEPS = 5
ACCEPT = 2.0 ** -29            # predicted remaining error / |x|
CONTRACT = 0.25                # a step must shrink the correction at least this much
SPLIT_CHUNK = 4096


def decide(t: int, dn: float, dprev: float, xn: float, max_steps: int = MAX_STEPS) -> str:
    """The rule after step t (1-based): dn = |d_t|, dprev = |d_t-1| (unused at t = 1), xn = |x| after the update, all
    max norms.  "accept", "give_up" or "continue" - in the kernel's order."""
    if not (np.isfinite(dn) and np.isfinite(xn)):
        return "give_up"
    pred = dn if t == 1 else dn * dn / dprev
    if pred <= ACCEPT * xn:
        return "accept"
    if t > 1 and dn > CONTRACT * dprev:
        return "give_up"
    if t >= max_steps:
        return "give_up"
    return "continue"


def run_rule(dnorms, xnorm: float = 1.0, max_steps: int = MAX_STEPS):
    """The rule on a given sequence |d_1|, |d_2|, ...: (accepted, steps taken)."""
    dprev = 0.0
    for t, dn in enumerate(dnorms, start=1):
        what = decide(t, float(dn), dprev, xnorm, max_steps)
        if what != "continue":
            return what == "accept", t
        dprev = float(dn)
    raise ValueError("the sequence ended before the rule decided")


def _solve32(L: np.ndarray, b: np.ndarray) -> np.ndarray:
    """(L L^T)^-1 b, float32 throughout."""
    k = L.shape[0]
    y = np.zeros(k, dtype=np.float32)
    for i in range(k):
        y[i] = (b[i] - np.dot(L[i, :i], y[:i])) / L[i, i]
    x = np.zeros(k, dtype=np.float32)
    for i in range(k - 1, -1, -1):
        x[i] = (y[i] - np.dot(L[i + 1:, i], x[i + 1:])) / L[i, i]
    return x


def refine_row(b: R.Batch, r: int, gram: str = "f32", max_steps: int = MAX_STEPS, seed: int = 0) -> Optional[dict]:
    """None for an empty row, else {"accepted", "steps", "why"} and - accepted rows - x, bias, sd, sd2."""
    k = b.k
    idx, Fr, vals = b.row(r)
    n = idx.size
    if n == 0:
        return None
    if n > SPLIT_CHUNK:
        return {"accepted": False, "steps": 0, "why": "split"}
    lam = R.lam_of(b.lam_row[r])
    rho_b = vals - b.mu - b.b_other[idx].astype(np.float64)          # without the row's own bias
    rho = rho_b - float(b.b_self[r])                                 # the OLD bias, throughout
    F32 = Fr.astype(np.float32)
    G = (F32.T @ F32).astype(np.float64)
    if gram == "f16x2":
        rng = np.random.default_rng(9000 + 131 * k + r + seed)
        G = G * (1.0 + 2.0 ** -21 * rng.uniform(-1, 1, size=G.shape))
        G = 0.5 * (G + G.T)
    A32 = (G + (float(np.float32(b.lam_row[r])) + 1e-10) * np.eye(k)).astype(np.float32)
    try:
        with np.errstate(all="ignore"):
            L = np.linalg.cholesky(A32)
        if not (np.all(np.isfinite(L)) and np.all(np.diag(L) > 0)):
            raise np.linalg.LinAlgError
    except np.linalg.LinAlgError:
        return {"accepted": False, "steps": 0, "why": "breakdown"}
    with np.errstate(all="ignore"):
        x = _solve32(L, (F32.T @ rho.astype(np.float32)).astype(np.float32)).astype(np.float64)
        dprev, steps, why = 0.0, 0, "give_up"
        for t in range(1, max_steps + 1):
            res = Fr.T @ (rho - Fr @ x) - lam * x
            rm = float(np.max(np.abs(res)))
            if not np.isfinite(rm):
                break
            e = int(np.floor(np.log2(rm))) if rm > 0 else 0
            d = np.ldexp(_solve32(L, np.ldexp(res, -e).astype(np.float32)).astype(np.float64), e)
            x = x + d
            steps = t
            dn, xn = float(np.max(np.abs(d))), float(np.max(np.abs(x)))
            what = decide(t, dn, dprev, xn, max_steps)
            if what != "continue":
                why = what
                break
            dprev = dn
    if why != "accept":
        return {"accepted": False, "steps": steps, "why": why}
    e_j = rho_b - Fr @ x
    se, se2 = float(e_j.sum()), float((e_j * e_j).sum())
    bias = se / (n + b.lam_b + R.EPS)
    return {"accepted": True, "steps": steps, "why": why, "x": x, "bias": bias, "sd": se - n * bias,
            "sd2": se2 - 2.0 * bias * se + n * bias * bias}


def refine_batch(b: R.Batch, gram: str = "f32", max_steps: int = MAX_STEPS) -> List[Optional[dict]]:
    return [refine_row(b, r, gram, max_steps) for r in range(b.nrows)]
