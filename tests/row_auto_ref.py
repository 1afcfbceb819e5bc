"""Fixtures and an fp64 reference for the kernel tests of solve_dtype="auto" (csrc/row_solve.hip: row_needs_f64,
the redo list; csrc/row_solve_f64.hip: k_row_redo_f64).  numpy only: tests/test_row_auto_ref_cpu.py validates it
without a device, tests/test_gpu_row_auto.py holds the kernels to it.

The estimate restated here is the DOCUMENTED one: lower bounds of cond_2(A) from the Cholesky pivots of the real
system (the k real columns of the primal form, the `len` real ratings of the dual form) - the padding of the kernels'
16-wide blocks is not part of A and has no say in it.

Every fixture row that is meant to sit at a given estimate gets its regulariser by bisection (`lam_for_target`), so
the expected partition at the limits 30 / 300 / 3e4 does not hang on a seed: the targets 6, 100, 2000 and 2e5 keep
a factor 2 and more from each limit.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from collaborative_filtering_amd import layout

LIMITS = (30.0, 300.0, 3e4)
KS = (16, 50, 64, 80, 128, 150)
NCOLS = 9000            # the catalogue: a split row of 8200 + k ratings needs that many distinct items
NPOOL = 4300            # its low-rank pool (items 0 ... NPOOL - 1): a split pool row needs more than 4096 of them
MU, LAM_B = 3.3, 1.7
STAT_RATIO = 1e-3       # row_solve.hip, finish_row: sum d^2 < 1e-3 sum (rho - b)^2 sends the row to fp64
EPS = 1e-10


def lam_of(lam_row, diag_extra=0.0) -> float:
    """The regulariser as the kernels form it: float32 inputs, + 1e-10."""
    return float(np.float32(lam_row)) + EPS + float(np.float32(diag_extra))


def is_dual(k: int, nnz: int, gram: str = "f16x2") -> bool:
    """Rows the engine's task list hands to the dual-form kernels (plain solve, f16x2 Gram)."""
    if gram != "f16x2" or nnz < 1:
        return False
    return nnz <= layout.dual_max_len(k) or nnz <= layout.dual_mid_len(k)


def system_matrix(Fr: np.ndarray, lam: float, k: int, dual: bool) -> np.ndarray:
    """A in the order the kernels eliminate it: primal F^T F + lam I over the k real columns in perm order, dual
    F F^T + lam I over the ratings in storage order.  float64."""
    Fr = np.asarray(Fr, dtype=np.float64)[:, :k]
    if dual:
        return Fr @ Fr.T + lam * np.eye(Fr.shape[0])
    order = np.argsort(layout.perm_of_col(k)[:k])
    Fp = Fr[:, order]
    return Fp.T @ Fp + lam * np.eye(k)


def estimate(Fr: np.ndarray, lam: float, k: int, nnz: int, dual: bool = False, dtype=np.float64) -> dict:
    """{"pivot", "mean", "short", "est"} of one row.  `dtype=np.float32`: the same with the matrix rounded to float32
    and a float32 Cholesky (a breakdown gives inf, as the kernel's spd == false branch does)."""
    A = system_matrix(Fr, lam, k, dual)
    trace = float(np.trace(A) - lam * A.shape[0])
    mean_eig = trace / max(min(k, nnz), 1) + lam
    try:
        with np.errstate(all="ignore"):
            d = np.diag(np.linalg.cholesky(A.astype(dtype))).astype(np.float64)
        if not (np.all(np.isfinite(d)) and np.all(d > 0)):
            raise np.linalg.LinAlgError
    except np.linalg.LinAlgError:
        return {"pivot": np.inf, "mean": np.inf, "short": np.inf, "est": np.inf}
    pivot = float((d.max() / d.min()) ** 2)
    mean = float(mean_eig / d.min() ** 2)
    short = float(mean_eig / lam) if (dual or nnz < 4 * k) else 0.0
    return {"pivot": pivot, "mean": mean, "short": short, "est": max(pivot, mean, short)}


def cond2(Fr: np.ndarray, lam: float, k: int, dual: bool = False) -> float:
    w = np.linalg.eigvalsh(system_matrix(Fr, lam, k, dual))
    return float(w[-1] / w[0])


def lam_for_target(Fr: np.ndarray, k: int, nnz: int, dual: bool, target: float) -> np.float32:
    """float32 lambda_row at which the row's estimate is `target` (the estimate falls as lambda grows)."""
    lo, hi = np.log(1e-9), np.log(1e6)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if estimate(Fr, lam_of(np.exp(mid)), k, nnz, dual)["est"] > target:
            lo = mid
        else:
            hi = mid
    return np.float32(np.exp(0.5 * (lo + hi)))


@dataclass
class Batch:
    k: int
    side: layout.SparseSide
    F: np.ndarray               # float32 [NCOLS + 1, ld], the zero row last
    b_self: np.ndarray          # float32 [nrows]
    b_other: np.ndarray         # float32 [NCOLS]
    lam_row: np.ndarray         # float32 [nrows]
    classes: List[str]
    mu: float = MU
    lam_b: float = LAM_B
    _ref: dict = field(default_factory=dict)

    @property
    def nrows(self) -> int:
        return self.side.nrows

    def lens(self) -> np.ndarray:
        return np.diff(self.side.indptr)

    def row(self, r: int):
        lo, hi = self.side.indptr[r], self.side.indptr[r + 1]
        idx = self.side.indices[lo:hi]
        return idx, self.F[idx, : self.k].astype(np.float64), self.side.vals[lo:hi].astype(np.float64)

    def reference(self, gram: str = "f16x2") -> List[Optional[dict]]:
        """Per row (None for empty rows): est / pivot / mean / short, cond2, x, bias, sd, sd2, s2 (= sum (rho - b_new)^2),
        rhs / colsum (perm space, padded), sumr / sumr2 (sums of rho and rho^2: the old bias is not in them), L (fp64
        Cholesky of the padded primal A, perm space), dual.
        Computed once per Gram mode (the dual classes exist with the f16x2 Gram only) and left unchanged."""
        if gram not in self._ref:
            self._ref[gram] = [row_reference(self, r, gram) for r in range(self.nrows)]
        return self._ref[gram]

    def flagged(self, limit: float, gram: str = "f16x2", stats: bool = False) -> set:
        """Rows the auto path must hand to fp64: estimate above the limit, or - primal rows of a call with stat_out -
        closed-form statistics that cancel."""
        out = set()
        for r, ref in enumerate(self.reference(gram)):
            if ref is None:
                continue
            if ref["est"] > limit or (stats and not ref["dual"] and ref["sd2"] < STAT_RATIO * ref["s2"]):
                out.add(r)
        return out

    def stat_ambiguous(self, gram: str = "f16x2") -> set:
        """Primal rows whose sum d^2 / sum (rho - b)^2 lies within a factor 4 of the statistics threshold: with
        stat_out they may land on either side (the kernel forms the ratio from fp32 sums and its fp32 x), so the tests
        that pass stat_out leave them out of the expected partition.  Without stat_out the partition is exact."""
        return {r for r, ref in enumerate(self.reference(gram)) if ref is not None and not ref["dual"]
                and STAT_RATIO / 4 <= ref["sd2"] / ref["s2"] <= STAT_RATIO * 4}


def row_reference(b: Batch, r: int, gram: str, bias_self: Optional[np.ndarray] = None) -> Optional[dict]:
    k = b.k
    idx, Fr, vals = b.row(r)
    nnz = idx.size
    if nnz == 0:
        return None
    ld = layout.padded_k(k)
    pos = layout.perm_of_col(k)[:k]
    dual = is_dual(k, nnz, gram)
    lam = lam_of(b.lam_row[r])
    bs = float((b.b_self if bias_self is None else bias_self)[r])
    out = estimate(Fr, lam, k, nnz, dual)
    out["dual"] = dual
    out["cond2"] = cond2(Fr, lam, k, dual)
    rho = vals - b.mu - b.b_other[idx].astype(np.float64)
    A = Fr.T @ Fr + lam * np.eye(k)
    rhs = Fr.T @ (rho - bs)
    x = np.linalg.solve(A, rhs)
    x = x + np.linalg.solve(A, rhs - A @ x)                  # one step of refinement: residual at rounding level
    bias = np.sum(rho - Fr @ x) / (nnz + b.lam_b + EPS)
    d = rho - Fr @ x - bias
    out.update(x=x, bias=bias, sd=float(d.sum()), sd2=float((d * d).sum()), s2=float(((rho - bias) ** 2).sum()),
               rho_abs=float(np.abs(rho).sum()), rho2=float((rho * rho).sum()), A=A, b=rhs)
    rhs_p, cs_p = np.zeros(ld), np.zeros(ld)
    rhs_p[pos], cs_p[pos] = rhs, Fr.sum(axis=0)
    Ap = np.eye(ld)
    Ap[np.ix_(pos, pos)] = A
    out.update(rhs=rhs_p, colsum=cs_p, sumr=float(rho.sum()), sumr2=float((rho * rho).sum()),
               L=np.linalg.cholesky(Ap))
    return out


def _ratings(rng, n):
    return (np.round(rng.uniform(0.5, 5.0, size=n) * 2) / 2).astype(np.float32)          # as _random_side: 0.5 ... 5


def make_factors(k: int, rng) -> np.ndarray:
    """[NCOLS + 1, ld] float32: items < NPOOL are the low-rank pool (B C of rank ~ k / 4 plus 1e-3 noise, entries of
    twice the size of the generic ones: N(0, 0.6^2)), the rest N(0, 0.3^2); padded columns and the last row are zero."""
    ld = layout.padded_k(k)
    r = max(k // 4, 1)
    F = np.zeros((NCOLS + 1, ld), dtype=np.float32)
    pool = rng.normal(size=(NPOOL, r)) @ rng.normal(scale=0.6 / np.sqrt(r), size=(r, k))
    F[:NPOOL, :k] = pool + 1e-3 * rng.normal(size=(NPOOL, k))
    F[NPOOL:NCOLS, :k] = rng.normal(scale=0.3, size=(NCOLS - NPOOL, k))
    return F


def row_specs(k: int) -> list:
    """(class, ratings, "gen" | "pool", lambda_row | ("target", estimate) | ("as", class of the row to copy))."""
    T = lambda t: ("target", float(t))                                                     # noqa: E731
    specs = [
        ("empty_a", 0, "gen", 1.0),
        ("one_lo", 1, "gen", T(6)),
        ("one_hi", 1, "gen", T(2000)),
        ("lt_k_lo", k // 2 + 1, "gen", T(6)),
        ("lt_k_mid", k - 1, "gen", T(100)),
        ("empty_b", 0, "gen", 1.0),
        ("lt_k_hi", k - 1, "gen", T(2e5)),
        ("eq_k_lo", k, "gen", T(6)),
        ("eq_k_hi", k, "gen", T(2000)),
        ("short_mid", 2 * k + 3, "gen", T(100)),
        ("short_last", 4 * k - 1, "gen", T(2000)),            # the short-row bound alone flags it ...
        ("long_first", 4 * k, "gen", ("as", "short_last")),   # ... and is off from 4 k ratings on: same lambda, not flagged
        ("long_second", 4 * k + 1, "gen", ("as", "short_last")),
        ("long_first_pool", 4 * k, "pool", T(2000)),
        ("n700", 700, "gen", 2.0),
        ("n700_pool", 700, "pool", T(2000)),
        ("split_4097", 4097, "gen", 1.0),
        ("split_8200", 8200 + k, "gen", 0.7),
        ("pool_1e-3", 3000, "pool", 1e-3),                # flagged by the pivot terms alone
        ("split_pool_hi", 4097 + 40, "pool", 1e-3),           # a flagged row that k_row_long finishes
        ("split_pool_mid", 4100, "pool", T(100)),
        ("breakdown", k - 2, "gen", 1e-6),                    # the fp32 factorisation may break down: spd == false
    ]
    if k > 64:          # the dual form (rows of at most 64 ratings)
        specs += [(f"dual_{n}", n, "gen", T(t)) for n, t in ((15, 6), (16, 2000), (17, 2e5), (48, 6), (49, 2e5), (64, 2000))]
    if k > 96:          # the dual mid form (65 ... 96 ratings)
        specs += [(f"mid_{n}", n, "gen", T(t)) for n, t in ((65, 6), (80, 2000), (81, 100), (96, 2e5))]
    return specs


_BATCHES: dict = {}
# seed 0 puts the 4 k-rating row of k = 16 at an estimate of 16, inside the guard band of the limit 30
# (tests/test_row_auto_ref_cpu.py): another seed there, not a narrower band
DEFAULT_SEED = {16: 1}


def make_batch(k: int, seed: Optional[int] = None) -> Batch:
    """The fixture batch of rank k (cached: the GPU tests share one instance and its references per k)."""
    seed = DEFAULT_SEED.get(k, 0) if seed is None else seed
    if (k, seed) in _BATCHES:
        return _BATCHES[(k, seed)]
    rng = np.random.default_rng(7000 + 13 * k + seed)
    F = make_factors(k, rng)
    specs = row_specs(k)
    nrows = len(specs)
    indptr = np.zeros(nrows + 1, dtype=np.int64)
    indptr[1:] = np.cumsum([s[1] for s in specs])
    parts = []
    for _, n, src, _ in specs:
        cand = np.arange(NPOOL) if src == "pool" else np.arange(NCOLS)
        parts.append(np.sort(rng.choice(cand, size=n, replace=False)))
    indices = np.concatenate(parts).astype(np.int32)
    side = layout.SparseSide(nrows, NCOLS, indptr, indices, _ratings(rng, indices.size))
    lam_row = np.ones(nrows, dtype=np.float32)
    by_class = {}
    for r, (name, n, _, lam) in enumerate(specs):
        if isinstance(lam, tuple) and lam[0] == "target":
            Fr = F[indices[indptr[r]:indptr[r + 1]], :k].astype(np.float64)
            lam_row[r] = lam_for_target(Fr, k, n, is_dual(k, n), lam[1])
        elif isinstance(lam, tuple):
            lam_row[r] = lam_row[by_class[lam[1]]]
        else:
            lam_row[r] = np.float32(lam)
        by_class[name] = r
    b = Batch(k=k, side=side, F=F, b_self=rng.normal(scale=0.2, size=nrows).astype(np.float32),
              b_other=rng.normal(scale=0.2, size=NCOLS).astype(np.float32), lam_row=lam_row,
              classes=[s[0] for s in specs])
    _BATCHES[(k, seed)] = b
    return b


def make_overfit_rows(k: int, seed: int = 0) -> Batch:
    """Rows the STATISTICS must flag while the estimate stays small: ~1000 generic items each, ratings that the model
    explains to 1e-3 (vals = mu + b_other + F x0 + b0 + 1e-3 noise), lambda = 0.5 - well conditioned, and the
    residuals are a 1e-5 fraction of the signal, where the fp32 closed form has cancelled."""
    key = ("overfit", k, seed)
    if key in _BATCHES:
        return _BATCHES[key]
    rng = np.random.default_rng(8000 + 13 * k + seed)
    F = make_factors(k, rng)
    lens = [1000, 997, 0, 1003]
    nrows = len(lens)
    indptr = np.zeros(nrows + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = np.concatenate([np.sort(rng.choice(np.arange(NPOOL, NCOLS), size=n, replace=False)) for n in lens]).astype(np.int32)
    b_other = rng.normal(scale=0.2, size=NCOLS).astype(np.float32)
    vals = np.zeros(indices.size, dtype=np.float32)
    b_self = np.zeros(nrows, dtype=np.float32)
    for r in range(nrows):
        sl = slice(indptr[r], indptr[r + 1])
        x0 = rng.normal(scale=1.0 / (0.3 * np.sqrt(k)), size=k)
        b0 = b_self[r] = np.float32(rng.normal(scale=0.2))       # the old bias is the one the ratings were made with
        Fr = F[indices[sl], :k].astype(np.float64)
        vals[sl] = (MU + b_other[indices[sl]] + Fr @ x0 + b0 + 1e-3 * rng.normal(size=Fr.shape[0])).astype(np.float32)
    b = Batch(k=k, side=layout.SparseSide(nrows, NCOLS, indptr, indices, vals), F=F,
              b_self=b_self, b_other=b_other,
              lam_row=np.full(nrows, 0.5, dtype=np.float32), classes=["overfit", "overfit", "empty", "overfit"])
    _BATCHES[key] = b
    return b
