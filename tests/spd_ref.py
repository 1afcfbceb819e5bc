"""Systems, references and the shared checker of the dense fp64 Cholesky solve (als_spd_solve_f64, spd_solve.hip).
numpy only.  tests/test_gpu_spd_solve.py holds the device kernel to `check_case`, tests/test_spd_ref_cpu.py holds
LAPACK, a numpy emulation of the kernel's blocked order and the CPU stand-in to the same assertions - so every cap
below is shown to be reachable by a correct solver before a device is asked to meet it.

The caps are relative to LAPACK (np.linalg.solve) on the same systems, never to the device's own output:
  backward error  |A x - b|_2 / (|A|_F |x|_2 + |b|_2)      <= BE_FACTOR x the largest LAPACK has at the same N
  forward error   |x - x_ld|_2 / |x_ld|_2 / (eps cond_2 A)  <= FE_FACTOR x the largest LAPACK has at the same N
The family maximum is used because a single system can give LAPACK an error of exactly 0.  4: the emulation of the
kernel's order (`blocked_cholesky_solve`, multipliers formed with y^2 for 1 / p as the kernel does) stays within
1.3x of LAPACK's family maximum from N = 63 on and reaches 2.4x at N = 1 and 3.1x on one system of order 7 (0.42 eps
against 0.13 eps), where a handful of roundings are the whole error; the rest is room for FMA contraction and the
deferred update order.  8: forward errors of two backward-stable solvers scatter more - the emulation reaches 2.4x.
What the caps catch (test_spd_ref_cpu.py): a reciprocal square root that is good to 44 bits instead of 53 is at 20x
and more on any system of a few tiles; one that is good to 50 bits stays below 2x - the caps cannot tell the last two
bits of the Newton iteration, and no cap that LAPACK itself meets with a margin could."""
from __future__ import annotations

import functools
from typing import NamedTuple, Optional

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "tests/spd_ref.py needs an extended-precision long double"
EPS = float(np.finfo(np.float64).eps)
NB = 64                     # panel width of spd_solve.hip
BE_FACTOR = 4.0
FE_FACTOR = 8.0
W_EPS = 1e-10               # what the engine adds to lambda_w (engine.py)


# ------------------------------------------------------------------------------------------------------ generators
def q_system(N, logc, seed):
    """A = Q diag(lam) Q^T, lam log-uniform in [10^-logc, 1] with both ends present (N = 1: 10^-logc); b normal."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
    lam = 10.0 ** (-logc * rng.uniform(size=N))
    lam[-1] = 1.0
    lam[0] = 10.0 ** -logc
    A = (Q * lam) @ Q.T
    return 0.5 * (A + A.T), rng.normal(size=N)


def kron_system(d, k, nitems, seed):
    """The W-step's own shape: A = sum_i (x_i x_i^T) (x) (U_i^T U_i), b = sum_i x_i (x) (U_i^T r_i); x_i sparse binary,
    L2-normalised, U_i 1 to 5 rows of N(0, 0.3^2).  nitems is small enough for rank(A) < d k: it is solved with
    diag_add = W_EPS, as the engine does at lambda_w = 0."""
    rng = np.random.default_rng(seed)
    A = np.zeros((d * k, d * k))
    b = np.zeros(d * k)
    rows = 0
    for _ in range(nitems):
        x = np.zeros(d)
        x[rng.choice(d, size=rng.integers(1, min(d, 3) + 1), replace=False)] = 1.0
        x /= np.linalg.norm(x)
        U = rng.normal(scale=0.3, size=(rng.integers(1, 6), k))
        rows += U.shape[0]
        A += np.kron(np.outer(x, x), U.T @ U)
        b += np.kron(x, U.T @ rng.normal(size=U.shape[0]))
    assert rows < d * k
    return 0.5 * (A + A.T), b


class Woodbury(NamedTuple):
    A: np.ndarray
    b: np.ndarray
    dg: np.ndarray
    W: np.ndarray


def woodbury_system(N, r=8, seed=0, matrix=True):
    """A = diag(dg) + W W^T with dg in [1, 2) on a 2^-20 grid and W in {-1, -3/4, ..., 1}: every entry of A is exact
    in fp64, so the closed form solves the very matrix the solvers get.  cond_2(A) <= 2 + |W|_2^2.  matrix=False leaves
    A out (None): the closed form needs dg, W and b only."""
    rng = np.random.default_rng(seed)
    dg = 1.0 + rng.integers(0, 1 << 20, size=N) / float(1 << 20)
    W = rng.integers(-4, 5, size=(N, r)) / 4.0
    A = None
    if matrix:
        A = W @ W.T
        A[np.arange(N), np.arange(N)] += dg
    return Woodbury(A, rng.normal(size=N), dg, W)


def indefinite_system(N, q_list, seed):
    """L diag(s) L^T, L the Cholesky factor of a q_system(N, 4) matrix, s = -1 at q_list and +1 elsewhere: the leading
    minors change sign exactly at min(q_list)."""
    A0, b = q_system(N, 4, seed)
    L = np.linalg.cholesky(A0)
    s = np.ones(N)
    s[list(q_list)] = -1.0
    A = (L * s) @ L.T
    return 0.5 * (A + A.T), b


# ------------------------------------------------------------------------------------------------------ references
def solve_ld(A, b, diag_add=0.0):
    """(A + diag_add I)^-1 b by a column-oriented Cholesky factorisation and two substitutions in long double."""
    N = A.shape[0]
    L = np.tril(np.asarray(A, dtype=LD))
    L[np.arange(N), np.arange(N)] += LD(diag_add)
    for j in range(N):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        assert L[j, j] > 0, f"solve_ld: pivot {j} is not positive"
        L[j:, j] /= np.sqrt(L[j, j])
    y = np.asarray(b, dtype=LD).copy()
    for j in range(N):
        y[j] = (y[j] - L[j, :j] @ y[:j]) / L[j, j]
    for j in range(N - 1, -1, -1):
        y[j] = (y[j] - L[j + 1:, j] @ y[j + 1:]) / L[j, j]
    return y


def woodbury_solve_ld(dg, W, b):
    """(diag(dg) + W W^T)^-1 b = D^-1 b - D^-1 W (I + W^T D^-1 W)^-1 W^T D^-1 b in long double, O(N r^2)."""
    dg, W, b = (np.asarray(a, dtype=LD) for a in (dg, W, b))
    Db, DW = b / dg, W / dg[:, None]
    S = np.eye(W.shape[1], dtype=LD) + W.T @ DW
    return Db - DW @ solve_ld(S, W.T @ Db)


def pivots(A):
    """Plain fp64 column-oriented Cholesky -> (first index whose pivot is not > 0 (NaN counts) or None, the pivots
    up to and including it)."""
    N = A.shape[0]
    L = np.tril(np.asarray(A, dtype=np.float64))
    p = np.zeros(N)
    with np.errstate(invalid="ignore"):
        for j in range(N):
            if j:
                L[j:, j] -= L[j:, :j] @ L[j, :j]
            p[j] = L[j, j]
            if not p[j] > 0:
                return j, p[: j + 1]
            L[j:, j] /= np.sqrt(p[j])
    return None, p


def first_bad_pivot(A) -> Optional[int]:
    return pivots(A)[0]


def backward_error(A, x, b, diag_add=0.0, block=512):
    """|(A + diag_add I) x - b|_2 / (|A + diag_add I|_F |x|_2 + |b|_2); the residual in long double, row block by row
    block (no long-double copy of a large matrix)."""
    N = A.shape[0]
    xl, bl = np.asarray(x, dtype=LD), np.asarray(b, dtype=LD)
    if not np.isfinite(np.asarray(x, dtype=np.float64)).all():
        return float("inf")
    r2, a2 = LD(0), LD(0)
    for lo in range(0, N, block):
        Ab = np.asarray(A[lo: lo + block], dtype=LD)
        i = np.arange(Ab.shape[0])
        Ab[i, lo + i] += LD(diag_add)
        r = Ab @ xl - bl[lo: lo + block]
        r2 += r @ r
        a2 += np.sum(Ab * Ab)
    return float(np.sqrt(r2) / (np.sqrt(a2) * np.sqrt(xl @ xl) + np.sqrt(bl @ bl)))


def forward_error(x, x_ref):
    x, x_ref = np.asarray(x, dtype=LD), np.asarray(x_ref, dtype=LD)
    if not np.isfinite(np.asarray(x, dtype=np.float64)).all():
        return float("inf")
    d = x - x_ref
    return float(np.sqrt(d @ d) / np.sqrt(x_ref @ x_ref))


def blocked_cholesky_solve(A, b, diag_add=0.0, nb=NB, rsq_rel_error=0.0):
    """Right-looking fp64 Cholesky solve in the block order of spd_solve.hip -> (x, status): the matrix padded to a
    multiple of nb by an identity tail and augmented by the row b^T; per panel the diagonal block and everything
    below it are eliminated column by column (y = 1 / sqrt p: multipliers -a y^2 with the row multipliers taken from
    the same column, final entries a y), then the trailing matrix takes C -= L L^T; the back-substitution walks the
    panels backwards.  status as the kernel's: first bad pivot + 1, the pivot replaced by 1.  rsq_rel_error spoils
    every 1 / sqrt p by that relative error (the checker's own test).  Not a second implementation to test against:
    it shows that a correct solver of this shape meets the caps."""
    N = A.shape[0]
    T = (N + nb - 1) // nb
    NP = T * nb
    M = np.zeros((NP + 1, NP))
    M[:N, :N] = A
    M[np.arange(N), np.arange(N)] += diag_add
    M[np.arange(N, NP), np.arange(N, NP)] = 1.0
    M[NP, :N] = b
    status = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(T):
            c0 = j * nb
            P = M[c0:, c0: c0 + nb]                       # view: the stacked panel [D; X; y^T]
            for t in range(nb):
                p = P[t, t]
                if not p > 0:
                    status = status or c0 + t + 1
                    p = 1.0
                y = (1.0 / np.sqrt(p)) * (1.0 + rsq_rel_error)
                col = P[:, t].copy()                      # rows t + 1 .. nb - 1 of it are the row multipliers too
                if t + 1 < nb:
                    P[:, t + 1:] -= np.outer(col * (y * y), col[t + 1: nb])
                P[:, t] = col * y
            X = M[c0 + nb:, c0: c0 + nb]
            if X.shape[0] > 1:
                M[c0 + nb:, c0 + nb:] -= X @ X[:-1].T
        s = M[NP].copy()
        x = np.zeros(NP)
        for j in range(T - 1, -1, -1):
            c0 = j * nb
            D = np.tril(M[c0: c0 + nb, c0: c0 + nb])
            v = s[c0: c0 + nb].copy()
            for c in range(nb - 1, -1, -1):
                v[c] = v[c] / D[c, c]
                v[:c] -= D[c, :c] * v[c]
            x[c0: c0 + nb] = v
            s[:c0] -= M[c0: c0 + nb, :c0].T @ v
    return x[:N], status


def lapack_solve(A, b, diag_add=0.0):
    """np.linalg.solve -> (x, status); the status as the header defines it, from LAPACK's own refusal to factorise."""
    An = A + diag_add * np.eye(A.shape[0])
    try:
        ok = bool(np.isfinite(np.linalg.cholesky(An)).all())      # some LAPACKs let a NaN pivot through
    except np.linalg.LinAlgError:
        ok = False
    if not ok:
        return np.zeros_like(b), first_bad_pivot(An) + 1
    return np.linalg.solve(An, b), 0


# ----------------------------------------------------------------------------------------------------------- cases
class Case(NamedTuple):
    kind: str            # "q" | "kron" | "scale" | "indef" | "nan" | "woodbury"
    args: tuple
    diag_add: float = 0.0

    @property
    def id(self):
        return self.kind + "-" + "-".join(str(a).replace(" ", "") for a in self.args)


LADDER_N = (1, 7, 63, 64, 65, 127, 128, 129, 192, 193, 257)
LADDER = tuple(Case("q", (N, logc)) for N in LADDER_N for logc in (0, 4, 8, 12)) + \
    tuple(Case("kron", a, W_EPS) for a in ((4, 16, 8), (3, 50, 20), (5, 64, 30), (2, 160, 12)))
SCALE_BASE = Case("q", (193, 8))
SCALING = tuple(Case("scale", (p,)) for p in (-400, -100, 100, 400))
STATUS_Q = (0, 1, 62, 63, 64, 65, 127, 128, 191, 192)
INDEFINITE = tuple(Case("indef", (193, (q, 150) if q < 100 else (q,))) for q in STATUS_Q) + \
    (Case("indef", (128, (127,))), Case("indef", (129, (128,))))
NAN_AT = tuple(Case("nan", rc) for rc in ((5, 2), (64, 0), (100, 70), (192, 191), (130, 130)))
LARGE_CAP_N = 4160          # LAPACK sets the caps of both large cases on this one (8128 takes it several seconds)
LARGE = (Case("woodbury", (8128,)), Case("woodbury", (LARGE_CAP_N,)))
SMALL_CASES = LADDER + SCALING + INDEFINITE + NAN_AT
CASES = SMALL_CASES + LARGE


def order_of(case):
    if case.kind == "q" or case.kind == "woodbury":
        return case.args[0]
    if case.kind == "kron":
        return case.args[0] * case.args[1]
    if case.kind == "indef":
        return case.args[0]
    return 193


def _seed(case):
    return 1000 * order_of(case) + sum(int(a) if np.isscalar(a) else sum(a) for a in case.args)


@functools.lru_cache(maxsize=None)
def _small_system(case):
    if case.kind == "q":
        A, b = q_system(*case.args, seed=_seed(case))
    elif case.kind == "kron":
        A, b = kron_system(*case.args, seed=_seed(case))
    elif case.kind == "scale":
        A, b = _small_system(SCALE_BASE)
        A = A * 2.0 ** case.args[0]
        assert np.isfinite(A).all() and (np.abs(A[A != 0]) >= np.finfo(np.float64).tiny).all()
    elif case.kind == "indef":
        A, b = indefinite_system(*case.args, seed=_seed(case))
    elif case.kind == "nan":
        A, b = q_system(193, 4, seed=_seed(case))
        r, c = case.args
        A[r, c] = A[c, r] = np.nan
    else:
        raise ValueError(case.kind)
    A.setflags(write=False)
    b.setflags(write=False)
    return A, b


def system(case):
    """(A, b) of a case; the small ones are built once and read-only."""
    if case.kind == "woodbury":
        return woodbury_system(case.args[0], seed=_seed(case))[:2]
    return _small_system(case)


def expected_status(case):
    if case.kind == "indef":
        return min(case.args[1]) + 1
    if case.kind == "nan":
        return case.args[0] + 1
    return 0


@functools.lru_cache(maxsize=None)
def reference(case):
    """(x in long double, cond_2) of a ladder case; both belong to A + diag_add I."""
    A, b = system(case)
    cond = float(np.linalg.cond(A + case.diag_add * np.eye(A.shape[0]), 2))
    return solve_ld(A, b, case.diag_add), cond


def figures(case, x):
    """(backward error, forward error / cond_2) of a ladder case's x, both in units of eps."""
    A, b = system(case)
    xr, cond = reference(case)
    return backward_error(A, x, b, case.diag_add) / EPS, forward_error(x, xr) / (EPS * cond)


@functools.lru_cache(maxsize=None)
def lapack_family(N):
    """The largest (backward error, forward error / cond_2) in eps np.linalg.solve has over the ladder cases of order
    N."""
    fam = [c for c in LADDER if order_of(c) == N]
    assert fam
    figs = [figures(c, lapack_solve(*system(c), c.diag_add)[0]) for c in fam]
    be, fe = max(f[0] for f in figs), max(f[1] for f in figs)
    assert be > 0 and fe > 0
    return be, fe


@functools.lru_cache(maxsize=None)
def large_reference(N):
    """(x in long double from the closed form, bound of cond_2) of the Woodbury system of order N."""
    wb = woodbury_system(N, seed=_seed(Case("woodbury", (N,))), matrix=False)
    return woodbury_solve_ld(wb.dg, wb.W, wb.b), 2.0 + float(np.linalg.norm(wb.W, 2)) ** 2


def large_figures(case, A, b, x):
    xr, cond = large_reference(case.args[0])
    return backward_error(A, x, b) / EPS, forward_error(x, xr) / (EPS * cond)


@functools.lru_cache(maxsize=None)
def lapack_large():
    """LAPACK's (backward error, forward error / cond bound) in eps on the Woodbury system of order LARGE_CAP_N; its
    backward error is flat in N for this family (0.07 eps at 4160, 0.05 eps at 8128)."""
    case = Case("woodbury", (LARGE_CAP_N,))
    A, b = system(case)
    be, fe = large_figures(case, A, b, np.linalg.solve(A, b))
    assert be > 0 and fe > 0
    return be, fe


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def check_case(case, solve, record=None):
    """One set of assertions for every solver: `solve(A, b, diag_add) -> (x, status)`.  Two calls (one on the large
    systems) must agree bit for bit and leave A and b alone; then the status is the contract's and, where the system
    is positive definite, both errors are inside the caps.  record(figures), when given, gets the observed and the
    LAPACK values before anything is asserted about them.  -> the figures."""
    A, b = system(case)
    A0, b0 = A.copy(), b.copy()
    x, status = solve(A, b, case.diag_add)
    x2, status2 = (x, status) if case.kind == "woodbury" else solve(A, b, case.diag_add)
    assert _same(A, A0) and _same(b, b0), "the solver modified its inputs"
    want = expected_status(case)
    fig = {"N": int(A.shape[0]), "status": int(status)}
    if want:
        if record:
            record(fig)
        assert status == want and status2 == want, (status, status2, want)
        return fig
    if case.kind == "woodbury":
        be, fe = large_figures(case, A, b, x)
        be_l, fe_l = lapack_large()
    elif case.kind == "scale":
        p = case.args[0]
        x0, status0 = solve(*system(SCALE_BASE), 0.0)
        assert status0 == 0
        xs = x * 2.0 ** p                                 # exact: a power of two, no entry near the range's ends
        fig["bitwise_same_as_p0"] = bool(_same(xs, x0))
        be = backward_error(A, x, b) / EPS
        fe = figures(SCALE_BASE, xs)[1]
        be_l, fe_l = lapack_family(order_of(case))
    else:
        be, fe = figures(case, x)
        be_l, fe_l = lapack_family(order_of(case))
    fig.update(be_eps=be, fe_over_eps_cond=fe, lapack_be_eps=be_l, lapack_fe_over_eps_cond=fe_l)
    if record:
        record(fig)
    assert status == 0 and status2 == 0, (status, status2)
    assert _same(x, x2), "two calls differ"
    assert be <= BE_FACTOR * be_l, f"backward error {be:.3g} eps, LAPACK's largest at this N {be_l:.3g} eps"
    assert fe <= FE_FACTOR * fe_l, f"forward error {fe:.3g} eps cond, LAPACK's largest at this N {fe_l:.3g}"
    return fig
