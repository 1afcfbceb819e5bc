"""The references of the dense Cholesky solve's kernel tests (tests/spd_ref.py) without a device: the long-double solve
is exact where exactness can be had and orders of magnitude below every cap elsewhere, the indefinite and NaN systems
fail where the tests say they do, and three correct solvers - LAPACK, a numpy emulation of the kernel's blocked order
and the CPU stand-in of the backend - pass the very assertions the device kernel is held to."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import spd_ref as R
from tests.cpu_backend import NumpyBackend


def _smallest_cap():
    """The smallest tolerance (in eps; cond_2 >= 1) any ladder case applies."""
    return min(min(R.BE_FACTOR * be, R.FE_FACTOR * fe) for be, fe in map(R.lapack_family, sorted(set(
        R.order_of(c) for c in R.LADDER))))


def _exact_system(N, seed):
    """A = L0 D L0^T, b = A x with an integer unit-lower L0 (at most 3 off-diagonal entries per row), D = 4^e and an
    integer x: every entry of A and b is an integer multiple of 2^-4 below 2^53."""
    rng = np.random.default_rng(seed)
    L0 = np.eye(N)
    for i in range(1, N):
        cols = rng.choice(i, size=min(i, 3), replace=False)
        L0[i, cols] = rng.integers(-2, 3, size=cols.size)
    D = 4.0 ** rng.integers(-2, 3, size=N)
    x = (rng.integers(1, 10, size=N) * rng.choice([-1, 1], size=N)).astype(np.float64)
    A = (L0 * D) @ L0.T
    return L0, D, x, A, A @ x


@pytest.mark.parametrize("N", [1, 2, 7, 33, 65])
def test_solve_ld_reproduces_exact_systems(N):
    L0, D, x, A, b = _exact_system(N, seed=N)
    F = lambda M: [[Fraction(float(v)) for v in row] for row in np.atleast_2d(M)]       # noqa: E731
    Lf, Af, xf = F(L0), F(A), [Fraction(float(v)) for v in x]
    for i in range(N):                     # A and b as fp64 holds them are the exact products
        for j in range(N):
            assert Af[i][j] == sum(Lf[i][t] * Fraction(float(D[t])) * Lf[j][t] for t in range(N))
        assert Fraction(float(b[i])) == sum(Af[i][j] * xf[j] for j in range(N))
    got = R.solve_ld(A, b)
    assert got.dtype == np.longdouble
    assert R.forward_error(got, x) <= 1e-3 * _smallest_cap() * R.EPS


@pytest.mark.parametrize("case", R.LADDER, ids=lambda c: c.id)
def test_solve_ld_is_far_inside_the_caps(case):
    """Its own backward error, measured in long double, is below a thousandth of the cap the device gets."""
    A, b = R.system(case)
    x, cond = R.reference(case)
    assert cond >= 1.0
    be = R.backward_error(A, x, b, case.diag_add) / R.EPS
    assert be <= 1e-3 * R.BE_FACTOR * R.lapack_family(R.order_of(case))[0], be


def test_woodbury_closed_form_agrees_with_the_factorisation():
    wb = R.woodbury_system(257, seed=3)
    assert np.array_equal(wb.A, wb.A.T)
    # exact entries: W W^T in multiples of 1/16, the diagonal on the 2^-20 grid
    assert np.array_equal(wb.A * 2.0 ** 20, np.round(wb.A * 2.0 ** 20))
    a, c = R.solve_ld(wb.A, wb.b), R.woodbury_solve_ld(wb.dg, wb.W, wb.b)
    cond = 2.0 + np.linalg.norm(wb.W, 2) ** 2
    assert np.linalg.cond(wb.A, 2) <= cond
    assert R.forward_error(a, c) <= 1e-3 * R.EPS * cond


def test_kron_systems_are_rank_deficient_with_safe_pivots():
    for case in R.LADDER:
        if case.kind != "kron":
            continue
        A, b = R.system(case)
        N = A.shape[0]
        assert np.linalg.matrix_rank(A) < N
        bad, p = R.pivots(A + case.diag_add * np.eye(N))
        assert bad is None and 0.9 * R.W_EPS <= p.min() <= 2.0 * R.W_EPS
        assert R.reference(case)[1] >= 1e10


@pytest.mark.parametrize("case", R.INDEFINITE, ids=lambda c: c.id)
def test_indefinite_systems_fail_at_the_first_flipped_pivot(case):
    A, b = R.system(case)
    q = min(case.args[1])
    bad, p = R.pivots(A)
    assert bad == q == R.first_bad_pivot(A) and R.expected_status(case) == q + 1
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(A)
    assert p[q] < 0 and (q == 0 or -p[q] >= 0.5 * p[:q].min())        # not a marginal failure


@pytest.mark.parametrize("case", R.NAN_AT, ids=lambda c: c.id)
def test_a_nan_entry_fails_at_its_row(case):
    """Only row r of L is NaN before pivot r: the recurrence of row i < r never reads row r."""
    A, b = R.system(case)
    r, c = case.args
    assert r >= c and np.isnan(A[r, c]) and np.isnan(A[c, r]) and np.isnan(A).sum() == (1 if r == c else 2)
    assert R.first_bad_pivot(A) == r and R.expected_status(case) == r + 1


def test_first_bad_pivot_accepts_definite_and_rejects_zero():
    assert R.first_bad_pivot(R.system(R.SCALE_BASE)[0]) is None
    assert R.first_bad_pivot(np.zeros((3, 3))) == 0
    assert R.first_bad_pivot(np.diag([1.0, 0.0, 1.0])) == 1


def test_scaled_systems_are_exact_multiples():
    A0, b0 = R.system(R.SCALE_BASE)
    for case in R.SCALING:
        A, b = R.system(case)
        assert np.array_equal(A * 2.0 ** -case.args[0], A0) and b is b0


SOLVERS = {"lapack": R.lapack_solve, "blocked": R.blocked_cholesky_solve}
# 8128 is the device's: LAPACK needs seconds for it
CPU_CASES = R.SMALL_CASES + (R.Case("woodbury", (R.LARGE_CAP_N,)),)


@pytest.mark.parametrize("solver", sorted(SOLVERS))
@pytest.mark.parametrize("case", CPU_CASES, ids=lambda c: c.id)
def test_correct_solvers_pass_the_shared_checker(case, solver):
    """The caps are reachable: LAPACK stays inside the caps set from its own family maximum, and so does a solver
    that works in the kernel's order."""
    R.check_case(case, SOLVERS[solver])


def _stand_in(A, b, diag_add):
    status = torch.full((1,), 7, dtype=torch.int32)
    x = NumpyBackend().spd_solve(torch.from_numpy(A.copy()), torch.from_numpy(b.copy()), diag_add, status)
    return x.numpy(), int(status.item())


@pytest.mark.parametrize("case", R.SMALL_CASES, ids=lambda c: c.id)
def test_cpu_stand_in_passes_the_shared_checker(case):
    R.check_case(case, _stand_in)


def test_checker_rejects_wrong_solvers():
    """A reciprocal square root that is good to 44 bits only, on a well and on a badly conditioned system, and a
    status that is off by one are caught."""
    def sloppy(A, b, diag_add):
        return R.blocked_cholesky_solve(A, b, diag_add, rsq_rel_error=2.0 ** -44)

    def off_by_one(A, b, diag_add):
        x, st = R.lapack_solve(A, b, diag_add)
        return x, st - 1 if st else 0

    for case in (R.Case("q", (129, 8)), R.LADDER[-3]):
        with pytest.raises(AssertionError, match="backward error"):
            R.check_case(case, sloppy)
    with pytest.raises(AssertionError):
        R.check_case(R.INDEFINITE[3], off_by_one)
