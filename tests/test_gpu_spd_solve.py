"""als_spd_solve_f64 (spd_solve.hip: the W-step's dense fp64 Cholesky solve) at kernel level: hard systems, exact
status, the promises of the ABI, input scale and the largest order the entry point accepts.

Systems, long-double references, the caps and the assertions themselves are tests/spd_ref.py (`check_case`), shown
without a device by tests/test_spd_ref_cpu.py to be met by LAPACK, by a numpy emulation of the kernel's order and by the
CPU stand-in.  The caps are multiples of LAPACK's error on the same systems, never of the device's: the observed
figures go to profiles/spd_solve_margins.json under ALS_RECORD_MARGINS=<file>."""
import ctypes as C

import numpy as np
import pytest

from tests import spd_ref as R
from tests.gpu_common import env, ptr, record_margins, same_bits, upload

pytestmark = pytest.mark.gpu


def _device_solver(E):
    """`solve(A, b, diag_add) -> (x, status)` of R.check_case on the backend of E; the status word starts from 7 and the
    device copies of A and b must come back unchanged."""
    torch = E.torch

    def solve(A, b, diag_add):
        At, bt = (upload(a if a.flags.writeable else a.copy(), E.dev) for a in (A, b))    # the cases are read-only
        status = torch.full((1,), 7, dtype=torch.int32, device=E.dev)
        x = E.be.spd_solve(At, bt, diag_add, status)
        torch.cuda.synchronize()
        assert same_bits(At.cpu(), A) and same_bits(bt.cpu(), b), "the kernel modified its inputs"
        return x.cpu().numpy(), int(status.item())
    return solve


def _check(case):
    return R.check_case(case, _device_solver(env()), record=lambda fig: record_margins("spd_solve/" + case.id, fig))


def _raw_solve(E, At, lda, bt, xt, diag_add=0.0, workspace=None, preset=7):
    """The entry point through ctypes -> status; x goes to xt (which may be bt)."""
    torch, lib = E.torch, E.be.lib
    N = bt.numel()
    ws = workspace if workspace is not None else torch.empty(int(lib.als_spd_solve_workspace_bytes(N)),
                                                             dtype=torch.uint8, device=E.dev)
    status = torch.full((1,), preset, dtype=torch.int32, device=E.dev)
    rc = lib.als_spd_solve_f64(N, ptr(At), lda, ptr(bt), C.c_double(diag_add), ptr(xt), ptr(ws), ptr(status),
                               E.be._stream())
    torch.cuda.synchronize()
    assert rc == 0
    return int(status.item())


# --------------------------------------------------------------------------------------------------- accuracy ladder
@pytest.mark.parametrize("case", R.LADDER, ids=lambda c: c.id)
def test_accuracy_ladder(case):
    """cond_2 from 1 to 10^12 (q) and the engine's own lambda_w = 0 regime, rank-deficient + 1e-10 (kron), at every
    tile edge: status 0, backward error <= 4x and forward error / cond <= 8x LAPACK's largest at the same order, two
    calls bit for bit the same, A and b untouched."""
    _check(case)


@pytest.mark.parametrize("case", R.SCALING, ids=lambda c: c.id)
def test_power_of_two_scaling(case):
    """A 2^p with b unchanged: the same backward cap (it is scale-free), and x 2^p against the unscaled reference in
    the forward cap.  Whether x 2^p is the unscaled output bit for bit is recorded, not asserted."""
    _check(case)


# ------------------------------------------------------------------------------------------------------------ status
@pytest.mark.parametrize("case", R.INDEFINITE, ids=lambda c: c.id)
def test_status_is_the_first_bad_pivot(case):
    """status == q + 1 exactly: first and last column of a tile, the last tile, next to the identity padding, the last
    pivot of a full tile (N = 128) and the first of a padded one (N = 129); with a second negative pivot behind it
    where q < 100."""
    _check(case)


@pytest.mark.parametrize("case", R.NAN_AT, ids=lambda c: c.id)
def test_status_of_a_nan_entry_is_its_row(case):
    _check(case)


def test_recovery_after_a_failed_call():
    """The status word is reset by every call, and a good call right after a failed one on the same backend (same
    cached workspace) gives the bits of a fresh backend's call."""
    bad, good = R.INDEFINITE[4], R.SCALE_BASE
    E, F = env(), env()
    first, fresh = _device_solver(E), _device_solver(F)
    _, st = first(*R.system(bad), 0.0)
    assert st == R.expected_status(bad)
    x, st = first(*R.system(good), 0.0)             # the solver presets the status word to 7
    assert st == 0
    xf, stf = fresh(*R.system(good), 0.0)
    assert stf == 0 and same_bits(x, xf)


# --------------------------------------------------------------------------------------------------------------- ABI
@pytest.mark.parametrize("N", [65, 193])
def test_lda_larger_than_n(N):
    """The system inside an [N][N + 3] array whose extra columns are NaN: the bits of the contiguous call."""
    E = env()
    torch = E.torch
    A, b = R.system(R.Case("q", (N, 4)))
    wide = np.full((N, N + 3), np.nan)
    wide[:, :N] = A
    bt = upload(b.copy(), E.dev)
    x0 = torch.full((N,), 7.0, dtype=torch.float64, device=E.dev)
    x1 = torch.full((N,), 7.0, dtype=torch.float64, device=E.dev)
    assert _raw_solve(E, upload(A.copy(), E.dev), N, bt, x0) == 0
    assert _raw_solve(E, upload(wide, E.dev), N + 3, bt, x1) == 0
    assert np.isfinite(x0.cpu().numpy()).all() and same_bits(x0.cpu(), x1.cpu())
    assert same_bits(x0.cpu(), _device_solver(E)(A, b, 0.0)[0])          # and of the backend's call


@pytest.mark.parametrize("N", [65, 193])
def test_x_may_alias_b(N):
    E = env()
    A, b = R.system(R.Case("q", (N, 4)))
    At, bt = upload(A.copy(), E.dev), upload(b.copy(), E.dev)
    x0 = E.torch.full((N,), 7.0, dtype=E.torch.float64, device=E.dev)
    assert _raw_solve(E, At, N, bt, x0) == 0
    assert _raw_solve(E, At, N, bt, bt) == 0
    assert same_bits(x0.cpu(), bt.cpu())


@pytest.mark.parametrize("fill", ["nan", "ff"])
def test_result_does_not_depend_on_the_workspace(fill):
    """Apart from the status word it resets, the kernel writes everything it later reads: the backend's cached
    workspace full of NaN (or 0xFF bytes, another NaN) before the call changes no bit."""
    E = env()
    torch = E.torch
    case = R.Case("q", (193, 8))
    solve = _device_solver(E)
    x0, st = solve(*R.system(case), 0.0)
    assert st == 0
    ws = E.be._ws["spd"]
    assert ws.numel() >= int(E.be.lib.als_spd_solve_workspace_bytes(193))
    if fill == "nan":
        ws[: ws.numel() // 8 * 8].view(torch.float64).fill_(float("nan"))
    else:
        ws.fill_(0xFF)
    x1, st = solve(*R.system(case), 0.0)
    assert st == 0 and E.be._ws["spd"] is ws and same_bits(x0, x1)


# ------------------------------------------------------------------------------------------------------- large sizes
@pytest.mark.parametrize("case", R.LARGE, ids=lambda c: c.id)
def test_large_orders(case):
    """ALS_SPD_MAX_N = 8128 (127 panels, 8127 update workgroups behind the first, 64 KB of dynamic LDS in the
    back-substitution) and 4160, diagonal + rank 8 against the closed form in long double: return code 0 (the backend
    raises otherwise), status 0, and the caps of LAPACK's errors on the 4160 system."""
    E = env()
    N = case.args[0]
    assert int(E.be.lib.als_spd_solve_workspace_bytes(N)) > 0
    R.check_case(case, _device_solver(E), record=lambda fig: record_margins("spd_solve/" + case.id, fig))
