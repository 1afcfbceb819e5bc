"""Fold-in without a GPU: the C struct mirror, the one-factorisation reformulation of the user half-step, and the
input normaliser of ALS.fold_in / recommend_new."""
import os

import numpy as np
import pytest

from oracle.als_oracle import EPS, OracleALS, OracleConfig, ratings_from_coo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_header(tmp_path):
    import ctypes as C
    import subprocess
    from collaborative_filtering_amd import _hip
    st = _hip.FoldInParams
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "als_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(als_fold_in_params));']
    src += [f'printf("%zu\\n", offsetof(als_fold_in_params, {f}));' for f, _ in st._fields_]
    src.append('return 0;}')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = iter(int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(st) == next(vals)
    for f, _ in st._fields_:
        assert getattr(st, f).offset == next(vals), f
    assert "als_fold_in" in _hip.EXPORTS


@pytest.mark.parametrize("n_rated,lam_u", [(3, 5.0), (12, 1e-2), (40, 0.5)])
def test_recurrence_and_fixed_point_equal_the_user_half_step(n_rated, lam_u):
    """p = A^-1 g, q = A^-1 h: T applications of OracleALS.user_step from b_u = 0 are the scalar recurrence
    b_t = (s - h.p + b_{t-1} h.q) / d, u_T = p - b_{T-1} q, and its limit is the bordered solve."""
    k, n = 8, 60
    rng = np.random.default_rng(n_rated)
    cols = np.sort(rng.permutation(n)[:n_rated])
    vals = rng.integers(1, 11, n_rated) * 0.5
    rt = ratings_from_coo(np.zeros(n_rated, np.int64), cols, vals, (1, n))
    o = OracleALS(OracleConfig(n_factors=k, n_iters=1, lambda_u=lam_u, lambda_v=1.0, lambda_bu=2.0, lambda_bi=1.0))
    Z = rng.normal(size=(n, k))
    o.mu, o.b_i = 3.1, rng.normal(scale=0.3, size=n)
    o.U, o.b_u = np.zeros((1, k)), np.zeros(1)
    Zs = Z[cols]
    res = vals - o.mu - o.b_i[cols]
    A = Zs.T @ Zs + (lam_u + EPS) * np.eye(k)
    g, h, s, d = Zs.T @ res, Zs.sum(axis=0), res.sum(), n_rated + 2.0 + EPS
    p, q = np.linalg.solve(A, g), np.linalg.solve(A, h)
    hp, hq = h @ p, h @ q
    b = 0.0
    for T in range(1, 6):
        b_prev = b
        b = (s - hp + b * hq) / d
        o.user_step(rt, Z)
        np.testing.assert_allclose(p - b_prev * q, o.U[0], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(b, o.b_u[0], rtol=1e-10, atol=1e-12)
    bs = (s - hp) / (d - hq)
    M = np.block([[A, h[:, None]], [h[None, :], np.array([[d]])]])
    x = np.linalg.solve(M, np.append(g, s))
    np.testing.assert_allclose(p - bs * q, x[:k], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(bs, x[k], rtol=1e-10, atol=1e-12)
    for _ in range(300):
        o.user_step(rt, Z)
    np.testing.assert_allclose(o.U[0], x[:k], rtol=1e-8, atol=1e-10)
    assert d - hq > 2.0                                  # Schur complement above lambda_bu: always solvable


# ------------------------------------------------------------------------------------------ normaliser
def test_dense_to_sorted_csr():
    from collaborative_filtering_amd.als import fold_in_csr
    R = np.full((3, 5), np.nan)
    R[0, [4, 1]] = [2.0, 3.5]
    R[2, 0] = 1.0
    ip, ix, vv = fold_in_csr(R, 5)
    assert ip.tolist() == [0, 2, 2, 3] and ix.tolist() == [1, 4, 0] and vv.tolist() == [3.5, 2.0, 1.0]
    assert ip.dtype == np.int64 and ix.dtype == np.int32 and vv.dtype == np.float32


def test_csr_rows_are_sorted_with_their_values():
    from collaborative_filtering_amd.als import fold_in_csr
    ip, ix, vv = fold_in_csr(([0, 3, 3, 5], [7, 2, 5, 1, 0], [1.0, 2.0, 3.0, 4.0, 5.0]), 8)
    assert ip.tolist() == [0, 3, 3, 5]
    assert ix.tolist() == [2, 5, 7, 0, 1] and vv.tolist() == [2.0, 3.0, 1.0, 5.0, 4.0]
    R = np.full((2, 8), np.nan)
    R[0, [7, 2, 5]] = [1.0, 2.0, 3.0]
    R[1, [1, 0]] = [4.0, 5.0]
    d = fold_in_csr(R, 8)
    c = fold_in_csr(([0, 3, 5], [7, 2, 5, 1, 0], [1.0, 2.0, 3.0, 4.0, 5.0]), 8)
    assert all((a == b).all() for a, b in zip(d, c))


@pytest.mark.parametrize("R,exc", [
    (([0, 2], [3, 3], [1.0, 2.0]), ValueError),                  # duplicate column
    (([0, 2], [1, 9], [1.0, 2.0]), IndexError),                  # column >= n
    (([0, 1], [-1], [1.0]), IndexError),                         # column < 0
    (([0, 1], [1], [np.inf]), ValueError),                       # non-finite
    (([0, 1], [1], [1e39]), ValueError),                         # beyond float32
    (([0, 2], [1], [1.0]), ValueError),                          # malformed indptr
    (([1, 2], [1], [1.0]), ValueError),
    (np.full((2, 7), np.nan), ValueError),                       # wrong dense width
    (np.where(np.eye(2, 5) > 0, np.inf, np.nan), ValueError),    # non-finite dense entry
])
def test_normaliser_rejections(R, exc):
    from collaborative_filtering_amd.als import fold_in_csr
    with pytest.raises(exc):
        fold_in_csr(R, 5)


# ------------------------------------------------------------------------------------------ model boundary
@pytest.fixture(scope="module")
def fitted():
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig
    from tests.cpu_backend import NumpyBackend
    from tests.synth import make_ratings
    r, c, v = make_ratings(20, 15, 150, seed=4)
    cfg = ALSConfig(core=CoreConfig(n_factors=4, n_iters=2, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    return ALS(cfg, device="cpu", backend=NumpyBackend()).fit_coo(r, c, v, (20, 15), tol=None, verbose=0)


def test_unfitted_model_raises_like_predict():
    from collaborative_filtering_amd import ALS, ALSConfig, CoreConfig
    from tests.cpu_backend import NumpyBackend
    model = ALS(ALSConfig(core=CoreConfig(n_factors=3, n_iters=1, lambda_u=1.0, lambda_v=1.0)), device="cpu",
                backend=NumpyBackend())
    with pytest.raises(RuntimeError, match="Model must be fitted before prediction."):
        model.fold_in(np.full((1, 4), np.nan))
    with pytest.raises(RuntimeError, match="Model must be fitted before prediction."):
        model.recommend_new(np.full((1, 4), np.nan))


@pytest.mark.parametrize("T", [0, -2, 1.5, True, "3"])
def test_bad_n_sweeps(fitted, T):
    with pytest.raises(ValueError):
        fitted.fold_in(np.full((1, 15), np.nan), n_sweeps=T)
    with pytest.raises(ValueError):
        fitted.recommend_new(np.full((1, 15), np.nan), n_sweeps=T)


def test_model_boundary_rejections(fitted):
    R = np.full((2, 15), np.nan)
    with pytest.raises(ValueError):
        fitted.fold_in(R[:, :14])
    with pytest.raises(ValueError):
        fitted.recommend_new(R, 0)
    with pytest.raises(IndexError):
        fitted.fold_in(([0, 1], [15], [1.0]))
    with pytest.raises(ValueError, match="infinite"):
        fitted.fold_in(R, features={"genres": np.full((15, 2), np.inf)})
