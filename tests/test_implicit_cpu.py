"""ImplicitALS without a GPU: the numpy reference (tests/implicit_ref.py) against brute force, the closed-form loss,
and the engine / facade end to end on the numpy stand-in backend (tests/implicit_cpu_backend.py)."""
import numpy as np
import pytest

from collaborative_filtering_amd import (ALSConfig, CoreConfig, GraphConfig, GraphSimConfig, ImplicitALS,
                                         ImplicitConfig, cv, layout)
from tests import implicit_ref as iref
from tests.implicit_cpu_backend import ImplicitNumpyBackend


def _sides(m, n, nnz, seed):
    r, c, v = iref.zipf_counts(m, n, nnz, seed)
    csr, csc = layout.coo_to_sides(r, c, v, (m, n))
    return (r, c, v), csr, csc


def _cfg(k, n_iters, lam_u=0.5, lam_v=0.5, **core):
    return ALSConfig(core=CoreConfig(n_factors=k, n_iters=n_iters, lambda_u=lam_u, lambda_v=lam_v, **core))


# ---------------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------------
def test_reference_against_brute_force():
    m, n, k, a0, lam_u, lam_v = 40, 30, 5, 0.7, 0.3, 0.4
    _, csr, csc = _sides(m, n, 300, 1)
    ua, ia = iref.weights(csr.vals, 2.0), iref.weights(csc.vals, 2.0)
    U0, V = iref.init_tables(m, n, k, 3)
    U, _ = iref.half_step(csr.indptr, csr.indices, ua, V, a0, lam_u)
    # normal-equation residual of every row, the system assembled entry by entry
    G = a0 * sum(np.outer(v, v) for v in V)
    for u in range(m):
        A = G + (lam_u + iref.EPS) * np.eye(k)
        b = np.zeros(k)
        for e in range(csr.indptr[u], csr.indptr[u + 1]):
            f = V[csr.indices[e]]
            A += float(ua[e]) * np.outer(f, f)
            b += (1.0 + float(ua[e])) * f
        if csr.indptr[u + 1] == csr.indptr[u]:
            assert not U[u].any()
        else:
            assert np.max(np.abs(A @ U[u] - b)) <= 1e-13 * max(1.0, np.max(np.abs(b)))
    # the direct loss against the dense sum_all evaluated literally
    d = iref.loss_direct(csr.indptr, csr.indices, ua, U, V, a0, lam_u, lam_v)
    e = iref.loss_dense(csr.indptr, csr.indices, ua, U, V, a0, lam_u, lam_v)
    assert abs(d - e) <= 1e-13 * abs(e)
    assert ia.sum() == pytest.approx(ua.sum())


@pytest.mark.parametrize("a0", [1.0, 0.25])
def test_closed_form_loss_equals_direct_loss(a0):
    """The gap is second order in the 2^-24 rounding of V (observed 1e-15 ... 1e-14); a first-order mistake shows at
    1e-7, and leaving out the 1e-10 |V|^2 that the solver's diagonal carries at 3e-11 ... 8e-11."""
    m, n, k, lam_u, lam_v = 200, 150, 64, 0.5, 0.5
    _, csr, csc = _sides(m, n, 3400, 2)
    ua, ia = iref.weights(csr.vals, 2.0), iref.weights(csc.vals, 2.0)
    U, _ = iref.init_tables(m, n, k, 5)
    U = U.astype(np.float32).astype(np.float64)
    X, xb = iref.half_step(csc.indptr, csc.indices, ia, U, a0, lam_v)
    V = X.astype(np.float32).astype(np.float64)
    closed = iref.loss_closed(ia, xb, U, V, lam_u)
    direct = iref.loss_direct(csr.indptr, csr.indices, ua, U, V, a0, lam_u, lam_v)
    assert abs(closed - direct) <= 1e-10 * abs(direct)


# ---------------------------------------------------------------------------------------------------------
# end to end on the stand-in
# ---------------------------------------------------------------------------------------------------------
M, N, K, ITERS = 300, 200, 20, 8


@pytest.fixture(scope="module")
def fitted():
    coo, csr, csc = _sides(M, N, 4900, 11)
    icfg = ImplicitConfig(alpha=2.0, unobserved_weight=0.25)
    model = ImplicitALS(_cfg(K, ITERS, random_state=7), icfg, backend=ImplicitNumpyBackend(), device="cpu")
    model.fit_coo(*coo, (M, N), tol=None, verbose=0)
    ua, ia = iref.weights(csr.vals, 2.0), iref.weights(csc.vals, 2.0)
    ref = iref.fit(csr.indptr, csr.indices, ua, csc.indptr, csc.indices, ia, (M, N), K, ITERS, 0.25, 0.5, 0.5, 7)
    return model, ref, coo, csr


def test_fit_reproduces_the_reference(fitted):
    model, (U, V, losses), _, _ = fitted
    assert model.U.shape == (M, K) and model.V.shape == (N, K)
    np.testing.assert_allclose(model.U, U, rtol=0, atol=1e-6 * np.max(np.abs(U)))
    np.testing.assert_allclose(model.V, V, rtol=0, atol=1e-6 * np.max(np.abs(V)))
    loss = np.asarray(model.history["loss"])
    assert loss.shape == (ITERS,)
    np.testing.assert_allclose(loss, losses, rtol=1e-9)
    assert (np.diff(loss) <= 1e-12 * loss[:-1]).all()
    assert model.mu == 0.0 and not model.b_u.any() and not model.b_i.any()


def test_fit_log_confidence_and_dense_entry():
    m, n, k = 60, 40, 8
    (r, c, v), csr, csc = _sides(m, n, 500, 4)
    R = np.full((m, n), np.nan)
    R[r, c] = v
    icfg = ImplicitConfig(alpha=3.0, confidence="log", eps=2.0)
    model = ImplicitALS(_cfg(k, 4), icfg, backend=ImplicitNumpyBackend(), device="cpu").fit(R, tol=None, verbose=0)
    ua, ia = iref.weights(csr.vals, 3.0, "log", 2.0), iref.weights(csc.vals, 3.0, "log", 2.0)
    U, V, losses = iref.fit(csr.indptr, csr.indices, ua, csc.indptr, csc.indices, ia, (m, n), k, 4, 1.0, 0.5, 0.5, 42)
    np.testing.assert_allclose(model.U, U, rtol=0, atol=1e-6 * np.max(np.abs(U)))
    np.testing.assert_allclose(model.history["loss"], losses, rtol=1e-9)


def test_early_stopping_on_the_relative_loss_decrease():
    (r, c, v), _, _ = _sides(60, 40, 500, 4)
    model = ImplicitALS(_cfg(8, 40), ImplicitConfig(alpha=2.0), backend=ImplicitNumpyBackend(), device="cpu")
    model.fit_coo(r, c, v, (60, 40), tol=2e-2, min_iters=3, verbose=0)
    loss = model.history["loss"]
    assert 3 <= len(loss) < 40 and loss[-3] - loss[-1] <= 2e-2 * loss[-3]


def test_serving_on_the_fitted_model(fitted):
    model, _, (r, c, v), csr = fitted
    users = np.arange(0, M, 7)
    items, scores = model.recommend(users, N=10)
    P = model.predict()
    assert P.shape == (M, N)
    np.testing.assert_array_equal(P, (model.U.astype(np.float32).astype(np.float64)
                                      @ model.V.astype(np.float32).astype(np.float64).T).astype(np.float32))
    for b, u in enumerate(users):
        seen = csr.indices[csr.indptr[u]:csr.indptr[u + 1]]
        assert not np.intersect1d(items[b][items[b] >= 0], seen).size
        np.testing.assert_array_equal(scores[b], P[u, items[b]])
    hr, hc, _ = iref.zipf_counts(M, N, 400, 99)              # held-out pairs (a seen one is never recommended)
    out = cv.ranking_at_k(model, hr, hc, K=10)
    assert out["users"] > 0 and 0.0 <= out["recall@K"] <= 1.0 and 0.0 <= out["ndcg@K"] <= 1.0


def test_fold_in_is_one_user_half_step(fitted):
    model, (U, V, _), _, csr = fitted
    users = np.array([0, 3, 50, 299])
    R_new = np.full((users.size + 1, N), np.nan)
    for b, u in enumerate(users):
        s = slice(csr.indptr[u], csr.indptr[u + 1])
        R_new[b, csr.indices[s]] = csr.vals[s]
    Un, bn = model.fold_in(R_new, n_sweeps=3)
    ptr = np.concatenate([[0], np.cumsum([csr.indptr[u + 1] - csr.indptr[u] for u in users]), ]).astype(np.int64)
    ptr = np.append(ptr, ptr[-1])
    idx = np.concatenate([csr.indices[csr.indptr[u]:csr.indptr[u + 1]] for u in users])
    a = iref.weights(np.concatenate([csr.vals[csr.indptr[u]:csr.indptr[u + 1]] for u in users]), 2.0)
    X, _ = iref.half_step(ptr, idx, a, model.V, 0.25, 0.5)
    np.testing.assert_allclose(Un, X, rtol=0, atol=2.0 ** -23 * np.max(np.abs(X)))
    assert not Un[-1].any() and not bn.any()
    items, _ = model.recommend_new(R_new[:2], N=5)
    assert not np.intersect1d(items[0], csr.indices[csr.indptr[0]:csr.indptr[1]]).size


# ---------------------------------------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------------------------------------
def _model(icfg=None, cfg=None, **kw):
    return ImplicitALS(cfg or _cfg(4, 2), icfg, backend=ImplicitNumpyBackend(), device="cpu", **kw)


@pytest.mark.parametrize("icfg", [ImplicitConfig(alpha=-1.0), ImplicitConfig(eps=0.0), ImplicitConfig(eps=-1.0),
                                  ImplicitConfig(unobserved_weight=-0.5), ImplicitConfig(confidence="sqrt")])
def test_bad_implicit_config_raises(icfg):
    with pytest.raises(ValueError):
        _model(icfg)


def test_unsupported_model_options_raise():
    with pytest.raises(ValueError):
        _model(lambda_w={"genres": 1.0})
    with pytest.raises(ValueError):
        _model(process_group="world")
    with pytest.raises(ValueError):
        _model(cfg=_cfg(4, 2, pop_reg_mode="inverse_sqrt"))
    with pytest.raises(ValueError):
        _model(cfg=ALSConfig(core=CoreConfig(n_factors=4, n_iters=2, lambda_u=1.0, lambda_v=1.0),
                             graph=GraphConfig(alpha=0.5, sim=GraphSimConfig())))
    _model(cfg=ALSConfig(core=CoreConfig(n_factors=4, n_iters=2, lambda_u=1.0, lambda_v=1.0),
                         graph=GraphConfig(alpha=0.5, sim=None)))        # the graph is off: accepted


@pytest.mark.parametrize("bad", [0.0, -1.0, np.inf])
def test_bad_ratings_raise(bad):
    R = np.full((6, 5), np.nan)
    R[0, 1], R[2, 3], R[4, 0] = 1.0, 2.0, bad
    with pytest.raises(ValueError):
        _model().fit(R, tol=None, verbose=0)


def test_features_raise():
    R = np.full((6, 5), np.nan)
    R[0, 1] = R[2, 3] = 1.0
    with pytest.raises(ValueError):
        _model().fit(R, features={"genres": np.ones((5, 2))}, tol=None, verbose=0)


def test_calls_not_defined_for_this_model_raise(fitted):
    model, _, _, _ = fitted
    R_new = np.full((1, N), np.nan)
    R_new[0, 3] = 1.0
    for name, call in (("explain", lambda: model.explain([0], [1])),
                       ("explain_new", lambda: model.explain_new(R_new, [[1]])),
                       ("recommend_explore", lambda: model.recommend_explore([0])),
                       ("recommend_new_explore", lambda: model.recommend_new_explore(R_new)),
                       ("fold_in_items", lambda: model.fold_in_items(np.full((M, 1), np.nan))),
                       ("predict_new_items", lambda: model.predict_new_items(None)),
                       ("recommend", lambda: model.recommend([0], new_items=object())),
                       ("recommend_deep", lambda: model.recommend_deep([0], N=200, new_items=object())),
                       ("recommend_group", lambda: model.recommend_group([[0, 1]], new_items=object())),
                       ("recommend_quota", lambda: model.recommend_quota([0], groups=np.zeros(N, np.int64),
                                                                         max_per_group=1, new_items=object()))):
        with pytest.raises(ValueError, match=name):
            call()
    with pytest.raises(ValueError):
        model.fold_in(np.where(np.isnan(R_new), np.nan, -1.0))


def test_implicit_params_layout_matches_header(tmp_path):
    """The ctypes mirror of als_implicit_params has exactly the C layout (as test_cabi_cpu checks the older structs)."""
    import ctypes as C
    import os
    import subprocess
    from collaborative_filtering_amd import _hip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "als_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(als_implicit_params));']
    src += [f'printf("%zu\\n", offsetof(als_implicit_params, {name}));' for name, _ in _hip.ImplicitParams._fields_]
    src.append('return 0;}')
    (tmp_path / "layout.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-I", os.path.join(root, "include"), str(tmp_path / "layout.c"), "-o",
                    str(tmp_path / "layout")], check=True)
    vals = [int(x) for x in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True,
                                           text=True).stdout.split()]
    assert C.sizeof(_hip.ImplicitParams) == vals[0]
    assert [getattr(_hip.ImplicitParams, name).offset for name, _ in _hip.ImplicitParams._fields_] == vals[1:]
