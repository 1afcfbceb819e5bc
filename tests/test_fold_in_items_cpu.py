"""Item fold-in without a GPU: the C struct mirror, the one-factorisation reformulation of the fit's item half-step
for a new column, the input validation of ALS.fold_in_items, and the torch formulation of the new items' graph
rows."""
import os

import numpy as np
import pytest

from oracle.als_oracle import EPS, OracleALS, OracleConfig, ratings_from_coo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_struct_layout_matches_header(tmp_path):
    import ctypes as C
    import subprocess
    from collaborative_filtering_amd import _hip
    st = _hip.FoldInItemsParams
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "als_hip.h"', 'int main(void){',
           'printf("%zu\\n", sizeof(als_fold_in_items_params));']
    src += [f'printf("%zu\\n", offsetof(als_fold_in_items_params, {f}));' for f, _ in st._fields_]
    src.append('return 0;}')
    cfile = tmp_path / "layout.c"
    cfile.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(cfile), "-o", str(exe)], check=True)
    vals = iter(int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert C.sizeof(st) == next(vals)
    for f, _ in st._fields_:
        assert getattr(st, f).offset == next(vals), f
    assert "als_fold_in_items" in _hip.EXPORTS


def fold_item_reference(U, b_u, mu, V, raters, r, nb_idx, nb_val, lam_v, pop_reg, lam_bi, alpha, T):
    """The contract of als_fold_in_items for one item, in float64: T >= 1 alternations from b = 0 through the
    recurrence on p = A^-1 g, q = A^-1 h, or (T = 0) the bordered fixed point."""
    k = U.shape[1]
    n_i = raters.size
    lv = lam_v / np.sqrt(n_i + 1.0) if pop_reg else lam_v
    lam = lv + EPS + alpha * nb_val.sum()
    Us = U[raters]
    res = r - mu - b_u[raters]
    A = Us.T @ Us + lam * np.eye(k)
    g = Us.T @ res + alpha * (nb_val @ V[nb_idx])
    h, s, d = Us.sum(axis=0), res.sum(), n_i + lam_bi + EPS
    p, q = np.linalg.solve(A, g), np.linalg.solve(A, h)
    if T == 0:
        b = (s - h @ p) / (d - h @ q)
        return p - b * q, b
    b = bp = 0.0
    for _ in range(T):
        bp, b = b, (s - h @ p + b * (h @ q)) / d
    return p - bp * q, b


@pytest.mark.parametrize("pop_reg", [None, "inverse_sqrt"])
@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("n_rated", [4, 30])
def test_recurrence_and_fixed_point_equal_the_item_half_step(pop_reg, alpha, n_rated):
    """T applications of OracleALS.item_step to a new column (its graph row, lambda_v_i and lambda_bi_i set as the
    fit would) equal the recurrence, and their limit is the bordered solve."""
    k, m, n = 6, 50, 20                                  # n fitted items + the new column n
    rng = np.random.default_rng(n_rated + int(alpha * 10) + (pop_reg is not None))
    raters = np.sort(rng.permutation(m)[:n_rated])
    vals = rng.integers(1, 11, n_rated) * 0.5
    rt = ratings_from_coo(raters, np.full(n_rated, n), vals, (m, n + 1))
    o = OracleALS(OracleConfig(n_factors=k, n_iters=1, lambda_u=1.0, lambda_v=3.0, pop_reg_mode=pop_reg,
                               lambda_bu=1.0, lambda_bi=2.0, alpha=alpha, sim={"feature_name": "x", "topk": 5}))
    o.U, o.b_u, o.mu = rng.normal(size=(m, k)), rng.normal(scale=0.3, size=m), 3.2
    o.V = np.vstack([rng.normal(size=(n, k)), np.zeros((1, k))])
    o.b_i = np.zeros(n + 1)
    nb_idx = np.array([2, 5, 11, 17])
    nb_val = np.array([0.9, 0.4, 0.7, 0.05])
    ptr = np.zeros(n + 2, np.int64)
    ptr[n + 1] = nb_idx.size
    o.S_csr, o.use_graph = (ptr, nb_idx, nb_val), alpha > 0
    o.D = np.zeros(n + 1)
    o.D[n] = nb_val.sum()
    o.lambda_v_i = o.item_reg(np.full(n + 1, float(n_rated)))
    o.lambda_bi_i = np.full(n + 1, o.lambda_bi)
    args = (o.U, o.b_u, o.mu, o.V[:n], raters, vals, nb_idx, nb_val, 3.0, pop_reg is not None, 2.0, alpha)
    for T in range(1, 6):
        o.item_step(rt, cols=[n])
        v, b = fold_item_reference(*args, T)
        np.testing.assert_allclose(v, o.V[n], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(b, o.b_i[n], rtol=1e-10, atol=1e-12)
    v, b = fold_item_reference(*args, 0)
    lam = o.lambda_v_i[n] + EPS + alpha * o.D[n]
    Us = o.U[raters]
    M = np.block([[Us.T @ Us + lam * np.eye(k), Us.sum(axis=0)[:, None]],
                  [Us.sum(axis=0)[None, :], np.array([[n_rated + 2.0 + EPS]])]])
    rhs = np.append(Us.T @ (vals - o.mu - o.b_u[raters]) + alpha * (nb_val @ o.V[nb_idx]),
                    (vals - o.mu - o.b_u[raters]).sum())
    x = np.linalg.solve(M, rhs)
    np.testing.assert_allclose(v, x[:k], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(b, x[k], rtol=1e-10, atol=1e-12)
    for _ in range(300):
        o.item_step(rt, cols=[n])
    np.testing.assert_allclose(o.V[n], x[:k], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(o.b_i[n], x[k], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("pop_reg", [False, True])
@pytest.mark.parametrize("alpha", [0.0, 0.5])
def test_zero_rating_item_is_the_graph_mean(pop_reg, alpha):
    """No ratings: A = lambda_i I, h = 0, so v = alpha sum_j s_j V_j / lambda_i and b = 0 for every T (v = 0 without
    a graph) - the minimiser the fit would skip."""
    rng = np.random.default_rng(3)
    V = rng.normal(size=(20, 5))
    nb_idx, nb_val = np.array([1, 4, 9]), np.array([0.5, 0.25, 0.8])
    lam = (3.0 if pop_reg else 3.0) + EPS + alpha * nb_val.sum()      # lambda_v / sqrt(0 + 1) = lambda_v
    for T in (0, 1, 4):
        v, b = fold_item_reference(np.zeros((2, 5)), np.zeros(2), 3.0, V, np.zeros(0, np.int64), np.zeros(0),
                                   nb_idx, nb_val, 3.0, pop_reg, 2.0, alpha, T)
        np.testing.assert_allclose(v, alpha * (nb_val @ V[nb_idx]) / lam, rtol=1e-13, atol=0)
        assert b == 0.0


# ------------------------------------------------------------------------------------------ validation
def test_new_item_features_validation():
    from collaborative_filtering_amd.als import new_item_features
    dims = {"genres": 3, "year": 1}
    ok = {"genres": np.zeros((4, 3)), "year": np.ones((4, 1))}
    out = new_item_features(ok, dims, 4)
    assert set(out) == set(dims)
    assert new_item_features(None, {}, 2) == {}
    bad = [
        ({"genres": np.zeros((4, 2)), "year": np.ones((4, 1))}, "shape"),                 # wrong width
        ({"genres": np.zeros((3, 3)), "year": np.ones((4, 1))}, "shape"),                 # wrong row count
        ({"genres": np.zeros((4, 3))}, "missing"),                                         # missing feature
        ({**ok, "extra": np.zeros((4, 1))}, "not fitted"),                                 # unknown feature
        ({"genres": np.zeros((4, 3)), "year": np.array([[1.0], [np.nan], [0], [0]])}, "non-finite"),
        ({"genres": np.full((4, 3), np.inf), "year": np.ones((4, 1))}, "non-finite"),
    ]
    for feats, msg in bad:
        with pytest.raises(ValueError, match=msg):
            new_item_features(feats, dims, 4)


def test_new_item_graph_validation():
    from collaborative_filtering_amd.als import new_item_graph_csr
    ptr, idx, val = new_item_graph_csr(([0, 2, 2, 3], [4, 1, 0], [0.5, 0.25, 1.0]), 3, 5)
    assert ptr.dtype == np.int64 and idx.dtype == np.int32 and val.dtype == np.float32
    assert ptr.tolist() == [0, 2, 2, 3] and idx.tolist() == [4, 1, 0]
    for S in [([0, 1, 2], [1, 2], [1.0, 1.0]),                   # 2 rows, 3 expected
              ([0, 1, 2, 4], [1, 2, 3], [1.0] * 3),              # ptr ends past nnz
              ([1, 1, 2, 3], [1, 2, 3], [1.0] * 3),              # ptr does not start at 0
              ([0, 2, 1, 3], [1, 2, 3], [1.0] * 3),              # decreasing ptr
              ([0, 1, 2, 3], [1, 5, 3], [1.0] * 3),              # index >= n
              ([0, 1, 2, 3], [1, -1, 3], [1.0] * 3),             # index < 0
              ([0, 1, 2, 3], [1, 2, 3], [1.0, np.nan, 1.0]),     # non-finite weight
              ([0, 1, 2, 3], [1, 2, 3], [1.0, 1.0]),             # lengths differ
              ([0, 1, 2, 3], [1.0, 2.0, 3.0], [1.0] * 3),        # float indices
              ([0, 1], [1]),                                     # not a triple
              ]:
        with pytest.raises(ValueError):
            new_item_graph_csr(S, 3, 5)


@pytest.fixture(scope="module")
def fitted_graph():
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, GraphConfig, GraphSimConfig
    from tests.cpu_backend import NumpyBackend
    from tests.synth import make_features, make_ratings
    r, c, v = make_ratings(30, 20, 200, seed=4)
    G, y = make_features(20, seed=5)
    cfg = ALSConfig(core=CoreConfig(n_factors=4, n_iters=2, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0),
                    graph=GraphConfig(alpha=0.5, sim=GraphSimConfig(topk=5)))
    model = ALS(cfg, {"genres": 1.0, "year": 1.0}, device="cpu", backend=NumpyBackend())
    model.fit_coo(r, c, v, (30, 20), features={"genres": G, "year": y}, tol=None, verbose=0)
    return model, G, y


def test_model_boundary_rejections(fitted_graph):
    model, G, y = fitted_graph
    fn = {"genres": G[:3], "year": y[:3]}
    assert model._eng.use_graph
    with pytest.raises(ValueError, match="needs"):
        model.fold_in_items()                                        # nothing to fold in
    with pytest.raises(ValueError, match="missing"):
        model.fold_in_items(features_new={"genres": G[:3]})
    with pytest.raises(ValueError, match="shape"):
        model.fold_in_items(features_new={"genres": G[:3, :5], "year": y[:3]})
    with pytest.raises(ValueError, match="disagree"):
        model.fold_in_items(np.full((2, 30), np.nan), features_new=fn)
    with pytest.raises(ValueError):
        model.fold_in_items(np.full((3, 29), np.nan), features_new=fn)   # wrong rating width
    with pytest.raises(ValueError, match="non-finite"):
        model.fold_in_items(features_new={"genres": np.full((3, 19), np.nan), "year": y[:3]})
    with pytest.raises(ValueError):
        model.fold_in_items(features_new=fn, S_new=([0, 1, 1], [3], [1.0]))   # 2 rows for 3 items
    with pytest.raises(ValueError):
        model.fold_in_items(features_new=fn, S_new=([0, 1, 1, 1], [20], [1.0]))   # index beyond the fit
    with pytest.raises(ValueError):
        model.fold_in_items(features_new=fn, n_sweeps=0)
    with pytest.raises(ValueError):
        model.fold_in_items(features_new=fn, features={"genres": G[:7]})   # fitted sim feature of the wrong size


def test_graph_needs_the_sim_feature_or_S_new():
    """A fit whose graph came from S= has no sim feature: the new items' graph rows must be passed."""
    from collaborative_filtering_amd import ALS, ALSConfig, CoreConfig, GraphConfig, GraphSimConfig
    from tests.cpu_backend import NumpyBackend
    from tests.synth import make_ratings
    r, c, v = make_ratings(30, 20, 200, seed=4)
    S = np.zeros((20, 20))
    S[0, 1] = S[1, 0] = 0.5
    ptr, idx = np.array([0, 1, 2] + [2] * 18, np.int64), np.array([1, 0], np.int32)
    cfg = ALSConfig(core=CoreConfig(n_factors=4, n_iters=1, lambda_u=2.0, lambda_v=2.0),
                    graph=GraphConfig(alpha=0.5, sim=GraphSimConfig(topk=5)))
    model = ALS(cfg, device="cpu", backend=NumpyBackend())
    model.fit_coo(r, c, v, (30, 20), tol=None, verbose=0, S=(ptr, idx, np.array([0.5, 0.5], np.float32)))
    assert model._eng.use_graph
    with pytest.raises(ValueError, match="S_new"):
        model.fold_in_items(np.full((2, 30), np.nan))
    plain = ALS(ALSConfig(core=CoreConfig(n_factors=4, n_iters=1, lambda_u=2.0, lambda_v=2.0)), device="cpu",
                backend=NumpyBackend()).fit_coo(r, c, v, (30, 20), tol=None, verbose=0)
    with pytest.raises(ValueError, match="without a similarity graph"):
        plain.fold_in_items(np.full((1, 30), np.nan), S_new=([0, 1], [0], [1.0]))
    with pytest.raises(ValueError, match="not fitted"):
        plain.fold_in_items(features_new={"genres": np.zeros((1, 19))})


def test_unfitted_model_raises_like_predict():
    from collaborative_filtering_amd import ALS, ALSConfig, CoreConfig
    from tests.cpu_backend import NumpyBackend
    model = ALS(ALSConfig(core=CoreConfig(n_factors=3, n_iters=1, lambda_u=1.0, lambda_v=1.0)), device="cpu",
                backend=NumpyBackend())
    with pytest.raises(RuntimeError, match="Model must be fitted before prediction."):
        model.fold_in_items(np.full((1, 4), np.nan))


# ------------------------------------------------------------------------------------------ graph rows
def _f64_topk(Xn_new, Xn_fit, topk):
    S = Xn_new @ Xn_fit.T
    rows = []
    for b in range(S.shape[0]):
        o = np.lexsort((np.arange(S.shape[1]), -S[b]))
        o = o if topk is None else o[:topk]
        o = o[S[b, o] > 0]
        rows.append((o, S[b, o]))
    return rows


@pytest.mark.parametrize("topk", [None, 7, 200, 1000])
def test_torch_graph_rows_against_float64_topk(topk):
    import torch
    from collaborative_filtering_amd import layout
    rng = np.random.default_rng(topk or 0)
    X_fit = rng.normal(size=(300, 12)) + 0.3
    X_new = np.vstack([rng.normal(size=(9, 12)) + 0.3, np.zeros((1, 12))])     # a zero row has no neighbours
    ptr, idx, val = layout.similarity_rows_torch(layout.normalize_rows_f32(X_new, 1e-10, "cpu"),
                                                 layout.normalize_rows_f32(X_fit, 1e-10, "cpu"), topk, block=4)
    assert ptr.dtype == torch.int64 and idx.dtype == torch.int32 and val.dtype == torch.float32
    n64 = lambda X: X / (np.sqrt((X * X).sum(1, keepdims=True)) + 1e-10)    # noqa: E731
    exp = _f64_topk(n64(X_new), n64(X_fit), topk)
    ptr, idx, val = ptr.numpy(), idx.numpy(), val.numpy()
    assert ptr[-1] == ptr[-2]                                                  # the zero row
    for b, (ei, ev) in enumerate(exp):
        gi, gv = idx[ptr[b]: ptr[b + 1]], val[ptr[b]: ptr[b + 1]]
        # continuous features: no ties within fp32 rounding, so the lists agree; values to fp32 rounding
        assert gi.tolist() == ei.tolist(), b
        np.testing.assert_allclose(gv, ev, rtol=0, atol=2e-6)
        assert (np.diff(gv) <= 0).all() and (gv > 0).all()


def test_torch_graph_rows_break_ties_by_index():
    import torch
    from collaborative_filtering_amd import layout
    X_fit = torch.tensor([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0], [1.0, 0.0], [-1.0, 0.0]])
    X_new = torch.tensor([[1.0, 0.0], [0.0, -1.0]])
    ptr, idx, val = layout.similarity_rows_torch(X_new, X_fit, 2)
    assert ptr.tolist() == [0, 2, 2] and idx.tolist() == [0, 2] and val.tolist() == [1.0, 1.0]
