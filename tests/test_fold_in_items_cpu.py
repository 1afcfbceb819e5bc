"""Item fold-in without a GPU: the C struct mirror, the zero-rating closed form of the contract (`fold_in_item` of
tests/serving_ref.py; its equivalence to the fit's item half-step is checked in tests/test_serving_ref_cpu.py), the
input validation of ALS.fold_in_items, and the torch formulation of the new items' graph rows."""
import os

import numpy as np
import pytest

from tests.serving_ref import EPS, fold_in_item

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
        v, b = fold_in_item(np.zeros((2, 5)), np.zeros(2), 3.0, V, np.zeros(0, np.int64), np.zeros(0), nb_idx, nb_val,
                            3.0, pop_reg, 2.0, alpha, T)
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
