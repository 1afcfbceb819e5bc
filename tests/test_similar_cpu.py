"""ALS.similar_items / similar_users host logic, without a GPU: the engine runs on the numpy stand-in backend, whose
row_inv_norms / similar_topk are the kernels' contract in tests/similar_ref.py."""
import numpy as np
import pytest

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig
from tests import similar_ref as sref
from tests.similar_ref import SimilarNumpyBackend
from tests.synth import make_features, make_ratings

M, N_ITEMS, K = 30, 25, 5


def _fit(features=None):
    r, c, v = make_ratings(M, N_ITEMS, 300, seed=3, empty_users=(4,))
    cfg = ALSConfig(core=CoreConfig(n_factors=K, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    be = SimilarNumpyBackend()
    kw = dict(lambda_w={f: 1.0 for f in features}) if features else {}
    model = ALS(cfg, device="cpu", backend=be, **kw)
    model.fit_coo(r, c, v, (M, N_ITEMS), features=features, tol=None, verbose=0)
    return model, be


@pytest.fixture(scope="module")
def fitted():
    return _fit()


@pytest.fixture(scope="module")
def fitted_feat():
    G, y = make_features(N_ITEMS, seed=4)
    feats = {"genres": G, "years": y}
    return _fit(feats) + (feats,)


def _expected(T, ids, N, ok=None):
    """similar_ref on a table (torch fp32 [rows, ld]): every row of `ids` against all rows, itself excluded."""
    T = T.numpy()
    inv = sref.inv_norms(T).astype(np.float32)
    dots = (T[ids].astype(np.float64) @ T.astype(np.float64).T).astype(np.float32)
    tv, ti, tc = sref.similar_topn(dots, inv[ids], inv, ids, ok, N)
    return ti.astype(np.int64), tv.astype(np.float64), tc


def _same(got, exp):
    assert (got[0] == exp[0]).all() and (got[1] == exp[1]).all()


def test_before_fit_raises_like_recommend():
    cfg = ALSConfig(core=CoreConfig(n_factors=3, n_iters=1, lambda_u=1.0, lambda_v=1.0))
    model = ALS(cfg, device="cpu", backend=SimilarNumpyBackend())
    for call in (model.similar_items, model.similar_users):
        with pytest.raises(RuntimeError, match="Model must be fitted before prediction."):
            call()


def test_shapes_dtypes_and_none_means_all(fitted):
    model, be = fitted
    for call, rows, T in ((model.similar_items, N_ITEMS, model._eng.V), (model.similar_users, M, model._eng.U)):
        ids, sims = call(None, 4)
        assert ids.shape == sims.shape == (rows, 4)
        assert ids.dtype == np.int64 and sims.dtype == np.float64
        _same((ids, sims), _expected(T, np.arange(rows), 4))
        assert (ids != np.arange(rows)[:, None]).all()                  # never its own neighbour
        assert (np.diff(sims, axis=1) <= 0).all() and (np.abs(sims) <= 1 + 1e-6).all()
        default = call()
        assert default[0].shape == (rows, 10)


def test_sims_are_the_cosines_of_the_rows(fitted):
    model, be = fitted
    ids, sims = model.similar_items(None, N_ITEMS - 1)
    V = model._eng.V.numpy()[:, :K].astype(np.float64)
    Vn = V / np.linalg.norm(V, axis=1, keepdims=True)
    cos = Vn @ Vn.T
    assert np.abs(sims - cos[np.arange(N_ITEMS)[:, None], ids]).max() < (K + 8) * 2.0 ** -24
    assert (np.sort(ids, axis=1) == np.array([np.delete(np.arange(N_ITEMS), i) for i in range(N_ITEMS)])).all()


def test_subset_order_duplicates_and_padding(fitted):
    model, be = fitted
    sub = [7, 2, 7, 0]
    full = model.similar_items(None, 3)
    got = model.similar_items(sub, 3)
    _same(got, (full[0][sub], full[1][sub]))
    full = model.similar_users(None, 3)
    _same(model.similar_users(np.array(sub), 3), (full[0][sub], full[1][sub]))
    ids, sims = model.similar_items([0, 1], 128)                        # N > n - 1: padded
    assert (ids[:, : N_ITEMS - 1] >= 0).all() and (ids[:, N_ITEMS - 1:] == -1).all()
    assert np.isfinite(sims[:, : N_ITEMS - 1]).all() and np.isneginf(sims[:, N_ITEMS - 1:]).all()
    ids, sims = model.similar_items(np.array([], dtype=np.int64), 5)
    assert ids.shape == sims.shape == (0, 5) and ids.dtype == np.int64 and sims.dtype == np.float64
    assert model.similar_users([], 7)[0].shape == (0, 7)


def test_allow_and_block_lists_as_ids_and_masks(fitted):
    model, be = fitted
    rng = np.random.default_rng(0)
    allow = rng.permutation(N_ITEMS)[:9]
    block = rng.random(N_ITEMS) < 0.3
    q = np.array([3, 24, 3, int(allow[0])])
    cases = [(dict(allow_items=allow), np.isin(np.arange(N_ITEMS), allow)),
             (dict(allow_items=np.isin(np.arange(N_ITEMS), allow)), np.isin(np.arange(N_ITEMS), allow)),
             (dict(filter_items=np.nonzero(block)[0]), ~block),
             (dict(filter_items=block), ~block),
             (dict(allow_items=np.concatenate([allow, allow[:2]]), filter_items=block),
              np.isin(np.arange(N_ITEMS), allow) & ~block)]
    for kw, ok in cases:
        ids, sims = model.similar_items(q, 6, **kw)
        _same((ids, sims), _expected(model._eng.V, q, 6, ok))
        valid = ids >= 0
        assert ok[ids[valid]].all() and (ids != q[:, None]).all()
    assert (model.similar_items(q, 6, allow_items=allow)[0][3] != allow[0]).all()     # allowed, still not its own
    ids, sims = model.similar_items([1, 2], 5, allow_items=[])           # an empty allow-list
    assert (ids == -1).all() and np.isneginf(sims).all()
    with pytest.raises(ValueError):
        model.similar_items(None, 3, allow_items=[N_ITEMS])
    with pytest.raises(ValueError):
        model.similar_items(None, 3, filter_items=np.zeros(N_ITEMS + 1, bool))


def test_features_decide_z(fitted_feat):
    model, be, feats = fitted_feat
    eng = model._eng
    with_f = model.similar_items(None, 5, features=feats)
    without = model.similar_items(None, 5)
    _same(with_f, _expected(eng._compose_for(feats), np.arange(N_ITEMS), 5))
    _same(without, _expected(eng.V, np.arange(N_ITEMS), 5))
    assert (with_f[0] != without[0]).any()
    with pytest.raises(ValueError, match="rows"):
        model.similar_items(None, 3, features={"genres": np.zeros((N_ITEMS + 1, 2))})


def test_norms_are_computed_once_per_call_on_the_table_of_that_call(fitted_feat):
    model, be, feats = fitted_feat
    del be.calls[:]
    model.similar_items(None, 3)
    model.similar_items([1, 2], 3, features=feats)
    model.similar_users(None, 3)
    norms = [c for c in be.calls if c[0] == "row_inv_norms"]
    assert [c[1] for c in norms] == [N_ITEMS, N_ITEMS, M]
    assert norms[0][2] == model._eng.V.data_ptr() and norms[1][2] != norms[0][2]      # V, then the composed Z
    assert norms[2][2] == model._eng.U.data_ptr()


@pytest.mark.parametrize("N", [0, 129, -1, 2.0, True])
def test_bad_N(fitted, N):
    for call in (fitted[0].similar_items, fitted[0].similar_users):
        with pytest.raises(ValueError):
            call(None, N)


@pytest.mark.parametrize("ids", [[N_ITEMS], [-1], [0, M + 5]])
def test_out_of_range_ids(fitted, ids):
    with pytest.raises(IndexError):
        fitted[0].similar_items(ids, 3)
    with pytest.raises(IndexError):
        fitted[0].similar_users([M if i == N_ITEMS else i for i in ids], 3)
    with pytest.raises(ValueError):
        fitted[0].similar_items([[0, 1]], 3)


def test_chunks_are_crossed(fitted, monkeypatch):
    model, be = fitted
    base_i, base_u = model.similar_items(None, 4), model.similar_users(None, 4)
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)
    del be.calls[:]
    _same(model.similar_items(None, 4), base_i)
    assert [c[1] for c in be.calls if c[0] == "similar_topk"] == [7, 7, 7, 4]
    assert sum(c[0] == "row_inv_norms" for c in be.calls) == 1
    _same(model.similar_users(None, 4), base_u)
    q = np.array([5, 5, 1, 0, 29, 3, 3, 3, 12])
    _same(model.similar_users(q, 4), (base_u[0][q], base_u[1][q]))


def test_zero_and_nan_rows_in_the_reference():
    T = np.zeros((6, 16), np.float32)
    T[:, :3] = [[1, 0, 0], [2, 0, 0], [0, 0, 0], [0, 3, 0], [np.nan, 1, 0], [-1, 0, 0]]
    inv = sref.inv_norms(T)
    assert inv[2] == 0 and np.isnan(inv[4]) and inv[1] == 0.5
    with np.errstate(invalid="ignore"):
        dots = (T.astype(np.float64) @ T.astype(np.float64).T).astype(np.float32)
    ids = np.arange(6)
    tv, ti, tc = sref.similar_topn(dots, inv.astype(np.float32), inv.astype(np.float32), ids, None, 5)
    assert list(ti[0]) == [1, 2, 3, 5, -1] and list(tv[0][:4]) == [1, 0, 0, -1]      # the NaN row never comes back
    assert list(ti[2]) == [0, 1, 3, 5, -1] and (tv[2][:4] == 0).all()                # zero row: sim 0 to everything
    assert tc[4] == 0 and (ti[4] == -1).all() and np.isneginf(tv[4]).all()           # NaN query: empty list
    tv, ti, tc = sref.similar_topn(dots, inv.astype(np.float32), inv.astype(np.float32), None, None, 1)
    assert list(ti[:, 0]) == [0, 0, 0, 3, -1, 5]                                      # no exclusion: self (or a tie) first


def test_library_exports_the_new_symbols():
    import os
    import __graft_entry__ as ge
    from collaborative_filtering_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    lib = _hip.load()
    for name in ("als_row_inv_norms", "als_similar_workspace_bytes", "als_similar_topk"):
        assert hasattr(lib, name)
    assert lib.als_version() == 103
    assert lib.als_similar_workspace_bytes(3, 5003, 10, 1) == 0
    assert lib.als_similar_workspace_bytes(3, 5003, 10, 7) == 7 * 3 * 10 * 8
