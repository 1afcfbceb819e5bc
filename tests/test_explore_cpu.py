"""ALS.recommend_explore / recommend_new_explore / cv.explore_at_k host logic, without a GPU: the engine runs on the
numpy stand-in backend, whose row_whitener / explore_topk are the kernels' contract in tests/explore_ref.py.  The
expected lists are written out again here from `predict`, the training rows and the fp64 whitener."""
import numpy as np
import pytest

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, cv, validate
from tests import explore_ref as xref
from tests import serving_ref as ref
from tests.synth import make_features, make_ratings

M, N_ITEMS, K = 30, 25, 5
LAM_U = 2.0
NOTHING, EVERYTHING = 4, 11         # a user without a rating, a user who rated every item


def _ratings():
    r, c, v = make_ratings(M, N_ITEMS, 220, seed=3, empty_users=(NOTHING,))
    keep = r != EVERYTHING
    r, c, v = r[keep], c[keep], v[keep]
    r = np.concatenate([r, np.full(N_ITEMS, EVERYTHING)])
    c = np.concatenate([c, np.arange(N_ITEMS)])
    v = np.concatenate([v, 3.0 + 0.5 * (np.arange(N_ITEMS) % 4)])
    o = np.lexsort((c, r))
    return r[o], c[o], v[o]


def _fit(features=None):
    r, c, v = _ratings()
    cfg = ALSConfig(core=CoreConfig(n_factors=K, n_iters=3, lambda_u=LAM_U, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    be = xref.ExploreNumpyBackend()
    kw = dict(lambda_w={f: 1.0 for f in features}) if features else {}
    model = ALS(cfg, device="cpu", backend=be, **kw)
    model.fit_coo(r, c, v, (M, N_ITEMS), features=features, tol=None, verbose=0)
    return model, be, [c[r == u] for u in range(M)]


@pytest.fixture(scope="module")
def fitted():
    return _fit()


@pytest.fixture(scope="module")
def fitted_feat():
    G, y = make_features(N_ITEMS, seed=4)
    feats = {"genres": G, "years": y}
    return _fit(feats) + (feats,)


USERS = np.array([7, 0, NOTHING, 7, 29, EVERYTHING, 3, 0, 12, 13, 14])


def _brute(Z, rows, N, beta, ok=None, exclude=True):
    """(items, keys, leverage) of batch rows [(base row of P, rated items)]: the key by the docstring of
    ALS.recommend_explore from the fp64 whitener rounded to fp32."""
    keys, levs, seen = [], [], []
    lam = float(np.float32(LAM_U)) + ref.EPS
    for base, S in rows:
        W = xref.whitener(Z, S, lam, K)[0].astype(np.float32).astype(np.float64)
        y = Z[:, :K].astype(np.float64) @ W.T
        lev = (y * y).sum(axis=1).astype(np.float32)
        keys.append(xref.key_f32(base.astype(np.float32), beta, lev))
        levs.append(lev)
        seen.append(np.asarray(S, np.int64) if exclude else np.zeros(0, np.int64))
    tv, ti, tc = ref.topn_batch(np.stack(keys), seen, ok, N)
    tl = np.where(ti >= 0, np.take_along_axis(np.stack(levs), np.maximum(ti, 0).astype(np.int64), axis=1), 0)
    return ti.astype(np.int64), tv.astype(np.float64), tl.astype(np.float64)


def _same(got, exp):
    for g, e in zip(got, exp):
        assert g.shape == e.shape and (g == e).all()


# ------------------------------------------------------------------------------------------------ validation
def test_explore_args():
    assert validate.explore_args(1, "ucb", None) == (1.0, None)
    assert validate.explore_args(np.float32(-0.5), "thompson", np.int64(3)) == (-0.5, 3)
    for beta in (np.nan, np.inf, -np.inf, "1", None, True):
        with pytest.raises(ValueError, match="beta must be a finite number"):
            validate.explore_args(beta, "ucb", None)
    for mode in ("UCB", "ts", None, 1):
        with pytest.raises(ValueError, match="mode must be one of"):
            validate.explore_args(1.0, mode, None)
    for seed in (-1, 1.5, "0", True):
        with pytest.raises(ValueError, match="seed must be a non-negative integer"):
            validate.explore_args(1.0, "thompson", seed)
    with pytest.raises(ValueError, match="needs a seed"):
        validate.explore_args(1.0, "thompson", None)
    with pytest.raises(ValueError, match="only used with"):
        validate.explore_args(1.0, "ucb", 3)
    with pytest.raises(ValueError, match="new_items is not supported"):
        validate.explore_args(1.0, "ucb", None, new_items=object())


def test_facade_rejections(fitted):
    model = fitted[0]
    with pytest.raises(ValueError, match="new_items"):
        model.recommend_explore([0], 3, new_items=object())
    with pytest.raises(ValueError, match="new_items"):
        model.recommend_new_explore((np.array([0, 1]), np.array([2]), np.array([4.0])), 3, new_items=object())
    with pytest.raises(ValueError, match="N must be an integer"):
        model.recommend_explore([0], 0)
    with pytest.raises(ValueError, match="beta"):
        model.recommend_explore([0], 3, beta=float("nan"))
    with pytest.raises(IndexError):
        model.recommend_explore([M], 3)
    with pytest.raises(ValueError, match="needs a seed"):
        model.recommend_new_explore((np.array([0, 1]), np.array([2]), np.array([4.0])), 3, mode="thompson")
    out = model.recommend_explore([], 4, return_leverage=True)
    assert [o.shape for o in out] == [(0, 4)] * 3
    assert len(model.recommend_explore([], 4)) == 2


# ------------------------------------------------------------------------------------------------ the lists
def test_beta_zero_is_recommend(fitted):
    model = fitted[0]
    for N in (1, 7, 25):
        _same(model.recommend_explore(USERS, N, beta=0.0), model.recommend(USERS, N))
    _same(model.recommend_explore(None, 5, beta=0.0, exclude_seen=False), model.recommend(None, 5, exclude_seen=False))


@pytest.mark.parametrize("beta", [-1.0, 0.5, 2.0])
def test_lists_are_the_brute_force_lists_in_caller_order(fitted, beta, monkeypatch):
    model, be, seen = fitted
    P, Z = model.predict(), model.V
    exp = _brute(Z, [(P[u], seen[u]) for u in USERS], 6, beta)
    _same(model.recommend_explore(USERS, 6, beta=beta, return_leverage=True), exp)
    assert (exp[0][list(USERS).index(EVERYTHING)] == -1).all()              # rated everything: an empty list
    assert (exp[0][1] == exp[0][7]).all()                                   # the duplicates of user 0
    monkeypatch.setattr(model._eng, "EXPLORE_BATCH", 3, raising=False)      # 11 rows: four chunks
    del be.calls[:]
    _same(model.recommend_explore(USERS, 6, beta=beta, return_leverage=True), exp)
    assert [c[1] for c in be.calls if c[0] == "explore_topk"] == [3, 3, 3, 2]
    assert [c[1] for c in be.calls if c[0] == "row_whitener"] == [3, 3, 3, 2]
    _same(model.recommend_explore(USERS, 6, beta=beta, exclude_seen=False, return_leverage=True),
          _brute(Z, [(P[u], seen[u]) for u in USERS], 6, beta, exclude=False))


def test_empty_user_convention(fitted):
    model = fitted[0]
    items, keys, lev = model.recommend_explore([NOTHING], N_ITEMS, beta=1.0, return_leverage=True)
    assert (items[0] >= 0).all()
    lam = float(np.float32(LAM_U)) + ref.EPS
    exp = (model.V[items[0]].astype(np.float64) ** 2).sum(axis=1) / lam
    assert np.allclose(lev[0], exp, rtol=1e-6, atol=0)


def test_filters(fitted):
    model, _, seen = fitted
    P, Z = model.predict(), model.V
    allow = np.array([1, 2, 3, 5, 8, 13, 21, 3])
    block = np.array([5, 24])
    ok = np.zeros(N_ITEMS, bool)
    ok[allow] = True
    ok[block] = False
    exp = _brute(Z, [(P[u], seen[u]) for u in USERS], 4, 0.5, ok=ok)
    _same(model.recommend_explore(USERS, 4, beta=0.5, items=allow, filter_items=block, return_leverage=True), exp)
    none = model.recommend_explore(USERS, 4, beta=0.5, items=np.zeros(0, np.int64))
    assert (none[0] == -1).all() and np.isneginf(none[1]).all()


def test_features_decide_z(fitted_feat):
    model, _, seen, feats = fitted_feat
    P = model.predict(feats)
    Z = model.V + sum(np.asarray(feats[f], np.float64) @ model.W[f] for f in feats)
    Z = Z.astype(np.float32).astype(np.float64)
    got = model.recommend_explore(USERS, 5, beta=1.0, features=feats, return_leverage=True)
    exp = _brute(Z, [(P[u], seen[u]) for u in USERS], 5, 1.0)
    assert (got[0] == exp[0]).all()
    assert np.allclose(got[2], exp[2], rtol=1e-5, atol=0)


def test_new_rows(fitted, monkeypatch):
    model, be, _ = fitted
    rng = np.random.default_rng(5)
    lens = [0, 1, 3, 8, N_ITEMS, 2, 5]
    rows = [np.sort(rng.permutation(N_ITEMS)[:L]) for L in lens]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate(rows).astype(np.int32)
    vals = (rng.integers(1, 11, size=idx.size) * 0.5).astype(np.float32)
    R = (ptr, idx, vals)
    _same(model.recommend_new_explore(R, 6, beta=0.0), model.recommend_new(R, 6))
    monkeypatch.setattr(model._eng, "EXPLORE_BATCH", 3, raising=False)
    got = model.recommend_new_explore(R, 6, beta=2.0, return_leverage=True)
    # the base of a folded row is the kernel epilogue on the folded factors: read it off the beta = 0 call
    it0, sc0 = model.recommend_new(R, N_ITEMS, exclude_seen=False)
    for b in range(len(lens)):
        P_b = np.full(N_ITEMS, np.nan)
        P_b[it0[b]] = sc0[b]
        exp = _brute(model.V, [(P_b, rows[b])], 6, 2.0)
        _same([g[b: b + 1] for g in got], exp)
    assert (got[0][4] == -1).all()                                          # rated everything


def test_thompson(fitted, monkeypatch):
    model, _, seen = fitted
    a = model.recommend_explore(USERS, 6, beta=1.0, mode="thompson", seed=3, return_leverage=True)
    b = model.recommend_explore(USERS, 6, beta=1.0, mode="thompson", seed=3, return_leverage=True)
    c = model.recommend_explore(USERS, 6, beta=1.0, mode="thompson", seed=4)
    _same(a, b)
    assert (a[0] != c[0]).any() and (a[1] != c[1]).any()
    monkeypatch.setattr(model._eng, "EXPLORE_BATCH", 4, raising=False)       # the draw does not depend on the chunks
    _same(model.recommend_explore(USERS, 6, beta=1.0, mode="thompson", seed=3, return_leverage=True), a)
    _same(model.recommend_explore(USERS, 6, beta=0.0, mode="thompson", seed=9), model.recommend(USERS, 6))
    # the sampled table, written out: u + beta W^T eps, scored by the predict epilogue
    eps = np.random.default_rng(3).standard_normal((USERS.size, K)).astype(np.float32)
    lam = float(np.float32(LAM_U)) + ref.EPS
    for r, u in enumerate(USERS):
        W = xref.whitener(model.V, seen[u], lam, K)[0].astype(np.float32)
        ut = model.U[u].astype(np.float32) + np.float32(1.0) * (W.T @ eps[r])
        s = ut.astype(np.float64) @ model.V.T + model.mu + model.b_u[u] + model.b_i
        filled = a[0][r] >= 0
        assert np.allclose(a[1][r][filled], s[a[0][r][filled]], rtol=1e-5, atol=1e-5)
        y = model.V[a[0][r][filled]] @ W.astype(np.float64).T
        assert np.allclose(a[2][r][filled], (y * y).sum(axis=1), rtol=1e-5, atol=0)
        assert not np.isin(a[0][r][filled], seen[u]).any()


def test_leverage_is_explains(fitted):
    model = fitted[0]
    users = np.array([0, 7, 12, NOTHING, 29])
    items, _, lev = model.recommend_explore(users, 5, beta=1.0, return_leverage=True)
    us = np.repeat(users, 5)
    e = model.explain(us, items.reshape(-1), 3)
    assert np.allclose(lev.reshape(-1), e.leverage, rtol=1e-5, atol=0)


# ------------------------------------------------------------------------------------------------ cv.explore_at_k
def test_explore_at_k_arithmetic(fitted):
    model = fitted[0]
    rng = np.random.default_rng(8)
    rows = rng.integers(0, M, 60)
    cols = rng.integers(0, N_ITEMS, 60)
    out = cv.explore_at_k(model, rows, cols, K=4, betas=(0.0, 1.5))
    base = cv.ranking_at_k(model, rows, cols, K=4)
    assert out["users"] == base["users"] and [e["beta"] for e in out["betas"]] == [0.0, 1.5]
    assert out["betas"][0]["recall@K"] == base["recall@K"] and out["betas"][0]["ndcg@K"] == base["ndcg@K"]
    users = np.unique(rows)
    for e in out["betas"]:
        top, _, lev = model.recommend_explore(users, 4, beta=e["beta"], return_leverage=True)
        assert e["leverage@K"] == float(lev[top >= 0].mean())
        assert e["coverage@K"] == np.unique(top[top >= 0]).size / N_ITEMS
    assert out["betas"][1]["leverage@K"] > out["betas"][0]["leverage@K"]
    f = cv.explore_at_k(model, rows, cols, K=4, betas=(1.0,), filter_items=np.arange(5))
    assert f["filtered_out"] == int((cols < 5).sum())
    top = model.recommend_explore(np.unique(rows[cols >= 5]), 4, beta=1.0, filter_items=np.arange(5))[0]
    assert f["betas"][0]["coverage@K"] == np.unique(top[top >= 0]).size / (N_ITEMS - 5)
    empty = cv.explore_at_k(model, np.zeros(0, np.int64), np.zeros(0, np.int64), K=4)
    assert empty["users"] == 0 and all(np.isnan(e["recall@K"]) for e in empty["betas"])
