"""ALS.recommend host logic and cv.ranking_at_k, without a GPU: the engine runs on the numpy stand-in backend, whose
recommend_topk is the kernel's contract in tests/serving_ref.py (`topn`) over predict_dense scores."""
import numpy as np
import pytest

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, cv
from tests.cpu_backend import NumpyBackend
from tests.synth import make_ratings


M, N_ITEMS = 30, 25


@pytest.fixture(scope="module")
def fitted():
    r, c, v = make_ratings(M, N_ITEMS, 300, seed=3, empty_users=(4,))
    cfg = ALSConfig(core=CoreConfig(n_factors=5, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    model = ALS(cfg, device="cpu", backend=NumpyBackend()).fit_coo(r, c, v, (M, N_ITEMS), tol=None, verbose=0)
    return model, r, c


def test_recommend_before_fit_raises_like_predict():
    cfg = ALSConfig(core=CoreConfig(n_factors=3, n_iters=1, lambda_u=1.0, lambda_v=1.0))
    model = ALS(cfg, device="cpu", backend=NumpyBackend())
    with pytest.raises(RuntimeError, match="Model must be fitted before prediction."):
        model.recommend()


def test_shapes_dtypes_and_all_users(fitted):
    model, r, c = fitted
    items, scores = model.recommend(None, 4)
    assert items.shape == scores.shape == (M, 4)
    assert items.dtype == np.int64 and scores.dtype == np.float64
    P = model.predict()
    for u in range(M):
        seen = c[r == u]
        assert not np.isin(items[u], seen).any()
        assert (scores[u] == P[u, items[u]]).all()
        cand = np.setdiff1d(np.arange(N_ITEMS), seen)
        assert (np.sort(P[u, cand])[::-1][:4] == scores[u]).all()


def test_subset_order_duplicates_and_padding(fitted):
    model, r, c = fitted
    sub = [7, 2, 7, 0]
    items, scores = model.recommend(sub, 3)
    full_i, full_s = model.recommend(None, 3)
    assert (items == full_i[sub]).all() and (scores == full_s[sub]).all()
    items, scores = model.recommend(np.array([0, 1]), 128)              # N > n - seen: padded
    nseen = np.array([np.unique(c[r == u]).size for u in (0, 1)])
    for b in range(2):
        valid = N_ITEMS - nseen[b]
        assert (items[b, :valid] >= 0).all() and (items[b, valid:] == -1).all()
        assert np.isneginf(scores[b, valid:]).all()
    items, _ = model.recommend([4], 3, exclude_seen=False)               # a user without ratings works either way
    assert (items >= 0).all()
    items, _ = model.recommend(np.array([], dtype=np.int64), 5)
    assert items.shape == (0, 5)


def test_exclude_seen_false_ranks_every_item(fitted):
    model, r, c = fitted
    items, scores = model.recommend([0], N_ITEMS, exclude_seen=False)
    P = model.predict()
    assert (np.sort(items[0]) == np.arange(N_ITEMS)).all()
    assert (scores[0] == np.sort(P[0])[::-1]).all()


@pytest.mark.parametrize("N", [0, 129, -1, 2.0, True])
def test_bad_N(fitted, N):
    with pytest.raises(ValueError):
        fitted[0].recommend(None, N)


@pytest.mark.parametrize("users", [[M], [-1], [0, M + 5]])
def test_out_of_range_user(fitted, users):
    with pytest.raises(IndexError):
        fitted[0].recommend(users, 3)


def test_bad_users_shape_and_features(fitted):
    model = fitted[0]
    with pytest.raises(ValueError):
        model.recommend([[0, 1]], 3)
    with pytest.raises(ValueError, match="rows"):
        model.recommend(None, 3, features={"genres": np.zeros((N_ITEMS + 1, 2))})
    with pytest.raises(ValueError, match="infinite"):
        model.recommend(None, 3, features={"genres": np.full((N_ITEMS, 2), np.inf)})


# ------------------------------------------------------------------------------------------ ranking_at_k
class _Fixed:
    """A model stand-in whose recommendations are fixed lists."""

    def __init__(self, lists, n):
        self.lists = {u: list(l) for u, l in lists.items()}
        self.V = np.zeros((n, 1))

    def recommend(self, users, N, features=None):
        out = np.full((len(users), N), -1, np.int64)
        for b, u in enumerate(users):
            l = self.lists[int(u)][:N]
            out[b, : len(l)] = l
        return out, np.where(out >= 0, 1.0, -np.inf)


def _brute(lists, held, K):
    rec, nd = [], []
    for u, rel in held.items():
        if not rel:
            continue
        top = lists[u][:K]
        hits = [i in rel for i in top]
        rec.append(sum(hits) / len(rel))
        dcg = sum(h / np.log2(r + 2) for r, h in enumerate(hits))
        idcg = sum(1 / np.log2(r + 2) for r in range(min(K, len(rel))))
        nd.append(dcg / idcg)
    return len(rec), float(np.mean(rec)), float(np.mean(nd))


def test_ranking_perfect_and_hand_computed():
    lists = {0: [3, 1, 4, 0], 1: [2, 0, 1, 3]}
    rows, cols = np.array([0, 0, 1]), np.array([3, 1, 2])
    res = cv.ranking_at_k(_Fixed(lists, 5), rows, cols, K=2)
    assert res == {"users": 2, "recall@K": 1.0, "ndcg@K": 1.0}
    # user 0: relevant {1, 4}, list [3, 1, 4]: hits at ranks 2 and 3
    res = cv.ranking_at_k(_Fixed(lists, 5), [0, 0], [1, 4], K=3)
    dcg = 1 / np.log2(3) + 1 / np.log2(4)
    idcg = 1 + 1 / np.log2(3)
    assert res["users"] == 1 and res["recall@K"] == 1.0
    assert res["ndcg@K"] == pytest.approx(dcg / idcg, rel=1e-12)
    assert res["ndcg@K"] == pytest.approx(0.693426, abs=1e-6)           # (1/log2 3 + 1/2) / (1 + 1/log2 3)


def test_ranking_min_rating_and_brute_force():
    rng = np.random.default_rng(0)
    n, m = 40, 25
    lists = {u: list(rng.permutation(n)[:15]) for u in range(m)}
    rows = rng.integers(0, m, 200)
    cols = rng.integers(0, n, 200)
    vals = rng.integers(1, 6, 200).astype(float)
    for K in (1, 5, 15):
        for thr in (None, 4.0):
            keep = np.ones(rows.size, bool) if thr is None else vals >= thr
            held = {u: set(cols[keep & (rows == u)].tolist()) for u in range(m)}
            users, rec, nd = _brute(lists, held, K)
            res = cv.ranking_at_k(_Fixed(lists, n), rows, cols, vals, K=K, min_rating=thr)
            assert res["users"] == users
            assert res["recall@K"] == pytest.approx(rec, rel=1e-12)
            assert res["ndcg@K"] == pytest.approx(nd, rel=1e-12)
    with pytest.raises(ValueError):
        cv.ranking_at_k(_Fixed(lists, n), rows, cols, None, K=5, min_rating=3.0)
    res = cv.ranking_at_k(_Fixed(lists, n), rows, cols, vals, K=5, min_rating=9.0)
    assert res["users"] == 0 and np.isnan(res["recall@K"])


def test_ranking_on_a_fitted_model(fitted):
    model, r, c = fitted
    res = cv.ranking_at_k(model, r[:40], c[:40], K=5)
    assert res["users"] == np.unique(r[:40]).size
    assert res["recall@K"] == 0.0 and res["ndcg@K"] == 0.0               # training items are never recommended
