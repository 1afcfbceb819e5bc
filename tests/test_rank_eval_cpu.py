"""ALS.rank_of / rank_of_new host logic and cv.rank_metrics / fold_in_rank_metrics, without a GPU: the engine runs on
the numpy stand-in backend, whose rank_count and fold_in are the contracts of als_rank_count and als_fold_in in
tests/serving_ref.py (`rank_counts`, `fold_in_user`) over predict_dense scores."""
import numpy as np
import pytest

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, cv
from tests import serving_ref as ref
from tests.cpu_backend import NumpyBackend
from tests.synth import make_ratings


M, N_ITEMS = 30, 25


def _fit(r, c, v, shape, k=5):
    cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    return ALS(cfg, device="cpu", backend=NumpyBackend()).fit_coo(r, c, v, shape, tol=None, verbose=0)


@pytest.fixture(scope="module")
def fitted():
    r, c, v = make_ratings(M, N_ITEMS, 300, seed=3, empty_users=(4,))
    return _fit(r, c, v, (M, N_ITEMS)), r, c


def _brute_rank(P, seen, u, t):
    """(rank, candidates) of item t for user u from the dense predictions, the seen items masked."""
    _, above, n_cand = ref.rank_counts(P[u], list(seen), None, [t])
    return int(above[0]), n_cand


# ------------------------------------------------------------------------------------------ rank_of
def test_rank_of_equals_brute_force_rank(fitted):
    model, r, c = fitted
    P = model.predict()
    rng = np.random.default_rng(0)
    us = np.concatenate([rng.integers(0, M, 200), [4, 4, 7, 7, 7]])     # user 4 has no ratings; duplicate pairs
    its = np.concatenate([rng.integers(0, N_ITEMS, 200), [0, 24, 3, 3, 3]])
    rank, cand, scores = model.rank_of(us, its)
    assert rank.dtype == np.int64 and cand.dtype == np.int64 and scores.dtype == np.float32
    assert rank.shape == cand.shape == scores.shape == us.shape
    seen_targets = 0
    for p, (u, t) in enumerate(zip(us, its)):
        seen = set(c[r == u].tolist())
        seen_targets += t in seen
        assert (rank[p], cand[p]) == _brute_rank(P, seen, u, t)
        assert scores[p] == P[u, t]
    assert seen_targets > 10                                            # the rank of a seen target is defined too
    rank_all, cand_all, _ = model.rank_of(us, its, exclude_seen=False)
    for p, (u, t) in enumerate(zip(us, its)):
        assert (rank_all[p], cand_all[p]) == _brute_rank(P, (), u, t)
    assert (cand_all == N_ITEMS).all()


def test_rank_of_agrees_with_recommend(fitted):
    model = fitted[0]
    items, _ = model.recommend(None, 10)
    for u in range(M):
        valid = items[u] >= 0
        rank, _, _ = model.rank_of(np.full(valid.sum(), u), items[u][valid])
        assert (rank == np.arange(valid.sum())).all()


def test_rank_of_empty_input(fitted):
    rank, cand, scores = fitted[0].rank_of([], np.array([], dtype=np.int64))
    assert rank.shape == cand.shape == scores.shape == (0,)
    assert rank.dtype == np.int64 and scores.dtype == np.float32


def test_rank_of_argument_errors(fitted):
    model = fitted[0]
    cfg = ALSConfig(core=CoreConfig(n_factors=3, n_iters=1, lambda_u=1.0, lambda_v=1.0))
    with pytest.raises(RuntimeError, match="Model must be fitted before prediction."):
        ALS(cfg, device="cpu", backend=NumpyBackend()).rank_of([0], [0])
    for users in ([M], [-1]):
        with pytest.raises(IndexError):
            model.rank_of(users, [0])
    for items in ([N_ITEMS], [-1]):
        with pytest.raises(IndexError):
            model.rank_of([0], items)
    with pytest.raises(ValueError):
        model.rank_of([[0, 1]], [[0, 1]])
    with pytest.raises(ValueError):
        model.rank_of([0, 1], [0])
    with pytest.raises(ValueError):
        model.rank_of([0.5], [0])
    with pytest.raises(ValueError, match="rows"):
        model.rank_of([0], [0], features={"genres": np.zeros((N_ITEMS + 1, 2))})
    with pytest.raises(ValueError, match="infinite"):
        model.rank_of([0], [0], features={"genres": np.full((N_ITEMS, 2), np.inf)})


def test_rank_of_new_matches_recommend_new(fitted):
    model = fitted[0]
    rng = np.random.default_rng(5)
    R_new = np.full((6, N_ITEMS), np.nan)
    for b in range(5):                                                   # row 5: no ratings
        cols = rng.permutation(N_ITEMS)[:6]
        R_new[b, cols] = rng.integers(1, 6, 6)
    items, scores = model.recommend_new(R_new, 8)
    tptr = np.arange(0, 8 * 6 + 1, 8)
    rank, cand, sc = model.rank_of_new(R_new, (tptr, items.ravel()))
    assert (rank.reshape(6, 8) == np.arange(8)).all()
    assert (sc.astype(np.float64).reshape(6, 8) == scores).all()
    assert (cand.reshape(6, 8) == (N_ITEMS - (~np.isnan(R_new)).sum(axis=1))[:, None]).all()
    with pytest.raises(ValueError):
        model.rank_of_new(R_new, (tptr[:-1], items.ravel()))
    with pytest.raises(IndexError):
        model.rank_of_new(R_new, (tptr, np.full(48, N_ITEMS)))


# ------------------------------------------------------------------------------------------ rank_metrics
class _FixedRanks:
    """A model stand-in with a fixed item order per user: rank = position in the order, every item a candidate."""

    def __init__(self, orders, n, seen=()):
        self.orders, self.V, self.seen = orders, np.zeros((n, 1)), set(seen)

    def rank_of(self, users, items, features=None):
        rank = np.array([self.orders[int(u)].index(int(i)) for u, i in zip(users, items)], dtype=np.int64)
        return rank, np.full(rank.size, self.V.shape[0], np.int64), np.zeros(rank.size, np.float32)

    def _seen_pairs(self, users, items):
        return np.array([(int(u), int(i)) in self.seen for u, i in zip(users, items)], dtype=bool)


def test_rank_metrics_perfect_and_reversed():
    n = 6
    perfect = _FixedRanks({0: [3, 1, 0, 2, 4, 5], 1: [2, 0, 1, 3, 4, 5]}, n)
    res = cv.rank_metrics(perfect, [0, 0, 1], [3, 1, 2], Ks=(1, 2, 1000))
    assert res["users"] == 2 and res["pairs"] == 3 and res["dropped"] == 0
    assert res["mrr"] == 1.0 and res["auc"] == 1.0
    assert res["recall@2"] == 1.0 and res["ndcg@2"] == 1.0 and res["recall@1000"] == 1.0 and res["ndcg@1000"] == 1.0
    assert res["recall@1"] == pytest.approx((0.5 + 1.0) / 2) and res["ndcg@1"] == 1.0
    assert res["mpr"] == pytest.approx(((0 + 1) / 5 / 2 + 0.0) / 2, rel=1e-12)
    one = cv.rank_metrics(perfect, [1], [2])
    assert one["mrr"] == 1.0 and one["auc"] == 1.0 and one["mpr"] == 0.0
    rev = _FixedRanks({0: [5, 4, 2, 0, 1, 3]}, n)                        # relevant {1, 3} at the bottom
    res = cv.rank_metrics(rev, [0, 0], [3, 1], Ks=(3,))
    assert res["auc"] == 0.0 and res["mrr"] == pytest.approx(1 / 5) and res["recall@3"] == 0.0
    assert res["mpr"] == pytest.approx((4 / 5 + 5 / 5) / 2, rel=1e-12)


def test_rank_metrics_all_candidates_relevant_leaves_auc_only():
    n = 3
    mdl = _FixedRanks({0: [2, 0, 1], 1: [1, 2, 0]}, n)
    res = cv.rank_metrics(mdl, [0, 0, 0, 1], [0, 1, 2, 2], Ks=(2,))    # user 0: every candidate relevant
    assert res["users"] == 2
    assert res["auc"] == pytest.approx(0.5)                             # user 1 alone: rank 1 of 3, one of two below
    assert res["mrr"] == pytest.approx((1.0 + 0.5) / 2)
    only = cv.rank_metrics(mdl, [0, 0, 0], [0, 1, 2])
    assert np.isnan(only["auc"]) and only["users"] == 1 and only["mrr"] == 1.0
    none = cv.rank_metrics(mdl, [], [])
    assert none["users"] == 0 and np.isnan(none["mrr"]) and np.isnan(none["recall@10"])
    with pytest.raises(ValueError):
        cv.rank_metrics(mdl, [0], [1], Ks=(0,))
    with pytest.raises(ValueError):
        cv.rank_metrics(mdl, [0], [1], None, min_rating=3.0)


def _brute_metrics(P, train, held, Ks):
    """held: {u: set of relevant items}, train: {u: set}; definitions of rank_metrics, pair by pair."""
    acc = {f"{a}@{K}": [] for K in Ks for a in ("recall", "ndcg")}
    acc.update(mrr=[], auc=[], mpr=[])
    dropped = pairs = 0
    for u, rel in held.items():
        seen = train.get(u, set())
        keep = sorted(t for t in rel if t not in seen and not np.isnan(P[u, t]))
        dropped += len(rel) - len(keep)
        if not keep:
            continue
        pairs += len(keep)
        rho = sorted(_brute_rank(P, seen, u, t)[0] for t in keep)
        c = _brute_rank(P, seen, u, keep[0])[1]
        for K in Ks:
            acc[f"recall@{K}"].append(sum(x < K for x in rho) / len(rho))
            dcg = sum(1 / np.log2(x + 2) for x in rho if x < K)
            acc[f"ndcg@{K}"].append(dcg / sum(1 / np.log2(x + 2) for x in range(min(K, len(rho)))))
        acc["mrr"].append(1 / (1 + rho[0]))
        if c > len(rho):
            acc["auc"].append(1 - sum(x - i for i, x in enumerate(rho)) / (len(rho) * (c - len(rho))))
        acc["mpr"].append(np.mean([x / max(c - 1, 1) for x in rho]))
    out = {k: float(np.mean(v)) for k, v in acc.items()}
    out.update(users=len(acc["mrr"]), pairs=pairs, dropped=dropped)
    return out


@pytest.fixture(scope="module")
def split():
    m, n = 40, 60
    r, c, v = make_ratings(m, n, 900, seed=11)
    flat = np.unique(r * n + c, return_index=True)[1]
    r, c, v = r[flat], c[flat], v[flat]
    rng = np.random.default_rng(1)
    test = rng.random(r.size) < 0.3
    model = _fit(r[~test], c[~test], v[~test], (m, n), k=6)
    return model, (r[~test], c[~test], v[~test]), (r[test], c[test], v[test])


def test_rank_metrics_against_brute_force_and_ranking_at_k(split):
    model, (tr, tc, _), (hr, hc, hv) = split
    P = model.predict()
    train = {u: set(tc[tr == u].tolist()) for u in np.unique(tr)}
    Ks = (1, 5, 20, 128, 1000)
    for thr in (None, 4.0):
        keep = np.ones(hr.size, bool) if thr is None else hv >= thr
        held = {int(u): set(hc[keep & (hr == u)].tolist()) for u in np.unique(hr[keep])}
        want = _brute_metrics(P, train, held, Ks)
        got = cv.rank_metrics(model, hr, hc, hv, Ks=Ks, min_rating=thr)
        assert got["dropped"] == 0                                       # a disjoint split: nothing is left out
        assert (got["users"], got["pairs"]) == (want["users"], want["pairs"])
        for key in want:
            assert got[key] == pytest.approx(want[key], rel=1e-12, abs=1e-15), key
        for K in (1, 5, 20, 128):
            old = cv.ranking_at_k(model, hr, hc, hv, K=K, min_rating=thr)
            assert old["users"] == got["users"]
            assert abs(old["recall@K"] - got[f"recall@{K}"]) <= 1e-12
            assert abs(old["ndcg@K"] - got[f"ndcg@{K}"]) <= 1e-12


def test_rank_metrics_counts_dropped_pairs(split):
    model, (tr, tc, _), (hr, hc, hv) = split
    rows = np.concatenate([hr, tr[:37], hr[:5]])                         # 37 training pairs, 5 duplicates
    cols = np.concatenate([hc, tc[:37], hc[:5]])
    got = cv.rank_metrics(model, rows, cols)
    base = cv.rank_metrics(model, hr, hc)
    assert got["dropped"] == 37 and got["pairs"] == base["pairs"] == hr.size
    assert {k: v for k, v in got.items() if k != "dropped"} == {k: v for k, v in base.items() if k != "dropped"}


def test_fold_in_rank_metrics_against_fold_in_ranking_at_k(split):
    model, _, _ = split
    n = model.V.shape[0]
    rng = np.random.default_rng(2)
    kr, kc, kv, hr, hc = [], [], [], [], []
    for u in (100, 7, 55, 3):                                            # labels of new users, any integers
        cols = rng.permutation(n)[:20]
        kr += [u] * 12; kc += cols[:12].tolist(); kv += rng.integers(1, 6, 12).astype(float).tolist()
        hr += [u] * 8; hc += cols[12:].tolist()
    hr += [999, 999]; hc += [1, 2]                                       # a held-out user without known ratings
    known, held = (np.array(kr), np.array(kc), np.array(kv)), (np.array(hr), np.array(hc))
    got = cv.fold_in_rank_metrics(model, known, held, Ks=(3, 10, 128, 500))
    assert got["dropped"] == 0 and got["users"] == 5 and got["pairs"] == len(hr)
    for K in (3, 10, 128):
        old = cv.fold_in_ranking_at_k(model, known, held, K=K)
        assert abs(old["recall@K"] - got[f"recall@{K}"]) <= 1e-12
        assert abs(old["ndcg@K"] - got[f"ndcg@{K}"]) <= 1e-12
    assert got["recall@500"] == 1.0 and 0.0 < got["auc"] <= 1.0 and 0.0 <= got["mpr"] < 1.0
    over = (np.concatenate([held[0], known[0][:9]]), np.concatenate([held[1], known[1][:9]]))
    got2 = cv.fold_in_rank_metrics(model, known, over, Ks=(3, 10, 128, 500))
    assert got2["dropped"] == 9
    assert {k: v for k, v in got2.items() if k != "dropped"} == {k: v for k, v in got.items() if k != "dropped"}
