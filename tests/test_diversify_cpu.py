"""Diversified top-N (ALS.recommend_diverse / recommend_new_diverse / list_diversity, cv.diversity_at_k) without a
GPU: validation, the host orchestration over the numpy stand-in backend, whose mmr_rerank / list_diversity are the
contract of als_mmr_rerank / als_list_diversity in float64 (tests/mmr_ref.py), the cv measure on a hand-made
example, and the presence of the new symbols in the built library."""
import ctypes
import os

import numpy as np
import pytest

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, cv, validate
from collaborative_filtering_amd.serving import FoldedItems
from tests import mmr_ref
from tests.cpu_backend import NumpyBackend
from tests.synth import make_ratings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "collaborative-filtering_amd", "csrc", "libals_hip.so")


M, N_ITEMS = 30, 70


@pytest.fixture(scope="module")
def fitted():
    r, c, v = make_ratings(M, N_ITEMS, 500, seed=3, empty_users=(4,))
    cfg = ALSConfig(core=CoreConfig(n_factors=5, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    model = ALS(cfg, device="cpu", backend=NumpyBackend()).fit_coo(r, c, v, (M, N_ITEMS), tol=None, verbose=0)
    return model, r, c


def _expect(model, Z, n, pool_items, pool_scores, lam, N):
    """The definition applied to recommend(N=pool)'s host output (float64 scores of fp32 values: exact)."""
    tv, ti, _, ild, _ = mmr_ref.rerank(Z, n, pool_scores.astype(np.float32), pool_items.astype(np.int32), lam, N)
    return ti.astype(np.int64), tv.astype(np.float64), ild


# ------------------------------------------------------------------------------------------ validation
@pytest.mark.parametrize("bad", [-0.1, 1.1, float("nan"), "0.3", None, True])
def test_diversity_must_be_a_number_in_the_unit_interval(fitted, bad):
    model = fitted[0]
    R_new = np.full((1, N_ITEMS), np.nan)
    R_new[0, 3] = 4.0
    with pytest.raises(ValueError, match="diversity"):
        model.recommend_diverse([0], 3, diversity=bad)
    with pytest.raises(ValueError, match="diversity"):
        model.recommend_new_diverse(R_new, 3, diversity=bad)
    with pytest.raises(ValueError, match="diversity"):
        validate.diversity_args(bad, 3, None)


def test_pool_bounds_and_default(fitted):
    model = fitted[0]
    assert validate.diversity_args(0.3, 10, None) == (0.3, 40)
    assert validate.diversity_args(1, 50, None) == (1.0, 128)            # min(128, 4 N)
    assert validate.diversity_args(np.float32(0.5), 10, 10) == (0.5, 10)
    assert validate.diversity_args(0.0, 128, 128) == (0.0, 128)
    for N, pool in ((10, 9), (10, 129), (1, 0), (5, 7.0), (5, True)):
        with pytest.raises(ValueError, match="pool"):
            validate.diversity_args(0.3, N, pool)
        with pytest.raises(ValueError, match="pool"):
            model.recommend_diverse([0], N, pool=pool)
    with pytest.raises(ValueError, match="N must be"):
        model.recommend_diverse([0], 129)
    with pytest.raises(ValueError):                                       # checked also without users
        model.recommend_diverse([], 3, diversity=2.0)
    items, scores = model.recommend_diverse([], 3)
    assert items.shape == (0, 3) and scores.shape == (0, 3)


def test_item_lists_validation(fitted):
    model = fitted[0]
    for bad in ([1, 2, 3], [[0.5, 1.0]], [[N_ITEMS]], [[-2, 0]], np.zeros((2, 129), np.int64), np.zeros((2, 0), np.int64)):
        with pytest.raises(ValueError, match="item_lists"):
            model.list_diversity(bad)
    assert model.list_diversity(np.zeros((0, 4), np.int64)).shape == (0,)


# ------------------------------------------------------------------------------------------ orchestration
def test_diversity_zero_equals_recommend_and_chunks_cross(fitted, monkeypatch):
    model = fitted[0]
    be = model._eng.be
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)        # 30 users: five chunks
    for N, pool in ((6, None), (6, 6), (1, 128)):
        be.calls.clear()
        got = model.recommend_diverse(None, N, diversity=0.0, pool=pool)
        want_pool = min(128, 4 * N) if pool is None else pool
        assert [c_[0] for c_ in be.calls] == ["recommend_topk"] * 5 + ["mmr_rerank"] * 5
        assert [c_[1:] for c_ in be.calls[5:]] == [(nb, want_pool, N, 0.0, N_ITEMS) for nb in (7, 7, 7, 7, 2)]
        want = model.recommend(None, N)
        assert got[0].dtype == np.int64 and got[1].dtype == np.float64
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    sub = [29, 0, 29, 4]                                                  # order and duplicates kept; user 4 is empty
    got, want = model.recommend_diverse(sub, 5, diversity=0.0, exclude_seen=False), model.recommend(sub, 5, exclude_seen=False)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


@pytest.mark.parametrize("lam", [0.3, 0.7, 1.0])
def test_rerank_follows_the_definition_on_the_pool_of_recommend(fitted, monkeypatch, lam):
    model, r, c = fitted
    monkeypatch.setattr(model._eng, "REC_BATCH", 11, raising=False)
    Z = model._eng.Z.numpy() if model._eng.feat_names else model._eng.V.numpy()
    N, pool = 8, 20
    pi, ps = model.recommend(None, pool)
    items, scores = model.recommend_diverse(None, N, diversity=lam, pool=pool)
    wi, ws, wild = _expect(model, Z, N_ITEMS, pi, ps, lam, N)
    assert (items == wi).all() and (scores == ws).all()
    assert (items[:, 0] == pi[:, 0]).all()                                # the first pick is the best item
    assert (items != model.recommend(None, N)[0]).any()                   # and something moved
    for u in range(M):                                                    # never a seen item
        assert not np.isin(items[u], c[r == u]).any()
    ild = model.list_diversity(items)
    np.testing.assert_allclose(ild, wild.astype(np.float32), rtol=0, atol=1e-6)
    _, _, ild2 = model._recommend_diverse(None, N, lam, pool, None, True, None, None, None, True)
    assert (ild2 == ild).all()


def test_filters_go_to_the_pool_call_and_are_not_applied_again(fitted):
    model = fitted[0]
    be = model._eng.be
    rng = np.random.default_rng(1)
    allow = rng.permutation(N_ITEMS)[:25]
    block = allow[:4]
    be.calls.clear()
    items, scores = model.recommend_diverse([0, 3, 9], 6, diversity=0.5, pool=12, items=allow, filter_items=block)
    names = [c_[0] for c_ in be.calls]
    assert names == ["recommend_topk_masked", "mmr_rerank"]               # one bitmap, one pool call, one re-rank
    ok = validate.allowed_mask(validate.item_filters(allow, block, N_ITEMS), N_ITEMS)
    assert ok[items[items >= 0]].all()
    pi, ps = model.recommend([0, 3, 9], 12, items=allow, filter_items=block)
    Z = model._eng.V.numpy()
    wi, ws, _ = _expect(model, Z, N_ITEMS, pi, ps, 0.5, 6)
    assert (items == wi).all() and (scores == ws).all()
    few = model.recommend_diverse([0], 6, diversity=0.5, items=[5, 9, 11], exclude_seen=False)     # a short pool: padded
    assert (np.sort(few[0][0, :3]) == [5, 9, 11]).all() and (few[0][0, 3:] == -1).all() and np.isneginf(few[1][0, 3:]).all()
    none = model.recommend_diverse([0, 1], 4, items=[])
    assert (none[0] == -1).all() and np.isneginf(none[1]).all()
    assert np.isnan(model.list_diversity(none[0])).all() and np.isnan(model.list_diversity(few[0][:, :1])).all()


def test_folded_users(fitted, monkeypatch):
    model = fitted[0]
    monkeypatch.setattr(model._eng, "REC_BATCH", 4, raising=False)
    rng = np.random.default_rng(5)
    R_new = np.full((6, N_ITEMS), np.nan)
    for b in range(5):                                                    # row 5 has no ratings
        R_new[b, rng.permutation(N_ITEMS)[:6]] = rng.integers(1, 6, 6)
    want = model.recommend_new(R_new, 7)
    got = model.recommend_new_diverse(R_new, 7, diversity=0.0)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    block = rng.random(N_ITEMS) < 0.4
    pi, ps = model.recommend_new(R_new, 28, filter_items=block)
    items, scores = model.recommend_new_diverse(R_new, 7, diversity=0.6, filter_items=block)
    wi, ws, _ = _expect(model, model._eng.V.numpy(), N_ITEMS, pi, ps, 0.6, 7)
    assert (items == wi).all() and (scores == ws).all()
    assert not np.isin(items, np.nonzero(block)[0]).any()
    for b in range(5):
        assert not np.isin(items[b], np.nonzero(~np.isnan(R_new[b]))[0]).any()
    assert model.recommend_new_diverse(np.empty((0, N_ITEMS)), 3)[0].shape == (0, 3)


def test_new_items_join_the_pool_and_the_similarity_table(fitted):
    model = fitted[0]
    be = model._eng.be
    rng = np.random.default_rng(6)
    B, k = 9, model.V.shape[1]
    Zf = (3.0 * rng.normal(size=(B, k))).astype(np.float32).astype(np.float64)
    folded = FoldedItems(Zf.copy(), rng.normal(size=B).astype(np.float32).astype(np.float64) + 1.0, Zf, None,
                         (np.zeros(B + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)))
    nt = N_ITEMS + B
    want = model.recommend([0, 7, 9], 10, new_items=folded)
    got = model.recommend_diverse([0, 7, 9], 10, diversity=0.0, new_items=folded)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (want[0] >= N_ITEMS).any()
    be.calls.clear()
    items, scores = model.recommend_diverse([0, 7, 9], 10, diversity=0.5, pool=30, new_items=folded,
                                            filter_items=[nt - 1])
    assert be.calls[-1][0] == "mmr_rerank" and be.calls[-1][-1] == nt     # scored against the joint table
    Zj = np.concatenate([model._eng.V.numpy()[:N_ITEMS], np.pad(Zf.astype(np.float32), ((0, 0), (0, model._eng.ld - k)))])
    pi, ps = model.recommend([0, 7, 9], 30, new_items=folded, filter_items=[nt - 1])
    wi, ws, wild = _expect(model, Zj, nt, pi, ps, 0.5, 10)
    assert (items == wi).all() and (scores == ws).all() and (items >= N_ITEMS).any() and not (items == nt - 1).any()
    np.testing.assert_allclose(model.list_diversity(items, new_items=folded), wild.astype(np.float32), atol=1e-6)
    with pytest.raises(ValueError, match="item_lists"):
        model.list_diversity(items)                                       # ids >= n without the folded table


# ------------------------------------------------------------------------------------------ cv
class _HandModel:
    """Four items on two orthogonal axes: 0, 1 along e1, 2 along e2, 3 = (e1 + e2) / sqrt(2).  Lists are fixed."""
    V = np.zeros((4, 2))
    Z = np.array([[1.0, 0.0], [2.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    LISTS = {0: [0, 1, 2], 1: [2, 3, -1], 2: [3, -1, -1]}

    def _recommend_diverse(self, users, K, diversity, pool, features, exclude_seen, new_items, items, filter_items,
                           with_ild):
        assert with_ild and exclude_seen and new_items is None
        top = np.array([self.LISTS[int(u)][:K] for u in users], dtype=np.int64)
        return top, np.zeros(top.shape), mmr_ref.list_diversity(self.Z, 4, top)


def test_cv_diversity_at_k_by_hand():
    model = _HandModel()
    rows, cols = np.array([0, 0, 1, 2, 2]), np.array([1, 3, 2, 3, 0])
    got = cv.diversity_at_k(model, rows, cols, K=3, diversity=0.4)
    # user 0: list [0, 1, 2], rel {1, 3}: one hit at rank 2.  user 1: [2, 3], rel {2}: hit at rank 1.  user 2: [3],
    # rel {0, 3}: hit at rank 1 of two relevant.
    d = lambda r: 1.0 / np.log2(r + 1.0)                                  # noqa: E731
    assert got["users"] == 3
    assert got["recall@K"] == pytest.approx((0.5 + 1.0 + 0.5) / 3, rel=1e-12)
    assert got["ndcg@K"] == pytest.approx((d(2) / (d(1) + d(2)) + 1.0 + d(1) / (d(1) + d(2))) / 3, rel=1e-12)
    # ILD: user 0 pairs (0,1) sim 1, (0,2) 0, (1,2) 0 -> 2/3; user 1 pair (2,3) sim 1/sqrt 2 -> 1 - 1/sqrt 2; user 2
    # has one item and is left out of the mean
    assert got["ild@K"] == pytest.approx((2.0 / 3.0 + 1.0 - 1.0 / np.sqrt(2.0)) / 2, rel=1e-12)
    assert got["coverage@K"] == 4 / 4                                     # items {0, 1, 2, 3} of 4
    one = cv.diversity_at_k(model, [2], [3], K=1)
    assert one["users"] == 1 and np.isnan(one["ild@K"]) and one["coverage@K"] == 1 / 4
    none = cv.diversity_at_k(model, [], [])
    assert none["users"] == 0 and np.isnan(none["coverage@K"]) and np.isnan(none["ild@K"])
    with pytest.raises(ValueError, match="min_rating"):
        cv.diversity_at_k(model, rows, cols, min_rating=3.0)


def test_cv_diversity_at_k_equals_ranking_at_k_at_zero(fitted):
    model = fitted[0]
    rng = np.random.default_rng(7)
    hr, hc, hv = rng.integers(0, M, 200), rng.integers(0, N_ITEMS, 200), rng.integers(1, 6, 200).astype(float)
    cat = np.arange(N_ITEMS) % 3 != 0
    for kw in ({}, dict(min_rating=3.0), dict(items=cat), dict(filter_items=np.nonzero(~cat)[0], min_rating=2.0)):
        base = cv.ranking_at_k(model, hr, hc, hv, K=5, **kw)
        got = cv.diversity_at_k(model, hr, hc, hv, K=5, diversity=0.0, **kw)
        for key, val in base.items():
            assert got[key] == val, key                                   # exactly
        assert 0.0 <= got["ild@K"] <= 2.0 and 0.0 < got["coverage@K"] <= 1.0
        assert set(got) == set(base) | {"ild@K", "coverage@K"}
    top, _ = model.recommend(np.unique(hr), 5, items=cat)
    assert cv.diversity_at_k(model, hr, hc, K=5, items=cat)["coverage@K"] == np.unique(top[top >= 0]).size / cat.sum()
    more = cv.diversity_at_k(model, hr, hc, K=5, diversity=0.8)
    assert more["ild@K"] > cv.diversity_at_k(model, hr, hc, K=5)["ild@K"]


# ------------------------------------------------------------------------------------------ library
def test_library_exports_the_diversity_entry_points():
    if not os.path.exists(LIB):             # fresh checkout: the .so is git-ignored
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(LIB)
    for name in ("als_mmr_rerank", "als_list_diversity"):
        assert hasattr(lib, name), name
    from collaborative_filtering_amd import _hip
    assert {"als_mmr_rerank", "als_list_diversity"} <= set(_hip.EXPORTS)
    header = open(os.path.join(ROOT, "include", "als_hip.h")).read()
    assert "int als_mmr_rerank(" in header and "int als_list_diversity(" in header
    lib = _hip.load()                       # argument errors need no device: nothing is launched
    E_BADARG, E_BADK = -1, -2
    assert lib.als_mmr_rerank(0, 16, 1, 5, None, 4, None, None, 0.5, 2, None, None, None, None, None) == E_BADK
    assert lib.als_mmr_rerank(8, 16, 1, 5, None, 4, None, None, 0.5, 2, None, None, None, None, None) == E_BADARG
    assert lib.als_mmr_rerank(8, 16, 0, 5, None, 4, None, None, 0.5, 2, None, None, None, None, None) == 0
    assert lib.als_list_diversity(161, 160, 1, 5, None, 4, None, None, None) == E_BADK
    assert lib.als_list_diversity(8, 16, 1, 5, None, 129, None, None, None) == E_BADARG
    assert lib.als_list_diversity(8, 16, 0, 5, None, 4, None, None, None) == 0
