"""Calibrated top-N (ALS.recommend_calibrated / recommend_new_calibrated / category_profile / list_miscalibration,
cv.calibration_at_k) without a GPU: validation, the host orchestration over a numpy stand-in backend whose
category_profile / calibrated_rerank / list_miscalibration are the contract of the three kernels in float64
(tests/calibrate_ref.py), the cv measure on an example worked by hand, the float64 definition's behaviour over the
calibration weight, and the presence of the new symbols in the built library."""
import ctypes
import os

import numpy as np
import pytest
import torch

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, cv, validate
from collaborative_filtering_amd.serving import FoldedItems
from tests import calibrate_ref as ref
from tests.cpu_backend import NumpyBackend
from tests.synth import make_ratings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "collaborative-filtering_amd", "csrc", "libals_hip.so")

M, N_ITEMS, NCAT = 30, 70, 5


class CalibratingBackend(NumpyBackend):
    """NumpyBackend plus the three calibration calls, each the float64 definition rounded to the kernel's output."""

    def category_profile(self, *, ncat, indptr, indices, rows, n, C, P_out):
        B = indptr.numel() - 1 if rows is None else rows.numel()
        self.calls.append(("category_profile", B, ncat, n, rows is None))
        assert C.dtype == torch.float32 and tuple(C.shape) == (n, 16 * ((ncat + 15) // 16)) and P_out.shape == (B, C.shape[1])
        assert indptr.dtype == torch.int64 and indices.dtype == torch.int32
        P = ref.profile(C.numpy()[:, :ncat], indptr.numpy(), indices.numpy(), None if rows is None else rows.numpy())
        P_out.zero_()
        P_out[:, :ncat] = torch.from_numpy(P.astype(np.float32))

    def calibrated_rerank(self, *, ncat, n, C, P, cand_val, cand_idx, lam, alpha, topn, top_val, top_idx, top_cnt,
                          top_kl=None):
        self.calls.append(("calibrated_rerank", cand_idx.shape[0], cand_idx.shape[1], topn, lam, alpha, n))
        assert cand_val.dtype == torch.float32 and cand_idx.dtype == torch.int32 and tuple(C.shape) == (n, P.shape[1])
        tv, ti, tc, kl, _ = ref.rerank(C.numpy()[:, :ncat], n, P.numpy()[:, :ncat], cand_val.numpy(), cand_idx.numpy(),
                                       lam, alpha, topn)
        top_val.copy_(torch.from_numpy(tv))
        top_idx.copy_(torch.from_numpy(ti))
        top_cnt.copy_(torch.from_numpy(tc))
        if top_kl is not None:
            top_kl.copy_(torch.from_numpy(kl.astype(np.float32)))

    def list_miscalibration(self, *, ncat, n, C, P, idx, alpha, kl):
        self.calls.append(("list_miscalibration", idx.shape[0], idx.shape[1], n))
        assert idx.dtype == torch.int32
        kl.copy_(torch.from_numpy(ref.list_miscalibration(C.numpy()[:, :ncat], n, P.numpy()[:, :ncat], idx.numpy(),
                                                          alpha).astype(np.float32)))


@pytest.fixture(scope="module")
def fitted():
    r, c, v = make_ratings(M, N_ITEMS, 500, seed=3, empty_users=(4,))
    cfg = ALSConfig(core=CoreConfig(n_factors=5, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    model = ALS(cfg, device="cpu", backend=CalibratingBackend()).fit_coo(r, c, v, (M, N_ITEMS), tol=None, verbose=0)
    rng = np.random.default_rng(11)
    G = (rng.random((N_ITEMS, NCAT)) < 0.35).astype(np.float64)
    G[::9] = 0.0                                                          # items without a category
    return model, r, c, G


def _profiles(G, r, c, users):
    """float32 profiles of the users' training rows, as float64: what the stand-in hands the re-rank."""
    Cn = ref.normalise(G)
    hist = [np.sort(c[r == u]) for u in users]
    ptr = np.concatenate([[0], np.cumsum([h.size for h in hist])]).astype(np.int64)
    idx = np.concatenate(hist).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return Cn, ref.profile(Cn, ptr, idx).astype(np.float32).astype(np.float64)


def _expect(Cn, n, P, pool_items, pool_scores, lam, alpha, N):
    """The definition applied to recommend(N=pool)'s host output (float64 scores of fp32 values: exact)."""
    tv, ti, _, kl, _ = ref.rerank(Cn, n, P, pool_scores.astype(np.float32), pool_items.astype(np.int32), lam, alpha, N)
    return ti.astype(np.int64), tv.astype(np.float64), kl.astype(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------ validation
def test_category_table_validation(fitted):
    model, _, _, G = fitted
    T = validate.category_table(G, N_ITEMS)
    assert T.dtype == np.float32 and T.shape == (N_ITEMS, 16) and not T[:, NCAT:].any()
    assert (T[:, :NCAT] == ref.normalise(G)).all() and not T[0].any()
    assert validate.category_table(np.ones((3, 64), np.int64), 3).shape == (3, 64)
    assert validate.category_table(np.ones((3, 17)), 3).shape == (3, 32)
    bad_neg, bad_nan = G.copy(), G.copy()
    bad_neg[3, 1], bad_nan[5, 0] = -1.0, np.nan
    for bad in (G[:-1], np.ones((N_ITEMS, 65)), bad_neg, bad_nan, G[:, 0], np.ones((N_ITEMS, 0)), G > 0):
        with pytest.raises(ValueError, match="categories"):
            validate.category_table(bad, N_ITEMS)
        with pytest.raises(ValueError, match="categories"):
            model.recommend_calibrated([0], 3, categories=bad)
        with pytest.raises(ValueError, match="categories"):
            model.category_profile([0], categories=bad)
        with pytest.raises(ValueError, match="categories"):
            model.list_miscalibration([[0, 1]], categories=bad, users=[0])


@pytest.mark.parametrize("bad", [-0.1, 1.1, float("nan"), "0.5", None, True])
def test_calibration_must_be_a_number_in_the_unit_interval(fitted, bad):
    model, _, _, G = fitted
    R_new = np.full((1, N_ITEMS), np.nan)
    R_new[0, 3] = 4.0
    with pytest.raises(ValueError, match="calibration"):
        model.recommend_calibrated([0], 3, categories=G, calibration=bad)
    with pytest.raises(ValueError, match="calibration"):
        model.recommend_new_calibrated(R_new, 3, categories=G, calibration=bad)
    with pytest.raises(ValueError, match="calibration"):
        validate.calibration_args(bad, 3, None, 0.01)


def test_smoothing_pool_and_target_bounds(fitted):
    model, _, _, G = fitted
    assert validate.calibration_args(0.5, 10, None, 0.01) == (0.5, 40, 0.01)
    assert validate.calibration_args(1, 50, None, 0.5) == (1.0, 128, 0.5)
    for bad in (0, 1, 0.0, 1.0, -0.2, float("nan"), "0.1", None, 1e-60):      # 1e-60 is 0 in fp32
        with pytest.raises(ValueError, match="smoothing"):
            validate.calibration_args(0.5, 3, None, bad)
        with pytest.raises(ValueError, match="smoothing"):
            model.recommend_calibrated([0], 3, categories=G, smoothing=bad)
        with pytest.raises(ValueError, match="smoothing"):
            model.list_miscalibration([[0, 1]], categories=G, users=[0], smoothing=bad)
    for N, pool in ((10, 9), (10, 129), (1, 0), (5, 7.0), (5, True)):
        with pytest.raises(ValueError, match="pool"):
            validate.calibration_args(0.5, N, pool, 0.01)
        with pytest.raises(ValueError, match="pool"):
            model.recommend_calibrated([0], N, categories=G, pool=pool)
    with pytest.raises(ValueError, match="N must be"):
        model.recommend_calibrated([0], 129, categories=G)
    for bad in (np.ones((2, NCAT)), np.ones((1, NCAT + 1)), -np.ones((1, NCAT)), np.full((1, NCAT), np.inf), np.ones(NCAT)):
        with pytest.raises(ValueError, match="target"):
            model.recommend_calibrated([0], 3, categories=G, target=bad)
    t = validate.target_rows(np.array([[3.0, 1.0, 0.0, 0.0, 1e-40]]), 1, NCAT)
    assert t.shape == (1, 16) and t[0, 0] == np.float32(0.75) and t[0, 4] == 0.0      # tiny entries count as zero
    with pytest.raises(ValueError):                                       # checked also without users
        model.recommend_calibrated([], 3, categories=G, calibration=2.0)
    items, scores = model.recommend_calibrated([], 3, categories=G)
    assert items.shape == (0, 3) and scores.shape == (0, 3)
    assert len(model.recommend_calibrated([], 3, categories=G, return_miscalibration=True)) == 3
    assert model.category_profile([], categories=G).shape == (0, NCAT)


def test_list_miscalibration_needs_exactly_one_of_users_and_target(fitted):
    model, _, _, G = fitted
    lists = np.array([[0, 1, 2], [3, 4, -1]])
    with pytest.raises(ValueError, match="exactly one"):
        model.list_miscalibration(lists, categories=G)
    with pytest.raises(ValueError, match="exactly one"):
        model.list_miscalibration(lists, categories=G, users=[0, 1], target=np.ones((2, NCAT)))
    with pytest.raises(ValueError, match="users"):
        model.list_miscalibration(lists, categories=G, users=[0])
    with pytest.raises(ValueError, match="item_lists"):
        model.list_miscalibration([[N_ITEMS]], categories=G, users=[0])
    assert model.list_miscalibration(np.zeros((0, 4), np.int64), categories=G, users=[]).shape == (0,)


# ------------------------------------------------------------------------------------------ orchestration
def test_calibration_zero_equals_recommend_and_chunks_cross(fitted, monkeypatch):
    model, _, _, G = fitted
    be = model._eng.be
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)        # 30 users: five chunks
    for N, pool in ((6, None), (6, 6), (1, 128)):
        be.calls.clear()
        got = model.recommend_calibrated(None, N, categories=G, calibration=0.0, pool=pool)
        want_pool = min(128, 4 * N) if pool is None else pool
        assert [c_[0] for c_ in be.calls] == ["recommend_topk"] * 5 + ["category_profile", "calibrated_rerank"] * 5
        assert [c_[1:] for c_ in be.calls[6::2]] == [(nb, want_pool, N, 0.0, 0.01, N_ITEMS) for nb in (7, 7, 7, 7, 2)]
        assert [c_[1:] for c_ in be.calls[5::2]] == [(nb, NCAT, N_ITEMS, False) for nb in (7, 7, 7, 7, 2)]
        want = model.recommend(None, N)
        assert got[0].dtype == np.int64 and got[1].dtype == np.float64
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    sub = [29, 0, 29, 4]                                                  # order and duplicates kept; user 4 is empty
    got = model.recommend_calibrated(sub, 5, categories=G, calibration=0.0, exclude_seen=False)
    want = model.recommend(sub, 5, exclude_seen=False)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    # a user without a history has an all-zero profile: recommend's list at any weight
    got = model.recommend_calibrated([4], 5, categories=G, calibration=1.0)
    want = model.recommend([4], 5)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


@pytest.mark.parametrize("lam", [0.3, 0.8, 1.0])
def test_rerank_follows_the_definition_on_the_pool_of_recommend(fitted, monkeypatch, lam):
    model, r, c, G = fitted
    monkeypatch.setattr(model._eng, "REC_BATCH", 11, raising=False)
    N, pool = 8, 20
    users = np.arange(M)
    Cn, P = _profiles(G, r, c, users)
    np.testing.assert_array_equal(model.category_profile(None, categories=G), P)
    assert not P[4].any() and abs(P[0].sum() - 1.0) < 1e-6
    pi, ps = model.recommend(None, pool)
    items, scores, kl = model.recommend_calibrated(None, N, categories=G, calibration=lam, pool=pool,
                                                   return_miscalibration=True)
    wi, ws, wkl = _expect(Cn, N_ITEMS, P, pi, ps, lam, 0.01, N)
    assert (items == wi).all() and (scores == ws).all() and (kl == wkl).all()
    assert (items != model.recommend(None, N)[0]).any()                   # something moved
    for u in range(M):                                                    # never a seen item
        assert not np.isin(items[u], c[r == u]).any()
    again = model.list_miscalibration(items, categories=G, users=users)
    assert (again == kl).all()
    base = model.list_miscalibration(model.recommend(None, N)[0], categories=G, users=users)
    assert kl.mean() < base.mean()
    pub = model.recommend_calibrated(None, N, categories=G, calibration=lam, pool=pool, smoothing=0.2)
    assert (pub[0] == _expect(Cn, N_ITEMS, P, pi, ps, lam, 0.2, N)[0]).all()


def test_an_explicit_target_overrides_the_profile(fitted):
    model, r, c, G = fitted
    be = model._eng.be
    users = [0, 3, 9, 4]
    T = np.zeros((4, NCAT))
    T[0, 0], T[1, [1, 2]], T[2, 4] = 2.0, (3.0, 1.0), 1.0                 # row 3 stays zero: recommend's list
    be.calls.clear()
    items, scores, kl = model.recommend_calibrated(users, 6, categories=G, calibration=0.9, pool=24, target=T,
                                                   return_miscalibration=True)
    assert [c_[0] for c_ in be.calls] == ["recommend_topk", "calibrated_rerank"]      # no profile kernel
    Cn = ref.normalise(G)
    pi, ps = model.recommend(users, 24)
    wi, ws, wkl = _expect(Cn, N_ITEMS, ref.normalise(T), pi, ps, 0.9, 0.01, 6)
    assert (items == wi).all() and (scores == ws).all() and (kl == wkl).all()
    assert (items[3] == pi[3, :6]).all() and kl[3] == 0.0
    assert (items != model.recommend_calibrated(users, 6, categories=G, calibration=0.9, pool=24)[0]).any()
    assert (model.list_miscalibration(items, categories=G, target=T) == kl).all()


def test_filters_go_to_the_pool_call_only(fitted):
    model, r, c, G = fitted
    be = model._eng.be
    rng = np.random.default_rng(1)
    allow = rng.permutation(N_ITEMS)[:25]
    block = allow[:4]
    be.calls.clear()
    items, scores = model.recommend_calibrated([0, 3, 9], 6, categories=G, calibration=0.5, pool=12, items=allow,
                                               filter_items=block)
    assert [c_[0] for c_ in be.calls] == ["recommend_topk_masked", "category_profile", "calibrated_rerank"]
    ok = validate.allowed_mask(validate.item_filters(allow, block, N_ITEMS), N_ITEMS)
    assert ok[items[items >= 0]].all()
    pi, ps = model.recommend([0, 3, 9], 12, items=allow, filter_items=block)
    Cn, P = _profiles(G, r, c, [0, 3, 9])                                 # the profile ignores the filters
    wi, ws, _ = _expect(Cn, N_ITEMS, P, pi, ps, 0.5, 0.01, 6)
    assert (items == wi).all() and (scores == ws).all()
    few = model.recommend_calibrated([0], 6, categories=G, items=[5, 9, 11], exclude_seen=False)      # a short pool
    assert (np.sort(few[0][0, :3]) == [5, 9, 11]).all() and (few[0][0, 3:] == -1).all() and np.isneginf(few[1][0, 3:]).all()
    none = model.recommend_calibrated([0, 1], 4, categories=G, items=[])
    assert (none[0] == -1).all() and np.isneginf(none[1]).all()


def test_folded_users_get_their_profile_from_r_new(fitted, monkeypatch):
    model, _, _, G = fitted
    be = model._eng.be
    monkeypatch.setattr(model._eng, "REC_BATCH", 4, raising=False)
    rng = np.random.default_rng(5)
    R_new = np.full((6, N_ITEMS), np.nan)
    for b in range(5):                                                    # row 5 has no ratings
        R_new[b, rng.permutation(N_ITEMS)[:6]] = rng.integers(1, 6, 6)
    want = model.recommend_new(R_new, 7)
    got = model.recommend_new_calibrated(R_new, 7, categories=G, calibration=0.0)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    block = rng.random(N_ITEMS) < 0.3
    pi, ps = model.recommend_new(R_new, 28, filter_items=block)
    be.calls.clear()
    items, scores, kl = model.recommend_new_calibrated(R_new, 7, categories=G, calibration=0.7, filter_items=block,
                                                       return_miscalibration=True)
    prof_calls = [c_ for c_ in be.calls if c_[0] == "category_profile"]
    assert prof_calls == [("category_profile", 4, NCAT, N_ITEMS, True), ("category_profile", 2, NCAT, N_ITEMS, True)]
    Cn = ref.normalise(G)
    rr, cc = np.nonzero(~np.isnan(R_new))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=6))]).astype(np.int64)
    P = ref.profile(Cn, ptr, cc.astype(np.int32)).astype(np.float32).astype(np.float64)
    wi, ws, wkl = _expect(Cn, N_ITEMS, P, pi, ps, 0.7, 0.01, 7)
    assert (items == wi).all() and (scores == ws).all() and (kl == wkl).all()
    assert (items[5] == pi[5, :7]).all()                                  # no ratings: no profile: the head of the pool
    assert not np.isin(items, np.nonzero(block)[0]).any()
    for b in range(5):
        assert not np.isin(items[b], np.nonzero(~np.isnan(R_new[b]))[0]).any()
    assert model.recommend_new_calibrated(np.empty((0, N_ITEMS)), 3, categories=G)[0].shape == (0, 3)


def test_new_items_bring_their_category_rows(fitted):
    model, r, c, G = fitted
    be = model._eng.be
    rng = np.random.default_rng(6)
    B, k = 9, model.V.shape[1]
    Zf = (3.0 * rng.normal(size=(B, k))).astype(np.float32).astype(np.float64)
    folded = FoldedItems(Zf.copy(), rng.normal(size=B).astype(np.float32).astype(np.float64) + 1.0, Zf, None,
                         (np.zeros(B + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)))
    nt = N_ITEMS + B
    Gj = np.concatenate([G, (rng.random((B, NCAT)) < 0.4).astype(np.float64)])
    with pytest.raises(ValueError, match="categories"):
        model.recommend_calibrated([0], 5, categories=G, new_items=folded)     # n rows for n + B items
    users = [0, 7, 9]
    want = model.recommend(users, 10, new_items=folded)
    got = model.recommend_calibrated(users, 10, categories=Gj, calibration=0.0, new_items=folded)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (want[0] >= N_ITEMS).any()
    be.calls.clear()
    items, scores = model.recommend_calibrated(users, 10, categories=Gj, calibration=0.6, pool=30, new_items=folded,
                                               filter_items=[nt - 1])
    assert be.calls[-1][0] == "calibrated_rerank" and be.calls[-1][-1] == nt
    assert be.calls[-2] == ("category_profile", 3, NCAT, nt, False)
    pi, ps = model.recommend(users, 30, new_items=folded, filter_items=[nt - 1])
    Cn = ref.normalise(Gj)
    _, P = _profiles(Gj, r, c, users)                                     # the training rows name fitted items only
    wi, ws, _ = _expect(Cn, nt, P, pi, ps, 0.6, 0.01, 10)
    assert (items == wi).all() and (scores == ws).all() and (items >= N_ITEMS).any() and not (items == nt - 1).any()


# ------------------------------------------------------------------------------------------ cv
class _HandModel:
    """Six items in two categories - 0, 1, 2 in A, 3, 4 in B, 5 in both; user 0 has rated A, A, A, B (3 : 1), user 1
    nothing.  The lists are fixed."""
    V = np.zeros((6, 2))
    G = np.array([[1, 0], [1, 0], [1, 0], [0, 1], [0, 1], [1, 1]], dtype=np.float64)
    HIST = {0: [0, 1, 2, 3], 1: []}
    LISTS = {0.0: {0: [0, 1, 2, 4], 1: [0, 3, -1, -1]}, 1.0: {0: [0, 1, 5, 3], 1: [0, 3, -1, -1]}}

    def category_profile(self, users, *, categories):
        Cn = ref.normalise(categories)
        return np.array([Cn[self.HIST[int(u)]].sum(axis=0) / max(len(self.HIST[int(u)]), 1) for u in users])

    def recommend_calibrated(self, users, K, *, categories, calibration, pool, smoothing, features,
                             return_miscalibration):
        assert return_miscalibration and smoothing == 0.01
        top = np.array([self.LISTS[calibration][int(u)][:K] for u in users], dtype=np.int64)
        P = self.category_profile(users, categories=categories)
        kl = ref.list_miscalibration(ref.normalise(categories), 6, P, top, smoothing)
        return top, np.zeros(top.shape), kl


def test_cv_calibration_at_k_by_hand():
    model = _HandModel()
    rows, cols = np.array([0, 0, 1]), np.array([4, 5, 3])
    got = cv.calibration_at_k(model, rows, cols, K=4, categories=model.G, calibrations=(0.0, 1.0))
    d = lambda rk: 1.0 / np.log2(rk + 1.0)                                # noqa: E731
    assert got["users"] == 2 and got["profiled_users"] == 1
    a, b = got["calibrations"]
    assert (a["calibration"], b["calibration"]) == (0.0, 1.0)
    # calibration 0: user 0 lists [0, 1, 2, 4], rel {4, 5}: one hit at rank 4; user 1 lists [0, 3], rel {3}: rank 2
    assert a["recall@K"] == pytest.approx((0.5 + 1.0) / 2, rel=1e-12)
    assert a["ndcg@K"] == pytest.approx((d(4) / (d(1) + d(2)) + d(2) / d(1)) / 2, rel=1e-12)
    # calibration 1: user 0 lists [0, 1, 5, 3], rel {4, 5}: one hit at rank 3
    assert b["recall@K"] == pytest.approx((0.5 + 1.0) / 2, rel=1e-12)
    assert b["ndcg@K"] == pytest.approx((d(3) / (d(1) + d(2)) + d(2) / d(1)) / 2, rel=1e-12)
    # miscalibration, user 0 only (user 1 has no profile): p = (3/4, 1/4), alpha = fp32(0.01).
    # [0, 1, 2, 4]: q = (3/4, 1/4) = p: KL = 0.   [0, 1, 5, 3]: q = (1 + 1 + 1/2, 1/2 + 1) / 4 = (5/8, 3/8).
    al = float(np.float32(0.01))
    p, q = np.array([0.75, 0.25]), np.array([0.625, 0.375])
    assert a["miscalibration@K"] == pytest.approx(0.0, abs=1e-12)
    assert b["miscalibration@K"] == pytest.approx(float(np.sum(p * np.log(p / ((1 - al) * q + al * p)))), abs=1e-12)
    none = cv.calibration_at_k(model, [], [], K=4, categories=model.G)
    assert none["users"] == 0 and none["profiled_users"] == 0 and np.isnan(none["calibrations"][1]["miscalibration@K"])
    only = cv.calibration_at_k(model, [1], [3], K=2, categories=model.G, calibrations=[1.0])
    assert only["profiled_users"] == 0 and np.isnan(only["calibrations"][0]["miscalibration@K"])


def test_cv_calibration_at_k_equals_ranking_at_k_at_zero(fitted):
    model, _, _, G = fitted
    rng = np.random.default_rng(7)
    hr, hc, hv = rng.integers(0, M, 200), rng.integers(0, N_ITEMS, 200), rng.integers(1, 6, 200).astype(float)
    cat = np.arange(N_ITEMS) % 3 != 0
    for kw in ({}, dict(min_rating=3.0), dict(items=cat), dict(filter_items=np.nonzero(~cat)[0], min_rating=2.0)):
        base = cv.ranking_at_k(model, hr, hc, hv, K=5, **kw)
        got = cv.calibration_at_k(model, hr, hc, hv, K=5, categories=G, calibrations=(0.0, 0.9), **kw)
        zero, most = got["calibrations"]
        assert got["users"] == base["users"] and got.get("filtered_out") == base.get("filtered_out")
        assert zero["recall@K"] == base["recall@K"] and zero["ndcg@K"] == base["ndcg@K"]      # exactly
        assert 0 < got["profiled_users"] <= got["users"]
        assert most["miscalibration@K"] < zero["miscalibration@K"]


# ------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("ncat", [7, 19])
def test_the_float64_list_kl_falls_monotonically_with_the_weight(ncat):
    n, B, pool, N = 1003, 43, 64, 10
    G, ptr, idx = ref.synthetic(n, B, ncat, seed=100 + ncat)
    C = ref.normalise(G)
    P = ref.profile(C, ptr, idx).astype(np.float32).astype(np.float64)
    assert not P[0].any() and not P[1].any() and ptr[2] - ptr[1] > 0      # no history / only uncategorised items
    rng = np.random.default_rng(ncat)
    ci = np.stack([rng.permutation(n)[:pool] for _ in range(B)]).astype(np.int32)
    cv_ = -np.sort(-rng.normal(size=(B, pool)).astype(np.float32), axis=1)
    known = P.any(axis=1)
    means = []
    for lam in (0.0, 0.3, 0.8, 1.0):
        tv, ti, tc, kl, picks = ref.rerank(C, n, P, cv_, ci, lam, 0.01, N)
        assert (tc == N).all() and all(len(set(p)) == N for p in picks)
        if lam == 0.0:
            assert (ti == ci[:, :N]).all()
        assert (ti[~known] == ci[~known, :N]).all()                       # no target: the head of the pool
        means.append(kl[known].mean())
    assert means[0] > means[1] > means[2] > means[3] > 0.0, means


# ------------------------------------------------------------------------------------------ library
def test_library_exports_the_calibration_entry_points():
    if not os.path.exists(LIB):             # fresh checkout: the .so is git-ignored
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(LIB)
    names = ("als_category_profile", "als_calibrated_rerank", "als_list_miscalibration")
    for name in names:
        assert hasattr(lib, name), name
    from collaborative_filtering_amd import _hip
    assert set(names) <= set(_hip.EXPORTS)
    header = open(os.path.join(ROOT, "include", "als_hip.h")).read()
    assert all(f"int {name}(" in header for name in names)
    lib = _hip.load()                       # argument errors need no device: nothing is launched
    E_BADARG, E_BADK = -1, -2

    def prof(ncat=19, ldc=32, nrows=1, n=5):
        return lib.als_category_profile(ncat, ldc, nrows, None, None, None, n, None, None, None)

    def rer(ncat=19, ldc=32, nrows=1, n=5, pool=4, lam=0.5, alpha=0.01, topn=2):
        return lib.als_calibrated_rerank(ncat, ldc, nrows, n, None, None, pool, None, None, lam, alpha, topn, None,
                                         None, None, None, None)

    def mis(ncat=19, ldc=32, nrows=1, n=5, length=4, alpha=0.01):
        return lib.als_list_miscalibration(ncat, ldc, nrows, n, None, None, length, None, alpha, None, None)
    for f in (prof, rer, mis):
        assert f(ncat=0, ldc=16) == E_BADK and f(ncat=65, ldc=80) == E_BADK
        assert f(ldc=16) == E_BADK and f(ldc=19) == E_BADK and f(ncat=16, ldc=32) == E_BADK
        assert f() == E_BADARG                                            # null pointers
        assert f(nrows=-1) == E_BADARG and f(n=0) == E_BADARG
        assert f(nrows=0) == 0 and f(ncat=64, ldc=64, nrows=0) == 0 and f(ncat=1, ldc=16, nrows=0) == 0
    assert rer(pool=0, nrows=0) == E_BADARG and rer(pool=129, nrows=0) == E_BADARG
    assert rer(topn=0, nrows=0) == E_BADARG and rer(topn=5, nrows=0) == E_BADARG
    assert rer(lam=-0.1, nrows=0) == E_BADARG and rer(lam=1.5, nrows=0) == E_BADARG
    assert rer(lam=float("nan"), nrows=0) == E_BADARG
    for bad in (0.0, 1.0, -0.5, float("nan")):
        assert rer(alpha=bad, nrows=0) == E_BADARG and mis(alpha=bad, nrows=0) == E_BADARG
    assert mis(length=0, nrows=0) == E_BADARG and mis(length=129, nrows=0) == E_BADARG
