"""Top-N with per-group caps inside each list (ALS.recommend_quota, recommend_new_quota, cv.quota_at_k) without a GPU:
the streaming model of the kernel against the scan of the definition (tests/quota_ref.py), validation, the host clamp,
and the facade over the stand-in backend - every list compared with == against `greedy_capped` on `predict()` rows."""
import os

import numpy as np
import pytest
import torch

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, _hip, cv, serving
from collaborative_filtering_amd.serving import FoldedItems
from tests import quota_ref as qref
from tests.synth import make_ratings

M, N_ITEMS, K_F = 24, 310, 5          # n not a multiple of 32, ten bitmap words


@pytest.fixture(scope="module")
def fitted():
    r, c, v = make_ratings(M, N_ITEMS, 900, seed=5, empty_users=(3,))
    cfg = ALSConfig(core=CoreConfig(n_factors=K_F, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    model = ALS(cfg, device="cpu", backend=qref.QuotaNumpyBackend()).fit_coo(r, c, v, (M, N_ITEMS), tol=None, verbose=0)
    seen = [np.sort(c[r == u]) for u in range(M)]
    return model, seen


def _want(P, seen_rows, allowed, groups, cap, N):
    tv, ti, _ = qref.greedy_capped_batch(P, seen_rows, allowed, groups, cap, N)
    return ti.astype(np.int64), tv


def _assert_lists(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    assert got[0].shape == want[0].shape
    assert (got[0] == want[0]).all(), np.argwhere(got[0] != want[0])[:5]
    assert (got[1] == want[1]).all()


# ------------------------------------------------------------------------------------------ the streaming argument
def _instance(seed):
    """Tie-heavy scores and one of the label layouts of the issue, chosen by the seed."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 700))
    N = int(rng.integers(1, 33))
    scores = (rng.integers(-3, 4, size=n) * 0.5).astype(np.float32)        # 7 distinct values: the item id decides
    kind = seed % 6
    if kind == 0:                                                          # one group, cap 2
        groups, cap = np.zeros(n, np.int64), np.array([2])
    elif kind == 1:                                                        # one group holds 90 % of the items
        G = int(rng.integers(2, 6))
        groups = np.where(rng.random(n) < 0.9, 0, rng.integers(1, G, n))
        cap = rng.integers(0, 4, G)
    elif kind == 2:                                                        # every item its own group
        groups, cap = rng.permutation(n), rng.integers(0, 4, n)
    elif kind == 3:                                                        # a few groups, 30 % of the labels -1
        G = int(rng.integers(1, 41))
        groups = np.where(rng.random(n) < 0.3, -1, rng.integers(0, G, n))
        cap = rng.integers(0, 4, G)
    elif kind == 4:                                                        # caps of 0 on half of the groups
        G = int(rng.integers(2, 12))
        groups = rng.integers(0, G, n)
        cap = np.where(np.arange(G) % 2 == 0, 0, rng.integers(1, 4, G))
    else:                                                                  # 1 ... n groups, caps 0 ... 3
        G = int(rng.integers(1, n + 1))
        groups, cap = rng.integers(0, G, n), rng.integers(0, 4, G)
    cand = np.nonzero(rng.random(n) < rng.choice([1.0, 0.7, 0.2]))[0]
    arrival = seed % 3
    if arrival == 1:                                                       # best items last
        cand = cand[np.lexsort((-cand, scores[cand]))]
    elif arrival == 2:
        cand = rng.permutation(cand)
    return scores, cand, groups, cap, N


@pytest.mark.parametrize("seed", range(120))
def test_stream_model_equals_the_scan(seed):
    scores, cand, groups, cap, N = _instance(seed)
    allowed = np.zeros(scores.size, bool)
    allowed[cand] = True
    tv, ti, cnt = qref.greedy_capped(scores, [], allowed, groups, cap, N)
    want = list(zip((tv + 0.0).tolist(), ti.tolist()))
    for nslices in (1, 3, 7):
        got, compactions = qref.stream_model(scores, cand, groups, cap, N, nslices)
        assert got == want, (nslices, got[:5], want[:5])
    assert cnt == qref.n_eff(allowed, groups, cap, N) or cnt < N            # the clamp is the length of a full list
    assert cnt <= qref.n_eff(allowed, groups, cap, N)


def test_unfilled_list_compacts_all_along_and_the_clamp_stops_it():
    """One group with cap 2 and N = 10: the list never fills, the threshold stays open and every candidate is buffered;
    asked for N_eff = 2 entries instead, the same list fills at once and the buffer rarely does."""
    rng = np.random.default_rng(0)
    n = 2000
    scores = rng.normal(size=n).astype(np.float32)
    groups, cap = np.zeros(n, np.int64), np.array([2])
    slow, many = qref.stream_model(scores, np.arange(n), groups, cap, 10)
    assert qref.n_eff(None, groups, cap, 10) == 2
    fast, few = qref.stream_model(scores, np.arange(n), groups, cap, 2)
    assert slow == fast and len(fast) == 2
    assert many >= n // 96 and few <= 4


# ------------------------------------------------------------------------------------------ exports, validation
def test_exports_and_header_name_the_new_entry_point():
    assert "als_recommend_topk_quota" in _hip.EXPORTS
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "als_hip.h")).read()
    assert "int als_recommend_topk_quota(" in text
    assert "quota.hip" in open(os.path.join(root, "collaborative-filtering_amd", "csrc", "Makefile")).read()
    assert callable(cv.quota_at_k) and callable(ALS.recommend_quota) and callable(ALS.recommend_new_quota)


def test_arguments_are_validated(fitted):
    model = fitted[0]
    g = np.arange(N_ITEMS) % 7
    with pytest.raises(TypeError):
        model.recommend_quota([0, 1], 5, groups=g)                         # max_per_group is required
    with pytest.raises(TypeError):
        model.recommend_quota([0, 1], 5, max_per_group=2)
    with pytest.raises(ValueError, match="None is not accepted"):
        model.recommend_quota([0, 1], 5, groups=None, max_per_group=2)
    with pytest.raises(ValueError, match="None is not accepted"):
        model.recommend_quota([0, 1], 5, groups=g, max_per_group=None)
    with pytest.raises(ValueError, match="Expected number of items"):
        model.recommend_quota([0, 1], 5, groups=g[:-1], max_per_group=2)
    with pytest.raises(ValueError, match="Expected number of items"):
        model.recommend_quota([0, 1], 5, groups=g[:, None], max_per_group=2)
    with pytest.raises(ValueError, match="integers"):
        model.recommend_quota([0, 1], 5, groups=g.astype(np.float64), max_per_group=2)
    with pytest.raises(ValueError, match="integers"):
        model.recommend_quota([0, 1], 5, groups=g > 3, max_per_group=2)
    with pytest.raises(ValueError, match="integers"):
        model.recommend_quota([0, 1], 5, groups=g, max_per_group=2.0)
    with pytest.raises(ValueError, match="integers"):
        model.recommend_quota([0, 1], 5, groups=g, max_per_group=np.ones(7))
    with pytest.raises(ValueError, match=">= 0, or -1"):
        model.recommend_quota([0, 1], 5, groups=g - 2, max_per_group=2)
    with pytest.raises(ValueError, match="negative"):
        model.recommend_quota([0, 1], 5, groups=g, max_per_group=-1)
    with pytest.raises(ValueError, match="negative"):
        model.recommend_quota([0, 1], 5, groups=g, max_per_group=np.array([1, 1, -1, 1, 1, 1, 1]))
    with pytest.raises(ValueError, match="label 6 has no cap"):
        model.recommend_quota([0, 1], 5, groups=g, max_per_group=np.ones(6, np.int64))
    with pytest.raises(ValueError, match="1-D"):
        model.recommend_quota([0, 1], 5, groups=g, max_per_group=np.ones((7, 1), np.int64))
    with pytest.raises(ValueError):
        model.recommend_quota([0, 1], 129, groups=g, max_per_group=2)
    with pytest.raises(IndexError):
        model.recommend_quota([0, M], 5, groups=g, max_per_group=2)
    folded = _folded(np.random.default_rng(0))
    with pytest.raises(ValueError, match="Expected number of items"):      # the labels span n + B ids
        model.recommend_quota([0], 5, groups=g, max_per_group=2, new_items=folded)
    with pytest.raises(ValueError, match="None is not accepted"):
        model.recommend_new_quota(np.full((2, N_ITEMS), np.nan), 5, groups=None, max_per_group=1)
    # more caps than labels, tensors, and an empty batch are fine
    model.recommend_quota([0, 1], 5, groups=torch.from_numpy(g), max_per_group=torch.ones(9, dtype=torch.int64))
    empty = model.recommend_quota([], 4, groups=g, max_per_group=1)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 4)


def test_quota_plan_counts_over_the_allowed_catalogue():
    labels = np.array([0, 0, 0, 1, 1, -1, 2, 2, -1, 0], np.int32)
    caps = np.array([2, 5, 0], np.int32)
    allowed, ne = serving.quota_plan(None, labels, caps, 10)
    assert allowed.tolist() == [True] * 6 + [False, False, True, True]     # group 2 is closed
    assert ne == 2 + 2 + 2                                                 # min(2, 4) + min(5, 2) + two free items
    assert serving.quota_plan(None, labels, caps, 4)[1] == 4
    mask = np.array([1, 0, 0, 1, 0, 0, 1, 1, 1, 0], bool)
    allowed, ne = serving.quota_plan(mask, labels, caps, 10)
    assert allowed.tolist() == [True, False, False, True, False, False, False, False, True, False] and ne == 3
    assert serving.quota_plan(None, np.full(4, -1, np.int32), np.zeros(0, np.int32), 10) == (None, 4)
    assert serving.quota_plan(None, np.zeros(4, np.int32), np.zeros(1, np.int32), 10)[1] == 0


# ------------------------------------------------------------------------------------------ the facade
def _folded(rng, B=9):
    Z = rng.normal(size=(B, K_F)).astype(np.float32).astype(np.float64)
    return FoldedItems(Z.copy(), rng.normal(size=B).astype(np.float32).astype(np.float64) + 1.0, Z, None,
                       (np.zeros(B + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)))


@pytest.mark.parametrize("exclude_seen", [True, False])
def test_facade_equals_the_scan_on_predict_rows(fitted, monkeypatch, exclude_seen):
    model, seen = fitted
    be = model._eng.be
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)         # chunks of 7 rows
    rng = np.random.default_rng(3)
    P = model.predict()
    users = np.concatenate([np.arange(M)[::-1], np.arange(M), [5, 5, 5]])
    B = users.size
    rows_seen = [seen[u] if exclude_seen else np.zeros(0, np.int64) for u in users]
    groups = np.where(rng.random(N_ITEMS) < 0.3, -1, rng.integers(0, 12, N_ITEMS))
    cap = rng.integers(0, 4, 12)
    for N in (1, 7, 40):
        del be.calls[:]
        got = model.recommend_quota(users, N, groups=groups, max_per_group=cap, exclude_seen=exclude_seen)
        _assert_lists(got, _want(P[users], rows_seen, None, groups, cap, N))
        assert [c[1] for c in be.calls] == [7] * (B // 7) + ([B % 7] if B % 7 else [])
        assert {c[2] for c in be.calls} == {N}                             # enough free items: no clamp
    for g in range(12):                                                    # the caps hold
        for row in got[0]:
            assert (groups[row[row >= 0]] == g).sum() <= cap[g]
    # both filters, an id list and a mask; a scalar cap; users=None: all m users in id order
    allow = rng.permutation(N_ITEMS)[:220]
    block = rng.random(N_ITEMS) < 0.2
    ok = np.isin(np.arange(N_ITEMS), allow) & ~block
    got = model.recommend_quota(users, 7, groups=groups, max_per_group=cap, exclude_seen=exclude_seen, items=allow,
                                filter_items=block)
    _assert_lists(got, _want(P[users], rows_seen, ok, groups, cap, 7))
    assert ok[got[0][got[0] >= 0]].all()
    got = model.recommend_quota(None, 7, groups=groups, max_per_group=1, exclude_seen=exclude_seen)
    _assert_lists(got, _want(P, rows_seen[M: 2 * M], None, groups, np.ones(12, np.int64), 7))


def test_new_items_span_the_joint_catalogue(fitted, monkeypatch):
    model, seen = fitted
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)
    rng = np.random.default_rng(6)
    folded = _folded(rng)
    nt = N_ITEMS + folded.n_items
    users = np.concatenate([rng.integers(0, M, 30), np.arange(M)])
    P = np.concatenate([model.predict()[users], model.predict_new_items(folded, users)], axis=1)
    groups = rng.integers(-1, 5, nt)
    groups[N_ITEMS:] = 5                                                   # the folded items: a group of their own
    cap = np.array([1, 2, 0, 3, 1, 2])
    block = rng.random(nt) < 0.1
    got = model.recommend_quota(users, 9, groups=groups, max_per_group=cap, new_items=folded, filter_items=block)
    _assert_lists(got, _want(P, [seen[u] for u in users], ~block, groups, cap, 9))
    assert ((got[0] >= N_ITEMS).sum(axis=1) <= 2).all() and (got[0] >= N_ITEMS).any()


def _new_user_scores(model, R_new):
    """The score rows of folded-in users: the predict epilogue on their folded factors, through the model's backend."""
    eng = model._eng
    U, b = model.fold_in(R_new)
    Ut = torch.zeros(U.shape[0], eng.ld, dtype=torch.float32)
    Ut[:, : eng.k] = torch.from_numpy(U).float()
    out = torch.empty(U.shape[0], eng.n, dtype=torch.float32, device=eng.dev)
    eng.be.predict_dense(k=eng.k, ld=eng.ld, m=U.shape[0], n=eng.n, U=Ut.to(eng.dev), Z=eng.V,
                         b_u=torch.from_numpy(b).float().to(eng.dev), b_i=eng.b_i, mu=eng.mu, out=out)
    return out.cpu().numpy().astype(np.float64)


def test_recommend_new_quota_equals_the_scan(fitted, monkeypatch):
    model = fitted[0]
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)
    rng = np.random.default_rng(4)
    B = 20
    R_new = np.full((B, N_ITEMS), np.nan)
    for b in range(B):
        if b != 4:                                                         # one row without ratings
            R_new[b, rng.permutation(N_ITEMS)[: 3 + b % 9]] = rng.integers(1, 6, 3 + b % 9)
    P = _new_user_scores(model, R_new)
    groups = rng.integers(-1, 30, N_ITEMS)
    cap = rng.integers(0, 3, 30)
    for exclude_seen in (True, False):
        rows_seen = [np.nonzero(~np.isnan(R_new[b]))[0] if exclude_seen else np.zeros(0, np.int64) for b in range(B)]
        got = model.recommend_new_quota(R_new, 6, groups=groups, max_per_group=cap, exclude_seen=exclude_seen)
        _assert_lists(got, _want(P, rows_seen, None, groups, cap, 6))


def test_loose_caps_are_recommend(fitted):
    model = fitted[0]
    users = np.concatenate([np.arange(M), np.arange(M)])
    g = np.arange(N_ITEMS) % 3
    want = model.recommend(users, 9)
    for groups, cap in ((g, 9), (g, np.array([9, 50, 1 << 40])), (np.full(N_ITEMS, -1), 0),
                        (np.arange(N_ITEMS), 1)):                          # every item its own group
        got = model.recommend_quota(users, 9, groups=groups, max_per_group=cap)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    # a cap of 0 is a block list over the group
    got = model.recommend_quota(users, 9, groups=g, max_per_group=np.array([9, 0, 9]))
    want = model.recommend(users, 9, filter_items=g == 1)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


def test_the_clamp_gives_short_rows_and_the_kernel_a_list_that_fills(fitted):
    model, seen = fitted
    be = model._eng.be
    users = np.arange(M)
    groups = np.arange(N_ITEMS) % 3
    cap = np.array([2, 2, 2])                                              # 3 groups x cap 2 < N = 10
    del be.calls[:]
    got = model.recommend_quota(users, 10, groups=groups, max_per_group=cap, exclude_seen=False)
    assert be.calls == [("recommend_topk_quota", M, 6)]                    # N_eff = 6
    _assert_lists(got, _want(model.predict(), [np.zeros(0, np.int64)] * M, None, groups, cap, 10))
    assert (got[0][:, :6] >= 0).all() and (got[0][:, 6:] == -1).all() and np.isneginf(got[1][:, 6:]).all()
    # counted over the allowed catalogue: group 0 has one allowed item left, and one free item joins
    groups = groups.copy()
    groups[7] = -1
    allow = np.concatenate([[0], np.nonzero(groups != 0)[0]])
    del be.calls[:]
    got = model.recommend_quota(users, 10, groups=groups, max_per_group=cap, items=allow)
    assert be.calls == [("recommend_topk_quota", M, 1 + 2 + 2 + 1)]
    ok = np.isin(np.arange(N_ITEMS), allow)
    _assert_lists(got, _want(model.predict(), seen, ok, groups, cap, 10))
    # nothing can be taken: no kernel call at all
    del be.calls[:]
    got = model.recommend_quota(users, 5, groups=np.zeros(N_ITEMS, np.int64), max_per_group=0)
    assert be.calls == [] and (got[0] == -1).all() and np.isneginf(got[1]).all()


# ------------------------------------------------------------------------------------------ cv
def test_quota_at_k_hand_checked(fitted):
    model = fitted[0]
    users = np.array([0, 1])
    top = model.recommend(users, 4)[0]
    rows, cols = users, top[:, 1]                                          # held out: each user's second-best item
    # user 0's two best items share group 0, user 1's two best share group 1; everything else has no group
    groups = np.full(N_ITEMS, -1)
    groups[top[0, :2]] = 0
    groups[top[1, :2]] = 1
    assert (groups[top[0]] >= 0).sum() == 2 and (groups[top[1]] >= 0).sum() == 2   # the lists do not cross
    loose = cv.quota_at_k(model, rows, cols, K=4, groups=groups, max_per_group=2)
    assert loose["users"] == 2 and loose["recall@K"] == loose["recall@K_uncapped"] == 1.0
    assert loose["ndcg@K"] == loose["ndcg@K_uncapped"]
    assert loose["groups_per_list"] == loose["groups_per_list_uncapped"] == 3.0    # one group and two free items
    assert loose["max_group_share"] == loose["max_group_share_uncapped"] == 0.5
    tight = cv.quota_at_k(model, rows, cols, K=4, groups=groups, max_per_group=1)
    capped = model.recommend_quota(users, 4, groups=groups, max_per_group=1)[0]
    assert (capped[:, 0] == top[:, 0]).all() and (capped[:, 1] == top[:, 2]).all()  # the second-best item is dropped
    assert tight["recall@K"] == 0.0 and tight["recall@K_uncapped"] == 1.0
    assert tight["groups_per_list"] == 4.0 and tight["max_group_share"] == 0.25
    assert tight["groups_per_list_uncapped"] == 3.0 and tight["max_group_share_uncapped"] == 0.5
    with pytest.raises(ValueError):
        cv.quota_at_k(model, rows, cols, K=4, groups=None, max_per_group=1)
