"""ALS.recommend_group / cv.group_ranking_at_k host logic, without a GPU: the engine runs on the numpy stand-in backend,
whose group_topk is the kernel's contract in tests/group_ref.py."""
import numpy as np
import pytest

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, cv, validate
from tests import serving_ref as ref
from tests.group_ref import AGGREGATES, GroupNumpyBackend, group_scores
from tests.synth import make_features, make_ratings

M, N_ITEMS, K = 30, 25, 5
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
    cfg = ALSConfig(core=CoreConfig(n_factors=K, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    be = GroupNumpyBackend()
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


GROUPS = [[0, 1, 2], [7], [5, NOTHING], [3, 8, 9, 10, 12, 13, 14], [2, 1, 0], [7], [20, 21], [NOTHING],
          [6, EVERYTHING], [29, 0, 15, 16]]


def _brute(P, groups, seen, N, aggregate, ok=None, exclude=True):
    """The lists of `groups` from a completion P [m, items] (float64 holding fp32 values), written out again: the
    aggregate by the docstring of ALS.recommend_group, the items any member has seen left out."""
    P32 = P.astype(np.float32)
    rows, out = [], []
    for g in groups:
        g = np.asarray(g)
        if aggregate == "min":
            rows.append(P32[g].min(axis=0))
        elif aggregate == "max":
            rows.append(P32[g].max(axis=0))
        else:
            rows.append(np.float32(P32[g].astype(np.float64).sum(axis=0) / len(g)))
        out.append(np.unique(np.concatenate([seen[u] for u in g])) if exclude else np.zeros(0, np.int64))
    tv, ti, tc = ref.topn_batch(np.stack(rows).astype(np.float32), out, ok, N)
    return ti.astype(np.int64), tv.astype(np.float64), tc


def _same(got, exp):
    assert (got[0] == exp[0]).all() and (got[1] == exp[1]).all()


# ----------------------------------------------------------------------------------------- validate.user_groups
def test_user_groups_ragged_and_2d():
    ptr, users = validate.user_groups([[3, 1], np.array([2]), (0, 5, 4)], 6)
    assert ptr.dtype == np.int64 and users.dtype == np.int32
    assert ptr.tolist() == [0, 2, 3, 6] and users.tolist() == [3, 1, 2, 0, 5, 4]
    ptr, users = validate.user_groups(np.array([[1, 2], [2, 1], [0, 3]]), 4)
    assert ptr.tolist() == [0, 2, 4, 6] and users.tolist() == [1, 2, 2, 1, 0, 3]
    ptr, users = validate.user_groups([], 4)
    assert ptr.tolist() == [0] and users.size == 0 and users.dtype == np.int32
    ptr, users = validate.user_groups([np.arange(64)], 64)                 # the limit itself is fine
    assert ptr.tolist() == [0, 64]


def test_user_groups_rejections():
    with pytest.raises(ValueError, match="group 1 is empty"):
        validate.user_groups([[0], []], 5)
    with pytest.raises(ValueError, match=r"group 0: user ids must lie in \[0, 5\)"):
        validate.user_groups([[0, 5]], 5)
    with pytest.raises(ValueError, match=r"group 2: user ids must lie in \[0, 5\)"):
        validate.user_groups([[0], [1], [-1, 2]], 5)
    with pytest.raises(ValueError, match="group 1 names a user more than once"):
        validate.user_groups([[0, 1], [3, 2, 3]], 5)
    with pytest.raises(ValueError, match="group 0 has 65 members; a group holds at most 64"):
        validate.user_groups([np.arange(65)], 100)
    with pytest.raises(ValueError, match="at most 64"):
        validate.user_groups(np.arange(130).reshape(2, 65), 200)
    with pytest.raises(ValueError, match="integer user ids"):
        validate.user_groups([[0.5, 1.0]], 5)
    with pytest.raises(ValueError, match="integer user ids"):
        validate.user_groups(np.zeros((2, 2)), 5)
    with pytest.raises(ValueError, match="1-D array"):
        validate.user_groups([[[0, 1]]], 5)
    with pytest.raises(ValueError, match="1-D array"):
        validate.user_groups([0, 1], 5)                                     # ids, not groups
    with pytest.raises(ValueError):
        validate.user_groups(np.zeros((1, 2, 2), dtype=np.int64), 5)
    with pytest.raises(ValueError):
        validate.user_groups(3, 5)


def test_bad_aggregate_and_bad_N(fitted):
    model = fitted[0]
    for a in ("median", "MEAN", None, 0):
        with pytest.raises(ValueError, match="aggregate must be one of"):
            model.recommend_group([[0, 1]], 3, aggregate=a)
    for N in (0, 129, -1, 2.0, True):
        with pytest.raises(ValueError):
            model.recommend_group([[0, 1]], N)
    with pytest.raises(ValueError, match="group 0 names a user more than once"):
        model.recommend_group([[1, 1]], 3)
    with pytest.raises(ValueError, match=rf"user ids must lie in \[0, {M}\)"):
        model.recommend_group([[0, M]], 3)


def test_before_fit_raises_like_recommend():
    cfg = ALSConfig(core=CoreConfig(n_factors=3, n_iters=1, lambda_u=1.0, lambda_v=1.0))
    model = ALS(cfg, device="cpu", backend=GroupNumpyBackend())
    with pytest.raises(RuntimeError, match="Model must be fitted before prediction."):
        model.recommend_group([[0]])


# ----------------------------------------------------------------------------------------- the reference itself
def test_the_reference_has_the_products_aggregates_propagates_nan_and_rounds_the_mean_once():
    assert AGGREGATES == validate.GROUP_AGGREGATES and validate.GROUP_MAX_MEMBERS == 64
    s = np.array([[1.0, np.nan, 3.0, np.inf], [2.0, 0.5, np.nan, -np.inf], [4.0, 9.0, 1.0, 1.0]], np.float32)
    for a in ("min", "max", "mean"):
        g = group_scores(s, a)
        assert g.dtype == np.float32 and np.isnan(g[1]) and np.isnan(g[2])
    assert group_scores(s, "min")[0] == 1.0 and group_scores(s, "max")[0] == 4.0
    assert group_scores(s, "min")[3] == -np.inf and group_scores(s, "max")[3] == np.inf
    assert np.isnan(group_scores(s, "mean")[3])
    t = np.array([[1.0], [1.0], [np.float32(1.0) + np.float32(2.0 ** -23)]], np.float32)
    exact = (2.0 + float(t[2, 0])) / 3.0
    assert group_scores(t, "mean")[0] == np.float32(exact)


# ----------------------------------------------------------------------------------------- recommend_group
def test_shapes_dtypes_and_empty_batch(fitted):
    model, be, seen = fitted
    items, scores = model.recommend_group(GROUPS, 4)
    assert items.shape == scores.shape == (len(GROUPS), 4)
    assert items.dtype == np.int64 and scores.dtype == np.float64
    assert model.recommend_group(GROUPS)[0].shape == (len(GROUPS), 10)
    items, scores = model.recommend_group([], 5)
    assert items.shape == scores.shape == (0, 5) and items.dtype == np.int64 and scores.dtype == np.float64


@pytest.mark.parametrize("aggregate", AGGREGATES)
def test_scores_are_the_aggregate_of_predict_exactly(fitted, fitted_feat, aggregate):
    for model, seen, feats in ((fitted[0], fitted[2], None), (fitted_feat[0], fitted_feat[2], fitted_feat[3]),
                               (fitted_feat[0], fitted_feat[2], None)):
        P = model.predict(feats)
        for N in (1, 10, 128):
            _same(model.recommend_group(GROUPS, N, aggregate=aggregate, features=feats),
                  _brute(P, GROUPS, seen, N, aggregate))
            _same(model.recommend_group(GROUPS, N, aggregate=aggregate, features=feats, exclude_seen=False),
                  _brute(P, GROUPS, seen, N, aggregate, exclude=False))
        items, scores = model.recommend_group(GROUPS, 6, aggregate=aggregate, features=feats)
        assert (scores[:, 1:] <= scores[:, :-1]).all()
    model, be, seen, feats = fitted_feat
    assert (model.recommend_group(GROUPS, 6, aggregate=aggregate, features=feats)[1]
            != model.recommend_group(GROUPS, 6, aggregate=aggregate)[1]).any()


def test_order_and_repeated_groups_are_kept(fitted):
    model, be, seen = fitted
    full = model.recommend_group(GROUPS, 5, aggregate="min")
    assert (full[0][1] == full[0][5]).all() and (full[1][1] == full[1][5]).all()          # [7] twice
    # [0, 1, 2] and [2, 1, 0]: the same members in another order - min and max do not care
    assert (full[0][0] == full[0][4]).all() and (full[1][0] == full[1][4]).all()
    sub = [8, 3, 3, 0]
    _same(model.recommend_group([GROUPS[i] for i in sub], 5, aggregate="min"), (full[0][sub], full[1][sub]))
    as2d = np.array([[0, 1, 2], [2, 1, 0], [9, 3, 8]])
    _same(model.recommend_group(as2d, 5, aggregate="max"), model.recommend_group(list(as2d), 5, aggregate="max"))


def test_an_item_seen_by_any_member_is_left_out(fitted):
    model, be, seen = fitted
    assert seen[NOTHING].size == 0 and seen[EVERYTHING].size == N_ITEMS
    items, scores = model.recommend_group(GROUPS, N_ITEMS)
    for b, g in enumerate(GROUPS):
        union = np.unique(np.concatenate([seen[u] for u in g]))
        got = items[b][items[b] >= 0]
        assert not np.isin(got, union).any() and got.size == N_ITEMS - union.size
        assert np.isneginf(scores[b][items[b] < 0]).all()
    # a member without ratings adds nothing: [5, NOTHING] leaves out what [5] leaves out
    assert (np.sort(items[2][items[2] >= 0]) == np.sort(np.setdiff1d(np.arange(N_ITEMS), seen[5]))).all()
    # the user without ratings alone: every item is a candidate
    assert (np.sort(items[7]) == np.arange(N_ITEMS)).all()
    # a member who has seen everything empties the list
    assert (items[8] == -1).all() and np.isneginf(scores[8]).all()
    assert (model.recommend_group([[6, EVERYTHING]], N_ITEMS, exclude_seen=False)[0] >= 0).all()


@pytest.mark.parametrize("aggregate", AGGREGATES)
def test_a_group_of_one_is_recommend(fitted, aggregate):
    model, be, seen = fitted
    users = np.array([7, NOTHING, EVERYTHING, 0, 7])
    for N in (1, 10, 128):
        _same(model.recommend_group(users[:, None], N, aggregate=aggregate), model.recommend(users, N))
        _same(model.recommend_group(users[:, None], N, aggregate=aggregate, exclude_seen=False),
              model.recommend(users, N, exclude_seen=False))


def test_chunks_are_crossed_and_what_each_launch_reads(fitted_feat, monkeypatch):
    model, be, seen, feats = fitted_feat
    eng = model._eng
    base = model.recommend_group(GROUPS, 4, aggregate="min")
    base_f = model.recommend_group(GROUPS, 4, aggregate="min", features=feats)
    monkeypatch.setattr(eng, "REC_BATCH", 3, raising=False)
    del be.calls[:]
    _same(model.recommend_group(GROUPS, 4, aggregate="min"), base)
    calls = [c for c in be.calls if c[0] == "group_topk"]
    assert [c[1] for c in calls] == [3, 3, 3, 1]
    # without features the item table is V itself; one seen row per batch group of the chunk; no bitmap
    assert all(c[2] == eng.V.data_ptr() and c[3] == N_ITEMS and c[4] == c[1] + 1 and c[5] is None for c in calls)
    assert [c[6] for c in calls] == [3, 7, 2, 4]                                     # the chunk's largest group
    assert all(c[7] == "min" for c in calls)
    del be.calls[:]
    _same(model.recommend_group(GROUPS, 4, aggregate="min", features=feats), base_f)
    calls = [c for c in be.calls if c[0] == "group_topk"]
    assert len({c[2] for c in calls}) == 1 and calls[0][2] != eng.V.data_ptr()       # one composed Z for all chunks
    del be.calls[:]
    got = model.recommend_group(GROUPS, 4, aggregate="max", exclude_seen=False, items=np.arange(0, N_ITEMS, 2))
    allowed = np.isin(np.arange(N_ITEMS), np.arange(0, N_ITEMS, 2))
    _same(got, _brute(model.predict(), GROUPS, seen, 4, "max", allowed, exclude=False))
    calls = [c for c in be.calls if c[0] == "group_topk"]
    assert all(c[4] is None for c in calls)                                          # no seen CSR
    assert calls[0][5] is not None and len({c[5] for c in calls}) == 1               # one bitmap per call
    assert not any(c[0] in ("recommend_topk", "recommend_topk_masked", "audience_topk") for c in be.calls)


@pytest.mark.parametrize("aggregate", AGGREGATES)
def test_allow_and_block_lists_as_ids_and_masks(fitted, aggregate):
    model, be, seen = fitted
    P = model.predict()
    rng = np.random.default_rng(0)
    allow = rng.permutation(N_ITEMS)[:11]
    block = rng.random(N_ITEMS) < 0.3
    inl = np.isin(np.arange(N_ITEMS), allow)
    cases = [(dict(items=allow), inl), (dict(items=inl), inl), (dict(filter_items=np.nonzero(block)[0]), ~block),
             (dict(filter_items=block), ~block),
             (dict(items=np.concatenate([allow, allow[:2]]), filter_items=block), inl & ~block)]
    for kw, ok in cases:
        items, scores = model.recommend_group(GROUPS, 6, aggregate=aggregate, **kw)
        _same((items, scores), _brute(P, GROUPS, seen, 6, aggregate, ok))
        assert ok[items[items >= 0]].all()
    items, scores = model.recommend_group([[1, 2]], 5, items=[])                     # an empty allow-list
    assert (items == -1).all() and np.isneginf(scores).all()
    with pytest.raises(ValueError, match=rf"items: item ids must lie in \[0, {N_ITEMS}\)"):
        model.recommend_group([[1, 2]], 5, items=[N_ITEMS])


@pytest.mark.parametrize("aggregate", AGGREGATES)
def test_new_items(fitted, aggregate):
    model, be, seen = fitted
    rng = np.random.default_rng(5)
    B = 4
    C_new = np.full((B, M), np.nan)
    for b in range(B - 1):                                                # the last one: no ratings
        C_new[b, rng.permutation(M)[: 5 + 3 * b]] = rng.integers(1, 6, 5 + 3 * b)
    folded = model.fold_in_items(C_new)
    Pj = np.concatenate([model.predict(), model.predict_new_items(folded)], axis=1)
    nt = N_ITEMS + B
    sj = [np.concatenate([seen[u], N_ITEMS + np.nonzero(~np.isnan(C_new[:, u]))[0]]) for u in range(M)]
    assert any(np.isin(sj[u], np.arange(N_ITEMS, nt)).any() for g in GROUPS for u in g)
    for N in (3, nt):
        _same(model.recommend_group(GROUPS, N, aggregate=aggregate, new_items=folded),
              _brute(Pj, GROUPS, sj, N, aggregate))
    _same(model.recommend_group(GROUPS, 5, aggregate=aggregate, new_items=folded, exclude_seen=False),
          _brute(Pj, GROUPS, sj, 5, aggregate, exclude=False))
    only_new = np.arange(nt) >= N_ITEMS
    _same(model.recommend_group(GROUPS, 5, aggregate=aggregate, new_items=folded, items=only_new),
          _brute(Pj, GROUPS, sj, 5, aggregate, only_new))
    with pytest.raises(ValueError):
        model.recommend_group(GROUPS, 3, new_items="folded")
    with pytest.raises(ValueError):
        model.recommend_group(GROUPS, 3, items=[N_ITEMS])                  # a folded id without new_items


def test_joint_tables_of_a_call_with_new_items(fitted):
    model, be, seen = fitted
    C_new = np.full((3, M), np.nan)
    C_new[0, [2, 5]] = 4.0
    folded = model.fold_in_items(C_new)
    del be.calls[:]
    model.recommend_group([[2, 3], [5]], 3, new_items=folded)
    (call,) = [c for c in be.calls if c[0] == "group_topk"]
    assert call[3] == N_ITEMS + 3 and call[4] == 2 + 1                      # joint table, one seen row per group


# ----------------------------------------------------------------------------------------- cv.group_ranking_at_k
def test_group_ranking_at_k_against_a_numpy_restatement(fitted):
    model, be, seen = fitted
    rng = np.random.default_rng(2)
    R = np.zeros((M, N_ITEMS), bool)
    for u in range(M):
        R[u, seen[u]] = True
    free = np.argwhere(~R)
    held = free[rng.permutation(len(free))[:150]]
    rows, cols = held[:, 0], held[:, 1]
    vals = rng.integers(1, 11, size=rows.size) * 0.5
    groups = [[0, 1, 2], [3, 8, 9, 10, 12], [5, NOTHING], [0, 1, 2], [6, EVERYTHING], [20, 21, 22, 23]]

    def brute(rows, cols, Kk, aggregate):
        rec_mean, rec_min, nd_mean, nd_min, members = [], [], [], [], 0
        disc = 1.0 / np.log2(np.arange(2, Kk + 2))
        for g in groups:
            union = set(np.concatenate([seen[u] for u in g]).tolist())
            per = []
            for u in g:
                rel = set(cols[rows == u].tolist()) - union
                if rel:
                    per.append(rel)
            if not per:
                continue
            top = model.recommend_group([g], Kk, aggregate=aggregate)[0][0]
            rec, nd = [], []
            for rel in per:
                hits = np.array([i in rel for i in top], dtype=np.float64)
                rec.append(hits.sum() / len(rel))
                nd.append((hits * disc).sum() / disc[: min(Kk, len(rel))].sum())
            members += len(per)
            rec_mean.append(np.mean(rec)); rec_min.append(np.min(rec))
            nd_mean.append(np.mean(nd)); nd_min.append(np.min(nd))
        return len(rec_mean), members, np.mean(rec_mean), np.mean(rec_min), np.mean(nd_mean), np.mean(nd_min)

    def check(got, exp):
        assert (got["groups"], got["members"]) == exp[:2]
        assert got["recall@K"]["mean_member"] == pytest.approx(exp[2], abs=1e-12)
        assert got["recall@K"]["min_member"] == pytest.approx(exp[3], abs=1e-12)
        assert got["ndcg@K"]["mean_member"] == pytest.approx(exp[4], abs=1e-12)
        assert got["ndcg@K"]["min_member"] == pytest.approx(exp[5], abs=1e-12)

    for aggregate in AGGREGATES:
        for Kk in (1, 5, 10):
            exp = brute(rows, cols, Kk, aggregate)
            assert exp[0] >= 4 and exp[1] > exp[0]
            check(cv.group_ranking_at_k(model, groups, rows, cols, K=Kk, aggregate=aggregate), exp)
    keep = vals >= 3.0
    check(cv.group_ranking_at_k(model, groups, rows, cols, vals, K=5, aggregate="min", min_rating=3.0),
          brute(rows[keep], cols[keep], 5, "min"))
    # a held-out item that a fellow member has in training cannot be a candidate: adding such pairs changes nothing
    fellow_item = seen[1][~np.isin(seen[1], seen[0])][:2]
    assert fellow_item.size == 2
    rows2, cols2 = np.concatenate([rows, [0, 0]]), np.concatenate([cols, fellow_item])
    assert (cv.group_ranking_at_k(model, [[0, 1, 2]], rows2, cols2, K=5)
            == cv.group_ranking_at_k(model, [[0, 1, 2]], rows, cols, K=5))
    # [6, EVERYTHING]: nothing is a candidate, so nobody in it is evaluated
    assert cv.group_ranking_at_k(model, [[6, EVERYTHING]], rows, cols, K=5)["groups"] == 0
    empty = cv.group_ranking_at_k(model, groups, [], [], K=5)
    assert empty["groups"] == 0 and empty["members"] == 0
    assert np.isnan(empty["recall@K"]["mean_member"]) and np.isnan(empty["ndcg@K"]["min_member"])
    with pytest.raises(ValueError, match="min_rating needs"):
        cv.group_ranking_at_k(model, groups, rows, cols, min_rating=3.0)
    with pytest.raises(ValueError, match="aggregate must be one of"):
        cv.group_ranking_at_k(model, groups, rows, cols, aggregate="median")


def test_library_exports_the_new_symbols():
    import os
    import __graft_entry__ as ge
    from collaborative_filtering_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    lib = _hip.load()
    for name in ("als_group_workspace_bytes", "als_group_topk"):
        assert hasattr(lib, name)
    assert lib.als_group_workspace_bytes(3, 5003, 10, 1) == 0
    assert lib.als_group_workspace_bytes(3, 5003, 10, 7) == 7 * 3 * 10 * 8
    assert lib.als_group_workspace_bytes(3, 5003, 129, 7) == 0
    assert lib.als_group_workspace_bytes(0, 5003, 10, 7) == 0
