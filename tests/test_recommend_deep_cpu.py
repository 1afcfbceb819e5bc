"""ALS.recommend_deep / recommend_new_deep host logic, without a GPU: the engine runs on the numpy stand-in backend,
whose recommend_deep is the kernel's contract in tests/recommend_deep_ref.py."""
import os
import re

import numpy as np
import pytest

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, serving, validate
from tests import recommend_deep_ref as dref
from tests.synth import make_features, make_ratings

M, N_ITEMS, K = 24, 310, 5
NOTHING = 4                         # a user without a rating
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fit(features=None):
    r, c, v = make_ratings(M, N_ITEMS, 900, seed=3, empty_users=(NOTHING,))
    cfg = ALSConfig(core=CoreConfig(n_factors=K, n_iters=2, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    be = dref.DeepNumpyBackend()
    kw = dict(lambda_w={f: 1.0 for f in features}) if features else {}
    model = ALS(cfg, device="cpu", backend=be, **kw)
    model.fit_coo(r, c, v, (M, N_ITEMS), features=features, tol=None, verbose=0)
    return model, be, [np.sort(c[r == u]) for u in range(M)]


@pytest.fixture(scope="module")
def fitted():
    return _fit()


@pytest.fixture(scope="module")
def fitted_feat():
    G, y = make_features(N_ITEMS, seed=4)
    feats = {"genres": G, "years": y}
    return _fit(feats) + (feats,)


def _expect(P, users, seen, N, ok=None, after=None, exclude=True):
    S = P.astype(np.float32)[np.asarray(users)]
    rows = [seen[u] if exclude else np.zeros(0, np.int64) for u in users]
    tv, ti, _ = dref.deep_topn_batch(S, rows, ok, N, after=after)
    return ti.astype(np.int64), tv.astype(np.float64)


def _same(got, exp):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    assert got[0].shape == exp[0].shape and (got[0] == exp[0]).all() and (got[1] == exp[1]).all()


def _page_through(call, B, N):
    """Pages of `call(after)` until every row came back short: per row the concatenated ids."""
    out = [[] for _ in range(B)]
    after = None
    for _ in range(10_000):
        items, scores = call(after)
        for b in range(B):
            out[b].extend(items[b][items[b] >= 0].tolist())
        if (items[:, -1] < 0).all():
            return out
        after = (items[:, -1], scores[:, -1])
    raise AssertionError("paging does not end")


# ----------------------------------------------------------------------------------------- validation
@pytest.mark.parametrize("N", [0, 1025, -1, 2.0, True])
def test_bad_N(fitted, N):
    model = fitted[0]
    with pytest.raises(ValueError, match=r"N must be an integer in \[1, 1024\]"):
        model.recommend_deep([0], N)
    with pytest.raises(ValueError, match=r"N must be an integer in \[1, 1024\]"):
        model.recommend_new_deep(np.full((1, N_ITEMS), np.nan), N)


def test_limits_are_named_and_the_old_one_stands():
    assert serving.RECOMMEND_DEEP_MAX_N == 1024 and serving.RECOMMEND_MAX_N == 128
    assert validate.deep_topn(1024) == 1024 and validate.deep_topn(np.int64(1)) == 1
    with pytest.raises(ValueError):
        validate.top_count(129, "N")


@pytest.mark.parametrize("after", [
    ([1, 2],),                                           # not a pair
    ([1, 2, 3], [0.0, 0.0]),                             # shapes
    ([[1, 2]], [[0.0, 0.0]]),
    ([1.0, 2.0], [0.0, 0.0]),                            # ids not integers
    ([True, False], [0.0, 0.0]),
    ([1, N_ITEMS], [0.0, 0.0]),                          # out of range
    ([-2, 1], [0.0, 0.0]),
    ([1, 2], [0.0, np.nan]),                             # NaN score
    ([1, 2], ["a", "b"]),
])
def test_bad_after(fitted, after):
    with pytest.raises(ValueError):
        fitted[0].recommend_deep([0, 1], 10, after=after)


def test_after_accepts_padding_and_infinities():
    it, sc = validate.deep_cursor(([-1, 3, 0], [-np.inf, np.inf, 1]), 3, 5)
    assert it.dtype == np.int64 and sc.dtype == np.float64 and it.tolist() == [-1, 3, 0]
    assert validate.deep_cursor(None, 3, 5) is None


def test_before_fit_raises_like_recommend():
    cfg = ALSConfig(core=CoreConfig(n_factors=K, n_iters=1, lambda_u=2.0, lambda_v=2.0))
    with pytest.raises(RuntimeError, match="fitted"):
        ALS(cfg, device="cpu", backend=dref.DeepNumpyBackend()).recommend_deep([0], 200)


def test_cursor_keys_are_the_headers_keys_and_order_like_the_entries():
    rng = np.random.default_rng(0)
    s = np.concatenate([rng.normal(size=50), [0.0, -0.0, np.inf, -np.inf, 1.5, 1.5, -2.0, -2.0]]).astype(np.float32)
    i = rng.integers(0, 2 ** 31 - 1, size=s.size)
    got = serving.cursor_keys(i.astype(np.int64), s.astype(np.float64)).view(np.uint64)
    assert (got == dref.keys(s, i)).all()
    assert (serving.cursor_keys(np.array([-1, -1]), np.array([3.0, -np.inf])) == 0).all()
    # key order == (score descending, item ascending), -0.0 and +0.0 one score
    for a in range(s.size):
        for b in range(s.size):
            before = s[a] > s[b] or (s[a] == s[b] and i[a] < i[b])
            assert (got[a] > got[b]) == before
    row = s.copy()
    for a in (3, 50, 51, 52, 53, 54, 57):
        assert (dref.below_key(row, dref.keys(row[a], a)) == dref.below_entry(row, a, row[a])).all()


# ----------------------------------------------------------------------------------------- results
def test_equals_recommend_up_to_128(fitted, fitted_feat):
    for model, feats in ((fitted[0], None), (fitted_feat[0], fitted_feat[3])):
        for N in (1, 10, 128):
            for kw in (dict(), dict(exclude_seen=False), dict(users=[3, NOTHING, 3, 0]),
                       dict(items=np.arange(0, N_ITEMS, 3), filter_items=[0, 3, 9])):
                _same(model.recommend_deep(N=N, features=feats, **kw), model.recommend(N=N, features=feats, **kw))


@pytest.mark.parametrize("N", [129, 200, 310, 1024])
def test_long_lists_are_the_reference_on_predict(fitted, N):
    model, be, seen = fitted
    P = model.predict()
    users = [0, NOTHING, 7, 0, 23]
    got = model.recommend_deep(users, N)
    _same(got, _expect(P, users, seen, N))
    cnt = (got[0] >= 0).sum(axis=1)
    assert (cnt == [min(N, N_ITEMS - len(seen[u])) for u in users]).all()
    assert (got[0][np.arange(len(users))[:, None], np.arange(N)[None, :]][got[0] < 0] == -1).all()
    assert np.isneginf(got[1][got[0] < 0]).all()
    _same(model.recommend_deep(users, N, exclude_seen=False), _expect(P, users, seen, N, exclude=False))
    allu = model.recommend_deep(N=N)
    assert allu[0].shape == (M, N)
    _same(allu, _expect(P, list(range(M)), seen, N))


def test_shapes_dtypes_and_empty_batch(fitted):
    items, scores = fitted[0].recommend_deep([], 300)
    assert items.shape == (0, 300) and items.dtype == np.int64 and scores.dtype == np.float64
    items, scores = fitted[0].recommend_new_deep(np.empty((0, N_ITEMS)), 300, after=([], []))
    assert items.shape == (0, 300)


@pytest.mark.parametrize("N", [1, 7, 128, 129, 1000])
def test_paging_enumerates_every_candidate_once_in_order(fitted, N):
    model, be, seen = fitted
    P32 = model.predict().astype(np.float32)
    users = [0, NOTHING, 7, 13]
    if N == 1:
        users = [7]
    pages = _page_through(lambda after: model.recommend_deep(users, N, after=after), len(users), N)
    for b, u in enumerate(users):
        assert pages[b] == dref.full_order(P32[u], seen[u], None).tolist()


def test_second_page_is_the_tail_of_a_longer_list_and_padding_ends_it(fitted):
    model, be, seen = fitted
    users = [0, 7, NOTHING, 13]
    both = model.recommend_deep(users, 300)
    first = model.recommend_deep(users, 150)
    second = model.recommend_deep(users, 150, after=(first[0][:, -1], first[1][:, -1]))
    _same(second, (both[0][:, 150:], both[1][:, 150:]))
    done = model.recommend_deep(users, 150, after=(np.full(4, -1), np.full(4, -np.inf)))
    assert (done[0] == -1).all() and np.isneginf(done[1]).all()
    mixed = model.recommend_deep(users, 150, after=(np.array([-1, first[0][1, -1], -1, first[0][3, -1]]),
                                                    np.array([0.0, first[1][1, -1], 0.0, first[1][3, -1]])))
    assert (mixed[0][[0, 2]] == -1).all()
    _same((mixed[0][[1, 3]], mixed[1][[1, 3]]), (second[0][[1, 3]], second[1][[1, 3]]))


def test_filters_and_cursor_against_the_reference(fitted):
    model, be, seen = fitted
    P = model.predict()
    users = [2, 9, 9, NOTHING]
    allow = np.arange(0, N_ITEMS, 2)
    block = np.zeros(N_ITEMS, bool)
    block[10:40] = True
    ok = validate.allowed_mask(validate.item_filters(allow, block, N_ITEMS), N_ITEMS)
    first = model.recommend_deep(users, 60, items=allow, filter_items=block)
    _same(first, _expect(P, users, seen, 60, ok))
    after = (first[0][:, -1], first[1][:, -1])
    _same(model.recommend_deep(users, 200, items=allow, filter_items=block, after=after),
          _expect(P, users, seen, 200, ok, after=after))
    empty = model.recommend_deep(users, 200, items=[])
    assert (empty[0] == -1).all()
    with pytest.raises(ValueError):
        model.recommend_deep(users, 200, items=[N_ITEMS])


def test_new_items(fitted):
    model, be, seen = fitted
    rng = np.random.default_rng(5)
    B = 4
    C_new = np.full((B, M), np.nan)
    for b in range(B - 1):
        C_new[b, rng.permutation(M)[: 5 + 3 * b]] = rng.integers(1, 6, 5 + 3 * b)
    folded = model.fold_in_items(C_new)
    Pj = np.concatenate([model.predict(), model.predict_new_items(folded)], axis=1)
    nt = N_ITEMS + B
    sj = [np.concatenate([seen[u], N_ITEMS + np.nonzero(~np.isnan(C_new[:, u]))[0]]) for u in range(M)]
    users = list(range(M))
    for N in (128, 250, nt):
        _same(model.recommend_deep(users, N, new_items=folded), _expect(Pj, users, sj, N))
    _same(model.recommend_deep(users, 100, new_items=folded), model.recommend(users, 100, new_items=folded))
    only_new = np.arange(nt) >= N_ITEMS
    got = model.recommend_deep(users, 200, new_items=folded, items=only_new, exclude_seen=False)
    _same(got, _expect(Pj, users, sj, 200, only_new, exclude=False))
    assert ((got[0] >= N_ITEMS) | (got[0] == -1)).all() and (got[0][:, :B] >= N_ITEMS).all()
    after = (np.full(M, nt - 1), Pj[:, nt - 1])                             # a cursor on a folded id
    _same(model.recommend_deep(users, 200, new_items=folded, after=after), _expect(Pj, users, sj, 200, after=after))
    with pytest.raises(ValueError):
        model.recommend_deep(users, 200, after=after)                       # that id without new_items


def test_recommend_new_deep(fitted_feat):
    model, be, seen, feats = fitted_feat
    rng = np.random.default_rng(8)
    B = 5
    R_new = np.full((B, N_ITEMS), np.nan)
    for b in range(B - 1):                                                   # the last row: no ratings
        R_new[b, rng.permutation(N_ITEMS)[: 20 + 30 * b]] = rng.integers(1, 11, 20 + 30 * b) * 0.5
    rated = [np.nonzero(~np.isnan(R_new[b]))[0] for b in range(B)]
    for T in (None, 2):
        U, bu = model.fold_in(R_new, features=feats, n_sweeps=T)
        short = model.recommend_new(R_new, 128, features=feats, n_sweeps=T)
        _same(model.recommend_new_deep(R_new, 128, features=feats, n_sweeps=T), short)
        full = model.recommend_new_deep(R_new, 400, features=feats, n_sweeps=T)
        assert (full[0][:, :128] == short[0]).all() and (full[1][:, :128] == short[1]).all()
        for b in range(B):
            ids = full[0][b][full[0][b] >= 0]
            assert ids.size == N_ITEMS - rated[b].size and not np.isin(ids, rated[b]).any()
            s = full[1][b][: ids.size]
            assert ((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (ids[:-1] < ids[1:]))).all()
        pages = _page_through(lambda after: model.recommend_new_deep(R_new, 130, features=feats, n_sweeps=T,
                                                                     after=after), B, 130)
        for b in range(B):
            assert pages[b] == full[0][b][full[0][b] >= 0].tolist()
    block = np.arange(0, N_ITEMS, 5)
    got = model.recommend_new_deep(R_new, 300, features=feats, filter_items=block, exclude_seen=False)
    assert not np.isin(got[0], block).any() and ((got[0] >= 0).sum(axis=1) == N_ITEMS - block.size).all()


def test_chunks_are_crossed_and_what_each_launch_reads(fitted, monkeypatch):
    model, be, seen = fitted
    whole = model.recommend_deep(N=200)
    monkeypatch.setattr(type(model._eng), "DEEP_BATCH", 7)
    del be.calls[:]
    after = (whole[0][:, 99], whole[1][:, 99])
    got = model.recommend_deep(N=100, after=after, items=np.arange(N_ITEMS))
    calls = [c for c in be.calls if c[0] == "recommend_deep"]
    assert [c[1] for c in calls] == [7, 7, 7, 3] and all(c[2] == 100 and c[4] for c in calls)
    assert len({c[3] for c in calls}) == 1 and calls[0][3] is not None     # one bitmap for the call
    _same(got, (whole[0][:, 100:], whole[1][:, 100:]))
    assert not [c for c in be.calls if c[0].startswith("recommend_topk")]
    monkeypatch.setattr(type(model._eng), "DEEP_BATCH", 1 << 12)
    monkeypatch.setattr(type(model._eng), "REC_BATCH", 5)                    # the chunk sources' own limit holds too
    del be.calls[:]
    _same(model.recommend_deep(N=200), whole)
    assert [c[1] for c in be.calls if c[0] == "recommend_deep"] == [5, 5, 5, 5, 4]
    # the workspace bound halves the chunk until the call fits: 24 -> 12 -> 6 rows of 74 240 bytes
    monkeypatch.setattr(type(model._eng), "REC_BATCH", 1 << 16)
    monkeypatch.setattr(type(model._eng), "DEEP_WS_BYTES", 6 * 74240 + 64)
    del be.calls[:]
    _same(model.recommend_deep(N=200), whole)
    assert [c[1] for c in be.calls if c[0] == "recommend_deep"] == [6, 6, 6, 6]
    assert [c[1:] for c in be.calls if c[0] == "recommend_deep_workspace_bytes"] == [(24, N_ITEMS, 200),
                                                                                     (12, N_ITEMS, 200),
                                                                                     (6, N_ITEMS, 200)]
    assert type(model._eng).DEEP_WS_BYTES == 6 * 74240 + 64


# ----------------------------------------------------------------------------------------- the library
def test_header_and_binding_carry_the_new_symbols():
    from collaborative_filtering_amd import _hip
    header = open(os.path.join(ROOT, "include", "als_hip.h")).read()
    for name in ("als_recommend_deep_workspace_bytes", "als_recommend_deep"):
        assert name in _hip.EXPORTS
        assert re.search(r"\b%s\(" % name, header)
    assert re.search(r"#define ALS_TOPK_DEEP_MAX 1024\b", header) and re.search(r"#define ALS_TOPK_MAX 128\b", header)


def test_library_exports_the_new_symbols():
    import __graft_entry__ as ge
    from collaborative_filtering_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        ge.build()
    lib = _hip.load()
    assert lib.als_version() == 103
    ws = lib.als_recommend_deep_workspace_bytes
    # 8 nusers (128 S + NL + S) + 64: a forced slice count is capped by one slice per 32 items
    assert ws(3, 5003, 10, 1) == 8 * 3 * (128 + 128 + 1) + 64
    assert ws(3, 5003, 129, 7) == 8 * 3 * (128 * 7 + 256 + 7) + 64
    assert ws(3, 5003, 257, 7) == 8 * 3 * (128 * 7 + 512 + 7) + 64
    assert ws(5, 5003, 1024, 64) == 8 * 5 * (128 * 64 + 1024 + 64) + 64
    assert ws(5, 100, 1024, 64) == 8 * 5 * (128 * 4 + 1024 + 4) + 64
    # automatic: als_recommend_topk's count (here 49: one slice per 2048 items), but at least 4 per round of 128
    assert ws(5, 100000, 1024, 0) == 8 * 5 * (128 * 49 + 1024 + 49) + 64
    assert ws(5, 20000, 1024, 0) == 8 * 5 * (128 * 32 + 1024 + 32) + 64
    assert ws(100000, 100000, 300, 0) == 8 * 100000 * (128 * 12 + 512 + 12) + 64
    assert ws(3, 5003, 1025, 7) == 0 and ws(3, 5003, 0, 7) == 0 and ws(0, 5003, 10, 7) == 0
    assert lib.als_recommend_workspace_bytes(3, 5003, 129, 7) == 0          # the old limit stands
