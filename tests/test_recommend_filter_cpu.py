"""Item allow / block lists (`items=` / `filter_items=`) of ALS.recommend*, rank_of* and the cv ranking measures,
without a GPU: validation, bitmap packing against a numpy definition, the host orchestration over the numpy stand-in
backend, whose *_masked methods are the contracts of tests/serving_ref.py with `allowed` unpacked from the bitmap, the cv
pass-through with its dropped-pair counts, and the presence of the new symbols in the built library."""
import ctypes
import os

import numpy as np
import pytest
import torch

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, cv, validate
from collaborative_filtering_amd.serving import FoldedItems, pack_bitmap
from tests import serving_ref as ref
from tests.cpu_backend import NumpyBackend
from tests.serving_ref import bitmap_numpy
from tests.synth import make_ratings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "collaborative-filtering_amd", "csrc", "libals_hip.so")


M, N_ITEMS = 30, 70             # n not a multiple of 32


@pytest.fixture(scope="module")
def fitted():
    r, c, v = make_ratings(M, N_ITEMS, 500, seed=3, empty_users=(4,))
    cfg = ALSConfig(core=CoreConfig(n_factors=5, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    model = ALS(cfg, device="cpu", backend=NumpyBackend()).fit_coo(r, c, v, (M, N_ITEMS), tol=None, verbose=0)
    return model, r, c


def _brute_top(P, seen, ok, N):
    """Dense oracle: predict() with seen and disallowed columns masked, (score desc, id asc)."""
    return ref.topn(P, list(seen), ok, N)[1]


# ------------------------------------------------------------------------------------------ validation
def test_item_filter_forms():
    n = 10
    assert validate.item_filters(None, None, n) is None
    ids, none = validate.item_filters([3, 1, 3, 9], None, n)
    assert none is None and ids.dtype == np.int64 and ids.tolist() == [3, 1, 3, 9]       # order, duplicates kept
    mask = np.zeros(n, bool)
    mask[[2, 5]] = True
    a, b = validate.item_filters(mask, np.array([5], dtype=np.int32), n)
    assert a.dtype == np.bool_ and b.tolist() == [5]
    assert validate.allowed_mask((a, b), n).nonzero()[0].tolist() == [2]                  # items minus filter_items
    assert validate.allowed_mask((None, b), n).sum() == n - 1
    assert validate.allowed_mask((ids, mask), n).nonzero()[0].tolist() == [1, 3, 9]
    empty, _ = validate.item_filters([], None, n)                                         # an empty allow-list is legal
    assert empty.size == 0 and validate.allowed_mask((empty, None), n).sum() == 0
    t, _ = validate.item_filters(torch.tensor([1, 2]), None, n)                           # tensors are taken too
    assert t.tolist() == [1, 2]


@pytest.mark.parametrize("name", ["items", "filter_items"])
@pytest.mark.parametrize("bad", [[10], [-1], [0, 99], np.ones(9, bool), np.ones(11, bool), [0.5, 1.0], [[1, 2]],
                                 np.zeros(0, bool)])
def test_item_filter_errors_name_the_argument(name, bad):
    with pytest.raises(ValueError, match=name):
        validate.item_filter(bad, 10, name)


def test_facade_validates_filters(fitted):
    model = fitted[0]
    for bad in ([N_ITEMS], [-1], np.ones(N_ITEMS + 1, bool), [1.5]):
        with pytest.raises(ValueError, match="filter_items"):
            model.recommend([0], 3, filter_items=bad)
        with pytest.raises(ValueError, match="items"):
            model.recommend([0], 3, items=bad)
        with pytest.raises(ValueError, match="items"):
            model.rank_of([0], [1], allow_items=bad)
        with pytest.raises(ValueError, match="filter_items"):
            model.rank_of([0], [1], filter_items=bad)
    R_new = np.full((1, N_ITEMS), np.nan)
    R_new[0, 3] = 4.0
    with pytest.raises(ValueError, match="items"):
        model.recommend_new(R_new, 3, items=[N_ITEMS])
    with pytest.raises(ValueError, match="filter_items"):
        model.rank_of_new(R_new, ([0, 1], [2]), filter_items=np.ones(3, bool))
    with pytest.raises(ValueError):                                       # also without users: arguments are checked
        model.recommend([], 3, items=[N_ITEMS])


# ------------------------------------------------------------------------------------------ bitmap
@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 70, 1000])
def test_pack_bitmap_equals_the_numpy_definition(n):
    rng = np.random.default_rng(n)
    for density in (0.0, 0.03, 0.5, 1.0):
        mask = rng.random(n) < density if 0.0 < density < 1.0 else np.full(n, bool(density))
        words = pack_bitmap(torch.from_numpy(mask))
        assert words.dtype == torch.int32 and words.numel() == (n + 31) // 32
        assert (words.numpy().view(np.uint32) == bitmap_numpy(mask)).all()
    top = np.zeros(n, bool)
    top[n - 1] = True                                                      # bit 31 when n is a multiple of 32
    assert (pack_bitmap(torch.from_numpy(top)).numpy().view(np.uint32) == bitmap_numpy(top)).all()


def test_engine_bitmap_from_ids_masks_and_joint_catalogue(fitted):
    eng = fitted[0]._eng
    assert eng.allow_bitmap(None, N_ITEMS) is None
    rng = np.random.default_rng(0)
    for n_total in (N_ITEMS, N_ITEMS + 27):                                # n + B: folded ids at the end
        ids = rng.integers(0, n_total, 40)
        block = rng.random(n_total) < 0.3
        for filters in ((ids, None), (None, ids), (ids, block), (block, ids), (np.empty(0, np.int64), None)):
            got = eng.allow_bitmap(filters, n_total).numpy().view(np.uint32)
            assert (got == bitmap_numpy(validate.allowed_mask(filters, n_total))).all()


# ------------------------------------------------------------------------------------------ orchestration
def test_recommend_filters_against_dense_oracle_across_chunks(fitted, monkeypatch):
    model, r, c = fitted
    be = model._eng.be
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)        # 30 users: five chunks
    P = model.predict()
    rng = np.random.default_rng(1)
    allow = rng.permutation(N_ITEMS)[:25]
    block = rng.random(N_ITEMS) < 0.2
    cases = [dict(items=allow), dict(items=np.isin(np.arange(N_ITEMS), allow)), dict(filter_items=block),
             dict(items=np.concatenate([allow, allow[:3]]), filter_items=np.nonzero(block)[0]),
             dict(items=[69]), dict(items=[])]
    for kw in cases:
        ok = validate.allowed_mask(validate.item_filters(kw.get("items"), kw.get("filter_items"), N_ITEMS), N_ITEMS)
        be.calls.clear()
        items, scores = model.recommend(None, 6, **kw)
        assert [c_[0] for c_ in be.calls] == ["recommend_topk_masked"] * 5
        assert len({c_[2] for c_ in be.calls}) == 1                        # one bitmap, built once, for every chunk
        for u in range(M):
            want = _brute_top(P[u], c[r == u], ok, 6)
            assert (items[u, : want.size] == want).all() and (items[u, want.size:] == -1).all()
            assert (scores[u, : want.size] == P[u, want]).all() and np.isneginf(scores[u, want.size:]).all()
        items_all, _ = model.recommend([0, 3], 6, exclude_seen=False, **kw)
        for b, u in enumerate((0, 3)):
            want = _brute_top(P[u], (), ok, 6)
            assert (items_all[b, : want.size] == want).all()
    items, scores = model.recommend([1, 2], 5, items=[])                   # rows of -1 / -inf
    assert (items == -1).all() and np.isneginf(scores).all()


def test_no_filter_takes_the_unmasked_backend_calls(fitted):
    model = fitted[0]
    be = model._eng.be
    be.calls.clear()
    a = model.recommend([0, 5], 4)
    model.rank_of([0, 5], [1, 2])
    assert [c_[0] for c_ in be.calls] == ["recommend_topk", "rank_count"]
    b = model.recommend([0, 5], 4, items=np.arange(N_ITEMS))               # all items allowed: the same lists
    c_ = model.recommend([0, 5], 4, filter_items=np.zeros(N_ITEMS, bool))
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and (a[0] == c_[0]).all() and (a[1] == c_[1]).all()


def test_rank_of_filters_and_consistency_with_recommend(fitted, monkeypatch):
    model, r, c = fitted
    monkeypatch.setattr(model._eng, "REC_BATCH", 4, raising=False)
    P = model.predict()
    rng = np.random.default_rng(2)
    allow = rng.permutation(N_ITEMS)[:30]
    block = allow[:5]
    ok = validate.allowed_mask(validate.item_filters(allow, block, N_ITEMS), N_ITEMS)
    items, _ = model.recommend(None, 8, items=allow, filter_items=block)
    j = np.arange(N_ITEMS)
    for u in range(M):
        valid = items[u] >= 0
        rank, cand, _ = model.rank_of(np.full(valid.sum(), u), items[u][valid], allow_items=allow, filter_items=block)
        assert (rank == np.arange(valid.sum())).all()
        seen = c[r == u]
        assert (cand == np.setdiff1d(np.nonzero(ok)[0], seen).size).all()
    us = rng.integers(0, M, 60)
    ts = rng.integers(0, N_ITEMS, 60)                                      # most targets are not allowed themselves
    rank, cand, sc = model.rank_of(us, ts, allow_items=allow, filter_items=block)
    assert (~ok[ts]).sum() > 20
    for p, (u, t) in enumerate(zip(us, ts)):
        cset = ok.copy()
        cset[c[r == u]] = False
        assert rank[p] == int((cset & ((P[u] > P[u, t]) | ((P[u] == P[u, t]) & (j < t)))).sum())
        assert cand[p] == cset.sum() and sc[p] == P[u, t]
    rank, cand, _ = model.rank_of([0, 1], [3, 4], allow_items=[])
    assert (rank == 0).all() and (cand == 0).all()


def test_new_user_entry_points(fitted):
    model = fitted[0]
    rng = np.random.default_rng(5)
    R_new = np.full((6, N_ITEMS), np.nan)
    for b in range(5):
        R_new[b, rng.permutation(N_ITEMS)[:6]] = rng.integers(1, 6, 6)
    block = rng.random(N_ITEMS) < 0.5
    full_i, full_s = model.recommend_new(R_new, 128)
    items, scores = model.recommend_new(R_new, 8, filter_items=block)
    for b in range(6):
        keep = (full_i[b] >= 0) & ~block[np.maximum(full_i[b], 0)]
        assert (items[b] == full_i[b][keep][:8]).all() and (scores[b] == full_s[b][keep][:8]).all()
    tptr = np.arange(0, 8 * 6 + 1, 8)
    rank, cand, _ = model.rank_of_new(R_new, (tptr, items.ravel()), filter_items=block)
    assert (rank.reshape(6, 8) == np.arange(8)).all()
    assert (cand.reshape(6, 8) == ((~block)[None, :] & np.isnan(R_new)).sum(axis=1)[:, None]).all()
    for kw in (dict(items=~block), dict(allow_items=~block)):                          # two names of the allow-list
        rank2, cand2, _ = model.rank_of_new(R_new, (tptr, items.ravel()), **kw)
        assert (rank2 == rank).all() and (cand2 == cand).all()
    with pytest.raises(ValueError, match="allow_items"):
        model.rank_of_new(R_new, (tptr, items.ravel()), items=~block, allow_items=~block)


def test_recommend_with_new_items_mask_spans_the_joint_catalogue(fitted):
    model = fitted[0]
    rng = np.random.default_rng(6)
    B, k = 9, model.V.shape[1]
    Z = rng.normal(size=(B, k)).astype(np.float32).astype(np.float64)
    folded = FoldedItems(Z.copy(), rng.normal(size=B).astype(np.float32).astype(np.float64) + 1.0, Z, None,
                         (np.zeros(B + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)))
    nt = N_ITEMS + B
    full_i, full_s = model.recommend([0, 7, 9], 128, new_items=folded)
    assert (full_i >= N_ITEMS).any()
    mask = rng.random(nt) < 0.5
    mask[N_ITEMS: N_ITEMS + 4] = True                                      # folded ids inside ...
    mask[N_ITEMS + 4:] = False                                             # ... and outside the mask
    for kw in (dict(items=mask), dict(items=np.nonzero(mask)[0]), dict(filter_items=~mask)):
        items, scores = model.recommend([0, 7, 9], 10, new_items=folded, **kw)
        for b in range(3):
            keep = (full_i[b] >= 0) & mask[np.maximum(full_i[b], 0)]
            assert (items[b] == full_i[b][keep][:10]).all() and (scores[b] == full_s[b][keep][:10]).all()
        assert ((items >= N_ITEMS) & (items < N_ITEMS + 4)).any() and not (items >= N_ITEMS + 4).any()
    with pytest.raises(ValueError, match="items"):
        model.recommend([0], 3, new_items=folded, items=[nt])
    with pytest.raises(ValueError, match="items"):
        model.recommend([0], 3, new_items=folded, items=np.ones(N_ITEMS, bool))      # the mask must span n + B
    model.recommend([0], 3, items=np.ones(N_ITEMS, bool))


# ------------------------------------------------------------------------------------------ cv
@pytest.fixture(scope="module")
def split():
    m, n = 40, 60
    r, c, v = make_ratings(m, n, 900, seed=11)
    flat = np.unique(r * n + c, return_index=True)[1]
    r, c, v = r[flat], c[flat], v[flat]
    test = np.random.default_rng(1).random(r.size) < 0.3
    cfg = ALSConfig(core=CoreConfig(n_factors=6, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    model = ALS(cfg, device="cpu", backend=NumpyBackend()).fit_coo(r[~test], c[~test], v[~test], (m, n), tol=None,
                                                                   verbose=0)
    return model, (r[~test], c[~test]), (r[test], c[test], v[test])


def test_cv_ranking_within_a_category(split):
    model, (tr, tc), (hr, hc, hv) = split
    n = model.V.shape[0]
    cat = np.arange(n) % 3 == 0                                            # "the category"
    inside = cat[hc]
    base = cv.ranking_at_k(model, hr, hc, K=5)
    assert "filtered_out" not in base                                      # unfiltered: today's result
    got = cv.ranking_at_k(model, hr, hc, K=5, items=cat)
    assert got["filtered_out"] == int((~inside).sum()) and got["users"] == np.unique(hr[inside]).size
    P = model.predict()
    rec = []
    for u in np.unique(hr[inside]):
        top = _brute_top(P[u], tc[tr == u], cat, 5)
        rel = set(hc[inside & (hr == u)].tolist())
        rec.append(len(rel & set(top.tolist())) / len(rel))
    assert got["recall@K"] == pytest.approx(np.mean(rec), rel=1e-12)
    same = cv.ranking_at_k(model, hr, hc, K=5, filter_items=np.nonzero(~cat)[0])
    assert same == got
    rm = cv.rank_metrics(model, hr, hc, Ks=(5, 10), items=cat)
    assert rm["dropped"] == int((~inside).sum()) and rm["pairs"] == int(inside.sum())
    assert rm["recall@5"] == pytest.approx(got["recall@K"], abs=1e-12)
    assert rm["ndcg@5"] == pytest.approx(got["ndcg@K"], abs=1e-12)
    assert cv.rank_metrics(model, hr, hc, Ks=(5, 10), filter_items=~cat) == rm
    none = cv.ranking_at_k(model, hr, hc, K=5, items=[])
    assert none["users"] == 0 and none["filtered_out"] == hr.size
    with pytest.raises(ValueError, match="items"):
        cv.ranking_at_k(model, hr, hc, K=5, items=[n])
    with pytest.raises(ValueError, match="items"):                        # checked with or without held-out pairs
        cv.rank_metrics(model, [], [], items=[n])
    assert cv.rank_metrics(model, [], [], items=cat)["users"] == 0


def test_cv_fold_in_measures_pass_the_filters_through(split):
    model = split[0]
    n = model.V.shape[0]
    rng = np.random.default_rng(2)
    kr, kc, kv, hr, hc = [], [], [], [], []
    for u in (100, 7, 55, 3):
        cols = rng.permutation(n)[:24]
        kr += [u] * 12; kc += cols[:12].tolist(); kv += rng.integers(1, 6, 12).astype(float).tolist()
        hr += [u] * 12; hc += cols[12:].tolist()
    known, held = (np.array(kr), np.array(kc), np.array(kv)), (np.array(hr), np.array(hc))
    block = np.arange(n) % 2 == 1
    out = int(block[held[1]].sum())
    assert 0 < out < len(hr)
    at_k = cv.fold_in_ranking_at_k(model, known, held, K=10, filter_items=block)
    rm = cv.fold_in_rank_metrics(model, known, held, Ks=(10,), filter_items=block)
    assert at_k["filtered_out"] == out and rm["dropped"] == out and rm["pairs"] == len(hr) - out
    assert rm["recall@10"] == pytest.approx(at_k["recall@K"], abs=1e-12)
    assert rm["ndcg@10"] == pytest.approx(at_k["ndcg@K"], abs=1e-12)
    assert cv.fold_in_rank_metrics(model, known, held, Ks=(10,), items=~block) == rm
    assert "filtered_out" not in cv.fold_in_ranking_at_k(model, known, held, K=10)


# ------------------------------------------------------------------------------------------ library
def test_library_exports_the_masked_entry_points():
    if not os.path.exists(LIB):             # fresh checkout: the .so is git-ignored
        import __graft_entry__ as ge
        ge.build()
    lib = ctypes.CDLL(LIB)
    for name in ("als_recommend_topk_masked", "als_rank_count_masked", "als_recommend_topk", "als_rank_count"):
        assert hasattr(lib, name), name
    from collaborative_filtering_amd import _hip
    assert {"als_recommend_topk_masked", "als_rank_count_masked"} <= set(_hip.EXPORTS)
    header = open(os.path.join(ROOT, "include", "als_hip.h")).read()
    assert "int als_recommend_topk_masked(" in header and "int als_rank_count_masked(" in header
