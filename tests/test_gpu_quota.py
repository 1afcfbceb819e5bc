"""K22 (GPU): als_recommend_topk_quota (csrc/quota.hip) and ALS.recommend_quota / recommend_new_quota.

The kernel is held to `greedy_capped` of tests/quota_ref.py - the scan of the definition - on als_predict_dense rows,
and to als_recommend_topk_masked where the caps cannot bind; the model calls to the same scan on `predict()` rows.
Every comparison is ==, every output buffer starts from a poison value, and every kernel test runs with 1, 3 and 7
item slices."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import quota_ref as qref
from tests.gpu_common import assert_same, env, factors, predict_dense, run_topk, seen_csr, upload
from tests.serving_ref import bitmap_numpy
from tests.synth import make_ratings

SLICES = ["1", "3", "7"]


def run_quota(torch, be, f, users, n, seen_ptr, seen_idx, N, dev, allow, groups, cap):
    """als_recommend_topk_quota into poisoned buffers -> numpy (values, items, counts); allow: uint32 words or None."""
    us = upload(np.asarray(users, np.int32), dev)
    B = us.numel()
    tv = torch.full((B, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((B, N), -7, dtype=torch.int32, device=dev)
    tc = torch.full((B,), -7, dtype=torch.int32, device=dev)
    be.recommend_topk_quota(k=f["k"], ld=f["ld"], users=us, n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"],
                            mu=f["mu"], seen_ptr=None if seen_ptr is None else upload(seen_ptr, dev),
                            seen_idx=None if seen_idx is None else upload(seen_idx, dev),
                            allow=None if allow is None else upload(allow.view(np.int32), dev),
                            item_group=upload(np.asarray(groups, np.int32), dev),
                            group_cap=upload(np.asarray(cap, np.int32), dev), topn=N, top_val=tv, top_idx=ti,
                            top_cnt=tc)
    return tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()


def _batch(m, seed):
    """150 batch rows: every user, 90 duplicates, reversed - partial last workgroups in both shapes."""
    rng = np.random.default_rng(seed)
    return np.concatenate([np.arange(m), rng.integers(0, m, 90)])[::-1].copy()


def _table(torch, layout, dev, U, Z):
    """Factor tables without biases from host arrays [m, k] / [n, k]."""
    m, k = U.shape
    n = Z.shape[0]
    ld = layout.padded_k(k)
    Up, Zp = np.zeros((m, ld), np.float32), np.zeros((n, ld), np.float32)
    Up[:, :k], Zp[:, :k] = U, Z
    return dict(k=k, ld=ld, U=upload(Up, dev), Z=upload(Zp, dev), b_u=upload(np.zeros(m, np.float32), dev),
                b_i=upload(np.zeros(n, np.float32), dev), mu=torch.tensor([0.0], dtype=torch.float64, device=dev))


# ------------------------------------------------------------------------------------------------ against the scan
@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("k", [1, 5, 64, 130])
def test_kernel_equals_the_scan(k, slices, monkeypatch):
    torch, layout, be, dev = env().short
    monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)
    m, n = 60, 333                                                         # n: not a multiple of 32
    f = factors(torch, layout, dev, m, n, k, seed=10 * k)
    P = predict_dense(torch, be, f, m, n, dev)
    ptr, idx, rows = seen_csr(m, n, seed=k)                                # user 0 has seen nothing, user 1 nearly all
    users = _batch(m, k)
    rng = np.random.default_rng(k)
    groups = np.where(rng.random(n) < 0.3, -1, rng.integers(0, 40, n))
    cap = rng.integers(0, 4, 40)
    allow = rng.random(n) < 0.6
    S, seen = P[users], [rows[u] for u in users]
    for N in (1, 10, 32, 33, 128):                                         # 32 / 33: the narrow and the wide workgroup
        got = run_quota(torch, be, f, users, n, ptr, idx, N, dev, None, groups, cap)
        assert_same(got, qref.greedy_capped_batch(S, seen, None, groups, cap, N))
        got = run_quota(torch, be, f, users, n, ptr, idx, N, dev, bitmap_numpy(allow), groups, cap)
        assert_same(got, qref.greedy_capped_batch(S, seen, allow, groups, cap, N))


@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("k", [5, 130])
def test_caps_that_cannot_bind_equal_the_masked_call(k, slices, monkeypatch):
    torch, layout, be, dev = env().short
    monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)
    m, n = 60, 333
    f = factors(torch, layout, dev, m, n, k, seed=3 * k)
    ptr, idx, rows = seen_csr(m, n, seed=k)
    users = _batch(m, k)
    rng = np.random.default_rng(k)
    groups = rng.integers(0, 5, n)
    allow = bitmap_numpy(rng.random(n) < 0.6)
    for N in (1, 10, 32, 33, 128):
        loose = (groups, np.full(5, N))                                    # caps >= N
        none = (np.full(n, -1), np.zeros(0, np.int64))                     # no group at all, ngroups = 0
        stray = (groups + 5, np.zeros(5, np.int64))                        # labels outside [0, G) count as -1
        own = (rng.permutation(n), np.ones(n, np.int64))                   # every item its own group
        for a in (None, allow):
            want = run_topk(torch, be, f, users, n, ptr, idx, N, dev,
                            allow=None if a is None else upload(a.view(np.int32), dev))
            for g, c in (loose, none, stray, own):
                assert_same(run_quota(torch, be, f, users, n, ptr, idx, N, dev, a, g, c), want)
        want = run_topk(torch, be, f, users, n, None, None, N, dev, allow=upload(allow.view(np.int32), dev))
        assert_same(run_quota(torch, be, f, users, n, None, None, N, dev, allow, *loose), want)


@pytest.mark.parametrize("slices", SLICES)
def test_cap_zero_is_a_block_list(slices, monkeypatch):
    torch, layout, be, dev = env().short
    monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)
    m, n, k = 60, 333, 5
    f = factors(torch, layout, dev, m, n, k, seed=21)
    ptr, idx, rows = seen_csr(m, n, seed=2)
    users = _batch(m, 2)
    rng = np.random.default_rng(2)
    groups = rng.integers(-1, 6, n)
    base = rng.random(n) < 0.7
    for N in (10, 128):
        cap = np.array([0, N, 0, N, N, 0])
        closed = np.isin(groups, [0, 2, 5])
        for mask in (None, base):
            a = None if mask is None else bitmap_numpy(mask)
            got = run_quota(torch, be, f, users, n, ptr, idx, N, dev, a, groups, cap)
            cleared = ~closed if mask is None else mask & ~closed
            want = run_topk(torch, be, f, users, n, ptr, idx, N, dev,
                            allow=upload(bitmap_numpy(cleared).view(np.int32), dev))
            assert_same(got, want)


# ------------------------------------------------------------------------------------------------ ties: the item decides
@pytest.fixture(scope="module")
def tied():
    """Tables of small integers: at most 9 distinct scores over 333 items, so the item id decides nearly every
    comparison; the scores come from als_predict_dense once."""
    torch, layout, be, dev = env().short
    m, n, k = 40, 333, 4
    rng = np.random.default_rng(7)
    f = _table(torch, layout, dev, rng.integers(-1, 2, size=(m, k)), rng.integers(-1, 2, size=(n, k)))
    P = predict_dense(torch, be, f, m, n, dev)
    assert np.unique(P).size <= 9
    P.setflags(write=False)
    ptr, idx, rows = seen_csr(m, n, seed=3)
    users = np.concatenate([np.arange(m), rng.integers(0, m, 110)])        # 150 batch rows
    return f, P, ptr, idx, rows, users, m, n


@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("layout_", ["G1", "G3", "G40", "Gn", "dominant"])
def test_caps_on_massively_tied_scores(tied, layout_, slices, monkeypatch):
    torch, _, be, dev = env().short
    monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)
    f, P, ptr, idx, rows, users, m, n = tied
    rng = np.random.default_rng(len(layout_))
    if layout_ == "dominant":                                              # one group holds 90 % of the items
        G = 4
        groups = np.where(rng.random(n) < 0.9, 0, rng.integers(1, G, n))
    else:
        G = {"G1": 1, "G3": 3, "G40": 40, "Gn": n}[layout_]
        groups = rng.permutation(n) if G == n else rng.integers(0, G, n)
        groups = np.where(rng.random(n) < 0.3, -1, groups)                 # 30 % of the labels -1
    cap = rng.integers(0, 4, G)
    if layout_ in ("G1", "dominant"):
        cap[0] = 2
    S, seen = P[users], [rows[u] for u in users]
    mask = np.zeros(n, bool)
    for w in (0, 2, 3, 7, 10):                                             # the other words are empty: skipped chunks
        mask[32 * w: 32 * w + 32] = rng.random(len(mask[32 * w: 32 * w + 32])) < 0.6
    none = [np.zeros(0, np.int64)] * users.size
    for N in (10, 33, 128):
        for allowed in (None, mask):
            a = None if allowed is None else bitmap_numpy(allowed)
            got = run_quota(torch, be, f, users, n, ptr, idx, N, dev, a, groups, cap)
            assert_same(got, qref.greedy_capped_batch(S, seen, allowed, groups, cap, N))
        got = run_quota(torch, be, f, users, n, None, None, N, dev, None, groups, cap)
        assert_same(got, qref.greedy_capped_batch(S, none, None, groups, cap, N))


@pytest.mark.parametrize("slices", SLICES)
def test_all_scores_equal_lists_the_lowest_ids_under_the_caps(slices, monkeypatch):
    torch, layout, be, dev = env().short
    monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)
    m, n, k = 20, 333, 3
    f = _table(torch, layout, dev, np.zeros((m, k)), np.zeros((n, k)))
    users = np.arange(m)
    groups = np.arange(n) // 4 % 7                                         # runs of four: ids 0 ... 3 in group 0, ...
    groups[5::11] = -1
    cap = np.array([1, 2, 0, 3, 1, 2, 1])
    allowed = np.ones(n, bool)
    allowed[:3] = False
    for N in (10, 40):
        tv, ti, tc = run_quota(torch, be, f, users, n, None, None, N, dev, bitmap_numpy(allowed), groups, cap)
        want, used = [], np.zeros(7, int)
        for i in range(3, n):                                              # the scan, written out: ascending ids
            if len(want) == N:
                break
            g = groups[i]
            if g < 0 or used[g] < cap[g]:
                want.append(i)
                used[max(g, 0)] += g >= 0
        assert (ti == np.array(want)[None, :]).all() and (tv == 0.0).all() and (tc == len(want)).all()


# ------------------------------------------------------------------------------------------------ the open threshold
@pytest.mark.parametrize("slices", SLICES)
@pytest.mark.parametrize("order", ["increasing", "decreasing"])
def test_one_group_with_cap_two_never_fills_the_list(order, slices, monkeypatch):
    """k = 1, score = the item's factor: increasing with the id every candidate beats every earlier one, so each is
    buffered and each row compacts every other chunk over about 1000 items.  One group with cap 2 and N = 10: the list
    never fills and the threshold stays 0 over the whole walk, in both orders."""
    torch, layout, be, dev = env().short
    monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)
    m, n = 40, 1003
    z = np.arange(n, dtype=np.float64) / 8.0 - 50.0
    z = z if order == "increasing" else z[::-1]
    f = _table(torch, layout, dev, np.ones((m, 1)), z[:, None])
    P = predict_dense(torch, be, f, m, n, dev)
    ptr, idx, rows = seen_csr(m, n, seed=5)
    users = np.arange(m)
    seen = [rows[u] for u in users]
    for N in (10, 40):
        one = (np.zeros(n, np.int64), np.array([2]))
        got = run_quota(torch, be, f, users, n, ptr, idx, N, dev, None, *one)
        assert_same(got, qref.greedy_capped_batch(P, seen, None, *one, N))
        assert (got[2] == 2).all()                                         # user 1 has three unseen items left
        few = (np.arange(n) % 3, np.array([2, 1, 3]))                      # the list holds 6 of N entries at the most
        got = run_quota(torch, be, f, users, n, ptr, idx, N, dev, None, *few)
        assert_same(got, qref.greedy_capped_batch(P, seen, None, *few, N))
        loose = (np.arange(n) % 3, np.array([N, N, N]))                    # a threshold that rises with every compaction
        got = run_quota(torch, be, f, users, n, ptr, idx, N, dev, None, *loose)
        assert_same(got, run_topk(torch, be, f, users, n, ptr, idx, N, dev))


@pytest.mark.parametrize("slices", SLICES)
def test_sparse_bitmap_with_empty_words_and_groups(slices, monkeypatch):
    torch, layout, be, dev = env().short
    monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)
    m, n, k = 60, 1003, 5
    f = factors(torch, layout, dev, m, n, k, seed=77)
    P = predict_dense(torch, be, f, m, n, dev)
    ptr, idx, rows = seen_csr(m, n, seed=9)
    users = _batch(m, 9)
    rng = np.random.default_rng(9)
    mask = np.zeros(n, bool)
    for w in (1, 2, 9, 17, 18, 30, 31):                                    # 7 of 32 words hold allowed items
        mask[32 * w: 32 * w + 32] = rng.random(len(mask[32 * w: 32 * w + 32])) < 0.7
    groups = np.where(rng.random(n) < 0.2, -1, rng.integers(0, 6, n))
    cap = np.array([1, 2, 3, 0, 2, 1])
    S, seen = P[users], [rows[u] for u in users]
    for N in (10, 33):
        got = run_quota(torch, be, f, users, n, ptr, idx, N, dev, bitmap_numpy(mask), groups, cap)
        assert_same(got, qref.greedy_capped_batch(S, seen, mask, groups, cap, N))
    got = run_quota(torch, be, f, users, n, ptr, idx, 10, dev, bitmap_numpy(np.zeros(n, bool)), groups, cap)
    assert (got[2] == 0).all() and (got[1] == -1).all() and np.isneginf(got[0]).all()


# ------------------------------------------------------------------------------------------------ model level
M, N_ITEMS, K_F = 150, 333, 5


@pytest.fixture(scope="module")
def fitted():
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig
    env()
    r, c, v = make_ratings(M, N_ITEMS, 4000, seed=11, empty_users=(3,))
    cfg = ALSConfig(core=CoreConfig(n_factors=K_F, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    model = ALS(cfg, device="cuda:0").fit_coo(r, c, v, (M, N_ITEMS), tol=None, verbose=0)
    seen = [np.sort(c[r == u]) for u in range(M)]
    return model, seen, model.predict()


def _want(P, seen_rows, allowed, groups, cap, N):
    tv, ti, _ = qref.greedy_capped_batch(P, seen_rows, allowed, groups, cap, N)
    return ti.astype(np.int64), tv


def _assert_lists(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[0].shape == want[0].shape
    assert (got[0] == want[0]).all(), np.argwhere(got[0] != want[0])[:5]
    assert (got[1] == want[1]).all()                                       # bitwise predict's: the scan copies them


def _folded(rng, B=9):
    from collaborative_filtering_amd.serving import FoldedItems
    Z = rng.normal(size=(B, K_F)).astype(np.float32).astype(np.float64)
    raters = [np.sort(rng.permutation(M)[: 2 + b]) for b in range(B)]      # with exclude_seen they lose the item
    ptr = np.zeros(B + 1, np.int64)
    ptr[1:] = np.cumsum([x.size for x in raters])
    idx = np.concatenate(raters).astype(np.int32)
    return FoldedItems(Z.copy(), rng.normal(size=B).astype(np.float32).astype(np.float64) + 2.0, Z, None,
                       (ptr, idx, np.ones(idx.size, np.float32))), raters


def test_model_equals_the_scan_end_to_end(fitted, monkeypatch):
    model, seen, P = fitted
    monkeypatch.setattr(model._eng, "REC_BATCH", 100, raising=False)       # B = 450: chunks of 100 and one of 50
    rng = np.random.default_rng(1)
    users = np.tile(np.arange(M), 3)
    B = users.size
    groups = np.where(rng.random(N_ITEMS) < 0.3, -1, rng.integers(0, 15, N_ITEMS))
    cap = rng.integers(0, 4, 15)
    none = [np.zeros(0, np.int64)] * B
    for N in (7, 40):
        for exclude_seen in (True, False):
            got = model.recommend_quota(users, N, groups=groups, max_per_group=cap, exclude_seen=exclude_seen)
            _assert_lists(got, _want(P[users], [seen[u] for u in users] if exclude_seen else none, None, groups, cap, N))
    allow = rng.permutation(N_ITEMS)[:250]
    block = rng.random(N_ITEMS) < 0.2
    ok = np.isin(np.arange(N_ITEMS), allow) & ~block
    got = model.recommend_quota(users, 7, groups=groups, max_per_group=cap, items=allow, filter_items=block)
    _assert_lists(got, _want(P[users], [seen[u] for u in users], ok, groups, cap, 7))
    # the clamp: 3 groups x cap 2 < N = 10
    g3 = np.arange(N_ITEMS) % 3
    got = model.recommend_quota(users, 10, groups=g3, max_per_group=2, exclude_seen=False)
    _assert_lists(got, _want(P[users], none, None, g3, np.array([2, 2, 2]), 10))
    assert (got[0][:, :6] >= 0).all() and (got[0][:, 6:] == -1).all()
    # new items: the joint catalogue, the raters of a folded item have seen it
    folded, raters = _folded(rng)
    PJ = np.concatenate([P[users], model.predict_new_items(folded, users)], axis=1)
    seen_j = [np.concatenate([seen[u], [N_ITEMS + b for b in range(folded.n_items) if u in raters[b]]]).astype(np.int64)
              for u in users]
    gj = np.concatenate([groups, np.full(folded.n_items, 15)])             # the folded items: one more group
    cj = np.concatenate([cap, [2]])
    got = model.recommend_quota(users, 9, groups=gj, max_per_group=cj, new_items=folded)
    _assert_lists(got, _want(PJ, seen_j, None, gj, cj, 9))
    assert (got[0] >= N_ITEMS).any() and ((got[0] >= N_ITEMS).sum(axis=1) <= 2).all()


def test_loose_caps_are_recommend(fitted):
    model, seen, P = fitted
    users = np.tile(np.arange(M), 2)
    g = np.arange(N_ITEMS) % 4
    for N in (7, 40):
        want = model.recommend(users, N)
        for groups, cap in ((g, N), (np.full(N_ITEMS, -1), 0), (np.arange(N_ITEMS), 1)):
            got = model.recommend_quota(users, N, groups=groups, max_per_group=cap)
            assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


def test_recommend_new_quota_equals_the_scan(fitted, monkeypatch):
    model, seen, P = fitted
    torch = env().torch
    monkeypatch.setattr(model._eng, "REC_BATCH", 64, raising=False)
    rng = np.random.default_rng(4)
    B, N = 120, 7
    R_new = np.full((B, N_ITEMS), np.nan)
    for b in range(B):
        if b != 4:                                                         # one row without ratings
            R_new[b, rng.permutation(N_ITEMS)[: 3 + b % 9]] = rng.integers(1, 6, 3 + b % 9)
    eng = model._eng
    Uf, bf = model.fold_in(R_new)
    Ut = torch.zeros(B, eng.ld, dtype=torch.float32)
    Ut[:, : eng.k] = torch.from_numpy(Uf).float()
    f = dict(k=eng.k, ld=eng.ld, U=Ut.to(eng.dev), Z=eng.V, b_u=torch.from_numpy(bf).float().to(eng.dev), b_i=eng.b_i,
             mu=eng.mu)
    PN = predict_dense(torch, eng.be, f, B, N_ITEMS, eng.dev).astype(np.float64)
    groups = rng.integers(-1, 30, N_ITEMS)
    cap = rng.integers(0, 3, 30)
    rows_seen = [np.nonzero(~np.isnan(R_new[b]))[0] for b in range(B)]
    got = model.recommend_new_quota(R_new, N, groups=groups, max_per_group=cap)
    _assert_lists(got, _want(PN, rows_seen, None, groups, cap, N))
