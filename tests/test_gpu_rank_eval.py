"""K11 (GPU): exact full-catalogue ranks (csrc/rank_eval.hip, als_rank_count), ALS.rank_of / rank_of_new.

The oracle is exact: every score is bitwise the fp32 value als_predict_dense writes and the counts are integers, so
the expected values are `rank_counts` of tests/serving_ref.py on the predict_dense rows with the seen items masked,
and every comparison is ==."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import serving_ref as ref
from tests.common import Golden, model_for
from tests.gpu_common import assert_same, env, factors, predict_dense, run_rank, run_topk, seen_csr


def _targets(n, nq, seed, rows_seen=None):
    """Target rows with 0, 1, 16, 17 and several hundred entries (duplicates included), then random sizes; the
    first target of a row with seen items is one of them."""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 16, 17, 300, 33][:nq] + list(rng.integers(0, 12, max(nq - 6, 0)))
    rows = [rng.integers(0, n, s).astype(np.int32) for s in sizes]
    if rows_seen is not None:
        for b, r in enumerate(rows):
            if r.size and rows_seen[b].size:
                r[0] = rows_seen[b][rng.integers(rows_seen[b].size)]
    ptr = np.zeros(nq + 1, np.int64)
    ptr[1:] = np.cumsum([r.size for r in rows])
    items = np.concatenate(rows).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, items


@pytest.mark.parametrize("k", [1, 16, 50, 64, 128, 160])
@pytest.mark.parametrize("n", [1, 17, 1000, 4099])
def test_kernel_equals_masked_dense_count(k, n):
    torch, layout, be, dev = env().short
    m = 40
    f = factors(torch, layout, dev, m, n, k, seed=10 * k + n)
    if n > 16:
        f["Z"][5, 0] = float("nan")                                      # NaN scores: item 5 for every user
    ptr, idx, rows = seen_csr(m, n, seed=k + n)                         # user 0 sees nothing, user 1 all but 3
    dense = predict_dense(torch, be, f, m, n, dev)
    users = np.concatenate([np.arange(m), [3, 1, 3, 0]])[::-1].copy()    # order and duplicates kept
    seen_rows = [rows[u] for u in users]
    q_ptr, q_items = _targets(n, users.size, seed=k * n, rows_seen=seen_rows)
    if n > 16:
        q_items[q_ptr[4]] = 5                                            # a NaN target
    got = run_rank(torch, be, f, users, n, ptr, idx, q_ptr, q_items, dev)
    assert_same(got, ref.rank_counts_batch(dense[users], seen_rows, None, q_ptr, q_items), nan_equal=True)
    if n > 16:
        assert got[1][q_ptr[4]] == -1 and np.isnan(got[0][q_ptr[4]])
    got = run_rank(torch, be, f, users, n, None, None, q_ptr, q_items, dev)              # no exclusion
    unseen = [np.empty(0, np.int64)] * users.size
    assert_same(got, ref.rank_counts_batch(dense[users], unseen, None, q_ptr, q_items), nan_equal=True)
    full_ptr = np.arange(m + 1, dtype=np.int64) * n                      # every user has seen everything
    got = run_rank(torch, be, f, np.arange(m), n, full_ptr, np.tile(np.arange(n, dtype=np.int32), m), q_ptr[: m + 1],
                   q_items[: q_ptr[m]], dev)
    assert (got[2] == 0).all() and (got[1][~np.isnan(got[0])] == 0).all()


def test_ties_follow_the_item_order():
    torch, layout, be, dev = env().short
    m, n = 64, 3001
    f = factors(torch, layout, dev, m, n, 5, seed=4, integer=True)     # duplicated Z rows, b_i = 0: equal scores
    ptr, idx, rows = seen_csr(m, n, seed=4, density=0.1)
    dense = predict_dense(torch, be, f, m, n, dev)
    users = np.arange(m)
    q_ptr = np.arange(m + 1, dtype=np.int64) * 40
    q_items = np.random.default_rng(4).integers(0, n, m * 40).astype(np.int32)
    assert sum(int((dense[u] == dense[u, q_items[40 * u]]).sum()) > 1 for u in range(m)) > m // 2
    got = run_rank(torch, be, f, users, n, ptr, idx, q_ptr, q_items, dev)
    assert_same(got, ref.rank_counts_batch(dense, rows, None, q_ptr, q_items), nan_equal=True)


@pytest.mark.parametrize("B", [1, 3000])
def test_result_does_not_depend_on_the_slice_count(B, monkeypatch):
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    m, n, k = 3000, 5003, 64
    f = factors(torch, layout, dev, m, n, k, seed=B)
    ptr, idx, rows = seen_csr(m, n, seed=B)
    users = np.random.default_rng(B).permutation(m)[:B]
    q_ptr, q_items = _targets(n, B, seed=B)
    if B == 1:
        q_ptr, q_items = np.array([0, 40], np.int64), np.random.default_rng(1).integers(0, n, 40).astype(np.int32)
    nt = q_items.size
    outs = []
    for s in (1, 2, 7, 64):
        need = _hip.load().als_rank_count_workspace_bytes(k, B, nt, n, s)
        assert need == (0 if s == 1 else s * (nt + B) * 4)
        monkeypatch.setenv("ALS_RECOMMEND_SLICES", str(s))
        outs.append(run_rank(torch, be, f, users, n, ptr, idx, q_ptr, q_items, dev))
    monkeypatch.delenv("ALS_RECOMMEND_SLICES")
    outs.append(run_rank(torch, be, f, users, n, ptr, idx, q_ptr, q_items, dev))            # automatic
    for o in outs[1:]:
        assert_same(o, outs[0], nan_equal=True)
    dense = predict_dense(torch, be, f, m, n, dev)
    exp = ref.rank_counts_batch(dense[users], [rows[u] for u in users], None, q_ptr, q_items)
    assert_same(outs[0], exp, nan_equal=True)


def _cross_check(torch, be, f, users, n, ptr, idx, dev, extra_seed):
    """recommend(N = 128) against rank_count: the item at position p has rank p, and every unseen target with a
    rank below 128 is in the list."""
    N = 128
    tv, ti, tc = run_topk(torch, be, f, users, n, ptr, idx, N, dev)
    B = len(users)
    rng = np.random.default_rng(extra_seed)
    extra = rng.integers(0, n, (B, 8)).astype(np.int32)
    rows = [np.concatenate([ti[b, : tc[b]], extra[b]]) for b in range(B)]
    q_ptr = np.zeros(B + 1, np.int64)
    q_ptr[1:] = np.cumsum([r.size for r in rows])
    q_items = np.concatenate(rows).astype(np.int32)
    sc, ab, nc = run_rank(torch, be, f, users, n, ptr, idx, q_ptr, q_items, dev)
    for b in range(B):
        lo = q_ptr[b]
        assert (ab[lo: lo + tc[b]] == np.arange(tc[b])).all()
        assert (sc[lo: lo + tc[b]] == tv[b, : tc[b]]).all()
        assert nc[b] >= tc[b] and (tc[b] == min(N, nc[b]))
        u = users[b]
        seen = idx[ptr[u]: ptr[u + 1]]
        for j, t in enumerate(extra[b]):
            r = ab[lo + tc[b] + j]
            if r >= 0 and r < N and not np.isin(t, seen):
                assert ti[b, r] == t


def test_cross_check_with_recommend():
    torch, layout, be, dev = env().short
    m, n, k = 300, 4099, 50
    f = factors(torch, layout, dev, m, n, k, seed=2)
    ptr, idx, rows = seen_csr(m, n, seed=2)
    _cross_check(torch, be, f, np.arange(m), n, ptr, idx, dev, 2)


# ---------------------------------------------------------------------------------------------- model level
def _brute(P, seen, u, t):
    """(rank, candidates) of item t for user u from the dense predictions, the seen items masked."""
    _, above, n_cand = ref.rank_counts(P[u], seen, None, [t])
    return int(above[0]), n_cand


@pytest.mark.parametrize("name,use_features", [("g3_empty", True), ("g4_feat_uw5", True), ("g4_feat_uw5", False),
                                               ("g5_graph_a5.0", True)])
def test_model_rank_of_on_fixtures(name, use_features):
    env()
    from collaborative_filtering_amd import cv
    g = Golden(name)
    r, c, v = g.train
    model = model_for(g, device="cuda:0")
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"], verbose=0)
    feats = g.features if use_features else None
    P = model.predict(feats).astype(np.float32)
    seen = [c[r == u] for u in range(g.m)]
    rng = np.random.default_rng(0)
    us, its = rng.integers(0, g.m, 500), rng.integers(0, g.n, 500)
    rank, cand, sc = model.rank_of(us, its, features=feats)
    assert rank.dtype == np.int64 and cand.dtype == np.int64 and sc.dtype == np.float32
    for p in range(500):
        assert (rank[p], cand[p]) == _brute(P, seen[us[p]], us[p], its[p]) and sc[p] == P[us[p], its[p]]
    rank, cand, _ = model.rank_of(us, its, features=feats, exclude_seen=False)
    for p in range(500):
        assert (rank[p], cand[p]) == _brute(P, [], us[p], its[p])
    items, scores = model.recommend(None, 128, features=feats)
    ok = items >= 0
    rank, _, sc = model.rank_of(np.repeat(np.arange(g.m), 128)[ok.ravel()], items[ok], features=feats)
    assert (rank == np.tile(np.arange(128), g.m)[ok.ravel()]).all() and (sc == scores[ok]).all()
    res = cv.rank_metrics(model, us, its, Ks=(10, 1000), features=feats)
    assert res["dropped"] == np.unique(us * g.n + its).size - res["pairs"] and res["recall@1000"] <= 1.0
    assert 0.0 <= res["auc"] <= 1.0 and 0.0 <= res["mpr"] <= 1.0 and res["recall@10"] <= res["recall@1000"]


def test_rank_of_new_agrees_with_recommend_new():
    env()
    g = Golden("g4_feat_uw5")
    r, c, v = g.train
    model = model_for(g, device="cuda:0")
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"], verbose=0)
    rng = np.random.default_rng(1)
    B = 9
    R_new = np.full((B, g.n), np.nan)
    for b in range(B - 1):                                               # the last row has no ratings
        cols = rng.permutation(g.n)[: rng.integers(1, 12)]
        R_new[b, cols] = rng.integers(1, 6, cols.size)
    N = min(128, g.n)
    items, scores = model.recommend_new(R_new, N, features=g.features)
    ok = items >= 0
    tptr = np.zeros(B + 1, np.int64)
    tptr[1:] = np.cumsum(ok.sum(axis=1))
    rank, cand, sc = model.rank_of_new(R_new, (tptr, items[ok]), features=g.features)
    assert (rank == np.tile(np.arange(N), B).reshape(B, N)[ok]).all()
    assert (sc.astype(np.float64) == scores[ok]).all()
    assert (cand == np.repeat(g.n - (~np.isnan(R_new)).sum(axis=1), ok.sum(axis=1))).all()


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_property():
    """1M users x 100K items, k = 64, ~100 seen items per user (as test_full_size_all_users): 4096 users, checked
    against recommend(N = 128) - the item at position p has rank p, unseen targets ranked below 128 are listed."""
    torch, layout, be, dev = env().short
    m, n, k = 1_000_000, 100_000, 64
    gen = torch.Generator(device=dev).manual_seed(3)
    ld = layout.padded_k(k)
    f = dict(k=k, ld=ld, U=torch.randn(m, ld, device=dev, generator=gen) * 0.3,
             Z=torch.randn(n, ld, device=dev, generator=gen) * 0.3,
             b_u=torch.randn(m, device=dev, generator=gen) * 0.1, b_i=torch.randn(n, device=dev, generator=gen) * 0.1,
             mu=torch.tensor([3.6], dtype=torch.float64, device=dev))
    raw = torch.randint(0, n, (m, 100), device=dev, generator=gen, dtype=torch.int64).sort(dim=1).values
    keep = torch.ones_like(raw, dtype=torch.bool)
    keep[:, 1:] = raw[:, 1:] != raw[:, :-1]
    seen_ptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    seen_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
    ptr, idx = seen_ptr.cpu().numpy(), raw[keep].to(torch.int32).cpu().numpy()
    users = np.random.default_rng(5).choice(m, 4096, replace=False)
    _cross_check(torch, be, f, users, n, ptr, idx, dev, 5)


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_return_the_documented_status():
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    m, n, k, T = 8, 5000, 64, 3
    f = factors(torch, layout, dev, m, n, k, seed=1)
    users = torch.arange(m, dtype=torch.int32, device=dev)
    q_ptr = torch.arange(m + 1, dtype=torch.int64, device=dev) * T
    q_items = torch.arange(m * T, dtype=torch.int32, device=dev)
    sc = torch.full((m * T,), 7.0, dtype=torch.float32, device=dev)
    ab = torch.full((m * T,), 7, dtype=torch.int32, device=dev)
    nc = torch.full((m,), 7, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(k=k, ld=f["ld"], n=n, nq=m, nt=m * T, nslices=0, out=(sc, ab, nc), q=(users, q_ptr, q_items), ws=None,
             wsb=0, seen=(None, None)):
        return lib.als_rank_count(k, ld, n, p(f["U"]), p(f["Z"]), p(f["b_u"]), p(f["b_i"]), p(f["mu"]), p(seen[0]),
                                  p(seen[1]), nq, p(q[0]), p(q[1]), p(q[2]), nt, nslices, p(out[0]), p(out[1]),
                                  p(out[2]), p(ws), wsb, stream)
    E_BADARG, E_BADK = -1, -2
    assert call(k=0) == E_BADK and call(k=161) == E_BADK
    assert call(ld=16) == E_BADARG and call(n=0) == E_BADARG and call(nq=-1) == E_BADARG and call(nt=-1) == E_BADARG
    assert call(nslices=-1) == E_BADARG and call(nslices=65) == E_BADARG
    assert call(out=(None, ab, nc)) == E_BADARG and call(out=(sc, None, nc)) == E_BADARG
    assert call(out=(sc, ab, None)) == E_BADARG
    assert call(q=(None, q_ptr, q_items)) == E_BADARG and call(q=(users, None, q_items)) == E_BADARG
    assert call(q=(users, q_ptr, None)) == E_BADARG
    assert call(seen=(q_ptr, None)) == E_BADARG
    need = lib.als_rank_count_workspace_bytes(k, m, m * T, n, 4)
    assert need == 4 * (m * T + m) * 4
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert call(nslices=4) == E_BADARG                                   # no workspace
    assert call(nslices=4, ws=ws, wsb=need - 1) == E_BADARG              # too small
    assert call(nq=0) == 0                                               # no-op
    torch.cuda.synchronize()
    assert (sc == 7.0).all() and (ab == 7).all() and (nc == 7).all()
    assert call(nslices=4, ws=ws, wsb=need) == 0
    torch.cuda.synchronize()
    assert (nc == n).all() and (ab >= 0).all() and (ab < n).all()
