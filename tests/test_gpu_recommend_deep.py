"""K8 deep (GPU): als_recommend_deep (csrc/recommend_deep.hip and the DEEP instantiations of k_recommend) and
ALS.recommend_deep / recommend_new_deep.

The oracle is exact, as in test_gpu_recommend.py: every score is bitwise the fp32 value als_predict_dense writes, so the
expected lists are tests/recommend_deep_ref.py (serving_ref's selection, cut below the cursor) on the predict_dense
rows, and everything is compared with ==.  The output buffers start from a poison value: a slot the call does not
write fails the comparison."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import recommend_deep_ref as dref
from tests import serving_ref as ref
from tests.common import Golden, model_for
from tests.gpu_common import assert_same, env, factors, predict_dense, ptr as cptr, run_topk, seen_csr, upload

NONE = np.zeros(0, np.int64)


def _bitmap(torch, mask, dev):
    return upload(ref.bitmap_numpy(mask).view(np.int32), dev)


def run_deep(torch, be, f, users, n, seen_ptr, seen_idx, N, dev, allow=None, after_keys=None):
    """als_recommend_deep into poisoned buffers -> ((values, items, counts), rounds)."""
    us = upload(np.asarray(users, np.int32), dev)
    B = us.numel()
    tv = torch.full((B, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((B, N), -7, dtype=torch.int32, device=dev)
    tc = torch.full((B,), -7, dtype=torch.int32, device=dev)
    rounds = torch.full((1,), -7, dtype=torch.int32, device=dev)
    be.recommend_deep(k=f["k"], ld=f["ld"], users=us, n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"], mu=f["mu"],
                      seen_ptr=None if seen_ptr is None else upload(seen_ptr, dev),
                      seen_idx=None if seen_idx is None else upload(seen_idx, dev), allow=allow,
                      after_key=None if after_keys is None else upload(np.asarray(after_keys).view(np.int64), dev),
                      topn=N, top_val=tv, top_idx=ti, top_cnt=tc, rounds=rounds)
    return (tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()), int(rounds.item())


def _last_keys(got):
    """The cursor keys of the last entries of a page: 0 for the padding of a short row."""
    tv, ti, _ = got
    last_i = ti[:, -1].astype(np.int64)
    return np.where(last_i < 0, np.uint64(0), dref.keys(tv[:, -1], np.maximum(last_i, 0)))


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("k", [1, 50, 128, 160])
@pytest.mark.parametrize("n", [1, 200, 4099])
def test_kernel_equals_masked_dense_sort(k, n):
    torch, layout, be, dev = env().short
    m = 40
    f = factors(torch, layout, dev, m, n, k, seed=10 * k + n)
    ptr, idx, rows = seen_csr(m, n, seed=k + n)
    dense = predict_dense(torch, be, f, m, n, dev)
    users = np.concatenate([np.arange(m), [3, 1, 3, 0]])[::-1].copy()      # order and duplicates kept
    for N in (129, 200, 1000, 1024):
        got, rounds = run_deep(torch, be, f, users, n, ptr, idx, N, dev)
        assert_same(got, dref.deep_topn_batch(dense[users], [rows[u] for u in users], None, N))
        assert 1 <= rounds <= (N + 127) // 128
        if n > 3:
            b = int(np.nonzero(users == 1)[0][0])                          # all but 3 seen: padded
            assert got[2][b] == 3 and (got[1][b, 3:] == -1).all() and np.isneginf(got[0][b, 3:]).all()
        got, _ = run_deep(torch, be, f, users, n, None, None, N, dev)       # no exclusion
        assert_same(got, dref.deep_topn_batch(dense[users], [NONE] * users.size, None, N))
        if n < N:                                                          # n = 200, N = 1024: every row is padded
            assert (got[2] == n).all() and (got[1][:, n:] == -1).all()


@pytest.mark.parametrize("N", [1, 10, 33, 128])
def test_up_to_128_it_is_recommend_element_for_element(N):
    torch, layout, be, dev = env().short
    m, n, k = 70, 4099, 64
    f = factors(torch, layout, dev, m, n, k, seed=N)
    ptr, idx, rows = seen_csr(m, n, seed=N)
    users = np.arange(m)[::-1].copy()
    got, rounds = run_deep(torch, be, f, users, n, ptr, idx, N, dev)
    assert_same(got, run_topk(torch, be, f, users, n, ptr, idx, N, dev))
    assert rounds == 1


@pytest.mark.parametrize("B,N", [(1, 129), (1, 1024), (300, 129), (300, 1024)])
def test_result_does_not_depend_on_the_slice_count_and_one_slice_takes_every_round(B, N, monkeypatch):
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    m, n, k = 300, 5003, 64
    f = factors(torch, layout, dev, m, n, k, seed=B + N)
    ptr, idx, rows = seen_csr(m, n, seed=B)
    users = np.random.default_rng(B).permutation(m)[:B]
    if B == 1:
        users = np.array([5])                                              # a user with more than 1024 candidates
    nl = 256 if N == 129 else 1024
    outs = []
    for s in (1, 2, 7, 64):
        assert _hip.load().als_recommend_deep_workspace_bytes(B, n, N, s) == 8 * B * (128 * s + nl + s) + 64
        monkeypatch.setenv("ALS_RECOMMEND_SLICES", str(s))
        got, rounds = run_deep(torch, be, f, users, n, ptr, idx, N, dev)
        outs.append(got)
        if s == 1:                                                         # the worst case of the bound
            assert rounds == (N + 127) // 128
    monkeypatch.delenv("ALS_RECOMMEND_SLICES")
    outs.append(run_deep(torch, be, f, users, n, ptr, idx, N, dev)[0])     # automatic
    for o in outs[1:]:
        assert_same(o, outs[0])
    dense = predict_dense(torch, be, f, m, n, dev)
    assert_same(outs[0], dref.deep_topn_batch(dense[users], [rows[u] for u in users], None, N))


@pytest.mark.parametrize("N", [200, 1024])
def test_rounds_on_an_id_correlated_and_on_an_iid_catalogue(N):
    torch, layout, be, dev = env().short
    m, n, k = 40, 16384, 64
    f = factors(torch, layout, dev, m, n, k, seed=N)
    ptr, idx, rows = seen_csr(m, n, seed=N, density=0.01)
    users = np.arange(m)
    seen = [rows[u] for u in users]
    # i.i.d. scores, automatic slicing (>= 4 slices per round of 128): a slice expects N / S <= 32 of the top N, so
    # no slice delivers 128 keys above the N-th and one round is enough - the condition the slice plan exists for
    dense = predict_dense(torch, be, f, m, n, dev)
    got, rounds = run_deep(torch, be, f, users, n, ptr, idx, N, dev)
    assert_same(got, dref.deep_topn_batch(dense, seen, None, N))
    assert rounds == 1
    # b_i strictly decreasing in the item id, 100 per item against dot products of a few tens: the top N are the
    # first unseen ids, all of them in the first slices
    f["b_i"] = upload((-100.0 * np.arange(n)).astype(np.float32), dev)
    dense = predict_dense(torch, be, f, m, n, dev)
    exp = dref.deep_topn_batch(dense, seen, None, N)
    assert (exp[1][:, -1] < N + 400).all()
    got, rounds = run_deep(torch, be, f, users, n, ptr, idx, N, dev)
    assert_same(got, exp)
    assert 1 < rounds <= (N + 127) // 128


@pytest.mark.parametrize("N", [129, 500])
def test_ties_go_to_the_lowest_item_index(N, monkeypatch):
    torch, layout, be, dev = env().short
    m, n = 64, 3001
    f = factors(torch, layout, dev, m, n, 5, seed=N, integer=True)
    ptr, idx, rows = seen_csr(m, n, seed=N, density=0.1)
    dense = predict_dense(torch, be, f, m, n, dev)
    users = np.arange(m)
    tv, ti, tc = dref.deep_topn_batch(dense, rows, None, N)
    # ties across the N-th boundary really occur, and across the 128-key boundary of a round of a single slice
    assert sum(int((dense[u] == tv[u, N - 1]).sum()) > 1 for u in range(3, m)) > m // 2
    assert sum(tv[u, 127] == tv[u, 128] for u in range(3, m)) > m // 2
    for s in ("1", "3", None):
        if s is None:
            monkeypatch.delenv("ALS_RECOMMEND_SLICES")
        else:
            monkeypatch.setenv("ALS_RECOMMEND_SLICES", s)
        got, _ = run_deep(torch, be, f, users, n, ptr, idx, N, dev)
        assert_same(got, (tv, ti, tc))
    # all scores of a user equal: the list is the first N unseen ids
    f["U"] = torch.zeros_like(f["U"])
    got, _ = run_deep(torch, be, f, users, n, ptr, idx, N, dev)
    for u in range(m):
        free = np.setdiff1d(np.arange(n), rows[u])[:N]
        assert (got[1][u, : free.size] == free).all() and got[2][u] == free.size
        assert (got[0][u, : free.size] == got[0][u, 0]).all()


def test_short_candidate_sets(monkeypatch):
    torch, layout, be, dev = env().short
    m, n, k = 40, 4099, 50
    f = factors(torch, layout, dev, m, n, k, seed=1)
    U = f["U"].cpu().numpy()
    U[7] = np.nan                                                          # a user whose every score is NaN
    f["U"] = upload(U, dev)
    ptr, idx, rows = seen_csr(m, n, seed=2)
    dense = predict_dense(torch, be, f, m, n, dev)
    assert np.isnan(dense[7]).all()
    users = np.arange(m)
    rng = np.random.default_rng(3)
    few = np.zeros(n, bool)
    few[rng.permutation(n)[:300]] = True
    got, _ = run_deep(torch, be, f, users, n, None, None, 1000, dev, _bitmap(torch, few, dev))
    assert_same(got, dref.deep_topn_batch(dense, [NONE] * m, few, 1000))
    assert (np.delete(got[2], 7) == 300).all() and got[2][7] == 0
    assert (got[1][:, 300:] == -1).all() and np.isneginf(got[0][:, 300:]).all()
    got, _ = run_deep(torch, be, f, users, n, ptr, idx, 1000, dev, _bitmap(torch, few, dev))
    assert_same(got, dref.deep_topn_batch(dense, rows, few, 1000))
    # allow minus block, seven slices of 608 items: slice 1 = [608, 1216) has no allowed chunk at all
    ok = np.ones(n, bool)
    ok[600:1300] = False
    ok[rng.permutation(n)[:500]] = False
    ok[2000:2100] = False
    for s in ("7", None):
        if s is None:
            monkeypatch.delenv("ALS_RECOMMEND_SLICES")
        else:
            monkeypatch.setenv("ALS_RECOMMEND_SLICES", s)
        for N in (300, 1024):
            got, _ = run_deep(torch, be, f, users, n, ptr, idx, N, dev, _bitmap(torch, ok, dev))
            assert_same(got, dref.deep_topn_batch(dense, rows, ok, N))
    got, _ = run_deep(torch, be, f, users, n, ptr, idx, 200, dev, _bitmap(torch, np.zeros(n, bool), dev))
    assert (got[2] == 0).all() and (got[1] == -1).all() and np.isneginf(got[0]).all()


def test_second_page_is_the_tail_of_a_longer_list_and_padding_ends_it():
    torch, layout, be, dev = env().short
    m, n, k, N = 40, 4099, 64, 300
    f = factors(torch, layout, dev, m, n, k, seed=4)
    ptr, idx, rows = seen_csr(m, n, seed=4)
    users = np.arange(m)
    both, _ = run_deep(torch, be, f, users, n, ptr, idx, 2 * N, dev)
    first, _ = run_deep(torch, be, f, users, n, ptr, idx, N, dev)
    assert_same(first[:2], (both[0][:, :N], both[1][:, :N]))
    second, _ = run_deep(torch, be, f, users, n, ptr, idx, N, dev, after_keys=_last_keys(first))
    assert_same(second[:2], (both[0][:, N:], both[1][:, N:]))
    assert (second[2] == np.maximum(both[2] - N, 0)).all()
    assert second[2][1] == 0 and first[2][1] == 3                          # user 1: three candidates, then none
    dense = predict_dense(torch, be, f, m, n, dev)
    assert_same(second, dref.deep_topn_batch(dense, rows, None, N, after=(first[1][:, -1], first[0][:, -1])))
    done, rounds = run_deep(torch, be, f, users, n, ptr, idx, N, dev, after_keys=np.zeros(m, np.uint64))
    assert (done[2] == 0).all() and (done[1] == -1).all() and np.isneginf(done[0]).all() and rounds == 1
    free, _ = run_deep(torch, be, f, users, n, ptr, idx, N, dev, after_keys=np.full(m, dref.NO_CURSOR))
    assert_same(free, first)


@pytest.mark.parametrize("N,integer", [(128, False), (1000, False), (100, True)])
def test_paging_yields_every_candidate_exactly_once_in_order(N, integer):
    torch, layout, be, dev = env().short
    m, n = 12, 4099
    f = factors(torch, layout, dev, m, n, 5 if integer else 64, seed=N, integer=integer)
    ptr, idx, rows = seen_csr(m, n, seed=N)
    dense = predict_dense(torch, be, f, m, n, dev)
    users = np.arange(m)
    pages = [[] for _ in users]
    keys, inside_a_tie = None, 0
    for _ in range(n // N + 2):
        got, _ = run_deep(torch, be, f, users, n, ptr, idx, N, dev, after_keys=keys)
        for b in users:
            pages[b].extend(got[1][b, : got[2][b]].tolist())
        if (got[2] < N).all():
            break
        if keys is not None:                                   # the cursor sat inside a run of equal scores
            inside_a_tie += int(((got[2] > 0) & (got[0][:, 0] == prev_last)).sum())
        prev_last = got[0][:, -1].copy()
        keys = _last_keys(got)
    else:
        raise AssertionError("paging does not end")
    for b in users:
        assert pages[b] == dref.full_order(dense[b], rows[b], None).tolist()
    if integer:
        assert inside_a_tie > 20


# ---------------------------------------------------------------------------------------------- model level
def test_model_recommend_deep_on_a_fixture(monkeypatch):
    env()
    g = Golden("g4_feat_uw5")
    r, c, v = g.train
    model = model_for(g, device="cuda:0")
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features, tol=g.cfg["tol"], verbose=0)
    monkeypatch.setattr(model._eng, "DEEP_BATCH", 16, raising=False)       # several chunks
    m, n = g.m, g.n
    rng = np.random.default_rng(0)
    B = 9
    C_new = np.full((B, m), np.nan)
    for b in range(B - 1):
        C_new[b, rng.permutation(m)[: 4 + b]] = rng.integers(1, 6, 4 + b)
    folded = model.fold_in_items(C_new, features_new={name: X[:B][::-1].copy() for name, X in g.features.items()})
    P = model.predict(g.features).astype(np.float32)
    Pj = np.concatenate([P, model.predict_new_items(folded).astype(np.float32)], axis=1)
    seen = [np.sort(c[r == u]) for u in range(m)]
    seen_j = [np.concatenate([seen[u], n + np.nonzero(~np.isnan(C_new[:, u]))[0]]) for u in range(m)]
    users = np.arange(m)[::-1].copy()
    allow = np.arange(n + B)[rng.random(n + B) < 0.8]
    block = rng.permutation(n)[:10]
    ok = np.zeros(n + B, bool)
    ok[allow] = True
    ok[block] = False
    N = min(1024, max(129, n // 2))

    def same(got, exp):
        assert got[0].dtype == np.int64 and got[1].dtype == np.float64
        assert (got[0] == exp[1]).all() and (got[1] == exp[0].astype(np.float64)).all()

    same(model.recommend_deep(users, N, features=g.features),
         dref.deep_topn_batch(P[users], [seen[u] for u in users], None, N))
    same(model.recommend_deep(users, N, features=g.features, new_items=folded, items=allow, filter_items=block),
         dref.deep_topn_batch(Pj[users], [seen_j[u] for u in users], ok, N))
    first = model.recommend_deep(users, 40, features=g.features, new_items=folded)
    after = (first[0][:, -1], first[1][:, -1])
    same(model.recommend_deep(users, N, features=g.features, new_items=folded, after=after),
         dref.deep_topn_batch(Pj[users], [seen_j[u] for u in users], None, N, after=after))
    short = model.recommend(users, 100, features=g.features, new_items=folded)
    got = model.recommend_deep(users, 100, features=g.features, new_items=folded)
    assert (got[0] == short[0]).all() and (got[1] == short[1]).all()

    # users outside the fit: the folded table's predict epilogue
    import torch
    R_new = np.full((21, n), np.nan)
    for b in range(20):                                                    # the last row: no ratings
        R_new[b, rng.permutation(n)[: 3 + 2 * b]] = rng.integers(1, 11, 3 + 2 * b) * 0.5
    eng = model._eng
    ip = np.zeros(22, np.int64)
    ip[1:] = np.cumsum((~np.isnan(R_new)).sum(axis=1))
    ix = np.nonzero(~np.isnan(R_new))[1].astype(np.int32)
    vv = R_new[~np.isnan(R_new)].astype(np.float32)
    with torch.cuda.device(eng.dev):
        Z = eng._compose_for(g.features)
        U, b_, _, _ = eng._fold_in_dev(ip, ix, vv, Z, 0)
        Pn = torch.empty(21, n, dtype=torch.float32, device=eng.dev)
        eng.be.predict_dense(k=eng.k, ld=eng.ld, m=21, n=n, U=U, Z=Z, b_u=b_, b_i=eng.b_i, mu=eng.mu, out=Pn)
        Pn = Pn.cpu().numpy()
    rated = [ix[ip[b]: ip[b + 1]].astype(np.int64) for b in range(21)]
    okn = ok[:n]
    first = model.recommend_new_deep(R_new, N, features=g.features, items=allow[allow < n], filter_items=block)
    same(first, dref.deep_topn_batch(Pn, rated, okn, N))
    after = (first[0][:, 10], first[1][:, 10])
    same(model.recommend_new_deep(R_new, N, features=g.features, items=allow[allow < n], filter_items=block,
                                  after=after), dref.deep_topn_batch(Pn, rated, okn, N, after=after))


# ---------------------------------------------------------------------------------------------- the C ABI
def test_bad_arguments():
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    m, n, k = 8, 500, 16
    f = factors(torch, layout, dev, m, n, k, seed=0)
    us = upload(np.arange(m, dtype=np.int32), dev)
    N = 200
    tv = torch.empty(m, N, dtype=torch.float32, device=dev)
    ti = torch.empty(m, N, dtype=torch.int32, device=dev)
    tc = torch.empty(m, dtype=torch.int32, device=dev)
    need = lib.als_recommend_deep_workspace_bytes(m, n, N, 0)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def call(k=k, ld=f["ld"], nusers=m, topn=N, nslices=0, top_val=tv, top_idx=ti, top_cnt=tc, workspace=ws,
             nbytes=need, seen_ptr=None, U=f["U"]):
        return lib.als_recommend_deep(k, ld, nusers, cptr(us), n, cptr(U), cptr(f["Z"]), cptr(f["b_u"]),
                                      cptr(f["b_i"]), cptr(f["mu"]), cptr(seen_ptr), None, None, None, topn, nslices,
                                      cptr(top_val), cptr(top_idx), cptr(top_cnt), None, cptr(workspace), nbytes, None)

    assert call() == 0
    torch.cuda.synchronize()
    assert call(topn=0) == -1 and call(topn=1025) == -1                     # ALS_E_BADARG
    assert call(top_val=None) == -1 and call(top_idx=None) == -1 and call(top_cnt=None) == -1 and call(U=None) == -1
    assert call(ld=32) == -1                                               # ld != als_padded_k(k)
    assert call(k=161, ld=176) == -2                                       # ALS_E_BADK
    assert call(nbytes=need - 1) == -1 and call(workspace=None) == -1
    assert call(nslices=65) == -1 and call(nslices=-1) == -1
    assert call(seen_ptr=us) == -1                                         # seen_ptr without seen_idx
    assert call(nusers=-1) == -1
    assert call(nusers=0, top_val=None, workspace=None, nbytes=0) == 0     # a no-op
    assert lib.als_version() == 103
