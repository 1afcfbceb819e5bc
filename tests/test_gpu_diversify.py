"""K12 (GPU): MMR re-ranking and list diversity (csrc/diversify.hip: als_mmr_rerank, als_list_diversity) and
ALS.recommend_diverse / recommend_new_diverse / list_diversity.

The reference is tests/mmr_ref.py (float64).  The picks are discrete, so the kernel's list is not compared with a
float64 greedy run (it would flip at near-ties): for every row and step the kernel's own previous picks are taken,
every remaining candidate's objective is computed in float64, and the kernel's pick has to be within TOL(k) of the
best.  TOL(k) = 4 (k + 8) 2^-24 is derived, not tuned: an fp32 dot product of k terms (k u relative to the norms),
two norms, one division and the relevance quotient, lambda <= 1, for the two candidates compared.  The largest
shortfalls observed go to the ALS_RECORD_MARGINS file (kept as profiles/diversify_margins.json)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import mmr_ref
from tests.common import Golden, model_for
from tests.gpu_common import env, factors, record_margins, upload

N_ITEMS, B = 1003, 43


def TOL(k):
    return 4.0 * (k + 8) * 2.0 ** -24


_POOLS = {}


def _setup(k, pool):
    """Random factors and every row's top-`pool` list (als_recommend_topk, nothing seen), made once per (k, pool):
    (f, Z float64 [n, k'], cand_val fp32 [B, pool], cand_idx int32 [B, pool]) - device tensors, never changed."""
    if (k, pool) not in _POOLS:
        torch, layout, be, dev = env().short
        f = factors(torch, layout, dev, B, N_ITEMS, k, seed=7 * k + 1)
        tv = torch.empty(B, pool, dtype=torch.float32, device=dev)
        ti = torch.empty(B, pool, dtype=torch.int32, device=dev)
        tc = torch.empty(B, dtype=torch.int32, device=dev)
        be.recommend_topk(k=k, ld=f["ld"], users=torch.arange(B, dtype=torch.int32, device=dev), n=N_ITEMS, U=f["U"],
                          Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"], mu=f["mu"], seen_ptr=None, seen_idx=None, topn=pool,
                          top_val=tv, top_idx=ti, top_cnt=tc)
        assert (tc == pool).all()
        _POOLS[(k, pool)] = (f, f["Z"].cpu().numpy().astype(np.float64), tv, ti)
    return _POOLS[(k, pool)]


def _rerank(f, n, cand_val, cand_idx, lam, N, ild=True):
    """als_mmr_rerank on device tensors -> numpy (top_val, top_idx, top_cnt, top_ild or None)."""
    torch, _, be, dev = env().short
    Bn = cand_idx.shape[0]
    tv = torch.full((Bn, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((Bn, N), 7, dtype=torch.int32, device=dev)
    tc = torch.full((Bn,), 7, dtype=torch.int32, device=dev)
    tl = torch.full((Bn,), 7.0, dtype=torch.float32, device=dev) if ild else None
    be.mmr_rerank(k=f["k"], ld=f["ld"], n=n, Z=f["Z"], cand_val=cand_val, cand_idx=cand_idx, lam=lam, topn=N,
                  top_val=tv, top_idx=ti, top_cnt=tc, top_ild=tl)
    return tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy(), None if tl is None else tl.cpu().numpy()


def _dev(a):
    return upload(a, env().dev)


def _follow(Z64, n, cv, ci, lam, N, got, tol):
    """Structure and path-following check of one call (cv / ci: the numpy pool; the ids of a list are distinct).
    Returns the largest shortfall max obj - obj[kernel pick] seen."""
    tv, ti, tc, tl = got
    worst = 0.0
    for b in range(ci.shape[0]):
        M = mmr_ref.list_len(ci[b], n)
        cnt = min(N, M)
        assert tc[b] == cnt
        assert (ti[b, cnt:] == -1).all() and np.isneginf(tv[b, cnt:]).all()
        ids = ci[b, :M]
        pos = {int(i): j for j, i in enumerate(ids)}
        assert len(pos) == M
        picks = [pos[int(i)] for i in ti[b, :cnt]]                       # KeyError: not from the pool
        assert len(set(picks)) == cnt                                    # distinct
        assert (tv[b, :cnt].view(np.int32) == cv[b, picks].view(np.int32)).all()     # the pool's scores, bitwise
        S = mmr_ref.similarities(Z64[ids])
        rel = mmr_ref.relevance(cv[b, :M])
        for t, p in enumerate(picks):
            obj = mmr_ref.objectives(rel, S, picks[:t], lam)
            rest = np.ones(M, bool)
            rest[picks[:t]] = False
            short = obj[rest].max() - obj[p]
            worst = max(worst, short)
            assert short <= tol, (b, t, p, short, tol)
        if tl is not None:
            want = mmr_ref.ild(S, picks)
            assert (np.isnan(tl[b]) and cnt < 2) if np.isnan(want) else abs(tl[b] - want) <= tol, (b, tl[b], want)
    return worst


# ------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("pool", [10, 17, 64, 65, 128])
@pytest.mark.parametrize("k", [8, 64, 160])
def test_lambda_zero_is_the_head_of_the_pool_and_lambda_one_starts_at_the_top(k, pool):
    f, _, cv, ci = _setup(k, pool)
    cvh, cih = cv.cpu().numpy(), ci.cpu().numpy()
    for N in (1, 10, pool):
        tv, ti, tc, _ = _rerank(f, N_ITEMS, cv, ci, 0.0, N, ild=False)
        assert (ti == cih[:, :N]).all() and (tv.view(np.int32) == cvh[:, :N].view(np.int32)).all() and (tc == N).all()
        tv, ti, tc, _ = _rerank(f, N_ITEMS, cv, ci, 1.0, N)
        assert (ti[:, 0] == cih[:, 0]).all() and (tv[:, 0] == cvh[:, 0]).all() and (tc == N).all()


# ------------------------------------------------------------------------------------------ 2. float64 path
@pytest.mark.parametrize("lam", [0.3, 0.7])
@pytest.mark.parametrize("k", [16, 64, 72, 160])
def test_every_pick_is_the_float64_best_given_the_kernels_own_path(k, lam):
    worst = 0.0
    for pool, N in ((128, 128), (40, 10), (65, 33)):
        f, Z64, cv, ci = _setup(k, pool)
        got = _rerank(f, N_ITEMS, cv, ci, lam, N)
        worst = max(worst, _follow(Z64, N_ITEMS, cv.cpu().numpy(), ci.cpu().numpy(), lam, N, got, TOL(k)))
        assert (got[1][:, 0] == ci.cpu().numpy()[:, 0]).all()
    print(f"k={k} lambda={lam}: largest shortfall {worst:.3e}, tol {TOL(k):.3e}")
    record_margins(f"mmr_rerank k={k} lambda={lam}", {"shortfall": worst, "tol": TOL(k)})


# ------------------------------------------------------------------------------------------ 3. exact ties
@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
def test_equal_objectives_go_to_the_lower_pool_position(lam):
    torch, layout, be, dev = env().short
    k, pool = 24, 128
    f = dict(factors(torch, layout, dev, B, N_ITEMS, k, seed=99))
    Z = f["Z"].cpu().numpy()
    twins = [[10, 20, 30, 40], [500, 77, 900, 3, 650]]                  # ids with identical rows
    for grp in twins:
        Z[grp] = Z[grp[0]]
    f["Z"] = _dev(Z)
    rng = np.random.default_rng(5)
    places = [[3, 4, 5, 6], [60, 64, 70, 100, 125]]                     # the second group spans both lane halves
    ci = np.empty((B, pool), np.int32)
    cv = np.empty((B, pool), np.float32)
    others = np.setdiff1d(np.arange(N_ITEMS), sum(twins, []))
    for b in range(B):
        ci[b] = rng.permutation(others)[:pool]
        cv[b] = np.sort(rng.normal(size=pool).astype(np.float32))[::-1]
        for grp, at in zip(twins, places):
            at = at if b % 2 == 0 else [a + b % 3 for a in at][: len(grp)]
            ci[b, at] = rng.permutation(grp)                            # any id order: the POSITION decides
            cv[b, at] = cv[b, at[0]]                                    # identical scores
    for N in (pool, 20):
        tv, ti, tc, _ = _rerank(f, N_ITEMS, _dev(cv), _dev(ci), lam, N)
        _follow(Z.astype(np.float64), N_ITEMS, cv, ci, lam, N, (tv, ti, tc, None), TOL(k))
        for b in range(B):
            pos = {int(i): j for j, i in enumerate(ci[b])}
            for grp in twins:
                order = [pos[int(i)] for i in ti[b, : tc[b]] if int(i) in grp]
                assert order == sorted(order), (b, order)
                # a twin is never passed over by a later-placed twin: the picked ones are the lowest placed
                assert order == sorted(pos[g] for g in grp)[: len(order)]


# ------------------------------------------------------------------------------------------ 4. clusters
def test_diversity_spreads_a_list_over_clusters():
    torch, layout, be, dev = env().short
    k, pool, N, nc = 64, 64, 8, 8
    f = dict(factors(torch, layout, dev, B, N_ITEMS, k, seed=4))
    rng = np.random.default_rng(8)
    centres = rng.normal(size=(nc, k))
    Z = np.zeros((N_ITEMS, f["ld"]), np.float32)
    Z[:, :k] = centres[np.arange(N_ITEMS) % nc] + 1e-3 * rng.normal(size=(N_ITEMS, k))      # item i: cluster i % 8
    f["Z"] = _dev(Z)
    ci = np.empty((B, pool), np.int32)
    for b in range(B):
        c0 = b % nc                                                     # positions 0 .. 15: all of cluster c0
        head = rng.permutation(np.arange(c0, N_ITEMS, nc))[:16]
        tail = rng.permutation(np.nonzero(np.arange(N_ITEMS) % nc != c0)[0])[: pool - 16]
        ci[b] = np.concatenate([head, tail])
    cv = np.tile((5.0 - 0.01 * np.arange(pool)).astype(np.float32), (B, 1))
    ref = mmr_ref.rerank(Z.astype(np.float64), N_ITEMS, cv, ci, 0.7, N)
    assert all(np.unique(ref[1][b] % nc).size == 8 for b in range(B))   # the float64 greedy: one item per cluster
    got = _rerank(f, N_ITEMS, _dev(cv), _dev(ci), 0.7, N)
    _follow(Z.astype(np.float64), N_ITEMS, cv, ci, 0.7, N, got, TOL(k))
    assert all(np.unique(got[1][b] % nc).size >= 4 for b in range(B))
    flat = _rerank(f, N_ITEMS, _dev(cv), _dev(ci), 0.0, N)
    assert all(np.unique(flat[1][b] % nc).size == 1 for b in range(B))
    assert (got[3] > 0.5).all() and (flat[3] < 1e-4).all()              # and the ILD says so


# ------------------------------------------------------------------------------------------ 5. short / degenerate
@pytest.mark.parametrize("pool", [10, 64, 65, 128])
def test_short_and_degenerate_pools(pool):
    k = 50
    f, Z64, cv_d, ci_d = _setup(k, pool)
    f = dict(f)
    Z = f["Z"].cpu().numpy().copy()
    cv, ci = cv_d.cpu().numpy().copy(), ci_d.cpu().numpy().copy()
    zero_item = int(ci[9, 2])
    Z[zero_item] = 0.0                                                  # row 9 (and whoever lists it): sim = 0, no NaN
    f["Z"] = _dev(Z)
    for b, valid in zip(range(4), (0, 1, 2, pool - 1)):                 # rows with 0, 1, 2, pool - 1 entries
        ci[b, valid:] = -1
        cv[b, valid:] = -np.inf
    cv[4] = cv[4, 0]                                                    # all scores equal: rel = 0 everywhere
    mid = min(5, pool - 1)
    ci[5, mid] = N_ITEMS + 7                                            # an id >= n ends the list there ...
    ci[6, mid] = 2 ** 31 - 1                                            # ... however large
    ci[7, mid] = N_ITEMS                                                # ... or just one past the table
    for lam, N in ((0.5, pool), (0.5, min(pool, 10)), (1.0, pool), (0.0, 1)):
        got = _rerank(f, N_ITEMS, _dev(cv), _dev(ci), lam, N)
        _follow(Z.astype(np.float64), N_ITEMS, cv, ci, lam, N, got, TOL(k))
        tv, ti, tc, tl = got
        assert tc[:4].tolist() == [min(N, v) for v in (0, 1, 2, pool - 1)]
        assert tc[5] == tc[6] == tc[7] == min(N, mid)
        assert np.isnan(tl[:2]).all() and (ti[0] == -1).all() and np.isneginf(tv[0]).all()
        assert not np.isnan(tl[(tc >= 2)]).any() and not np.isnan(tv).any()
        if lam == 0.5:                                                  # rel = 0: the first pick is position 0
            assert ti[4, 0] == ci[4, 0]
    torch, _, be, dev = env().short
    ild = torch.empty(B, dtype=torch.float32, device=dev)
    be.list_diversity(k=k, ld=f["ld"], n=N_ITEMS, Z=f["Z"], idx=_dev(ci), ild=ild)
    want = mmr_ref.list_diversity(Z.astype(np.float64), N_ITEMS, ci)
    got = ild.cpu().numpy()
    assert (np.isnan(got) == np.isnan(want)).all() and np.isnan(got[:2]).all()
    assert np.nanmax(np.abs(got - want)) <= TOL(k)


# ------------------------------------------------------------------------------------------ 6. reproducible
@pytest.mark.parametrize("k,pool", [(64, 128), (24, 40)])
def test_two_runs_are_bitwise_equal(k, pool):
    f, _, cv, ci = _setup(k, pool)
    a = _rerank(f, N_ITEMS, cv, ci, 0.6, pool // 2)
    b = _rerank(f, N_ITEMS, cv, ci, 0.6, pool // 2)
    for x, y in zip(a, b):
        assert (x.view(np.int32) == y.view(np.int32)).all()


# ------------------------------------------------------------------------------------------ 7. end to end
def test_model_level_calls():
    env()
    from collaborative_filtering_amd.serving import FoldedItems
    g = Golden("g4_feat_uw5")
    r, c, v = g.train
    model = model_for(g, device="cuda:0")
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"], verbose=0)
    model._eng.REC_BATCH = 16
    ft = g.features
    rng = np.random.default_rng(3)
    allow = rng.permutation(g.n)[: g.n // 2]
    block = allow[:5]
    k, Bn = model.V.shape[1], 6
    Zf = rng.normal(size=(Bn, k)).astype(np.float32).astype(np.float64)
    folded = FoldedItems(Zf.copy(), rng.normal(size=Bn).astype(np.float32).astype(np.float64) + 1.0, Zf, None,
                         (np.zeros(Bn + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)))
    N = 10
    for kw in ({}, dict(items=allow, filter_items=block), dict(new_items=folded), dict(exclude_seen=False)):
        want = model.recommend(None, N, features=ft, **kw)
        got = model.recommend_diverse(None, N, diversity=0.0, features=ft, **kw)
        assert got[0].dtype == np.int64 and got[1].dtype == np.float64 and got[0].shape == (g.m, N)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
        pool = 40
        pi, ps = model.recommend(None, pool, features=ft, **kw)
        items, scores, ild = model._recommend_diverse(None, N, 0.5, None, ft, kw.get("exclude_seen", True),
                                                      kw.get("new_items"), kw.get("items"), kw.get("filter_items"), True)
        pub = model.recommend_diverse(None, N, diversity=0.5, features=ft, **kw)
        assert (pub[0] == items).all() and (pub[1] == scores).all()
        for u in range(g.m):
            ok = items[u] >= 0
            at = [int(np.nonzero(pi[u] == i)[0][0]) for i in items[u][ok]]           # IndexError: not in the pool
            assert len(set(at)) == len(at) and (scores[u][ok] == ps[u][at]).all()
            assert ok.sum() == min(N, (pi[u] >= 0).sum()) and at[:1] == [0][: len(at)]
        ld_kw = {"new_items": folded} if "new_items" in kw else {}
        again = model.list_diversity(items, features=ft, **ld_kw)
        assert (again.astype(np.float32).view(np.int32) == ild.astype(np.float32).view(np.int32)).all()
        assert (items != want[0]).any()
    R_new = np.full((5, g.n), np.nan)
    for b in range(4):
        R_new[b, rng.permutation(g.n)[:8]] = rng.integers(1, 6, 8)
    want = model.recommend_new(R_new, N, features=ft)
    got = model.recommend_new_diverse(R_new, N, diversity=0.0, features=ft)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    pi, ps = model.recommend_new(R_new, 40, features=ft, filter_items=block)
    items, scores = model.recommend_new_diverse(R_new, N, diversity=0.5, features=ft, filter_items=block)
    for b in range(5):
        at = [int(np.nonzero(pi[b] == i)[0][0]) for i in items[b][items[b] >= 0]]
        assert (scores[b][: len(at)] == ps[b][at]).all() and at[0] == 0
    from collaborative_filtering_amd import cv
    base = cv.ranking_at_k(model, g.rows, g.cols, g.vals, K=N, features=ft)
    dv = cv.diversity_at_k(model, g.rows, g.cols, g.vals, K=N, features=ft)
    assert all(dv[key] == val for key, val in base.items())
    more = cv.diversity_at_k(model, g.rows, g.cols, g.vals, K=N, diversity=0.7, features=ft)
    assert more["ild@K"] > dv["ild@K"] and 0.0 < dv["coverage@K"] <= 1.0


# ------------------------------------------------------------------------------------------ 8. bad arguments
def test_bad_arguments_return_the_documented_status():
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    k, pool, N = 64, 40, 10
    f, _, cv, ci = _setup(k, pool)
    tv = torch.full((B, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((B, N), 7, dtype=torch.int32, device=dev)
    tc = torch.full((B,), 7, dtype=torch.int32, device=dev)
    tl = torch.full((B,), 7.0, dtype=torch.float32, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())       # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def mmr(k=k, ld=f["ld"], nrows=B, n=N_ITEMS, Z=f["Z"], pool=pool, cv=cv, ci=ci, lam=0.5, topn=N, out=(tv, ti, tc)):
        return lib.als_mmr_rerank(k, ld, nrows, n, p(Z), pool, p(cv), p(ci), lam, topn, p(out[0]), p(out[1]),
                                  p(out[2]), p(tl), stream)

    def ild(k=k, ld=f["ld"], nrows=B, n=N_ITEMS, Z=f["Z"], length=pool, idx=ci, out=tl):
        return lib.als_list_diversity(k, ld, nrows, n, p(Z), length, p(idx), p(out), stream)
    E_BADARG, E_BADK = -1, -2
    assert mmr(k=0) == E_BADK and mmr(k=161) == E_BADK and ild(k=0) == E_BADK and ild(k=161) == E_BADK
    assert mmr(ld=16) == E_BADARG and ild(ld=80) == E_BADARG
    assert mmr(pool=0) == E_BADARG and mmr(pool=129, topn=1) == E_BADARG
    assert ild(length=0) == E_BADARG and ild(length=129) == E_BADARG
    assert mmr(topn=0) == E_BADARG and mmr(topn=pool + 1) == E_BADARG
    assert mmr(lam=-0.1) == E_BADARG and mmr(lam=1.5) == E_BADARG and mmr(lam=float("nan")) == E_BADARG
    assert mmr(n=0) == E_BADARG and ild(n=0) == E_BADARG and mmr(nrows=-1) == E_BADARG
    assert mmr(Z=None) == E_BADARG and mmr(cv=None) == E_BADARG and mmr(ci=None) == E_BADARG
    assert mmr(out=(None, ti, tc)) == E_BADARG and mmr(out=(tv, None, tc)) == E_BADARG
    assert mmr(out=(tv, ti, None)) == E_BADARG
    assert ild(Z=None) == E_BADARG and ild(idx=None) == E_BADARG and ild(out=None) == E_BADARG
    assert mmr(nrows=0) == 0 and ild(nrows=0) == 0                       # no-ops
    torch.cuda.synchronize()
    assert (tv == 7.0).all() and (ti == 7).all() and (tc == 7).all() and (tl == 7.0).all()      # nothing launched
    assert mmr() == 0
    torch.cuda.synchronize()
    assert (tc == N).all()
