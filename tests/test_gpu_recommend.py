"""K8 (GPU): fused top-N recommendation (csrc/recommend.hip, als_recommend_topk) and ALS.recommend.

The oracle is exact: every returned score is bitwise the fp32 value als_predict_dense writes, so the expected
lists are `topn` of tests/serving_ref.py on the predict_dense rows (seen items removed, sorted stably by (score
descending, item ascending)), and outputs are compared with ==."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import serving_ref as ref
from tests.common import Golden, model_for
from tests.gpu_common import assert_same, env, factors, predict_dense, run_topk, seen_csr


@pytest.mark.parametrize("k", [1, 16, 50, 64, 128, 160])
@pytest.mark.parametrize("n", [1, 17, 1000, 4099])
def test_kernel_equals_masked_dense_sort(k, n):
    torch, layout, be, dev = env().short
    m = 40
    f = factors(torch, layout, dev, m, n, k, seed=10 * k + n)
    ptr, idx, rows = seen_csr(m, n, seed=k + n)
    dense = predict_dense(torch, be, f, m, n, dev)
    users = np.concatenate([np.arange(m), [3, 1, 3, 0]])[::-1].copy()      # order and duplicates kept
    for N in (1, 10, 128):
        got = run_topk(torch, be, f, users, n, ptr, idx, N, dev)
        assert_same(got, ref.topn_batch(dense[users], [rows[u] for u in users], None, N))
        if n > 3 and N >= 3:
            b = int(np.nonzero(users == 1)[0][0])                          # all but 3 seen: padded
            assert got[2][b] == 3 and (got[1][b, 3:] == -1).all() and np.isneginf(got[0][b, 3:]).all()
    # no exclusion
    got = run_topk(torch, be, f, users, n, None, None, 10, dev)
    assert_same(got, ref.topn_batch(dense[users], [np.empty(0, np.int64)] * users.size, None, 10))


@pytest.mark.parametrize("N", [1, 10, 33, 128])
def test_ties_go_to_the_lowest_item_index(N):
    torch, layout, be, dev = env().short
    m, n = 64, 3001
    f = factors(torch, layout, dev, m, n, 5, seed=N, integer=True)
    ptr, idx, rows = seen_csr(m, n, seed=N, density=0.1)
    dense = predict_dense(torch, be, f, m, n, dev)
    users = np.arange(m)
    got = run_topk(torch, be, f, users, n, ptr, idx, N, dev)
    tv, ti, tc = ref.topn_batch(dense, rows, None, N)
    # ties across the N-th boundary really occur
    assert sum(int((dense[u] == tv[u, N - 1]).sum()) > 1 for u in range(3, m)) > m // 2
    assert_same(got, (tv, ti, tc))


@pytest.mark.parametrize("B,N", [(1, 10), (1, 128), (3000, 10), (3000, 100)])
def test_result_does_not_depend_on_the_slice_count(B, N, monkeypatch):
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    m, n, k = 3000, 5003, 64
    f = factors(torch, layout, dev, m, n, k, seed=B + N)
    ptr, idx, rows = seen_csr(m, n, seed=B)
    users = np.random.default_rng(B).permutation(m)[:B]
    outs = []
    for s in (1, 2, 7, 64):
        assert s <= 64 and _hip.load().als_recommend_workspace_bytes(B, n, N, s) == (0 if s == 1 else s * B * N * 8)
        monkeypatch.setenv("ALS_RECOMMEND_SLICES", str(s))
        outs.append(run_topk(torch, be, f, users, n, ptr, idx, N, dev))
    monkeypatch.delenv("ALS_RECOMMEND_SLICES")
    outs.append(run_topk(torch, be, f, users, n, ptr, idx, N, dev))          # automatic
    for o in outs[1:]:
        assert_same(o, outs[0])
    dense = predict_dense(torch, be, f, m, n, dev)
    assert_same(outs[0], ref.topn_batch(dense[users], [rows[u] for u in users], None, N))


# ---------------------------------------------------------------------------------------------- model level
def _check_model(model, m, n, train_rows, train_cols, features):
    P = model.predict(features).astype(np.float32)            # fp32 values widened: exact round trip
    seen = [train_cols[train_rows == u] for u in range(m)]
    for N in (1, 10, 128):
        items, scores = model.recommend(None, N, features=features)
        assert items.shape == (m, N) and items.dtype == np.int64 and scores.dtype == np.float64
        tv, ti, _ = ref.topn_batch(P, seen, None, N)
        assert (items == ti).all() and (scores == tv.astype(np.float64)).all()
        for u in range(m):                                   # no training item is ever returned
            assert not np.isin(items[u], seen[u]).any()
    pad = [u for u in range(m) if n - seen[u].size < 128]
    if pad:                                                  # N > n - seen pads
        items, scores = model.recommend(pad, 128, features=features)
        assert (items[:, -1] == -1).all() and np.isneginf(scores[:, -1]).all()
    sub = np.array([m - 1, 0, m - 1, m // 2])                # order and duplicates kept
    items, scores = model.recommend(sub, 7, features=features)
    full_i, full_s = model.recommend(None, 7, features=features)
    assert (items == full_i[sub]).all() and (scores == full_s[sub]).all()
    # the documented contract
    ok = items >= 0
    assert (scores[ok] == model.predict(features)[np.repeat(sub, 7).reshape(-1, 7)[ok], items[ok]]).all()


@pytest.mark.parametrize("name,use_features,kw", [
    ("g3_empty", True, {}),
    ("g4_feat_uw5", True, {}),
    ("g4_feat_uw5", False, {}),
    ("g5_graph_a5.0", True, {}),
    ("g1_plain", True, {"solve_dtype": "float64"}),
])
def test_model_recommend_on_fixtures(name, use_features, kw):
    env()
    g = Golden(name)
    r, c, v = g.train
    model = model_for(g, device="cuda:0", **kw)
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"], verbose=0)
    _check_model(model, g.m, g.n, r, c, g.features if use_features else None)


def test_sweep_fold_excludes_that_folds_training_ratings():
    env()
    from collaborative_filtering_amd import cv, sweep
    g = Golden("g4_feat_uw2")
    ratings = cv.CooRatings(g.rows, g.cols, g.vals, (g.m, g.n))
    folds = cv.make_entrywise_folds(ratings, n_splits=3, seed=42)
    drv = sweep.SweepDriver(ratings, g.features, folds)
    f = drv.folds[1]
    model = model_for(g, device=drv.dev, fit_cache=f.cache)
    model._fit_sides(f.csr, f.csc, g.features, None, 1, 0, None, S_trusted=True)     # as SweepDriver.cv_score fits
    (tr, tc, _), (vr, vc, vv), _ = cv.train_valid_split(ratings, folds, 1)
    _check_model(model, g.m, g.n, tr, tc, g.features)
    items, _ = model.recommend(None, 128, features=g.features)
    held = set(zip(vr.tolist(), vc.tolist()))
    assert any((u, int(i)) in held for u in range(g.m) for i in items[u])            # held-out items can come back
    res = cv.ranking_at_k(model, vr, vc, vv, K=10, features=g.features)
    assert res["users"] == np.unique(vr).size and 0.0 <= res["recall@K"] <= 1.0 and 0.0 <= res["ndcg@K"] <= 1.0


# ------------------------------------------------------------------------------------------------ full size
def test_full_size_all_users():
    """configs[3] shape: 1M users x 100K items, k = 64, ~100 seen items per user, all users, N = 10."""
    torch, layout, be, dev = env().short
    m, n, k, N = 1_000_000, 100_000, 64, 10
    gen = torch.Generator(device=dev).manual_seed(3)
    ld = layout.padded_k(k)
    U = torch.randn(m, ld, device=dev, generator=gen) * 0.3
    Z = torch.randn(n, ld, device=dev, generator=gen) * 0.3
    b_u = torch.randn(m, device=dev, generator=gen) * 0.1
    b_i = torch.randn(n, device=dev, generator=gen) * 0.1
    mu = torch.tensor([3.6], dtype=torch.float64, device=dev)
    raw = torch.randint(0, n, (m, 100), device=dev, generator=gen, dtype=torch.int64).sort(dim=1).values
    keep = torch.ones_like(raw, dtype=torch.bool)
    keep[:, 1:] = raw[:, 1:] != raw[:, :-1]
    seen_ptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    seen_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
    seen_idx = raw[keep].to(torch.int32)
    users = torch.arange(m, dtype=torch.int32, device=dev)
    tv = torch.empty(m, N, dtype=torch.float32, device=dev)
    ti = torch.empty(m, N, dtype=torch.int32, device=dev)
    tc = torch.empty(m, dtype=torch.int32, device=dev)
    be.recommend_topk(k=k, ld=ld, users=users, n=n, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, seen_ptr=seen_ptr,
                      seen_idx=seen_idx, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)
    torch.cuda.synchronize()
    assert (tc == N).all() and (ti >= 0).all()
    # no seen item anywhere: (user, item) keys against the globally sorted seen keys
    skeys = torch.repeat_interleave(torch.arange(m, device=dev), seen_ptr[1:] - seen_ptr[:-1]) * n + seen_idx
    rkeys = (torch.arange(m, device=dev)[:, None] * n + ti.to(torch.int64)).reshape(-1)
    pos = torch.searchsorted(skeys, rkeys).clamp(max=skeys.numel() - 1)
    assert not (skeys[pos] == rkeys).any()
    # 512 sampled users: predict_dense on their gathered rows, seen removed, stable sort
    samp = torch.from_numpy(np.random.default_rng(5).choice(m, 512, replace=False)).to(dev)
    out = torch.empty(512, n, dtype=torch.float32, device=dev)
    be.predict_dense(k=k, ld=ld, m=512, n=n, U=U[samp].contiguous(), Z=Z, b_u=b_u[samp].contiguous(), b_i=b_i,
                     mu=mu, out=out)
    sp, si = seen_ptr.cpu().numpy(), seen_idx.cpu().numpy()
    s_np = samp.cpu().numpy()
    exp = ref.topn_batch(out.cpu().numpy(), [si[sp[u]: sp[u + 1]] for u in s_np], None, N)
    assert_same((tv[samp].cpu().numpy(), ti[samp].cpu().numpy(), tc[samp].cpu().numpy()), exp)


# ------------------------------------------------------------------------------------------------ bad arguments
def test_bad_arguments_return_the_documented_status():
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    m, n, k, N = 8, 5000, 64, 10
    f = factors(torch, layout, dev, m, n, k, seed=1)
    users = torch.arange(m, dtype=torch.int32, device=dev)
    tv = torch.full((m, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((m, N), 7, dtype=torch.int32, device=dev)
    tc = torch.full((m,), 7, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(k=k, ld=f["ld"], nusers=m, topn=N, nslices=0, out=(tv, ti, tc), ws=None, wsb=0):
        return lib.als_recommend_topk(k, ld, nusers, p(users), n, p(f["U"]), p(f["Z"]), p(f["b_u"]), p(f["b_i"]),
                                      p(f["mu"]), None, None, topn, nslices, p(out[0]), p(out[1]), p(out[2]),
                                      p(ws), wsb, stream)
    E_BADARG, E_BADK = -1, -2
    assert call(k=0) == E_BADK and call(k=161) == E_BADK
    assert call(ld=16) == E_BADARG
    assert call(topn=0) == E_BADARG and call(topn=129) == E_BADARG
    assert call(nslices=-1) == E_BADARG and call(nslices=65) == E_BADARG
    assert call(out=(None, ti, tc)) == E_BADARG and call(out=(tv, None, tc)) == E_BADARG
    assert call(out=(tv, ti, None)) == E_BADARG
    need = lib.als_recommend_workspace_bytes(m, n, N, 4)
    assert need == 4 * m * N * 8
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert call(nslices=4) == E_BADARG                                   # no workspace
    assert call(nslices=4, ws=ws, wsb=need - 1) == E_BADARG              # too small
    assert call(nusers=0) == 0                                           # no-op
    torch.cuda.synchronize()
    assert (tv == 7.0).all() and (ti == 7).all() and (tc == 7).all()
    assert call(nslices=4, ws=ws, wsb=need) == 0
    torch.cuda.synchronize()
    assert (tc == N).all()
