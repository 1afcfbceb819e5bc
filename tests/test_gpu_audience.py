"""K14 (GPU): als_audience_topk (csrc/audience.hip) and ALS.recommend_users.

Everything in the contract is exact, so every comparison is ==: the expected lists are `audience_topn` of
tests/audience_ref.py on the columns als_predict_dense itself writes for (U, Z = Q, b_u, b_i = q_bias, mu) - the kernel's
scores have to equal those bitwise - with the rater rows and the allow mask of the call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import audience_ref as aref
from tests.common import Golden, model_for
from tests.gpu_common import assert_same, env, factors, predict_dense, same_bits, seen_csr, upload

ROWS = 40                            # rows of the query table Q in the kernel tests


# ------------------------------------------------------------------------------------------------ launches
def run_audience(torch, be, f, q_ids, m, seen_ptr, seen_idx, N, allow=None):
    """als_audience_topk of the items q_ids (rows of f["Z"] / f["b_i"]) over the first m users of f, into buffers
    that start from 7 -> numpy (values, users, counts).  seen_ptr / seen_idx: host arrays or None (NULL)."""
    dev = f["U"].device
    q = upload(np.asarray(q_ids, np.int32), dev)
    B = q.numel()
    tv = torch.full((B, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((B, N), 7, dtype=torch.int32, device=dev)
    tc = torch.full((B,), 7, dtype=torch.int32, device=dev)
    be.audience_topk(k=f["k"], ld=f["ld"], q_ids=q, Q=f["Z"], q_bias=f["b_i"], m=m, U=f["U"], b_u=f["b_u"], mu=f["mu"],
                     seen_ptr=None if seen_ptr is None else upload(np.asarray(seen_ptr, np.int64), dev),
                     seen_idx=None if seen_idx is None else upload(np.asarray(seen_idx, np.int32), dev),
                     allow=allow, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)
    return tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()


def columns(torch, be, f, m, rows, dev):
    """als_predict_dense over (m users, rows items), transposed -> fp32 [rows, m]: row i = the scores of item i."""
    return np.ascontiguousarray(predict_dense(torch, be, f, m, rows, dev).T)


def oracle(cols, q_ids, rater_lists, ok, N):
    q_ids = np.asarray(q_ids)
    return aref.audience_topn(cols[q_ids], [rater_lists[i] for i in q_ids], ok, N)


def _bitmap(torch, mask, dev):
    """The C ABI's bitmap, packed here with numpy: user u = bit u & 31 of word u >> 5."""
    bits = np.zeros((mask.size + 31) // 32 * 32, np.uint8)
    bits[: mask.size] = mask
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return torch.from_numpy(words.view(np.int32).copy()).to(dev)


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(s) for s in lists])
    idx = np.concatenate([np.asarray(s, np.int64) for s in lists]).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, idx


# ------------------------------------------------------------------------------------------------ shape sweep
@pytest.mark.parametrize("k", [1, 16, 17, 64, 65, 128, 160])
@pytest.mark.parametrize("m", [1, 17, 1000, 4099])
def test_kernel_equals_the_column_sort_of_predict_dense(k, m):
    torch, layout, be, dev = env().short
    f = factors(torch, layout, dev, m, ROWS, k, seed=10 * k + m)
    ptr, idx, raters = seen_csr(ROWS, m, seed=k + m)                       # by ITEM id: item 0 none, item 1 all but 3
    cols = columns(torch, be, f, m, ROWS, dev)
    for nq in (1, 17, 129):
        q = ((np.arange(nq) * 7 + 1) % ROWS)[::-1].copy()                  # order kept, duplicates at nq = 129
        for N in (1, 10, 32, 33, 128):
            got = run_audience(torch, be, f, q, m, ptr, idx, N)
            assert_same(got, oracle(cols, q, raters, None, N))
            tv, ti, tc = got
            assert (tc == np.minimum(N, [m - raters[i].size for i in q])).all()
            for b in range(nq):                                            # padding (N > candidates)
                assert (ti[b, tc[b]:] == -1).all() and np.isneginf(tv[b, tc[b]:]).all()


# ------------------------------------------------------------------------------------------------ rater lists
@pytest.mark.parametrize("m", [4090, 4099])             # automatic slices of 2048 (two) and of 1376 (three) users
def test_rater_lists(m):
    torch, layout, be, dev = env().short
    k = 16
    f = factors(torch, layout, dev, m, 8, k, seed=m)
    rng = np.random.default_rng(m)
    edges = [31, 32, 1375, 1376, 2047, 2048, 2751, 2752, m - 1]
    raters = [np.zeros(0, np.int64),                    # 0 nobody
              np.array([100]),                          # 1 a single rater
              np.arange(m),                             # 2 everybody
              np.array(edges),                          # 3 chunk and slice boundaries, the last user
              np.arange(60, 100),                       # 4 a run of 40: more than one 16-entry load in one chunk
              np.arange(0, 200),                        # 5 a run across chunks from user 0
              np.nonzero(rng.random(m) < 0.1)[0],       # 6 scattered
              np.setdiff1d(np.arange(m), edges)]        # 7 everybody but the boundary users
    ptr, idx = _csr(raters)
    cols = columns(torch, be, f, m, 8, dev)
    q = np.array([0, 1, 2, 3, 4, 5, 6, 7, 3, 2, 0])
    for N in (10, 128):
        got = run_audience(torch, be, f, q, m, ptr, idx, N)
        assert_same(got, oracle(cols, q, raters, None, N))
        tv, ti, tc = got
        assert tc[2] == 0 and (ti[2] == -1).all() and np.isneginf(tv[2]).all()         # everybody rated it
        assert tc[7] == len(edges) and sorted(ti[7][: tc[7]].tolist()) == edges        # N >= 9: exactly those
        for b, i in enumerate(q):
            assert not np.isin(ti[b], raters[i]).any()
        none = run_audience(torch, be, f, q, m, None, None, N)                          # both pointers NULL
        assert_same(none, oracle(cols, q, [raters[0]] * 8, None, N))
        assert (none[2] == min(N, m)).all()


# ------------------------------------------------------------------------------------------------ slices
@pytest.mark.parametrize("B,N", [(1, 10), (1, 128), (200, 10), (200, 128)])
def test_result_does_not_depend_on_the_slice_count(B, N, monkeypatch):
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    m, k = 4099, 64
    f = factors(torch, layout, dev, m, ROWS, k, seed=B + N)
    ptr, idx, raters = seen_csr(ROWS, m, seed=B, density=0.1)              # raters in every slice; item 2: 3200 of them
    q = np.random.default_rng(B).integers(0, ROWS, size=B)
    outs = []
    for s in (1, 2, 3, 64):
        assert _hip.load().als_audience_workspace_bytes(B, m, N, s) == (0 if s == 1 else s * B * N * 8)
        monkeypatch.setenv("ALS_RECOMMEND_SLICES", str(s))
        outs.append(run_audience(torch, be, f, q, m, ptr, idx, N))
    monkeypatch.delenv("ALS_RECOMMEND_SLICES")
    outs.append(run_audience(torch, be, f, q, m, ptr, idx, N))             # automatic
    for o in outs[1:]:
        for g, e in zip(o, outs[0]):
            assert same_bits(g, e)
    assert_same(outs[0], oracle(columns(torch, be, f, m, ROWS, dev), q, raters, None, N))


# ------------------------------------------------------------------------------------------------ allow bitmap
def test_allow_bitmap():
    torch, layout, be, dev = env().short
    m, k = 4099, 64                                                        # three slices, the last chunk ragged
    f = factors(torch, layout, dev, m, ROWS, k, seed=5)
    ptr, idx, raters = seen_csr(ROWS, m, seed=6, density=0.1)
    cols = columns(torch, be, f, m, ROWS, dev)
    rng = np.random.default_rng(7)
    q = np.concatenate([rng.permutation(ROWS)[:20], [0, 1, 2, 2]])
    only = np.zeros(m, bool)
    only[1234] = True
    sparse = np.zeros(m, bool)             # whole zero words between the set ones; raters inside the skipped chunks
    sparse[[40, 41, 2000, 2001, 2002, 3990, m - 1]] = True
    assert raters[2].size > 3000 and np.isin([40, 2001], raters[2]).any() and not np.isin(np.nonzero(sparse)[0],
                                                                                          raters[2]).all()
    assert ((raters[2] > 41) & (raters[2] < 1984)).sum() > 1000            # > 16 raters under the skipped words
    masks = {"30 %": rng.random(m) < 0.3, "one bit": only, "sparse": sparse, "none": np.zeros(m, bool),
             "all": np.ones(m, bool)}
    for name, ok in masks.items():
        for N in (10, 128):
            got = run_audience(torch, be, f, q, m, ptr, idx, N, _bitmap(torch, ok, dev))
            assert_same(got, oracle(cols, q, raters, ok, N))
            if name == "none":
                assert (got[2] == 0).all() and (got[1] == -1).all()
            if name == "sparse":                                           # without exclusion as well
                free = run_audience(torch, be, f, q, m, None, None, N, _bitmap(torch, ok, dev))
                assert_same(free, oracle(cols, q, [raters[0]] * ROWS, ok, N))
                assert (free[2] == int(ok.sum())).all()
    null = run_audience(torch, be, f, q, m, ptr, idx, 10)                  # NULL
    assert_same(null, oracle(cols, q, raters, None, 10))
    ones = _bitmap(torch, np.ones(m, bool), dev)
    ones[-1] = -1                                                          # bits at positions >= m are ignored
    for g, e in zip(run_audience(torch, be, f, q, m, ptr, idx, 10, ones), null):
        assert same_bits(g, e)


# ------------------------------------------------------------------------------------------------ ties, NaN
@pytest.mark.parametrize("N", [1, 10, 33, 128])
def test_ties_go_to_the_lowest_user_id(N, monkeypatch):
    torch, layout, be, dev = env().short
    m, k = 3001, 5
    rng = np.random.default_rng(N)
    ld = layout.padded_k(k)
    U = np.zeros((m, ld), np.float32)
    Q = np.zeros((ROWS, ld), np.float32)
    U[:, :k] = rng.integers(-2, 3, size=(m, k))                            # small integers: many equal scores
    Q[:, :k] = rng.integers(-2, 3, size=(ROWS, k))
    U[1::3] = U[0::3][: U[1::3].shape[0]]                                  # user 3j + 1 is a copy of user 3j
    bu = np.repeat(rng.integers(-1, 2, size=(m + 2) // 3), 3)[:m].astype(np.float32)   # ... with the same bias
    f = dict(k=k, ld=ld, U=upload(U, dev), Z=upload(Q, dev), b_u=upload(bu, dev),
             b_i=upload(rng.integers(-1, 2, size=ROWS).astype(np.float32), dev),
             mu=torch.tensor([0.0], dtype=torch.float64, device=dev))
    cols = columns(torch, be, f, m, ROWS, dev)
    q = np.arange(ROWS)
    none = [np.zeros(0, np.int64)] * ROWS
    exp = oracle(cols, q, none, None, N)
    # ties across the N-th boundary really occur
    assert sum(int((cols[b] == exp[0][b, N - 1]).sum()) > 1 for b in range(ROWS)) > ROWS // 2
    for s in ("1", "4"):                   # 4 slices of 768 users: equal scores on both sides of every boundary
        monkeypatch.setenv("ALS_RECOMMEND_SLICES", s)
        got = run_audience(torch, be, f, q, m, None, None, N)
        assert_same(got, exp)
        for b in range(ROWS):                                              # a copy never precedes its original
            ids = list(got[1][b])
            for u in ids:
                if u % 3 == 1 and u - 1 in ids:
                    assert ids.index(u - 1) < ids.index(u)
    for b in range(ROWS):
        tied = np.nonzero(cols[b] == exp[0][b, 0])[0]
        assert exp[1][b, 0] == tied[0]
    assert any(((cols[b][:768] == exp[0][b, N - 1]).any() and (cols[b][768:] == exp[0][b, N - 1]).any())
               for b in range(ROWS))


def test_nan_rows_are_never_returned_and_a_nan_query_gets_an_empty_list():
    torch, layout, be, dev = env().short
    m, k = 1000, 17
    f = factors(torch, layout, dev, m, ROWS, k, seed=3)
    f["U"][5, 0] = float("nan")
    f["U"][999, k - 1] = float("nan")
    f["Z"][7, 1] = float("nan")
    f["b_u"][40] = float("nan")
    ptr, idx, raters = seen_csr(ROWS, m, seed=4)
    cols = columns(torch, be, f, m, ROWS, dev)
    q = np.arange(ROWS)
    for N in (10, 128):
        tv, ti, tc = got = run_audience(torch, be, f, q, m, ptr, idx, N)
        assert_same(got, oracle(cols, q, raters, None, N))
        assert not np.isin(ti, [5, 40, 999]).any() and not np.isnan(tv).any()
        assert tc[7] == 0 and (ti[7] == -1).all() and np.isneginf(tv[7]).all()
        assert (tc[np.arange(ROWS) != 7] > 0).all()


# ------------------------------------------------------------------------------------------------ bias association
def test_scores_add_the_user_bias_before_the_item_bias():
    """The reason the kernel exists: als_recommend_topk with the two sides swapped forms ((d + mu) + b_i) + b_u, which
    is not the fp32 value ((d + mu) + b_u) + b_i that als_predict_dense writes."""
    torch, layout, be, dev = env().short
    m, k = 1000, 64
    rng = np.random.default_rng(21)
    f = factors(torch, layout, dev, m, ROWS, k, seed=20)
    sign = lambda n: rng.choice([-1.0, 1.0], size=n)                       # noqa: E731
    bu = (sign(m) * rng.uniform(0.1, 1.0, size=m)).astype(np.float32)
    bi = (sign(ROWS) * rng.uniform(0.1, 1.0, size=ROWS)).astype(np.float32)
    f["b_u"], f["b_i"] = upload(bu, dev), upload(bi, dev)
    f["mu"] = torch.tensor([3.3], dtype=torch.float64, device=dev)
    # the dots alone: als_predict_dense with zero biases and mu = 0
    z = dict(f, b_u=torch.zeros_like(f["b_u"]), b_i=torch.zeros_like(f["b_i"]),
             mu=torch.zeros(1, dtype=torch.float64, device=dev))
    d = columns(torch, be, z, m, ROWS, dev)                                # fp32 [ROWS, m]
    mu = np.float32(3.3)
    first = ((d + mu) + bu[None, :]) + bi[:, None]
    swapped = ((d + mu) + bi[:, None]) + bu[None, :]
    assert first.dtype == swapped.dtype == np.float32
    share = float((first != swapped).mean())
    print(f"bias association: {share:.1%} of the {d.size} (item, user) pairs differ in the last bit")
    assert share > 0
    cols = columns(torch, be, f, m, ROWS, dev)
    assert (cols == first).all()                                           # als_predict_dense is the first form
    q = np.arange(ROWS)
    none = [np.zeros(0, np.int64)] * ROWS
    tv, ti, tc = got = run_audience(torch, be, f, q, m, None, None, 128)
    assert_same(got, aref.audience_topn(first, none, None, 128))
    assert (tv == first[q[:, None], ti]).all()
    assert (tv != swapped[q[:, None], ti]).any()                           # and the lists do hold such pairs


# ------------------------------------------------------------------------------------------------ model level
def _check_model(model, g, features, with_new_items):
    r, c, _ = g.train
    m, n = g.m, g.n
    P = model.predict(features).astype(np.float32)                         # fp32 values widened: exact round trip
    raters = [np.sort(r[c == i]) for i in range(n)]
    cols = np.ascontiguousarray(P.T)
    for N in (1, 10, 128):
        users, scores = model.recommend_users(None, N, features=features)
        assert users.shape == (n, N) and users.dtype == np.int64 and scores.dtype == np.float64
        tv, ti, _ = aref.audience_topn(cols, raters, None, N)
        assert (users == ti).all() and (scores == tv.astype(np.float64)).all()
        for i in range(n):                                                 # no training rater is ever returned
            assert not np.isin(users[i], raters[i]).any()
    tv, ti, _ = aref.audience_topn(cols, [raters[0][:0]] * n, None, 10)
    users, scores = model.recommend_users(None, 10, features=features, exclude_seen=False)
    assert (users == ti).all() and (scores == tv.astype(np.float64)).all()
    sub = np.array([n - 1, 0, n - 1, n // 2])                              # order and duplicates kept
    users, scores = model.recommend_users(sub, 7, features=features)
    full_u, full_s = model.recommend_users(None, 7, features=features)
    assert (users == full_u[sub]).all() and (scores == full_s[sub]).all()
    ok = users >= 0                                                        # the documented contract
    assert (scores[ok] == model.predict(features)[users[ok], np.repeat(sub, 7).reshape(-1, 7)[ok]]).all()
    allow = np.random.default_rng(1).random(m) < 0.5                       # filters reach the kernel
    tv, ti, _ = aref.audience_topn(cols, raters, allow, 10)
    for kw in (dict(users=allow), dict(users=np.nonzero(allow)[0]), dict(filter_users=~allow)):
        users, scores = model.recommend_users(None, 10, features=features, **kw)
        assert (users == ti).all() and (scores == tv.astype(np.float64)).all()
    if not with_new_items:
        return
    rng = np.random.default_rng(9)
    B = 5
    C_new = np.full((B, m), np.nan)
    for b in range(B - 1):                                                 # the last one: no ratings
        C_new[b, rng.permutation(m)[:12]] = rng.integers(1, 6, 12)
    fn = {name: X[:B] for name, X in (g.features or {}).items()} or None
    folded = model.fold_in_items(C_new, features_new=fn)
    Pj = np.concatenate([P, model.predict_new_items(folded).astype(np.float32)], axis=1)
    rj = raters + [np.nonzero(~np.isnan(C_new[b]))[0] for b in range(B)]
    tv, ti, _ = aref.audience_topn(np.ascontiguousarray(Pj.T), rj, None, 10)
    users, scores = model.recommend_users(None, 10, features=features, new_items=folded)
    assert users.shape == (n + B, 10) and (users == ti).all() and (scores == tv.astype(np.float64)).all()
    mixed = np.array([n + 1, 3, n + B - 1, 0, n])                          # fitted and folded in one call
    users, scores = model.recommend_users(mixed, 10, features=features, new_items=folded)
    assert (users == ti[mixed]).all() and (scores == tv[mixed].astype(np.float64)).all()
    for b, i in enumerate(mixed):
        assert not np.isin(users[b], rj[i]).any()


@pytest.mark.parametrize("name,use_features,kw,with_new_items", [
    ("g3_empty", True, {}, False),
    ("g4_feat_uw5", True, {}, True),
    ("g4_feat_uw5", False, {}, False),
    ("g5_graph_a5.0", True, {}, False),
    ("g1_plain", True, {"solve_dtype": "float64"}, True),
])
def test_model_recommend_users_on_fixtures(name, use_features, kw, with_new_items):
    env()
    g = Golden(name)
    r, c, v = g.train
    model = model_for(g, device="cuda:0", **kw)
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"], verbose=0)
    _check_model(model, g, (g.features or None) if use_features else None, with_new_items)


# ------------------------------------------------------------------------------------------------ C ABI
def test_bad_arguments_return_the_documented_status():
    import ctypes as C
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    m, k, nq, N = 5000, 64, 8, 10
    f = factors(torch, layout, dev, m, ROWS, k, seed=1)
    q = torch.arange(nq, dtype=torch.int32, device=dev)
    tv = torch.full((nq, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((nq, N), 7, dtype=torch.int32, device=dev)
    tc = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    sp = torch.zeros(ROWS + 1, dtype=torch.int64, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())          # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(k=k, ld=f["ld"], nq=nq, m=m, topn=N, nslices=0, out=(tv, ti, tc), ws=None, wsb=0, bias=f["b_i"],
             seen=(None, None)):
        return lib.als_audience_topk(k, ld, nq, p(q), p(f["Z"]), p(bias), m, p(f["U"]), p(f["b_u"]), p(f["mu"]),
                                     p(seen[0]), p(seen[1]), None, topn, nslices, p(out[0]), p(out[1]), p(out[2]),
                                     p(ws), wsb, stream)
    E_BADARG, E_BADK = -1, -2
    assert call(k=0) == E_BADK and call(k=161) == E_BADK
    assert call(ld=16) == E_BADARG
    assert call(topn=0) == E_BADARG and call(topn=129) == E_BADARG
    assert call(nslices=-1) == E_BADARG and call(nslices=65) == E_BADARG
    assert call(m=0) == E_BADARG and call(m=2 ** 31) == E_BADARG
    assert call(out=(None, ti, tc)) == E_BADARG and call(out=(tv, ti, None)) == E_BADARG and call(bias=None) == E_BADARG
    assert call(seen=(sp, None)) == E_BADARG                               # one of the two pointers
    need = lib.als_audience_workspace_bytes(nq, m, N, 4)
    assert need == 4 * nq * N * 8
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert call(nslices=4) == E_BADARG and call(nslices=4, ws=ws, wsb=need - 1) == E_BADARG
    assert call(nq=0) == 0                                                 # no-op
    torch.cuda.synchronize()
    assert (tv == 7.0).all() and (ti == 7).all() and (tc == 7).all()       # nothing was launched
    assert call(nslices=4, ws=ws, wsb=need) == 0
    torch.cuda.synchronize()
    assert (tc == N).all()
