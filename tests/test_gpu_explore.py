"""K16 (GPU): als_row_whitener / als_explore_topk (csrc/explore.hip) and ALS.recommend_explore.

What the contract states exactly is compared with ==: the zero pattern of W, beta = 0 against
als_recommend_topk_masked, top_val against float32 arithmetic on the kernel's own top_lev and the row
als_predict_dense writes, slice independence, repeated rows, candidates, counts, order.  The leverages and keys are held
to the bounds DERIVED in tests/explore_ref.py (tau_lev, tau_s, whitener_residual_bound) against the fp64 reference - for
every returned entry of every case, and completeness for every candidate left out.  The largest observed error / bound
ratios are collected in MARGINS and written to the file ALS_RECORD_MARGINS names, when it is set."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import explore_ref as xref
from tests import serving_ref as ref
from tests.gpu_common import (assert_same, csr_rows, env, factors, predict_dense, ratio, record_margins, run_topk,
                              same_bits, upload)
from tests.synth import make_features, make_ratings

BETAS = (-1.0, 0.0, 0.5, 2.0)
TOPS = (1, 10, 32, 33, 128)
LAMS = (5.0, 1e-2)
SLICES = (2, 7, 64)
N_BATCH = 40
MARGINS = {"lev": 0.0, "key": 0.0, "whitener": 0.0}


@contextlib.contextmanager
def slices(s):
    old = os.environ.get("ALS_RECOMMEND_SLICES")
    os.environ["ALS_RECOMMEND_SLICES"] = str(s)
    try:
        yield
    finally:
        if old is None:
            del os.environ["ALS_RECOMMEND_SLICES"]
        else:
            os.environ["ALS_RECOMMEND_SLICES"] = old


def _note(name, value):
    MARGINS[name] = max(MARGINS[name], value)


def row_lengths(k, n):
    """Rows of 0, 1, k/2, k, 300 and 4500 ratings (what n allows of them: a longer row rates everything), 7 and 40."""
    return [min(L, n) for L in (0, 1, k // 2, k, 300, 4500, 7, 40)]


def run_whitener(torch, be, f, csr_d, rows, n, lam, nrows):
    """als_row_whitener into a buffer that starts from 7 -> (device W [nrows, ld, ld], status)."""
    dev = f["Z"].device
    W = torch.full((nrows, f["ld"], f["ld"]), 7.0, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    be.row_whitener(k=f["k"], ld=f["ld"], indptr=csr_d[0], indices=csr_d[1], rows=rows, n=n, Z=f["Z"], lam_u=lam,
                    W_out=W, status=status)
    return W, int(status.item())


def run_explore(torch, be, f, users_d, n, W, beta, seen_d, N, allow, nsl=1):
    """als_explore_topk with `nsl` slices, into buffers that start from 7 -> numpy (keys, items, counts, leverages)."""
    dev = f["Z"].device
    B = users_d.numel()
    tv = torch.full((B, N), 7.0, dtype=torch.float32, device=dev)
    tl = torch.full((B, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((B, N), 7, dtype=torch.int32, device=dev)
    tc = torch.full((B,), 7, dtype=torch.int32, device=dev)
    with slices(nsl):
        be.explore_topk(k=f["k"], ld=f["ld"], users=users_d, n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"],
                        mu=f["mu"], W=W, beta=beta, seen_ptr=seen_d[0], seen_idx=seen_d[1], allow=allow, topn=N,
                        top_val=tv, top_idx=ti, top_cnt=tc, top_lev=tl)
    return tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy(), tl.cpu().numpy()


def _bitmap(torch, mask, dev):
    return torch.from_numpy(ref.bitmap_numpy(mask).view(np.int32).copy()).to(dev)


def problem(torch, layout, dev, k, n, seed):
    """Eight users with the rows of `row_lengths` as training / seen CSR, factors of unit scale, two NaN item biases
    (a NaN base), and a batch of N_BATCH rows that repeats every user."""
    m = 8
    f = factors(torch, layout, dev, m, n, k, seed)
    if n >= 17:
        f["b_i"][[3, n // 2]] = float("nan")
    ptr, idx, _ = csr_rows(row_lengths(k, n), n, seed + 1)
    users = np.random.default_rng(seed + 2).permutation(np.arange(N_BATCH) % m).astype(np.int32)
    csr_d = (upload(ptr, dev), upload(idx if idx.size else np.zeros(1, np.int32), dev))
    return f, ptr, idx, users, csr_d


def check_lists(got, users, dense, seen, allowed, refs, beta, N):
    """Every check of the module docstring on one call's outputs; refs[u] = explore_keys of user u."""
    tv, ti, tc, tl = got
    n = dense.shape[1]
    first = {}
    for b, u in enumerate(users):
        cand = ref.candidates(dense[u], seen[u], allowed)
        c = int(tc[b])
        assert c == min(N, int(cand.sum()))
        assert (ti[b, c:] == -1).all() and np.isneginf(tv[b, c:]).all() and (tl[b, c:] == 0).all()
        ids = ti[b, :c].astype(np.int64)
        assert np.unique(ids).size == c and (ids >= 0).all() and (ids < n).all() and cand[ids].all()
        keys = tv[b, :c]
        assert (keys == xref.key_f32(dense[u, ids], beta, tl[b, :c])).all()
        assert ((keys[:-1] > keys[1:]) | ((keys[:-1] == keys[1:]) & (ids[:-1] < ids[1:]))).all()
        r = refs[u]
        _note("lev", ratio(tl[b, :c], r["lev"][ids], r["tau_lev"][ids], "leverage"))
        _note("key", ratio(keys, r["key"][ids], r["tau_s"][ids], "key"))
        assert (np.abs(tl[b, :c].astype(np.float64) - r["lev"][ids]) <= r["tau_lev"][ids]).all()
        assert (np.abs(keys.astype(np.float64) - r["key"][ids]) <= r["tau_s"][ids]).all()
        if c == N:                                                          # completeness
            out = cand.copy()
            out[ids] = False
            last = ids[-1]
            assert (r["key"][out] - r["tau_s"][out] <= float(keys[-1]) + r["tau_s"][last]).all()
        if u in first:                                                      # repeated batch rows
            a = first[u]
            assert same_bits(tv[a], tv[b]) and same_bits(ti[a], ti[b]) and same_bits(tl[a], tl[b]) and tc[a] == tc[b]
        first.setdefault(u, b)


def explore_case(k, n, seed, case):
    torch, layout, be, dev = env().short
    f, ptr, idx, users, csr_d = problem(torch, layout, dev, k, n, seed)
    m = ptr.size - 1
    Zh = f["Z"].cpu().numpy()
    dense = predict_dense(torch, be, f, m, n, dev)
    seen = [idx[ptr[u]: ptr[u + 1]].astype(np.int64) for u in range(m)]
    users_d = upload(users, dev)
    mask = np.random.default_rng(seed + 3).random(n) < 0.7
    allow_d = _bitmap(torch, mask, dev)
    pair = 0
    for lam in LAMS:
        W, status = run_whitener(torch, be, f, csr_d, users_d, n, lam, users.size)
        assert status == 0
        lam64 = float(np.float32(lam)) + ref.EPS
        winv = [xref.whitener(Zh, seen[u], lam64, k)[0] for u in range(m)]
        for beta in BETAS:
            N = TOPS[(pair + case) % len(TOPS)]
            allowed, allow = (mask, allow_d) if (pair + pair // 4) % 2 else (None, None)    # beta = 0: both ways
            pair += 1
            refs = [xref.explore_keys(dense[u], Zh, winv[u], beta, k) for u in range(m)]
            got = run_explore(torch, be, f, users_d, n, W, beta, csr_d, N, allow)
            check_lists(got, users, dense, seen, allowed, refs, beta, N)
            for s in SLICES:
                other = run_explore(torch, be, f, users_d, n, W, beta, csr_d, N, allow, nsl=s)
                assert all(same_bits(a, b) for a, b in zip(got, other)), s
            if beta == 0.0:
                full = allow if allow is not None else _bitmap(torch, np.ones(n, bool), dev)
                assert_same(got[:3], run_topk(torch, be, f, users, n, ptr, idx, N, dev, full))
        none = run_explore(torch, be, f, users_d, n, W, 1.0, csr_d, 10, _bitmap(torch, np.zeros(n, bool), dev))
        assert (none[2] == 0).all() and (none[1] == -1).all() and np.isneginf(none[0]).all() and (none[3] == 0).all()


# ------------------------------------------------------------------------------------------------ the whitener
@pytest.mark.parametrize("k", [1, 16, 17, 64, 65, 128, 160])
def test_whitener_zero_pattern_residual_and_empty_row(k):
    torch, layout, be, dev = env().short
    n = 5000
    f = factors(torch, layout, dev, 1, n, k, seed=900 + k)
    lens = [0, 1, k // 2, k, 300, 4500]
    ptr, idx, _ = csr_rows(lens, n, seed=901 + k)
    csr_d = (upload(ptr, dev), upload(idx, dev))
    Zh = f["Z"].cpu().numpy()
    ld = f["ld"]
    rows = np.array([5, 0, 3, 3, 1, 2, 4, 0, 5], np.int32)
    low = np.tril(np.ones((ld, ld), bool))
    low[k:, :] = False
    for lam in LAMS:
        W, status = run_whitener(torch, be, f, csr_d, None, n, lam, len(lens))
        assert status == 0
        W = W.cpu().numpy()
        assert (W[:, ~low] == 0).all()                                      # upper triangle, padding rows / columns
        lam64 = float(np.float32(lam)) + ref.EPS
        assert (W[0, :k, :k] == (np.eye(k) / np.sqrt(lam64)).astype(np.float32)).all()      # the empty row
        for r in range(len(lens)):
            Winv, A, L = xref.whitener(Zh, idx[ptr[r]: ptr[r + 1]], lam64, k)
            W64 = W[r, :k, :k].astype(np.float64)
            res = np.abs(W64 @ A @ W64.T - np.eye(k)).max()
            bound = xref.whitener_residual_bound(A, L, Winv)
            _note("whitener", res / bound)
            assert res <= bound, (r, lam, res, bound)
            assert (np.abs(W64 - Winv) <= 2.0 ** -24 * np.abs(Winv) + 64 * k * 2.0 ** -53 * np.linalg.cond(A)
                    * np.abs(Winv).max()).all()
        Wr, status = run_whitener(torch, be, f, csr_d, upload(rows, dev), n, lam, rows.size)
        assert status == 0 and same_bits(Wr.cpu().numpy(), W[rows])        # a row's W depends on the row alone


# ------------------------------------------------------------------------------------------------ shape sweep
@pytest.mark.parametrize("k", [1, 16, 17, 64, 65, 128, 160])
@pytest.mark.parametrize("n", [1, 17, 1000, 4099])
def test_explore_topk_contract(k, n):
    explore_case(k, n, seed=20 * k + n, case=k + n)


def test_explore_topk_with_a_row_of_4500_ratings():
    explore_case(64, 5000, seed=77, case=0)


def test_bad_arguments_are_refused():
    torch, layout, be, dev = env().short
    f, ptr, idx, users, csr_d = problem(torch, layout, dev, 16, 100, 5)
    users_d = upload(users, dev)
    W, _ = run_whitener(torch, be, f, csr_d, users_d, 100, 1.0, users.size)
    for beta in (float("nan"), float("inf")):
        with pytest.raises(RuntimeError):
            run_explore(torch, be, f, users_d, 100, W, beta, csr_d, 5, None)


# ------------------------------------------------------------------------------------------------ the model
@pytest.fixture(scope="module")
def fitted():
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig
    env()
    m, n, k = 120, 150, 24
    r, c, v = make_ratings(m, n, 3000, seed=11, empty_users=(5,))
    G, y = make_features(n, seed=12)
    feats = {"genres": G, "years": y}
    cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=3, lambda_u=3.0, lambda_v=4.0),
                    biases=BiasesConfig(lambda_bu=2.0, lambda_bi=2.0))
    model = ALS(cfg, device="cuda:0", lambda_w={"genres": 1.0, "years": 1.0})
    model.fit_coo(r, c, v, (m, n), features=feats, tol=None, verbose=0)
    return model, feats, (m, n, k)


def _kernel_level(torch, eng, Z, users_d, U, b_u, wr, seen, beta, N, allow=None):
    """als_row_whitener + als_explore_topk on the engine's own tables -> host (items, keys, leverage, device W)."""
    B = users_d.numel()
    W = torch.empty(B, eng.ld, eng.ld, dtype=torch.float32, device=eng.dev)
    status = torch.zeros(1, dtype=torch.int32, device=eng.dev)
    eng.be.row_whitener(k=eng.k, ld=eng.ld, indptr=wr[0], indices=wr[1], rows=wr[2], n=eng.n, Z=Z,
                        lam_u=eng.model.lambda_u, W_out=W, status=status)
    assert int(status.item()) == 0
    tv = torch.empty(B, N, dtype=torch.float32, device=eng.dev)
    tl = torch.empty(B, N, dtype=torch.float32, device=eng.dev)
    ti = torch.empty(B, N, dtype=torch.int32, device=eng.dev)
    tc = torch.empty(B, dtype=torch.int32, device=eng.dev)
    eng.be.explore_topk(k=eng.k, ld=eng.ld, users=users_d, n=eng.n, U=U, Z=Z, b_u=b_u, b_i=eng.b_i, mu=eng.mu, W=W,
                        beta=beta, seen_ptr=seen[0], seen_idx=seen[1], allow=allow, topn=N, top_val=tv, top_idx=ti,
                        top_cnt=tc, top_lev=tl)
    return (ti.cpu().numpy().astype(np.int64), tv.cpu().numpy().astype(np.float64),
            tl.cpu().numpy().astype(np.float64), W)


@pytest.mark.parametrize("use_features", [False, True])
def test_model_calls_are_the_kernel_calls(fitted, use_features, monkeypatch):
    import torch
    model, feats, (m, n, k) = fitted
    features = feats if use_features else None
    eng = model._eng
    users = np.array([7, 5, 0, 7, 119, 33, 5, 64, 2, 90, 91], np.int32)
    with torch.cuda.device(eng.dev):
        Z = eng._compose_for(model._check_predict(features))
        users_d = upload(users, eng.dev)
        csr = (eng.csr.indptr, eng.csr.indices)
        for beta, N in ((1.0, 10), (-0.5, 33), (0.0, 7)):
            exp = _kernel_level(torch, eng, Z, users_d, eng.U, eng.b_u, (*csr, users_d), csr, beta, N)
            monkeypatch.setattr(eng, "EXPLORE_BATCH", 4, raising=False)        # three chunks
            got = model.recommend_explore(users, N, beta=beta, features=features, return_leverage=True)
            assert_same(got, exp[:3])
        assert_same(model.recommend_explore(users, 7, beta=0.0, features=features),
                    model.recommend(users, 7, features=features))
        # rows outside the fit: the folded table, the rows themselves as work rows and as seen rows
        lens = [0, 1, 12, 24, 100, 3]
        ptr, idx, vals = csr_rows(lens, n, seed=13)
        U, b, ptr_d, idx_d = eng._fold_in_dev(ptr, idx, vals, Z, 0)
        rows_d = torch.arange(len(lens), dtype=torch.int32, device=eng.dev)
        exp = _kernel_level(torch, eng, Z, rows_d, U, b, (ptr_d, idx_d, None), (ptr_d, idx_d), 2.0, 10)
        got = model.recommend_new_explore((ptr, idx, vals), 10, beta=2.0, features=features, return_leverage=True)
        assert_same(got, exp[:3])
        assert_same(model.recommend_new_explore((ptr, idx, vals), 10, beta=0.0, features=features),
                    model.recommend_new((ptr, idx, vals), 10, features=features))


def test_thompson_is_recommend_on_the_sampled_table(fitted):
    import torch
    model, feats, (m, n, k) = fitted
    eng = model._eng
    users = np.array([7, 5, 0, 7, 119, 33], np.int32)
    beta, seed, N = 0.7, 21, 10
    with torch.cuda.device(eng.dev):
        Z = eng._compose_for(model._check_predict(None))
        users_d = upload(users, eng.dev)
        csr = (eng.csr.indptr, eng.csr.indices)
        W = _kernel_level(torch, eng, Z, users_d, eng.U, eng.b_u, (*csr, users_d), csr, 0.0, 1)[3]
        eps = np.zeros((users.size, eng.ld), np.float32)
        eps[:, :k] = np.random.default_rng(seed).standard_normal((users.size, k)).astype(np.float32)
        us = users_d.to(torch.int64)
        Ut = (eng.U[us] + beta * torch.bmm(W.transpose(1, 2), upload(eps, eng.dev).unsqueeze(2)).squeeze(2)).contiguous()
        f = dict(k=eng.k, ld=eng.ld, U=Ut, Z=Z, b_u=eng.b_u[us].contiguous(), b_i=eng.b_i, mu=eng.mu)
        sp = eng.csr.indptr.cpu().numpy()
        si = eng.csr.indices.cpu().numpy()
        rows = [si[sp[u]: sp[u + 1]] for u in users]
        bptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
        tv, ti, tc = run_topk(torch, eng.be, f, np.arange(users.size), n, bptr, np.concatenate(rows).astype(np.int32),
                              N, eng.dev)
        got = model.recommend_explore(users, N, beta=beta, mode="thompson", seed=seed)
        assert_same(got, (ti.astype(np.int64), tv.astype(np.float64)))
        again = model.recommend_explore(users, N, beta=beta, mode="thompson", seed=seed)
        assert_same(got, again)


def test_leverage_is_explains_to_the_bound(fitted):
    import torch
    model, feats, (m, n, k) = fitted
    users = np.array([7, 5, 0, 119, 33, 64], np.int32)
    items, _, lev = model.recommend_explore(users, 10, beta=1.0, return_leverage=True)
    e = model.explain(np.repeat(users, 10), items.reshape(-1), 3)
    eng = model._eng
    Zh = eng._compose_for(model._check_predict(None)).cpu().numpy()
    sp, si = eng.csr.indptr.cpu().numpy(), eng.csr.indices.cpu().numpy()
    lam64 = float(np.float32(model.lambda_u)) + ref.EPS
    for r, u in enumerate(users):
        Winv = xref.whitener(Zh, si[sp[u]: sp[u + 1]], lam64, k)[0]
        ek = xref.explore_keys(np.zeros(n, np.float32), Zh, Winv, 1.0, k)
        ex = e.leverage[10 * r: 10 * r + 10]
        assert (np.abs(ex - ek["lev"][items[r]]) <= 1e-9 * ek["lev"][items[r]]).all()     # explain: fp64
        assert (np.abs(lev[r] - ex) <= ek["tau_lev"][items[r]] + 1e-9 * ex).all()


def test_zz_record_margins():
    """Runs last in the module: the largest error / bound ratios of the cases above (all below 1, or they failed)."""
    assert all(v <= 1.0 for v in MARGINS.values()), MARGINS
    record_margins("explore", MARGINS)
