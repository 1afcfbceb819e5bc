"""K9b (GPU): fold-in of items outside the fit (csrc/fold_in_items.hip, als_fold_in_items), the new items' graph
rows, ALS.fold_in_items / predict_new_items / recommend(new_items=...) and cv.cold_item_rmse.

The kernel is checked against the float64 contract in tests/serving_ref.py (`fold_in_item`) on the same fp32 U, b_u,
V, graph weights, mu and lambda values: the expected error is the fp32 rounding of the outputs.  Graph rows,
predictions and recommendations are checked exactly (==) against the device's own fp32 cosines and predict-epilogue
scores."""
import ctypes as C

import numpy as np
import pytest

from tests import serving_ref
from tests.gpu_common import csr_rows, env, record_margins, upload

pytestmark = pytest.mark.gpu


def _oracle(U, b_u, mu, V, lam_v, pop_reg, lam_bi, alpha, indptr, indices, vals, S, k, T):
    """`fold_in_item` of tests/serving_ref.py on every CSR row (S: the rows' graph CSR or None), the parameters rounded
    to fp32 as the kernel reads them."""
    f = lambda x: float(np.float32(x))              # noqa: E731
    B = indptr.size - 1
    Vo, bo = np.zeros((B, k)), np.zeros(B)
    for r in range(B):
        sl = slice(indptr[r], indptr[r + 1])
        sj = S[1][S[0][r]: S[0][r + 1]] if S is not None else np.zeros(0, np.int64)
        sv = S[2][S[0][r]: S[0][r + 1]] if S is not None else np.zeros(0)
        Vo[r], bo[r] = serving_ref.fold_in_item(U, b_u, mu, V[:, :k], indices[sl], vals[sl], sj, sv, f(lam_v), pop_reg,
                                                f(lam_bi), f(alpha), T)
    return Vo, bo


def _tables(layout, m, n, k, seed):
    ld = layout.padded_k(k)
    rng = np.random.default_rng(seed)
    U = np.zeros((m, ld), np.float32)
    U[:, :k] = rng.normal(scale=0.5, size=(m, k))
    V = np.zeros((n, ld), np.float32)
    V[:, :k] = rng.normal(scale=0.5, size=(n, k))
    bu = rng.normal(scale=0.3, size=m).astype(np.float32)
    return ld, U, V, bu


def _run(torch, be, dev, k, ld, U, bu, V, ratings, S, lam_v, pop_reg, lam_bi, alpha, T):
    indptr, indices, vals = ratings
    B = indptr.size - 1
    d = lambda a: upload(a, dev)                                         # noqa: E731
    nz = lambda a, dt: a if a.size else np.zeros(1, dt)                  # noqa: E731
    Vout = torch.full((B, ld), float("nan"), dtype=torch.float32, device=dev)
    b = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    Sd = None if S is None else (d(S[0]), d(nz(S[1], np.int32)), d(nz(S[2], np.float32)))
    be.fold_in_items(k=k, ld=ld, indptr=d(indptr), indices=d(nz(indices, np.int32)), vals=d(nz(vals, np.float32)),
                     m=U.shape[0], U=d(U), b_u=d(bu), mu=torch.tensor([3.5], dtype=torch.float64, device=dev), S=Sd,
                     n=V.shape[0], V=d(V), lam_v=lam_v, pop_reg=pop_reg, lam_bi=lam_bi, alpha=alpha, n_sweeps=T,
                     V_out=Vout, b_i_out=b, status=status)
    torch.cuda.synchronize()
    return Vout.cpu().numpy(), b.cpu().numpy(), int(status.item())


# relative to max(1, max |v|) per row
TOL = 5e-7
RATERS = lambda k: [0, 1, max(k // 2, 1), k, 300, 4500]       # noqa: E731
NEIGHBOURS = [0, 1, 50, 128]


@pytest.mark.parametrize("k", [1, 8, 16, 33, 50, 64, 80, 128, 150, 160])
@pytest.mark.parametrize("pop_reg,alpha", [(False, 0.5), (True, 0.5), (False, 0.0)])
def test_kernel_against_float64_oracle(k, pop_reg, alpha):
    torch, layout, be, dev = env().short
    m, n = 4600, 3000
    ld, U, V, bu = _tables(layout, m, n, k, seed=k)
    lengths = [L for L in RATERS(k) for _ in NEIGHBOURS]
    ratings = csr_rows(lengths, m, seed=k + 1)
    S = csr_rows(NEIGHBOURS * len(RATERS(k)), n, seed=k + 2, weights=True)
    worst = []
    for T in (1, 3, 0):
        Vg, bg, st = _run(torch, be, dev, k, ld, U, bu, V, ratings, S, 4.0, pop_reg, 2.0, alpha, T)
        assert st == 0
        Vo, bo = _oracle(U, bu, 3.5, V, 4.0, pop_reg, 2.0, alpha, *ratings, S, k, T)
        assert (Vg[:, k:] == 0).all()
        scale = np.maximum(1.0, np.abs(Vo).max(axis=1))
        err_v = (np.abs(Vg[:, :k] - Vo).max(axis=1) / scale).max()
        err_b = (np.abs(bg - bo) / np.maximum(1.0, np.abs(bo))).max()
        worst.append((T, err_v, err_b))
        assert err_v < TOL and err_b < TOL, (T, err_v, err_b)
        assert (bg[: len(NEIGHBOURS)] == 0).all()                 # rows without ratings: b = 0
        if alpha == 0.0:
            assert (Vg[0] == 0).all()                              # no ratings, no graph: v = 0
    print(f"k={k} pop_reg={pop_reg} alpha={alpha} (T, err_v, err_b): {worst}")
    record_margins(f"fold_in_items[k={k},pop_reg={pop_reg},alpha={alpha}]",
                   {"v": float(max(w[1] for w in worst)), "b": float(max(w[2] for w in worst))})


def test_no_graph_equals_an_empty_graph():
    torch, layout, be, dev = env().short
    m, n, k = 500, 200, 32
    ld, U, V, bu = _tables(layout, m, n, k, seed=3)
    ratings = csr_rows([0, 5, 40, 200], m, seed=4)
    empty = (np.zeros(5, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32))
    a = _run(torch, be, dev, k, ld, U, bu, V, ratings, None, 2.0, False, 1.0, 0.5, 0)
    b = _run(torch, be, dev, k, ld, U, bu, V, ratings, empty, 2.0, False, 1.0, 0.5, 0)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


def test_nan_in_U_sets_the_status_word():
    torch, layout, be, dev = env().short
    m, n, k = 300, 100, 16
    ld, U, V, bu = _tables(layout, m, n, k, seed=7)
    U[17, 3] = np.nan
    ratings = (np.array([0, 2, 4, 5], np.int64), np.array([1, 2, 5, 17, 4], np.int32), np.ones(5, np.float32))
    _, _, st = _run(torch, be, dev, k, ld, U, bu, V, ratings, None, 1.0, False, 1.0, 0.0, 0)
    assert st == 2                                        # row 1 holds user 17


def test_c_abi_status_codes():
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    p = _hip.FoldInItemsParams()
    p.k, p.ld, p.nrows, p.m, p.n = 161, 176, 1, 10, 10
    assert lib.als_fold_in_items(C.byref(p), None) == -2              # ALS_E_BADK
    p.k, p.ld, p.nrows = 16, 16, 0
    assert lib.als_fold_in_items(C.byref(p), None) == 0               # nrows = 0: no-op, pointers unused
    p.nrows = 3
    assert lib.als_fold_in_items(C.byref(p), None) == -1              # NULL pointers: ALS_E_BADARG
    p.nrows, p.ld = 0, 32
    assert lib.als_fold_in_items(C.byref(p), None) == -1              # ld != als_padded_k(k)
    p.ld, p.n_sweeps = 16, -1
    assert lib.als_fold_in_items(C.byref(p), None) == -1
    p.n_sweeps, p.alpha = 0, -1.0
    assert lib.als_fold_in_items(C.byref(p), None) == -1
    p.alpha, p.pop_reg = 0.0, 2
    assert lib.als_fold_in_items(C.byref(p), None) == -1
    p.pop_reg, p.m = 0, 0
    assert lib.als_fold_in_items(C.byref(p), None) == -1
    # a partial graph (S_ptr without S_idx / S_val) is refused
    buf = torch.zeros(64, dtype=torch.int64, device=dev)
    p.m, p.nrows = 10, 1
    for f in ("indptr", "indices", "vals", "U", "b_u", "mu", "V_out", "b_i_out", "status", "S_ptr", "V"):
        setattr(p, f, buf.data_ptr())
    assert lib.als_fold_in_items(C.byref(p), None) == -1


# ---------------------------------------------------------------------------------------------- model level
M, N_ALL, N_FIT, K = 400, 300, 260, 24


@pytest.fixture(scope="module")
def fitted():
    from collaborative_filtering_amd import (ALS, ALSConfig, BiasesConfig, CoreConfig, GraphConfig,
                                             GraphSimConfig)
    from tests.synth import make_features, make_ratings
    r, c, v = make_ratings(M, N_ALL, 14000, seed=11)
    G, y = make_features(N_ALL, seed=12)
    held = c >= N_FIT                                   # the last 40 items: outside the fit entirely
    feats_fit = {"genres": G[:N_FIT], "year": y[:N_FIT]}
    feats_new = {"genres": G[N_FIT:], "year": y[N_FIT:]}
    cfg = ALSConfig(core=CoreConfig(n_factors=K, n_iters=4, lambda_u=3.0, lambda_v=4.0,
                                    pop_reg_mode="inverse_sqrt"),
                    biases=BiasesConfig(lambda_bu=2.0, lambda_bi=2.0),
                    graph=GraphConfig(alpha=0.5, sim=GraphSimConfig(topk=10)))
    model = ALS(cfg, {"genres": 1.0, "year": 1.0}, device="cuda:0")
    model.fit_coo(r[~held], c[~held], v[~held], (M, N_FIT), features=feats_fit, tol=None, verbose=0)
    C = np.full((N_ALL - N_FIT, M), np.nan)                 # the held-out items' ratings, by item
    C[c[held] - N_FIT, r[held]] = v[held]
    return dict(model=model, feats_fit=feats_fit, feats_new=feats_new, C=C, train=(r[~held], c[~held]))


def _few(C, per_item, seed):
    """At most `per_item` ratings of every held-out item (the rest NaN)."""
    rng = np.random.default_rng(seed)
    out = np.full_like(C, np.nan)
    for b in range(C.shape[0]):
        rated = np.nonzero(~np.isnan(C[b]))[0]
        keep = rng.permutation(rated)[:per_item]
        out[b, keep] = C[b, keep]
    return out


def _device_cosines(fx):
    """The device's own fp32 cosines of the new items against the fitted ones (the predict kernel on the
    normalised sim feature, zero biases, mu = 0: bitwise the scores als_recommend_topk ranks)."""
    import torch
    from collaborative_filtering_amd import layout
    model = fx["model"]
    eng = model._eng
    Xn_new = layout.normalize_rows_f32(fx["feats_new"]["genres"], model.S_eps, eng.dev)
    Xn_fit = layout.normalize_rows_f32(fx["feats_fit"]["genres"], model.S_eps, eng.dev)
    d = Xn_new.shape[1]
    ldd = layout.padded_k(d)
    pad = lambda X: torch.nn.functional.pad(X, (0, ldd - d)).contiguous()     # noqa: E731
    B, n = Xn_new.shape[0], Xn_fit.shape[0]
    P = torch.empty(B, n, dtype=torch.float32, device=eng.dev)
    eng.be.predict_dense(k=d, ld=ldd, m=B, n=n, U=pad(Xn_new), Z=pad(Xn_fit),
                         b_u=torch.zeros(B, device=eng.dev), b_i=torch.zeros(n, device=eng.dev),
                         mu=torch.zeros(1, dtype=torch.float64, device=eng.dev), out=P)
    return P.cpu().numpy()


def test_graph_rows_are_the_masked_sort_of_the_device_cosines(fitted):
    fx = fitted
    model = fx["model"]
    folded = model.fold_in_items(features_new=fx["feats_new"])
    ptr, idx, val = folded.graph
    P = _device_cosines(fx)
    topk = model.S_topk
    for b in range(P.shape[0]):
        o = np.lexsort((np.arange(P.shape[1]), -P[b]))[:topk]
        o = o[P[b, o] > 0]
        assert idx[ptr[b]: ptr[b + 1]].tolist() == o.tolist(), b
        assert (val[ptr[b]: ptr[b + 1]] == P[b, o]).all(), b
    # and float64 cosines to fp32 rounding
    G64n = lambda X: X / (np.sqrt((X * X).sum(1, keepdims=True)) + model.S_eps)     # noqa: E731
    S64 = G64n(fx["feats_new"]["genres"].astype(np.float64)) @ G64n(fx["feats_fit"]["genres"].astype(np.float64)).T
    rows = np.repeat(np.arange(P.shape[0]), np.diff(ptr))
    assert np.abs(val - S64[rows, idx]).max() < 1e-6
    assert ptr[-1] > 0


@pytest.mark.parametrize("few", [None, 3])
@pytest.mark.parametrize("T", [None, 2])
def test_fold_in_items_against_the_oracle(fitted, few, T):
    fx = fitted
    model = fx["model"]
    eng = model._eng
    C = None if few is None else _few(fx["C"], few, seed=5)
    folded = model.fold_in_items(C, features_new=fx["feats_new"], n_sweeps=T)
    B = N_ALL - N_FIT
    assert folded.V.shape == folded.Z.shape == (B, K) and folded.b_i.shape == (B,) and folded.V.dtype == np.float64
    ip, ix, vv = folded.ratings
    assert ip.size == B + 1 and ip[-1] == (0 if C is None else int((~np.isnan(C)).sum()))
    U = eng.U[:M].cpu().numpy()
    V = eng.V[:N_FIT].cpu().numpy()
    Vo, bo = _oracle(U, eng.b_u[:M].cpu().numpy(), float(eng.mu.item()), V, model.lambda_v, True,
                     model.lambda_bi, model.alpha, ip, ix, vv, folded.graph, K, T or 0)
    assert np.abs(folded.V - Vo).max() < 1e-5 * max(1.0, np.abs(Vo).max())
    assert np.abs(folded.b_i - bo).max() < 1e-5 * max(1.0, np.abs(bo).max())
    if C is None:
        assert (folded.b_i == 0).all()
    Zo = folded.V + sum(fx["feats_new"][f] @ model.W[f] for f in ("genres", "year"))
    assert np.abs(folded.Z - Zo).max() < 1e-5 * max(1.0, np.abs(Zo).max())
    # the feature part lifts the cold items: Z differs from V
    assert not np.array_equal(folded.Z, folded.V)


def test_bitwise_invariance(fitted, monkeypatch):
    fx = fitted
    model = fx["model"]
    fn = fx["feats_new"]
    C = _few(fx["C"], 6, seed=9)
    ref = model.fold_in_items(C, features_new=fn)
    same = lambda a, rows=None: (all((getattr(a, f) == (getattr(ref, f) if rows is None else getattr(ref, f)[rows])).all()
                                     for f in ("V", "b_i", "Z")))           # noqa: E731
    perm = np.random.default_rng(0).permutation(C.shape[0])
    p = model.fold_in_items(C[perm], features_new={f: X[perm] for f, X in fn.items()})
    assert same(p, perm)
    a = model.fold_in_items(C[:13], features_new={f: X[:13] for f, X in fn.items()})
    b = model.fold_in_items(C[13:], features_new={f: X[13:] for f, X in fn.items()})
    for f in ("V", "b_i", "Z"):
        assert (np.concatenate([getattr(a, f), getattr(b, f)]) == getattr(ref, f)).all()
    dup = model.fold_in_items(np.vstack([C, C]), features_new={f: np.vstack([X, X]) for f, X in fn.items()})
    for f in ("V", "b_i", "Z"):
        assert (getattr(dup, f) == np.concatenate([getattr(ref, f)] * 2)).all()
    rp, rx, rv = ref.ratings
    rng = np.random.default_rng(1)
    rx2, rv2 = rx.copy(), rv.copy()
    for r in range(C.shape[0]):                             # columns shuffled within every row
        s = slice(rp[r], rp[r + 1])
        o = rng.permutation(rp[r + 1] - rp[r])
        rx2[s], rv2[s] = rx[s][o], rv[s][o]
    sh = model.fold_in_items((rp, rx2, rv2), features_new=fn)
    assert same(sh)
    for nsl in ("1", "2", "5"):                            # graph rows do not depend on the recommend slice count
        monkeypatch.setenv("ALS_RECOMMEND_SLICES", nsl)
        g = model.fold_in_items(C, features_new=fn)
        assert same(g) and all((x == y).all() for x, y in zip(g.graph, ref.graph))
    monkeypatch.delenv("ALS_RECOMMEND_SLICES")
    # the supplied graph rows are the computed ones
    s = model.fold_in_items(C, features_new=fn, S_new=ref.graph)
    assert same(s)


def test_predict_new_items_is_the_predict_epilogue(fitted):
    from collaborative_filtering_amd import FoldedItems
    fx = fitted
    model = fx["model"]
    fn = fx["feats_new"]
    folded = model.fold_in_items(_few(fx["C"], 4, seed=2), features_new=fn)
    P = model.predict_new_items(folded)
    assert P.shape == (M, N_ALL - N_FIT) and P.dtype == np.float64
    users = np.array([5, 0, 399, 5, 17])
    assert (model.predict_new_items(folded, users) == P[users]).all()
    # host-composed fp32 epilogue ((U.Z + mu) + b_u) + b_i (the dot product to fp32 rounding)
    U32, Z32 = model.U.astype(np.float32), folded.Z.astype(np.float32)
    dot = (U32.astype(np.float64) @ Z32.T.astype(np.float64)).astype(np.float32)
    host = ((dot + np.float32(model.mu)) + model.b_u.astype(np.float32)[:, None]) + folded.b_i.astype(np.float32)
    assert np.abs(P - host).max() < 1e-5 * max(1.0, np.abs(host).max())
    # exactly: folded items that carry fitted items' Z and b_i score bitwise as predict() does on those items
    items = np.array([3, 0, 259, 3, 100])
    Zfit = model.V + sum(fx["feats_fit"][f] @ model.W[f] for f in ("genres", "year"))
    Zdev = model._eng._compose_for(fx["feats_fit"])[:N_FIT, :K].cpu().numpy().astype(np.float64)
    assert np.abs(Zdev - Zfit).max() < 1e-5
    fake = FoldedItems(V=Zdev[items], b_i=model.b_i[items], Z=Zdev[items], graph=None,
                       ratings=(np.zeros(items.size + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)))
    assert (model.predict_new_items(fake) == model.predict(fx["feats_fit"])[:, items]).all()
    assert model.predict_new_items(folded, np.zeros(0, np.int64)).shape == (0, N_ALL - N_FIT)
    with pytest.raises(IndexError):
        model.predict_new_items(folded, [M])


@pytest.mark.parametrize("N", [1, 10, 128])
@pytest.mark.parametrize("exclude_seen", [True, False])
def test_recommend_with_new_items_against_the_masked_dense_sort(fitted, N, exclude_seen):
    fx = fitted
    model = fx["model"]
    fn, ff = fx["feats_new"], fx["feats_fit"]
    C = _few(fx["C"], 8, seed=4)
    folded = model.fold_in_items(C, features_new=fn)
    users = np.array([0, 7, 7, 123, 399, 250, 31])
    P = np.hstack([model.predict(ff), model.predict_new_items(folded)])[users]
    tr_r, tr_c = fx["train"]
    seen = []
    for u in users:
        s = np.concatenate([tr_c[tr_r == u], N_FIT + np.nonzero(~np.isnan(C[:, u]))[0]]) if exclude_seen else []
        seen.append(np.asarray(s, np.int64))
    items, scores = model.recommend(users, N, features=ff, exclude_seen=exclude_seen, new_items=folded)
    es, ei, _ = serving_ref.topn_batch(P, seen, None, N)
    assert (items == ei).all() and (scores == es).all()
    if N == 128:
        assert (items >= N_FIT).any()                      # new items do compete
    # new_items=None leaves the call unchanged
    i0, s0 = model.recommend(users, N, features=ff, exclude_seen=exclude_seen)
    i1, s1 = model.recommend(users, N, features=ff, exclude_seen=exclude_seen, new_items=None)
    assert (i0 == i1).all() and (s0 == s1).all()


def test_nan_in_U_raises_linalg_error(fitted):
    fx = fitted
    model = fx["model"]
    eng = model._eng
    C = np.full((2, M), np.nan)
    C[1, 17] = 4.0
    saved = eng.U[17, 0].item()
    eng.U[17, 0] = float("nan")
    try:
        with pytest.raises(np.linalg.LinAlgError, match="row 1"):
            model.fold_in_items(C, features_new={f: X[:2] for f, X in fx["feats_new"].items()})
    finally:
        eng.U[17, 0] = saved
    model.fold_in_items(C, features_new={f: X[:2] for f, X in fx["feats_new"].items()})


def test_cold_item_rmse_matches_a_host_computation(fitted):
    from collaborative_filtering_amd import cv
    fx = fitted
    model = fx["model"]
    C = fx["C"]
    hb, hu = np.nonzero(~np.isnan(C))
    hv = C[hb, hu]
    rng = np.random.default_rng(3)
    k_mask = rng.random(hb.size) < 0.3
    for known in (None, (hu[k_mask], hb[k_mask], hv[k_mask])):
        held = (hu, hb, hv) if known is None else (hu[~k_mask], hb[~k_mask], hv[~k_mask])
        res = cv.cold_item_rmse(model, held, known=known, features_new=fx["feats_new"])
        Ck = np.full_like(C, np.nan)
        if known is not None:
            Ck[known[1], known[0]] = known[2]
        folded = model.fold_in_items(Ck, features_new=fx["feats_new"])
        pred = model.predict_new_items(folded)[held[0], held[1]]
        assert res["pairs"] == held[0].size
        assert res["rmse"] == pytest.approx(np.sqrt(np.mean((pred - held[2]) ** 2)), rel=1e-12)
        base = model.mu + model.b_u[held[0]]
        assert res["baseline_rmse"] == pytest.approx(np.sqrt(np.mean((base - held[2]) ** 2)), rel=1e-12)
        print(f"cold-item RMSE known={'none' if known is None else known[0].size}: {res}")
