"""K9 (GPU): fold-in of users outside the fit (csrc/fold_in.hip, als_fold_in), ALS.fold_in / recommend_new and
cv.fold_in_ranking_at_k.

The kernel is checked against the float64 contract in tests/serving_ref.py (`fold_in_user`) on the same fp32 Z, b_i,
mu and lambda values: the expected error is the fp32 rounding of the outputs.  recommend_new is checked exactly (==)
against predict-epilogue scores of the folded table."""
import ctypes as C

import numpy as np
import pytest

from tests import serving_ref as ref
from tests.gpu_common import csr_rows, env, item_table, record_margins, upload

pytestmark = pytest.mark.gpu


def _oracle(Z, b_i, mu, lam_u, lam_bu, indptr, indices, vals, k, T):
    """`fold_in_user` of tests/serving_ref.py on every CSR row, the lambdas rounded to fp32 as the kernel reads them:
    T alternations of the user half-step from b = 0, or (T = 0) their fixed point."""
    f = lambda x: float(np.float32(x))              # noqa: E731
    rows = [ref.fold_in_user(Z, b_i, mu, f(lam_u), f(lam_bu), indices[indptr[r]: indptr[r + 1]],
                             vals[indptr[r]: indptr[r + 1]], k, T) for r in range(indptr.size - 1)]
    return np.array([u for u, _ in rows]), np.array([b for _, b in rows])


def _run(torch, be, dev, t, k, indptr, indices, vals, n, lam_u, lam_bu, T):
    B = indptr.size - 1
    d = lambda a: upload(a, dev)                    # noqa: E731
    U = torch.full((B, t["ld"]), float("nan"), dtype=torch.float32, device=dev)
    b = torch.full((B,), float("nan"), dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    be.fold_in(k=k, ld=t["ld"], indptr=d(indptr), indices=d(indices if indices.size else np.zeros(1, np.int32)),
               vals=d(vals if vals.size else np.zeros(1, np.float32)), n=n, Z=t["Zd"], b_i=t["bid"], mu=t["mud"],
               lam_u=lam_u, lam_bu=lam_bu, n_sweeps=T, U_out=U, b_u_out=b, status=status)
    torch.cuda.synchronize()
    return U.cpu().numpy(), b.cpu().numpy(), int(status.item())


# observed (max over the cases below, relative to max(1, max |u|) per row): u 3.0e-8 (lambda_u = 5), 5.6e-8
# (lambda_u = 1e-4), b 2.9e-8 - the fp32 rounding of the outputs
TOL = 5e-7


@pytest.mark.parametrize("k", [1, 8, 16, 33, 50, 64, 80, 128, 150, 160])
@pytest.mark.parametrize("lam_u", [5.0, 1e-4])
def test_kernel_against_float64_oracle(k, lam_u):
    torch, layout, be, dev = env().short
    n = 4600
    t = item_table(torch, layout, dev, n, k, seed=k)
    lengths = [0, 1, max(k // 2, 1), k, 300, 4500]
    indptr, indices, vals = csr_rows(lengths, n, seed=k + 1)
    worst = {"u": 0.0, "b": 0.0}
    for T in (1, 3, 0):
        U, b, st = _run(torch, be, dev, t, k, indptr, indices, vals, n, lam_u, 3.0, T)
        assert st == 0
        Uo, bo = _oracle(t["Z"], t["b_i"], 3.5, lam_u, 3.0, indptr, indices, vals, k, T)
        assert (U[:, k:] == 0).all()
        scale = np.maximum(1.0, np.abs(Uo).max(axis=1))
        err_u = (np.abs(U[:, :k] - Uo).max(axis=1) / scale).max()
        err_b = (np.abs(b - bo) / np.maximum(1.0, np.abs(bo))).max()
        worst = {"u": max(worst["u"], float(err_u)), "b": max(worst["b"], float(err_b))}
        assert err_u < TOL and err_b < TOL, (T, err_u, err_b)
        assert (U[0] == 0).all() and b[0] == 0          # no ratings: u = 0, b = 0
    record_margins(f"fold_in[k={k},lambda_u={lam_u}]", worst)


def test_many_sweeps_reach_the_fixed_point():
    torch, layout, be, dev = env().short
    n, k = 2000, 64
    t = item_table(torch, layout, dev, n, k, seed=5)
    indptr, indices, vals = csr_rows([3, 40, 64, 200], n, seed=6)
    U0, b0, _ = _run(torch, be, dev, t, k, indptr, indices, vals, n, 2.0, 1.0, 0)
    U5, b5, _ = _run(torch, be, dev, t, k, indptr, indices, vals, n, 2.0, 1.0, 500)
    assert np.abs(U5 - U0).max() < 1e-6 * max(1.0, np.abs(U0).max())
    assert np.abs(b5 - b0).max() < 1e-6 * max(1.0, np.abs(b0).max())
    U1, b1, _ = _run(torch, be, dev, t, k, indptr, indices, vals, n, 2.0, 1.0, 1)
    assert not np.array_equal(b1, b0)                    # one sweep is not the fixed point


def test_nan_in_Z_sets_the_status_word():
    torch, layout, be, dev = env().short
    n, k = 300, 16
    t = item_table(torch, layout, dev, n, k, seed=7)
    t["Z"][17, 3] = np.nan
    t["Zd"] = torch.from_numpy(t["Z"]).to(dev)
    indptr = np.array([0, 2, 4, 5], np.int64)
    indices = np.array([1, 2, 5, 17, 4], np.int32)
    vals = np.ones(5, np.float32)
    _, _, st = _run(torch, be, dev, t, k, indptr, indices, vals, n, 1.0, 1.0, 0)
    assert st == 2                                        # row 1 holds item 17


def test_c_abi_status_codes():
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    p = _hip.FoldInParams()
    p.k, p.ld, p.nrows, p.n = 161, 176, 1, 10
    assert lib.als_fold_in(C.byref(p), None) == -2                    # ALS_E_BADK
    p.k, p.ld, p.nrows = 16, 16, 0
    assert lib.als_fold_in(C.byref(p), None) == 0                     # nrows = 0: no-op, pointers unused
    p.nrows = 3
    assert lib.als_fold_in(C.byref(p), None) == -1                    # NULL pointers: ALS_E_BADARG
    p.nrows, p.ld = 0, 32
    assert lib.als_fold_in(C.byref(p), None) == -1                    # ld != als_padded_k(k)
    p.ld, p.n_sweeps = 16, -1
    assert lib.als_fold_in(C.byref(p), None) == -1


# ---------------------------------------------------------------------------------------------- model level
M, N_ITEMS, K = 400, 300, 24


@pytest.fixture(scope="module")
def fitted():
    from collaborative_filtering_amd import (ALS, ALSConfig, BiasesConfig, CoreConfig, GraphConfig,
                                             GraphSimConfig)
    from tests.synth import make_features, make_ratings
    r, c, v = make_ratings(M, N_ITEMS, 12000, seed=11)
    G, y = make_features(N_ITEMS, seed=12)
    features = {"genres": G, "year": y}
    held = r >= M - 40                                   # the last 40 users: outside the fit
    cfg = ALSConfig(core=CoreConfig(n_factors=K, n_iters=4, lambda_u=3.0, lambda_v=4.0),
                    biases=BiasesConfig(lambda_bu=2.0, lambda_bi=2.0),
                    graph=GraphConfig(alpha=0.5, sim=GraphSimConfig(topk=10)))
    model = ALS(cfg, {"genres": 1.0, "year": 1.0}, device="cuda:0")
    model.fit_coo(r[~held], c[~held], v[~held], (M, N_ITEMS), features=features, tol=None, verbose=0)
    R = np.full((40, N_ITEMS), np.nan)
    R[r[held] - (M - 40), c[held]] = v[held]
    return model, features, R


def _csr(R):
    mask = ~np.isnan(R)
    indptr = np.zeros(R.shape[0] + 1, np.int64)
    indptr[1:] = np.cumsum(mask.sum(axis=1))
    return indptr, np.nonzero(mask)[1].astype(np.int32), R[mask].astype(np.float32)


def test_fold_in_on_a_fitted_model_against_the_oracle(fitted):
    model, features, R = fitted
    ip, ix, vv = _csr(R)
    Zf = (model.V + sum(features[f] @ model.W[f] for f in features)).astype(np.float32)
    for feats, Z in ((features, Zf), (None, model.V.astype(np.float32))):
        for T in (None, 2):
            U, b = model.fold_in(R, features=feats, n_sweeps=T)
            assert U.shape == (40, K) and b.shape == (40,) and U.dtype == np.float64
            Uo, bo = _oracle(Z, model.b_i.astype(np.float32), model.mu, model.lambda_u, model.lambda_bu,
                             ip, ix, vv, K, T or 0)
            assert np.abs(U - Uo).max() < 1e-5 * max(1.0, np.abs(Uo).max())
            assert np.abs(b - bo).max() < 1e-5 * max(1.0, np.abs(bo).max())
    # features change Z as in predict
    assert not np.array_equal(model.fold_in(R, features=features)[0], model.fold_in(R)[0])


def test_bitwise_invariance(fitted):
    model, features, R = fitted
    U, b = model.fold_in(R, features=features)
    perm = np.random.default_rng(0).permutation(40)
    Up, bp = model.fold_in(R[perm], features=features)
    assert (Up == U[perm]).all() and (bp == b[perm]).all()
    U1, b1 = model.fold_in(R[:13], features=features)
    U2, b2 = model.fold_in(R[13:], features=features)
    assert (np.vstack([U1, U2]) == U).all() and (np.concatenate([b1, b2]) == b).all()
    Ud, bd = model.fold_in(np.vstack([R, R]), features=features)
    assert (Ud == np.vstack([U, U])).all() and (bd == np.concatenate([b, b])).all()
    ip, ix, vv = _csr(R)
    Uc, bc = model.fold_in((ip, ix, vv), features=features)
    assert (Uc == U).all() and (bc == b).all()
    rng = np.random.default_rng(1)
    ix2, vv2 = ix.copy(), vv.copy()
    for r in range(40):                                  # columns shuffled within every row
        s = slice(ip[r], ip[r + 1])
        o = rng.permutation(ip[r + 1] - ip[r])
        ix2[s], vv2[s] = ix[s][o], vv[s][o]
    Us, bs = model.fold_in((ip, ix2, vv2), features=features)
    assert (Us == U).all() and (bs == b).all()


def test_empty_batch(fitted):
    model, features, R = fitted
    U, b = model.fold_in(R[:0])
    assert U.shape == (0, K) and b.shape == (0,)
    items, scores = model.recommend_new(R[:0], 5)
    assert items.shape == scores.shape == (0, 5)


@pytest.mark.parametrize("N", [1, 10, 128])
@pytest.mark.parametrize("exclude_seen", [True, False])
def test_recommend_new_against_the_masked_dense_sort(fitted, N, exclude_seen):
    import torch
    model, features, R = fitted
    R = np.vstack([R, np.full((1, N_ITEMS), np.nan)])             # plus a user without ratings
    eng = model._eng
    ip, ix, vv = _csr(R)
    with torch.cuda.device(eng.dev):
        Z = eng._compose_for(features)
        U, b, _, _ = eng._fold_in_dev(ip, ix, vv, Z, 0)
        P = torch.empty(R.shape[0], eng.n, dtype=torch.float32, device=eng.dev)
        eng.be.predict_dense(k=eng.k, ld=eng.ld, m=R.shape[0], n=eng.n, U=U, Z=Z, b_u=b, b_i=eng.b_i, mu=eng.mu,
                             out=P)
        P = P.cpu().numpy().astype(np.float64)
    seen = [ix[ip[r]: ip[r + 1]] if exclude_seen else np.zeros(0, np.int64) for r in range(R.shape[0])]
    items, scores = model.recommend_new(R, N, features=features, exclude_seen=exclude_seen)
    es, ei, _ = ref.topn_batch(P, seen, None, N)
    assert (items == ei).all() and (scores == es).all()
    Uf, bf = model.fold_in(R, features=features)
    assert (Uf == U[:, :K].cpu().numpy()).all() and (bf == b.cpu().numpy()).all()


def test_fold_in_ranking_at_k_matches_a_host_computation(fitted):
    from collaborative_filtering_amd import cv
    model, features, R = fitted
    rng = np.random.default_rng(3)
    ur, uc = np.nonzero(~np.isnan(R))
    vals = R[ur, uc]
    hold = rng.random(ur.size) < 0.3
    labels = ur + 1000                                   # any labels for the new users
    known = (labels[~hold], uc[~hold], vals[~hold])
    held = (labels[hold], uc[hold], vals[hold])
    for K_, thr in ((5, None), (10, 3.0)):
        res = cv.fold_in_ranking_at_k(model, known, held, K=K_, min_rating=thr, features=features)
        keep = np.ones(hold.sum(), bool) if thr is None else held[2] >= thr
        users = np.unique(held[0][keep])
        Rk = np.full((users.size, N_ITEMS), np.nan)
        for lab, c_, v_ in zip(*known):
            j = np.searchsorted(users, lab)
            if j < users.size and users[j] == lab:
                Rk[j, c_] = v_
        items, _ = model.recommend_new(Rk, K_, features=features)
        rec, nd = [], []
        for j, u in enumerate(users):
            rel = set(held[1][keep][held[0][keep] == u].tolist())
            hits = [i in rel for i in items[j]]
            rec.append(sum(hits) / len(rel))
            dcg = sum(h / np.log2(r + 2) for r, h in enumerate(hits))
            nd.append(dcg / sum(1 / np.log2(r + 2) for r in range(min(K_, len(rel)))))
        assert res["users"] == users.size
        assert res["recall@K"] == pytest.approx(np.mean(rec), rel=1e-12)
        assert res["ndcg@K"] == pytest.approx(np.mean(nd), rel=1e-12)
