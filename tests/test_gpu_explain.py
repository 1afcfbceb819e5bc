"""K11 (GPU): explanations (csrc/explain.hip, als_explain), ALS.explain / explain_new.

The kernel is checked against the float64 contract in tests/serving_ref.py (`explain_pair`) on the same fp32 Z, b_i,
mu and lambda values.  The
outputs are fp64, so the expected error is cond(A) * 1e-16 - the rounding of two different fp64 solution paths
(Cholesky in the kernel, LU in numpy) - not an fp32 rounding.  Errors are relative to
max(1, max_j |contribution[j]|) of the (row, target) (weights: max(1, max_j |weight[j]|); leverage and b_u: to
themselves, floored at 1 for b_u)."""
import ctypes as C

import numpy as np
import pytest

from tests import serving_ref as ref
from tests.gpu_common import csr_rows, env, item_table, record_margins, upload
from tests.serving_ref import EPS

pytestmark = pytest.mark.gpu

MU = 3.5


def _run(torch, be, dev, t, k, indptr, indices, vals, n, lam_u, lam_bu, T, tptr, titems, M, largest, rows=None):
    """One als_explain launch; every output buffer is poisoned first."""
    W, P = tptr.size - 1, titems.size
    d = lambda a: upload(a, dev)                    # noqa: E731
    nan64 = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)
    o = dict(score=nan64(P), latent=nan64(P), leverage=nan64(P), top_contrib=nan64(P, M), top_weight=nan64(P, M),
             b_u_out=nan64(W), top_item=torch.full((P, M), -7, dtype=torch.int32, device=dev),
             top_cnt=torch.full((P,), -7, dtype=torch.int32, device=dev))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    be.explain(k=k, ld=t["ld"], indptr=d(indptr), indices=d(indices if indices.size else np.zeros(1, np.int32)),
               vals=d(vals if vals.size else np.zeros(1, np.float32)), rows=None if rows is None else d(rows), n=n,
               Z=t["Zd"], b_i=t["bid"], mu=t["mud"], lam_u=lam_u, lam_bu=lam_bu, n_sweeps=T, t_ptr=d(tptr),
               t_items=d(titems), topm=M, largest=largest, status=status, **o)
    torch.cuda.synchronize()
    out = {name: v.cpu().numpy() for name, v in o.items()}
    out["status"] = int(status.item())
    return out


def _oracle_row(Z, b_i, lam_u, lam_bu, idx, vals, k, T, targets):
    """`explain_row` of tests/serving_ref.py, the lambdas rounded to fp32 as the kernel reads them."""
    return ref.explain_row(Z, b_i, MU, float(np.float32(lam_u)), float(np.float32(lam_bu)), idx, vals, k, T, targets)


def _targets(indptr, indices, n, seed):
    """5 targets per row: the row's first rated item (a random item for the empty row), three random items, the
    second one repeated."""
    rng = np.random.default_rng(seed)
    tt = []
    for r in range(indptr.size - 1):
        a = rng.integers(0, n, size=4)
        first = indices[indptr[r]] if indptr[r + 1] > indptr[r] else a[3]
        tt.append([first, a[0], a[1], a[0], a[2]])
    return np.asarray(tt, dtype=np.int32)


def _check_lists(out, p, orc, j, idx, M, largest, tol):
    """The list of target position p against oracle target j of the row; returns the largest relative error."""
    nr = idx.size
    sgn = 1.0 if largest else -1.0
    oc, ow = orc["contrib"][j], orc["weights"][j]
    cs = max(1.0, np.abs(oc).max()) if nr else 1.0
    ws = max(1.0, np.abs(ow).max()) if nr else 1.0
    cnt = out["top_cnt"][p]
    assert cnt == min(M, nr)
    items, cc, ww = out["top_item"][p], out["top_contrib"][p], out["top_weight"][p]
    assert (items[cnt:] == -1).all() and (cc[cnt:] == 0).all() and (ww[cnt:] == 0).all()
    if cnt == 0:
        return 0.0
    pos = np.searchsorted(idx, items[:cnt])
    assert (idx[pos] == items[:cnt]).all() and np.unique(items[:cnt]).size == cnt     # rated items, no repeats
    err = max(np.abs(cc[:cnt] - oc[pos]).max() / cs, np.abs(ww[:cnt] - ow[pos]).max() / ws)
    key, it = (sgn * cc[:cnt]).astype(np.float32) + np.float32(0.0), items[:cnt]
    later = (key[:-1] > key[1:]) | ((key[:-1] == key[1:]) & (it[:-1] < it[1:]))
    assert later.all()                                          # (float32(contribution), item) in the stated order
    rest = np.setdiff1d(np.arange(nr), pos)
    if rest.size:                                               # nothing left out beats the last kept entry
        assert (sgn * oc[rest]).max() <= sgn * oc[pos[-1]] + tol * cs
    return err


# Largest errors observed on an MI355X over every case of test_kernel_against_float64_oracle (lists, score, latent
# relative to the scales in the module docstring; leverage relative to itself), and the bounds = ~10x these:
#   lambda_u = 5:     values 6.3e-15, leverage 7.0e-15, b_u 1.7e-15          -> 7e-14   (cond(A) <= 32)
#   lambda_u = 1e-4:  values 2.8e-10, leverage 2.8e-11, b_u 1.3e-12          -> 3e-9    (cond(A) <= 1.1e6)
# i.e. a few hundred cond(A) * 2^-52 at k = 160, as two fp64 factorisations of the same A differ.  The figures of
# every case are recorded under ALS_RECORD_MARGINS (profiles/serving_kernel_test_margins.json).
TOL = {5.0: 7e-14, 1e-4: 3e-9}


@pytest.mark.parametrize("k", [1, 8, 16, 33, 50, 64, 80, 128, 150, 160])
@pytest.mark.parametrize("lam_u", [5.0, 1e-4])
def test_kernel_against_float64_oracle(k, lam_u):
    torch, layout, be, dev = env().short
    n = 4600
    tol = TOL[lam_u]
    t = item_table(torch, layout, dev, n, k, seed=k, mu=MU)
    lengths = [0, 1, max(k // 2, 1), k, 300, 4500]
    indptr, indices, vals = csr_rows(lengths, n, seed=k + 1)
    W = len(lengths)
    tg5 = _targets(indptr, indices, n, seed=k + 2)
    worst = dict(val=0.0, lev=0.0, b=0.0, cond=0.0)
    for T in (1, 3, 0):
        orc = [_oracle_row(t["Z"], t["b_i"], lam_u, 3.0, indices[indptr[r]: indptr[r + 1]],
                           vals[indptr[r]: indptr[r + 1]], k, T, tg5[r]) for r in range(W)]
        worst["cond"] = max(worst["cond"], max(o["cond"] for o in orc))
        for nt in (5, 1):
            # one target per row: the row's second target (a random item)
            cols = np.arange(5) if nt == 5 else np.array([1])
            tptr = np.arange(W + 1, dtype=np.int64) * nt
            titems = np.ascontiguousarray(tg5[:, cols]).ravel()
            for M in (1, 10, 128):
                for largest in (True, False):
                    out = _run(torch, be, dev, t, k, indptr, indices, vals, n, lam_u, 3.0, T, tptr, titems, M, largest)
                    assert out["status"] == 0
                    for r in range(W):
                        o = orc[r]
                        idx = indices[indptr[r]: indptr[r + 1]]
                        worst["b"] = max(worst["b"], abs(out["b_u_out"][r] - o["b_u"]) / max(1.0, abs(o["b_u"])))
                        for e, j in enumerate(cols):
                            p = r * nt + e
                            cs = max(1.0, np.abs(o["contrib"][j]).max()) if idx.size else 1.0
                            worst["val"] = max(worst["val"], abs(out["score"][p] - o["score"][j]) / cs,
                                               abs(out["latent"][p] - o["latent"][j]) / cs,
                                               _check_lists(out, p, o, j, idx, M, largest, tol))
                            assert out["leverage"][p] > 0
                            worst["lev"] = max(worst["lev"], abs(out["leverage"][p] / o["leverage"][j] - 1.0))
                    # a row without ratings: the contract's closed form
                    p0 = np.arange(nt)
                    z0 = t["Z"][titems[p0], :k].astype(np.float64)
                    assert out["b_u_out"][0] == 0 and (out["latent"][p0] == 0).all()
                    assert (out["score"][p0] == MU + t["b_i"][titems[p0]].astype(np.float64)).all()
                    np.testing.assert_allclose(out["leverage"][p0],
                                               (z0 * z0).sum(axis=1) / (float(np.float32(lam_u)) + EPS), rtol=1e-14)
    print(f"explain k={k} lambda_u={lam_u}: max err values {worst['val']:.2e} leverage {worst['lev']:.2e} "
          f"b_u {worst['b']:.2e} cond(A) <= {worst['cond']:.2e}")
    record_margins(f"explain[k={k},lambda_u={lam_u}]", {name: float(worst[name]) for name in ("val", "lev", "b")})
    assert worst["val"] < tol and worst["lev"] < tol and worst["b"] < tol, worst


def test_repeated_target_and_single_target_are_bitwise_the_block_results():
    """Targets are served in blocks that share one pass over the row: a repeated target, and the same target
    asked for alone, give the same bits."""
    torch, layout, be, dev = env().short
    n, k = 4600, 50
    t = item_table(torch, layout, dev, n, k, seed=50, mu=MU)
    indptr, indices, vals = csr_rows([0, 1, 25, 50, 300, 4500], n, seed=51)
    tg5 = _targets(indptr, indices, n, seed=52)
    W = indptr.size - 1
    o5 = _run(torch, be, dev, t, k, indptr, indices, vals, n, 5.0, 3.0, 0, np.arange(W + 1, dtype=np.int64) * 5,
              tg5.ravel(), 10, True)
    o1 = _run(torch, be, dev, t, k, indptr, indices, vals, n, 5.0, 3.0, 0, np.arange(W + 1, dtype=np.int64),
              np.ascontiguousarray(tg5[:, 1]), 10, True)
    for name in ("score", "latent", "leverage", "top_item", "top_contrib", "top_weight", "top_cnt"):
        a = o5[name].reshape(W, 5, -1)
        assert np.array_equal(a[:, 1], a[:, 3]), name
        assert np.array_equal(a[:, 1], o1[name].reshape(W, -1)), name
    assert np.array_equal(o5["b_u_out"], o1["b_u_out"])


def test_a_result_depends_on_its_row_and_target_alone():
    """Alone, inside a batch of 1000, with the targets permuted, through `rows` or with the CSR pre-gathered."""
    torch, layout, be, dev = env().short
    n, k = 3000, 64
    t = item_table(torch, layout, dev, n, k, seed=11, mu=MU)
    rng = np.random.default_rng(12)
    lengths = rng.integers(0, 200, size=1000)
    lengths[[0, 500, 999]] = [150, 700, 64]
    indptr, indices, vals = csr_rows(lengths.tolist(), n, seed=13)
    nt = rng.integers(1, 8, size=1000)
    tptr = np.zeros(1001, np.int64)
    tptr[1:] = np.cumsum(nt)
    titems = rng.integers(0, n, size=tptr[-1]).astype(np.int32)
    args = (n, 2.0, 1.0, 0)
    names = ("score", "latent", "leverage", "top_item", "top_contrib", "top_weight", "top_cnt")
    big = _run(torch, be, dev, t, k, indptr, indices, vals, *args, tptr, titems, 10, True)
    assert big["status"] == 0
    # targets permuted within every row
    perm = np.concatenate([tptr[r] + rng.permutation(nt[r]) for r in range(1000)])
    shuf = _run(torch, be, dev, t, k, indptr, indices, vals, *args, tptr, titems[perm], 10, True)
    for name in names:
        assert np.array_equal(shuf[name], big[name][perm]), name
    for r in (0, 500, 999):
        sl = slice(indptr[r], indptr[r + 1])
        tl = slice(tptr[r], tptr[r + 1])
        one_ptr = np.array([0, nt[r]], np.int64)
        # alone, the CSR pre-gathered
        alone = _run(torch, be, dev, t, k, np.array([0, lengths[r]], np.int64), indices[sl], vals[sl], *args, one_ptr,
                     titems[tl], 10, True)
        # alone, read from the big CSR through `rows`
        via = _run(torch, be, dev, t, k, indptr, indices, vals, *args, one_ptr, titems[tl], 10, True,
                   rows=np.array([r], np.int32))
        for name in names:
            assert np.array_equal(alone[name], big[name][tl]), (r, name)
            assert np.array_equal(via[name], big[name][tl]), (r, name)
        assert alone["b_u_out"][0] == big["b_u_out"][r] == via["b_u_out"][0]
    # work rows in another order, rows repeated
    rows = np.array([999, 0, 500, 0], np.int32)
    tp = np.zeros(5, np.int64)
    tp[1:] = np.cumsum(nt[rows])
    ti = np.concatenate([titems[tptr[r]: tptr[r + 1]] for r in rows])
    sub = _run(torch, be, dev, t, k, indptr, indices, vals, *args, tp, ti, 10, True, rows=rows)
    ref = np.concatenate([np.arange(tptr[r], tptr[r + 1]) for r in rows])
    for name in names:
        assert np.array_equal(sub[name], big[name][ref]), name
    assert np.array_equal(sub["b_u_out"], big["b_u_out"][rows])


def test_nan_in_Z_sets_the_status_word():
    torch, layout, be, dev = env().short
    n, k = 300, 16
    t = item_table(torch, layout, dev, n, k, seed=7, mu=MU)
    t["Z"][17, 3] = np.nan
    t["Zd"] = torch.from_numpy(t["Z"]).to(dev)
    indptr = np.array([0, 2, 4, 5], np.int64)
    indices = np.array([1, 2, 5, 17, 4], np.int32)
    out = _run(torch, be, dev, t, k, indptr, indices, np.ones(5, np.float32), n, 1.0, 1.0, 0,
               np.arange(4, dtype=np.int64), np.array([3, 3, 3], np.int32), 5, True)
    assert out["status"] == 2                             # work row 1 holds item 17


def test_c_abi_status_codes():
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    p = _hip.ExplainParams()
    p.k, p.ld, p.nrows, p.n, p.topm = 161, 176, 1, 10, 10
    assert lib.als_explain(C.byref(p), None) == -2                    # ALS_E_BADK
    p.k, p.ld, p.nrows = 16, 16, 0
    assert lib.als_explain(C.byref(p), None) == 0                     # nrows = 0: no-op, pointers unused
    p.nrows = 3
    assert lib.als_explain(C.byref(p), None) == -1                    # NULL pointers: ALS_E_BADARG
    assert lib.als_explain(None, None) == -1
    p.nrows = 0
    for field, bad in (("topm", 0), ("topm", 129), ("ld", 32), ("n", 0), ("n_sweeps", -1), ("nrows", -1),
                       ("lambda_u", -1.0), ("lambda_bu", float("nan"))):
        old = getattr(p, field)
        setattr(p, field, bad)
        assert lib.als_explain(C.byref(p), None) == -1, field
        setattr(p, field, old)
    assert lib.als_explain(C.byref(p), None) == 0


def _fit_with_features():
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig
    from tests.synth import make_features, make_ratings
    m, n, k = 300, 200, 24
    r, c, v = make_ratings(m, n, 9000, seed=21, empty_users=(5,))
    G, y = make_features(n, seed=22)
    feats = {"genres": G, "years": y}
    cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=4, lambda_u=4.0, lambda_v=5.0),
                    biases=BiasesConfig(lambda_bu=3.0, lambda_bi=2.0))
    model = ALS(cfg, lambda_w={"genres": 1.0, "years": 1.0}, device="cuda:0")
    model.fit_coo(r, c, v, (m, n), features=feats, tol=None, verbose=0)
    return model, feats, r, c, v, m, n


def _user_rows(r, c, v, users):
    ptr = np.zeros(len(users) + 1, np.int64)
    cols, vals = [], []
    for b, u in enumerate(users):
        sel = r == u
        cols.append(c[sel])
        vals.append(v[sel])
        ptr[b + 1] = ptr[b] + sel.sum()
    return ptr, np.concatenate(cols), np.concatenate(vals)


def test_model_explain_equals_explain_new_on_the_training_rows():
    env()
    model, feats, r, c, v, m, n = _fit_with_features()
    rng = np.random.default_rng(3)
    users = np.concatenate([rng.integers(0, m, size=60), [5, 5, 17, 17]])      # user 5 has no ratings
    items = np.concatenate([rng.integers(0, n, size=60), [0, 9, 33, 33]])
    fields = ("score", "latent", "leverage", "b_u", "items", "contributions", "weights", "counts")
    for fs in (feats, None):
        for largest in (True, False):
            ex = model.explain(users, items, 128, features=fs, largest=largest)
            new = model.explain_new(_user_rows(r, c, v, users), (np.arange(users.size + 1), items), 128,
                                    features=fs, largest=largest)
            for f in fields:
                assert np.array_equal(getattr(ex, f), getattr(new, f)), f
            nr = np.array([(r == u).sum() for u in users])
            assert (ex.counts == np.minimum(nr, 128)).all()
            # M >= n: the list is the whole row, and its sum is `latent` up to the rounding of two fp64 sums of at
            # most 128 terms in different orders (each within 128 * 2^-53 * sum |c_j| of the exact sum)
            whole = nr <= 128
            assert whole.sum() > 50
            s = ex.contributions.sum(axis=1)
            assert (np.abs(s - ex.latent) <= 2 * 128 * 2.0 ** -53 * np.abs(ex.contributions).sum(axis=1))[whole].all()
            assert (ex.leverage[users == 5] > 0).all() and (ex.latent[users == 5] == 0).all()
    with_f = model.explain(users, items, 5, features=feats)
    without = model.explain(users, items, 5)
    assert not np.array_equal(with_f.latent, without.latent)           # the composed Z is the one used


def test_explain_new_agrees_with_fold_in_and_recommend_new():
    """b_u and score of explain_new against fold_in / recommend_new(exclude_seen=False) on the same rows: what
    separates them is the fp32 rounding of fold-in's outputs and of the predict epilogue.
    Observed on an MI355X: |b_u - fold_in b| 9.0e-9 (relative to max(1, max |b|)), |score - recommend_new score|
    9.3e-7 (scores of size ~4, fp32 accumulation over k = 24 and three fp32 additions); bounds 10x."""
    env()
    model, feats, r, c, v, m, n = _fit_with_features()
    users = np.arange(0, 120)
    R_new = _user_rows(r, c, v, users)
    _, b = model.fold_in(R_new, features=feats)
    items, scores = model.recommend_new(R_new, 3, features=feats, exclude_seen=False)
    ex = model.explain_new(R_new, (np.arange(users.size + 1) * 3, items.ravel()), 10, features=feats)
    db = np.abs(ex.b_u.reshape(-1, 3) - b[:, None]).max() / max(1.0, np.abs(b).max())
    ds = np.abs(ex.score - scores.ravel()).max()
    print(f"explain_new vs fold_in: |d b_u| {db:.2e}; vs recommend_new: |d score| {ds:.2e}")
    assert db < 1e-7 and ds < 1e-5


def test_full_size_properties():
    """Z for 100K items at k = 64, 4096 rows of ~100 ratings from the synth distribution, one target each."""
    torch, layout, be, dev = env().short
    from tests.synth import make_ratings
    NI, k, B, lam_u = 100_000, 64, 4096, 5.0
    t = item_table(torch, layout, dev, NI, k, seed=3, scale=0.3, mu=MU)
    r, c, v = make_ratings(B, NI, 100 * B, seed=B, user_exp=0.0)
    ptr = np.zeros(B + 1, np.int64)
    np.add.at(ptr, r + 1, 1)
    ptr = np.cumsum(ptr)
    titems = np.random.default_rng(1).integers(0, NI, size=B).astype(np.int32)
    out = _run(torch, be, dev, t, k, ptr, c.astype(np.int32), v.astype(np.float32), NI, lam_u, 3.0, 0,
               np.arange(B + 1, dtype=np.int64), titems, 10, True)
    assert out["status"] == 0
    for name in ("score", "latent", "leverage", "top_contrib", "top_weight", "b_u_out"):
        assert np.isfinite(out[name]).all(), name
    zt = t["Z"][titems, :k].astype(np.float64)
    cap = (zt * zt).sum(axis=1) / (float(np.float32(lam_u)) + EPS)
    assert (np.diff(ptr) > 0).all()                       # every row has ratings: the cap is not attained
    assert (out["leverage"] > 0).all() and (out["leverage"] <= cap).all()
    assert (out["top_cnt"] == np.minimum(np.diff(ptr), 10)).all()
