"""ImplicitALS on the device: als_table_gram_f64 and als_implicit_row_solve against the fp64 numpy definitions of
tests/implicit_ref.py, the fit against `implicit_ref.fit` with fp32 storage, and the serving calls on a fitted model.

Tolerances
  table Gram   per element nrows 2^-52 (|F|^T |F|)_ij (fp64 accumulation), exactly zero in the padding.
  row solve    |x - x_ref| <= 2^-23 max|x_row|: one fp32 rounding (2^-24) plus an fp64 solve error far below it - the
               cases' cond(A) is asserted < 1e6 on the CPU side, so that error is < 1e-10.  x.b to 1e-12 relative.
  fit          max|dU| / max|U| (and V) after 8 iterations.  Observed over the eight cases: 0.0 - every fp32 entry of
               both tables equals the reference's (profiles/implicit_margins.json, recorded under
               ALS_RECORD_MARGINS).  Ten times nothing is no bound, so FIT_TOL is ten times what a different rounding
               of the stored tables can move them by: `implicit_ref.fit` with and without fp32 storage differs by
               7e-8 ... 2.0e-7 of the maximum over these eight cases - 2e-6, below the 1e-5 the tolerance has to stay
               under; a dropped term or weight shows at 1e-2.  Loss 1e-9 relative (observed 4.3e-14).
"""
import functools

import numpy as np
import pytest

from tests import gpu_common as gc
from tests import implicit_ref as iref

pytestmark = pytest.mark.gpu

FIT_TOL = 2e-6


@functools.lru_cache(maxsize=None)
def _env():
    return gc.env()


def _image_doubles(ld):
    return ld // 16 * (ld // 16 + 1) // 2 * 256


def _table_gram(F, k):
    torch, layout, be, dev = _env().short
    ld = F.shape[1]
    out = torch.full((_image_doubles(ld),), float("nan"), dtype=torch.float64, device=dev)
    be.table_gram(k, ld, gc.upload(F, dev), out)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------
# table Gram
# ---------------------------------------------------------------------------------------------------------
def _gram_rows_big():
    """Every workgroup of the fixed grid gets three 16-row tiles and a ragged one, the last workgroup a short range."""
    from collaborative_filtering_amd import _hip
    P = int(_hip.load().als_table_gram_partials())
    return P * 50 - 37


@pytest.mark.parametrize("k", [1, 17, 64, 160])
@pytest.mark.parametrize("nrows", [0, 1, 63, 1000, "big"])
def test_table_gram_matches_fp64(k, nrows):
    torch, layout, be, dev = _env().short
    nrows = _gram_rows_big() if nrows == "big" else nrows
    ld = layout.padded_k(k)
    rng = np.random.default_rng(1000 * k + nrows % 997)
    F = np.full((max(nrows, 1), ld), 3.0, dtype=np.float32)         # padding columns hold garbage: they must not count
    F[:, :k] = rng.normal(scale=0.5, size=(max(nrows, 1), k))
    F = F[:nrows]
    img = _table_gram(F, k)
    img2 = _table_gram(F, k)
    assert gc.same_bits(img.cpu(), img2.cpu())
    G, padding = iref.gram_from_image(img.cpu().numpy(), k)
    assert not padding.any()
    F64 = F[:, :k].astype(np.float64)
    worst = gc.ratio(G, F64.T @ F64, nrows * 2.0 ** -52 * (np.abs(F64).T @ np.abs(F64)), "table gram")
    gc.record_margins(f"table_gram/k{k}/n{nrows}", worst)
    assert worst <= 1.0
    assert np.array_equal(G, G.T)


# ---------------------------------------------------------------------------------------------------------
# row solve
# ---------------------------------------------------------------------------------------------------------
LENS = (0, 1, 3, 63, 64, 65, 200, 4096, 4097, 9000)
NCOLS = 9100
LAM = 0.5


@functools.lru_cache(maxsize=None)
def _side():
    return gc.random_side(_env().layout, len(LENS), NCOLS, list(LENS), seed=5)


@functools.lru_cache(maxsize=None)
def _tables(k):
    """(F [NCOLS + 1, ld] with a zero last row, the Gram image of a separate table T by the kernel, and that G)."""
    layout = _env().layout
    ld = layout.padded_k(k)
    rng = np.random.default_rng(77 + k)
    F = gc.pad(rng.normal(scale=0.3, size=(NCOLS, k)).astype(np.float32), ld, extra_rows=1)
    T = gc.pad(rng.normal(scale=0.3, size=(500, k)).astype(np.float32), ld)
    img = _table_gram(T, k)
    return F, img, iref.gram_from_image(img.cpu().numpy(), k)[0]


def _weights(case):
    side = _side()
    rng = np.random.default_rng(9)
    a = rng.uniform(0.5, 5.0, size=side.indices.size).astype(np.float32)
    t = rng.uniform(0.5, 3.0, size=side.indices.size).astype(np.float32)
    lam_row = rng.uniform(0.25, 1.0, size=len(LENS)).astype(np.float32)
    if case == "default":           # t = 1 + a, scalar lambda, F with a zero row
        return a, None, None, 1.0, True
    if case == "given":             # rhs_w and lambda_row given, a0 = 0.25, F without a zero row
        return a, t, lam_row, 0.25, False
    return np.zeros_like(a), None, None, 1.0, False         # "azero": x = (G + lambda I)^-1 sum f


def _solve(k, a, t, lam_row, g_scale, zero_row, img, F, rows=None, lam=LAM):
    """One als_implicit_row_solve over the rows `rows` (None: all) of `_side()`: (X [rows, ld], xb, status)."""
    e = _env()
    torch, layout, be, dev = e.short
    side = _side()
    ld = layout.padded_k(k)
    sd = e.side_dev(layout.SparseSide(side.nrows, side.ncols, side.indptr, side.indices, a), dev)
    if rows is None:
        tasks = layout.build_row_tasks(side.indptr, dual_len=0, mid_len=0)
    else:
        tasks = layout.build_row_tasks(side.indptr, rows[0], rows[0] + 1, dual_len=0, mid_len=0)
    X = torch.full((side.nrows, ld), float("nan"), dtype=torch.float32, device=dev)
    xb = torch.full((side.nrows,), float("nan"), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    Fd = gc.upload(F if zero_row else F[:NCOLS], dev)
    be.implicit_row_solve(k=k, ld=ld, side=sd, F=Fd, zero_row=NCOLS if zero_row else -1, G=img, g_scale=g_scale,
                          lam=lam, lam_row=None if lam_row is None else gc.upload(lam_row, dev), X_out=X, xb_out=xb,
                          status=status, tasks=e.tasks_dev(tasks, dev),
                          rhs_w=None if t is None else gc.upload(t, dev))
    torch.cuda.synchronize()
    return X.cpu().numpy(), xb.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("case", ["default", "given", "azero"])
@pytest.mark.parametrize("k", [1, 16, 17, 50, 64, 65, 128, 160])
def test_row_solve_matches_fp64(k, case):
    side = _side()
    F, img, G = _tables(k)
    a, t, lam_row, g_scale, zero_row = _weights(case)
    X, xb, status = _solve(k, a, t, lam_row, g_scale, zero_row, img, F)
    assert status == 0
    assert not X[:, k:].any()                                           # padding columns are written as zero
    t64 = 1.0 + a.astype(np.float64) if t is None else t.astype(np.float64)
    worst_x = worst_xb = 0.0
    for r, n_r in enumerate(LENS):
        s = slice(side.indptr[r], side.indptr[r + 1])
        Fr = F[side.indices[s], :k].astype(np.float64)
        lam = LAM if lam_row is None else float(lam_row[r])
        x, b = iref.row_solve(Fr, a[s], t64[s], g_scale * G, lam)
        if n_r == 0:
            assert not X[r].any() and xb[r] == 0.0
            continue
        A = g_scale * G + (Fr * a[s].astype(np.float64)[:, None]).T @ Fr + (lam + iref.EPS) * np.eye(k)
        assert np.linalg.cond(A) < 1e6
        worst_x = max(worst_x, np.max(np.abs(X[r, :k] - x)) / (2.0 ** -23 * np.max(np.abs(x))))
        worst_xb = max(worst_xb, abs(xb[r] - x @ b) / (1e-12 * abs(x @ b)))
    gc.record_margins(f"implicit_row_solve/{case}/k{k}", {"x": worst_x, "xb": worst_xb})
    assert worst_x <= 1.0 and worst_xb <= 1.0


@pytest.mark.parametrize("k", [17, 64, 160])
def test_row_solve_bits_do_not_depend_on_the_launch(k):
    """A row alone or among the others, with or without a zero row in F, and a second run: the same bits."""
    F, img, _ = _tables(k)
    a, t, lam_row, g_scale, _ = _weights("default")
    X, xb, _ = _solve(k, a, t, lam_row, g_scale, True, img, F)
    X2, xb2, _ = _solve(k, a, t, lam_row, g_scale, True, img, F)
    assert gc.same_bits(X, X2) and gc.same_bits(xb, xb2)
    X3, xb3, _ = _solve(k, a, t, lam_row, g_scale, False, img, F)
    assert gc.same_bits(X, X3) and gc.same_bits(xb, xb3)
    for r in (LENS.index(65), LENS.index(4097), LENS.index(9000)):
        Xr, xbr, _ = _solve(k, a, t, lam_row, g_scale, True, img, F, rows=(r,))
        assert gc.same_bits(X[r], Xr[r]) and xb[r] == xbr[r]
        others = [q for q, n_q in enumerate(LENS) if q != r and n_q > 0]
        assert np.isnan(Xr[others]).all()               # rows with entries that no task names: untouched


def test_row_solve_reports_a_non_positive_pivot():
    """The kernel reports a failed factorisation itself (status = row + 1) and nothing faults.  With the model's own
    G = 0, a = 0, lambda = 0 the system is 1e-10 I - positive definite, status 0; an indefinite image (G = -I) with
    a = 0, lambda = 0 has the pivot -1 + 1e-10."""
    from collaborative_filtering_amd.serving import _raise_unless_solved
    torch, layout, be, dev = _env().short
    k = 17
    F, _, _ = _tables(k)
    side = _side()
    a0 = np.zeros(side.indices.size, np.float32)
    zero = torch.zeros(_image_doubles(layout.padded_k(k)), dtype=torch.float64, device=dev)
    X, _, status = _solve(k, a0, None, None, 1.0, True, zero, F, lam=0.0)
    assert status == 0
    r = LENS.index(3)
    s = slice(side.indptr[r], side.indptr[r + 1])
    x_ref = F[side.indices[s], :k].astype(np.float64).sum(0) / 1e-10
    assert np.max(np.abs(X[r, :k] - x_ref)) <= 2.0 ** -23 * np.max(np.abs(x_ref))
    neg = gc.upload(iref.gram_image(-np.eye(k), k), dev)
    _, _, status = _solve(k, a0, None, None, 1.0, True, neg, F, rows=(r,), lam=0.0)
    assert status == r + 1
    with pytest.raises(np.linalg.LinAlgError):
        _raise_unless_solved(torch.tensor([status]), "implicit")


# ---------------------------------------------------------------------------------------------------------
# fit
# ---------------------------------------------------------------------------------------------------------
SHAPES = {"k20": (300, 200, 20, 4900), "k64": (200, 150, 64, 3400)}
ITERS, ALPHA, FIT_LAM = 8, 2.0, 0.5


@functools.lru_cache(maxsize=None)
def _ratings(shape):
    m, n, k, nnz = SHAPES[shape]
    r, c, v = iref.zipf_counts(m, n, nnz, seed=31)
    csr, csc = _env().layout.coo_to_sides(r, c, v, (m, n))
    return (r, c, v), csr, csc


@functools.lru_cache(maxsize=None)
def _fit(shape, confidence, a0):
    from collaborative_filtering_amd import ALSConfig, CoreConfig, ImplicitALS, ImplicitConfig
    m, n, k, _ = SHAPES[shape]
    coo, csr, csc = _ratings(shape)
    cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=ITERS, lambda_u=FIT_LAM, lambda_v=FIT_LAM, random_state=3))
    model = ImplicitALS(cfg, ImplicitConfig(alpha=ALPHA, confidence=confidence, eps=1.0, unobserved_weight=a0),
                        device="cuda:0").fit_coo(*coo, (m, n), tol=None, verbose=0)
    ua, ia = (iref.weights(s.vals, ALPHA, confidence, 1.0) for s in (csr, csc))
    ref = iref.fit(csr.indptr, csr.indices, ua, csc.indptr, csc.indices, ia, (m, n), k, ITERS, a0, FIT_LAM, FIT_LAM, 3)
    return model, ref


@pytest.mark.parametrize("a0", [1.0, 0.25])
@pytest.mark.parametrize("confidence", ["linear", "log"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fit_matches_the_fp32_storage_reference(shape, confidence, a0):
    model, (U, V, losses) = _fit(shape, confidence, a0)
    du = np.max(np.abs(model.U - U)) / np.max(np.abs(U))
    dv = np.max(np.abs(model.V - V)) / np.max(np.abs(V))
    loss = np.asarray(model.history["loss"])
    dl = np.max(np.abs(loss - losses) / np.abs(losses))
    print(f"implicit fit {shape} {confidence} a0={a0}: dU {du:.3e} dV {dv:.3e} dloss {dl:.3e}")
    gc.record_margins(f"implicit_fit/{shape}/{confidence}/a0_{a0}", {"dU": du, "dV": dv, "dloss": dl})
    assert du <= FIT_TOL and dv <= FIT_TOL
    assert dl <= 1e-9
    assert (np.diff(loss) <= 0).all()


# ---------------------------------------------------------------------------------------------------------
# serving on the fitted model
# ---------------------------------------------------------------------------------------------------------
def test_serving_on_the_fitted_model():
    model, _ = _fit("k20", "linear", 1.0)
    m, n, k, _ = SHAPES["k20"]
    _, csr, _ = _ratings("k20")
    users = np.arange(0, m, 5)
    N = 10
    items, scores = model.recommend(users, N=N)
    P = model.predict()
    for b, u in enumerate(users):
        seen = csr.indices[csr.indptr[u]:csr.indptr[u + 1]]
        assert (items[b] >= 0).all() and not np.intersect1d(items[b], seen).size
        assert gc.same_bits(scores[b], P[u, items[b]].astype(np.float64))
    # rank_of and recommend_quota agree with recommend where they overlap
    rank, _, rscore = model.rank_of(np.repeat(users, N), items.reshape(-1))
    assert np.array_equal(rank.reshape(-1, N), np.tile(np.arange(N), (users.size, 1)))
    assert np.array_equal(rscore.reshape(-1, N).astype(np.float64), scores)
    qi, qs = model.recommend_quota(users, N=N, groups=np.arange(n) % 4, max_per_group=N)
    assert np.array_equal(qi, items) and np.array_equal(qs, scores)


def test_recommend_new_equals_a_reference_user_half_step():
    model, _ = _fit("k20", "linear", 1.0)
    m, n, k, _ = SHAPES["k20"]
    _, csr, _ = _ratings("k20")
    users = np.arange(16) * 7
    N = 10
    lens = np.array([csr.indptr[u + 1] - csr.indptr[u] for u in users])
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([csr.indices[csr.indptr[u]:csr.indptr[u + 1]] for u in users])
    val = np.concatenate([csr.vals[csr.indptr[u]:csr.indptr[u + 1]] for u in users])
    items, scores = model.recommend_new((ptr, idx, val), N=N)
    Uf, bf = model.fold_in((ptr, idx, val))
    X, _ = iref.half_step(ptr, idx, iref.weights(val, ALPHA), model.V, 1.0, FIT_LAM)
    assert np.max(np.abs(Uf - X)) <= 2.0 ** -23 * np.max(np.abs(X)) and not bf.any()
    # the folded rows equal the fitted rows' last half-step only up to V's own last update; against the reference
    # half-step on the FINAL V the lists agree up to near-ties of the fp32 rounding of u
    S = X.astype(np.float32).astype(np.float64) @ model.V.T
    tol = 2.0 ** -22 * np.max(np.abs(S))
    for b in range(users.size):
        seen = idx[ptr[b]:ptr[b + 1]]
        assert (items[b] >= 0).all() and not np.intersect1d(items[b], seen).size
        assert np.max(np.abs(scores[b] - S[b, items[b]])) <= tol
        rest = np.setdiff1d(np.arange(n), np.concatenate([seen, items[b]]))
        assert S[b, rest].max() <= scores[b, -1] + tol
        assert (np.diff(scores[b]) <= 0).all()


def test_inherited_serving_calls_run_on_the_fitted_model():
    """The calls that see only the tables and the training CSR work unchanged; where one of them is documented to
    reduce to `recommend`, it does."""
    from collaborative_filtering_amd import cv
    model, _ = _fit("k20", "linear", 1.0)
    m, n, k, _ = SHAPES["k20"]
    (r, c, v), csr, csc = _ratings("k20")
    users = np.arange(0, m, 9)
    B, N = users.size, 10
    items, scores = model.recommend(users, N=N)
    P = model.predict()
    flat = users[:, None] * n + items
    # (predict_at sums the k products in another order than predict: equal to fp32 rounding, not bitwise)
    at = model.predict_at(flat.reshape(-1))
    assert np.max(np.abs(at - P[users[:, None], items].reshape(-1))) <= k * 2.0 ** -24 * np.max(np.abs(P))
    di, ds = model.recommend_deep(users, N=N)
    assert np.array_equal(di, items) and np.array_equal(ds, scores)
    ci, cs = model.recommend_capacity(users, N=N, capacity=B)
    assert np.array_equal(ci, items) and np.array_equal(cs, scores)
    table = model.eligibility(np.ones((2, n), dtype=bool))
    ei, es = model.recommend_eligible(users, N=N, eligibility=table, segments=np.arange(B) % 2)
    assert np.array_equal(ei, items) and np.array_equal(es, scores)
    vi, vs = model.recommend_diverse(users, N=N, diversity=0.3)
    assert vi.shape == (B, N) and np.isfinite(vs).all() and np.isfinite(model.list_diversity(vi)).all()
    cats = np.zeros((n, 3), dtype=np.float64)
    cats[np.arange(n), np.arange(n) % 3] = 1.0
    ki, ks = model.recommend_calibrated(users, N=N, categories=cats, calibration=0.5)
    assert ki.shape == (B, N) and np.isfinite(ks).all()
    assert np.isfinite(model.list_miscalibration(ki, categories=cats, users=users)).all()
    gi, gs = model.recommend_group([[0, 1, 2], [5, 9]], N=N, aggregate="min")
    assert gi.shape == (2, N) and np.isfinite(gs).all()
    si, ss = model.similar_items([0, 7], N=N)
    ui, us = model.similar_users([0, 7], N=N)
    assert si.shape == ui.shape == (2, N) and (np.abs(ss) <= 1 + 1e-6).all() and (np.abs(us) <= 1 + 1e-6).all()
    ai, a_s = model.recommend_users([0, 3], N=N)
    for b, i in enumerate((0, 3)):
        assert not np.intersect1d(ai[b], csc.indices[csc.indptr[i]:csc.indptr[i + 1]]).size
        assert gc.same_bits(a_s[b], P[ai[b], i].astype(np.float64))
    hr, hc, _ = iref.zipf_counts(m, n, 400, 99)
    out = cv.ranking_at_k(model, hr, hc, K=N)
    assert out["users"] > 0 and 0.0 <= out["recall@K"] <= 1.0
