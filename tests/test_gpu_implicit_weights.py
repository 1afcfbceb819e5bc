"""The weights p_u q_i on the unobserved entries of ImplicitALS on the device:
als_table_gram_weighted_f64 and als_implicit_params.g_scale_row against the fp64 numpy definitions of
tests/implicit_weighted_ref.py, the weighted fit against `implicit_weighted_ref.fit` with fp32 storage, the exact ties
to the unweighted path, and fold-in on a weighted fit.

Tolerances (those of tests/test_gpu_implicit.py, whose bases carry over)
  weighted Gram  per element nrows 2^-52 (|F|^T diag(w) |F|)_ij: fp64 accumulation of nrows terms, each operand product
                 f w exact; exactly zero in the padding.
  row solve      |x - x_ref| <= 2^-23 max|x_row| (x is rounded to fp32; cond(A) < 1e6 is asserted, so the fp64 solve
                 error is < 1e-10), x.b to 1e-12 relative.
  fit            max|dU| / max|U| (and V) <= 2e-6 after 8 iterations, the loss to 1e-12 relative.
  equivalences   bit for bit.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import gpu_common as gc
from tests import implicit_ref as iref
from tests import implicit_weighted_ref as wref

pytestmark = pytest.mark.gpu

FIT_TOL = 2e-6


@functools.lru_cache(maxsize=None)
def _env():
    return gc.env()


def _image_doubles(ld):
    return ld // 16 * (ld // 16 + 1) // 2 * 256


def _table_gram(F, k, w=None):
    """be.table_gram on host arrays: the image (device).  w None: the unweighted entry point."""
    torch, layout, be, dev = _env().short
    out = torch.full((_image_doubles(F.shape[1]),), float("nan"), dtype=torch.float64, device=dev)
    if w is None:
        be.table_gram(k, F.shape[1], gc.upload(F, dev), out)
    else:
        be.table_gram(k, F.shape[1], gc.upload(F, dev), out, w=gc.upload(w, dev))
    torch.cuda.synchronize()
    return out


def _table_gram_null_weights(F, k):
    """als_table_gram_weighted_f64 itself with w = NULL (the backend sends an unweighted call to the older entry)."""
    torch, layout, be, dev = _env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    ld = F.shape[1]
    out = torch.full((_image_doubles(ld),), float("nan"), dtype=torch.float64, device=dev)
    partials = torch.empty(int(lib.als_table_gram_partials()) * _image_doubles(ld), dtype=torch.float64, device=dev)
    Fd = gc.upload(F, dev)
    rc = lib.als_table_gram_weighted_f64(k, ld, F.shape[0], gc.ptr(Fd), None, gc.ptr(partials), gc.ptr(out),
                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    return out


# ---------------------------------------------------------------------------------------------------------
# weighted table Gram
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 17, 64, 160])
@pytest.mark.parametrize("nrows", [0, 1, 63, 1000])
def test_weighted_table_gram_matches_fp64(k, nrows):
    layout = _env().layout
    ld = layout.padded_k(k)
    rng = np.random.default_rng(1000 * k + nrows)
    F = np.full((max(nrows, 1), ld), 3.0, dtype=np.float32)         # padding columns hold garbage: they must not count
    F[:, :k] = rng.normal(scale=0.5, size=(max(nrows, 1), k))
    F = F[:nrows]
    w = rng.uniform(0.0, 3.0, size=nrows).astype(np.float32)
    F64, absF = F[:, :k].astype(np.float64), np.abs(F[:, :k].astype(np.float64))

    def check(img, w_ref, rows, what):
        G, padding = iref.gram_from_image(img.cpu().numpy(), k)
        assert not padding.any()                                    # the padding positions are exactly zero
        w64 = w_ref.astype(np.float64)
        bound = nrows * 2.0 ** -52 * ((absF[rows] * w64[rows, None]).T @ absF[rows])
        return gc.ratio(G, wref.table_gram(F64[rows], w64[rows]), bound, what)

    everything = np.arange(nrows)
    img = _table_gram(F, k, w)
    assert gc.same_bits(img.cpu(), _table_gram(F, k, w).cpu())      # two runs: the same bits
    worst = check(img, w, everything, "weighted table gram")
    # w = 1 (and w = NULL) give the bits of als_table_gram_f64
    plain = _table_gram(F, k)
    assert gc.same_bits(_table_gram(F, k, np.ones(nrows, np.float32)).cpu(), plain.cpu())
    assert gc.same_bits(_table_gram_null_weights(F, k).cpu(), plain.cpu())
    # w = 0 on a subset: the Gram with those rows deleted
    w0 = w.copy()
    w0[rng.random(nrows) < 0.4] = 0.0
    worst0 = check(_table_gram(F, k, w0), w0, np.nonzero(w0 > 0)[0], "weighted table gram, rows of weight 0 deleted")
    print(f"weighted table gram k={k} nrows={nrows}: {worst:.4f} and {worst0:.4f} of the bound")
    gc.record_margins(f"weighted_table_gram/k{k}/n{nrows}", {"all": worst, "zeroed": worst0})
    assert worst <= 1.0 and worst0 <= 1.0


# ---------------------------------------------------------------------------------------------------------
# row solve with a per-row scale of G: the rows of tests/test_gpu_implicit.py's side (0 ... 9000 entries: the task
# path and the split-row finish)
# ---------------------------------------------------------------------------------------------------------
LENS = (0, 1, 3, 63, 64, 65, 200, 4096, 4097, 9000)
NCOLS = 9100
LAM = 0.5
G_SCALE = 0.8


@functools.lru_cache(maxsize=None)
def _side():
    return gc.random_side(_env().layout, len(LENS), NCOLS, list(LENS), seed=5)


@functools.lru_cache(maxsize=None)
def _tables(k):
    """(F [NCOLS + 1, ld] with a zero last row, the weighted Gram image of a separate table T by the kernel, that G)."""
    layout = _env().layout
    ld = layout.padded_k(k)
    rng = np.random.default_rng(77 + k)
    F = gc.pad(rng.normal(scale=0.3, size=(NCOLS, k)).astype(np.float32), ld, extra_rows=1)
    T = gc.pad(rng.normal(scale=0.3, size=(500, k)).astype(np.float32), ld)
    img = _table_gram(T, k, rng.uniform(0.5, 1.5, size=500).astype(np.float32))
    G = iref.gram_from_image(img.cpu().numpy(), k)[0]
    return F, img, np.tril(G) + np.tril(G, -1).T


@functools.lru_cache(maxsize=None)
def _row_weights():
    rng = np.random.default_rng(9)
    a = rng.uniform(0.5, 5.0, size=_side().indices.size).astype(np.float32)
    scale = rng.uniform(0.25, 2.5, size=len(LENS)).astype(np.float32)
    return a, scale


def _solve(k, scale, rows=None):
    """One als_implicit_row_solve over the rows `rows` (None: all) of `_side()` with g_scale_row = scale (None: the
    field is NULL): (X [rows, ld], xb, status)."""
    e = _env()
    torch, layout, be, dev = e.short
    side = _side()
    F, img, _ = _tables(k)
    a, _ = _row_weights()
    ld = layout.padded_k(k)
    sd = e.side_dev(layout.SparseSide(side.nrows, side.ncols, side.indptr, side.indices, a), dev)
    if rows is None:
        tasks = layout.build_row_tasks(side.indptr, dual_len=0, mid_len=0)
    else:
        tasks = layout.build_row_tasks(side.indptr, rows[0], rows[0] + 1, dual_len=0, mid_len=0)
    X = torch.full((side.nrows, ld), float("nan"), dtype=torch.float32, device=dev)
    xb = torch.full((side.nrows,), float("nan"), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    kw = {} if scale is None else {"g_scale_row": gc.upload(scale, dev)}
    be.implicit_row_solve(k=k, ld=ld, side=sd, F=gc.upload(F, dev), zero_row=NCOLS, G=img, g_scale=G_SCALE, lam=LAM,
                          lam_row=None, X_out=X, xb_out=xb, status=status, tasks=e.tasks_dev(tasks, dev), **kw)
    torch.cuda.synchronize()
    return X.cpu().numpy(), xb.cpu().numpy(), int(status.item())


@pytest.mark.parametrize("k", [1, 17, 64, 65, 160])
def test_row_solve_with_a_row_scale_matches_fp64(k):
    side = _side()
    F, _, G = _tables(k)
    a, scale = _row_weights()
    X, xb, status = _solve(k, scale)
    assert status == 0
    assert not X[:, k:].any()
    a64 = a.astype(np.float64)
    worst_x = worst_xb = 0.0
    for r, n_r in enumerate(LENS):
        s = slice(side.indptr[r], side.indptr[r + 1])
        Fr = F[side.indices[s], :k].astype(np.float64)
        Gr = (G_SCALE * float(scale[r])) * G
        x, b = iref.row_solve(Fr, a64[s], 1.0 + a64[s], Gr, LAM)
        if n_r == 0:
            assert not X[r].any() and xb[r] == 0.0
            continue
        A = Gr + (Fr * a64[s][:, None]).T @ Fr + (LAM + iref.EPS) * np.eye(k)
        assert np.linalg.cond(A) < 1e6
        worst_x = max(worst_x, np.max(np.abs(X[r, :k] - x)) / (2.0 ** -23 * np.max(np.abs(x))))
        worst_xb = max(worst_xb, abs(xb[r] - x @ b) / (1e-12 * abs(x @ b)))
    print(f"row solve with g_scale_row k={k}: x {worst_x:.4f}, x.b {worst_xb:.4f} of the bound")
    gc.record_margins(f"implicit_row_solve_row_scale/k{k}", {"x": worst_x, "xb": worst_xb})
    assert worst_x <= 1.0 and worst_xb <= 1.0
    # the scale is in the comparison: without it the rows differ far beyond the tolerance
    X_null, _, _ = _solve(k, None)
    assert np.max(np.abs(X_null[1:, :k] - X[1:, :k])) > 1e-3 * np.max(np.abs(X[1:, :k]))


@pytest.mark.parametrize("k", [1, 17, 64, 65, 160])
def test_row_solve_unit_scale_and_launch_independence(k):
    """g_scale_row of ones: the bits of the NULL call.  A row alone or among the others: the same bits."""
    _, scale = _row_weights()
    X_null, xb_null, _ = _solve(k, None)
    X_one, xb_one, _ = _solve(k, np.ones(len(LENS), np.float32))
    assert gc.same_bits(X_null, X_one) and gc.same_bits(xb_null, xb_one)
    X, xb, _ = _solve(k, scale)
    for r in (LENS.index(65), LENS.index(4097), LENS.index(9000)):
        Xr, xbr, _ = _solve(k, scale, rows=(r,))
        assert gc.same_bits(X[r], Xr[r]) and xb[r] == xbr[r]
        others = [q for q, n_q in enumerate(LENS) if q != r and n_q > 0]
        assert np.isnan(Xr[others]).all()               # rows with entries that no task names: untouched


# ---------------------------------------------------------------------------------------------------------
# fit
# ---------------------------------------------------------------------------------------------------------
SHAPES = {"k20": (300, 200, 20, 4900), "k64": (200, 150, 64, 3400)}
ITERS, ALPHA, FIT_LAM = 8, 2.0, 0.5
WEIGHTINGS = ("popularity", "user", "both")


@functools.lru_cache(maxsize=None)
def _ratings(shape):
    m, n, k, nnz = SHAPES[shape]
    r, c, v = iref.zipf_counts(m, n, nnz, seed=31)
    csr, csc = _env().layout.coo_to_sides(r, c, v, (m, n))
    return (r, c, v), csr, csc


def _user_weights(m):
    return np.random.default_rng(17).uniform(0.5, 2.0, size=m).astype(np.float32)


def _model(shape, a0=1.0, **weights):
    from collaborative_filtering_amd import ALSConfig, CoreConfig, ImplicitALS, ImplicitConfig
    m, n, k, _ = SHAPES[shape]
    coo, _, _ = _ratings(shape)
    cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=ITERS, lambda_u=FIT_LAM, lambda_v=FIT_LAM, random_state=3))
    return ImplicitALS(cfg, ImplicitConfig(alpha=ALPHA, unobserved_weight=a0, **weights),
                       device="cuda:0").fit_coo(*coo, (m, n), tol=None, verbose=0)


@functools.lru_cache(maxsize=None)
def _fit(shape, weighting):
    """(fitted model, (U, V, losses) of the fp32-storage weighted reference, p, q)."""
    m, n, k, _ = SHAPES[shape]
    _, csr, csc = _ratings(shape)
    p = q = None
    kw = {}
    if weighting in ("popularity", "both"):
        kw.update(item_weight="popularity", popularity_exponent=0.5)
        q = wref.popularity_weights(np.diff(csc.indptr), 0.5)
    if weighting in ("user", "both"):
        p = _user_weights(m)
        kw.update(user_weight=p)
    model = _model(shape, **kw)
    ua, ia = iref.weights(csr.vals, ALPHA), iref.weights(csc.vals, ALPHA)
    ref = wref.fit(csr.indptr, csr.indices, ua, csc.indptr, csc.indices, ia, (m, n), k, ITERS, 1.0, FIT_LAM, FIT_LAM, 3,
                   p=p, q=q)
    return model, ref, p, q


@pytest.mark.parametrize("weighting", WEIGHTINGS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_weighted_fit_matches_the_fp32_storage_reference(shape, weighting):
    model, (U, V, losses), p, q = _fit(shape, weighting)
    m, n, _, _ = SHAPES[shape]
    du = np.max(np.abs(model.U - U)) / np.max(np.abs(U))
    dv = np.max(np.abs(model.V - V)) / np.max(np.abs(V))
    loss = np.asarray(model.history["loss"])
    dl = np.max(np.abs(loss - losses) / np.abs(losses))
    print(f"weighted implicit fit {shape} {weighting}: dU {du:.3e} dV {dv:.3e} dloss {dl:.3e}")
    gc.record_margins(f"implicit_weighted_fit/{shape}/{weighting}", {"dU": du, "dV": dv, "dloss": dl})
    assert du <= FIT_TOL and dv <= FIT_TOL
    assert dl <= 1e-12
    assert (np.diff(loss) <= 0).all()
    mp, mq = model.missing_weights()
    assert np.array_equal(mp, np.ones(m, np.float32) if p is None else p)
    assert np.array_equal(mq, np.ones(n, np.float32) if q is None else q)


# ---------------------------------------------------------------------------------------------------------
# exact ties to the unweighted path
# ---------------------------------------------------------------------------------------------------------
def _same_fit(a, b):
    return (gc.same_bits(a.U, b.U) and gc.same_bits(a.V, b.V)
            and gc.same_bits(np.asarray(a.history["loss"]), np.asarray(b.history["loss"])))


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_power_of_two_user_weight_is_the_unobserved_weight(shape):
    """p = 0.25 with a0 = 1 against the unweighted a0 = 0.25: a power-of-two scale is exact in every product and every
    sum (the U-step's per-row scale 1 * 0.25, the V-step's Gram of 0.25 u), so every bit agrees."""
    m = SHAPES[shape][0]
    weighted = _model(shape, a0=1.0, user_weight=np.full(m, 0.25))
    plain = _model(shape, a0=0.25)
    assert _same_fit(weighted, plain)
    assert len(plain.history["loss"]) == ITERS


@pytest.mark.parametrize("shape", list(SHAPES))
def test_popularity_exponent_zero_is_the_unweighted_fit(shape):
    """eta = 0: q = 1 through the weighted Gram and the per-row scale - the bits of the unweighted kernels."""
    n = SHAPES[shape][1]
    weighted = _model(shape, item_weight="popularity", popularity_exponent=0.0)
    assert np.array_equal(weighted.missing_weights()[1], np.ones(n, np.float32))
    assert _same_fit(weighted, _model(shape))


# ---------------------------------------------------------------------------------------------------------
# serving on a weighted fit
# ---------------------------------------------------------------------------------------------------------
def test_recommend_new_equals_a_reference_user_half_step_with_unit_user_weight():
    """As tests/test_gpu_implicit.py holds it for the unweighted model; a new user has p = 1, and the Gram is G_q."""
    model, _, p, q = _fit("k20", "both")
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
    X, _ = wref.half_step(ptr, idx, iref.weights(val, ALPHA), model.V, 1.0, FIT_LAM, w_table=q, w_rows=None)
    assert np.max(np.abs(Uf - X)) <= 2.0 ** -23 * np.max(np.abs(X)) and not bf.any()
    X_plain, _ = iref.half_step(ptr, idx, iref.weights(val, ALPHA), model.V, 1.0, FIT_LAM)
    assert np.max(np.abs(Uf - X_plain)) > 1e-3 * np.max(np.abs(X))      # G_q, not the unweighted Gram
    S = X.astype(np.float32).astype(np.float64) @ model.V.T
    tol = 2.0 ** -22 * np.max(np.abs(S))
    for b in range(users.size):
        seen = idx[ptr[b]:ptr[b + 1]]
        assert (items[b] >= 0).all() and not np.intersect1d(items[b], seen).size
        assert np.max(np.abs(scores[b] - S[b, items[b]])) <= tol
        rest = np.setdiff1d(np.arange(n), np.concatenate([seen, items[b]]))
        assert S[b, rest].max() <= scores[b, -1] + tol
        assert (np.diff(scores[b]) <= 0).all()
