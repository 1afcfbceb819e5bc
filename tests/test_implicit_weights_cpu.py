"""The weights p_u q_i on the unobserved entries of ImplicitALS (`user_weight`, `item_weight`)
without a GPU: the weighted numpy reference (tests/implicit_weighted_ref.py) against the dense loss, the popularity
weights, and the engine / facade end to end on the weighted numpy stand-in."""
import numpy as np
import pytest

from collaborative_filtering_amd import ALSConfig, CoreConfig, ImplicitALS, ImplicitConfig, layout
from collaborative_filtering_amd import implicit as implicit_mod
from tests import implicit_ref as iref
from tests import implicit_weighted_ref as wref
from tests.implicit_cpu_backend import ImplicitNumpyBackend
from tests.implicit_weighted_cpu_backend import WeightedImplicitNumpyBackend

ALPHA = 2.0


def _sides(m, n, nnz, seed):
    r, c, v = iref.zipf_counts(m, n, nnz, seed)
    csr, csc = layout.coo_to_sides(r, c, v, (m, n))
    return (r, c, v), csr, csc


def _cfg(k, n_iters, lam_u=0.5, lam_v=0.5, **core):
    return ALSConfig(core=CoreConfig(n_factors=k, n_iters=n_iters, lambda_u=lam_u, lambda_v=lam_v, **core))


def _random_weights(size, seed, zeros=0):
    """fp32 weights in [0.25, 3], `zeros` of them exactly 0 (a user / item the all-entries term leaves out)."""
    rng = np.random.default_rng(seed)
    w = rng.uniform(0.25, 3.0, size=size).astype(np.float32)
    w[rng.choice(size, size=zeros, replace=False)] = 0.0
    return w


# ---------------------------------------------------------------------------------------------------------
# the reference itself
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m, n, k, nnz", [(40, 30, 8, 300), (200, 150, 64, 3400)])
def test_closed_form_loss_equals_the_dense_loss(m, n, k, nnz):
    """As tests/test_implicit_cpu.py holds it for the unweighted model: the gap is second order in the 2^-24 rounding
    of V.  sum_all is evaluated literally, entry by entry of the dense m x n product."""
    a0, lam_u, lam_v = 0.7, 0.5, 0.4
    _, csr, csc = _sides(m, n, nnz, 2)
    ua, ia = iref.weights(csr.vals, ALPHA), iref.weights(csc.vals, ALPHA)
    p, q = _random_weights(m, 21, zeros=3), _random_weights(n, 22, zeros=2)
    U, _ = iref.init_tables(m, n, k, 5)
    U = U.astype(np.float32).astype(np.float64)
    X, xb = wref.half_step(csc.indptr, csc.indices, ia, U, a0, lam_v, w_table=p, w_rows=q)
    V = X.astype(np.float32).astype(np.float64)
    closed = wref.loss_closed(ia, xb, U, V, lam_u)
    dense = wref.loss_dense(csr.indptr, csr.indices, ua, U, V, a0, lam_u, lam_v, p, q)
    print(f"closed-form loss {m} x {n}, k = {k}: relative gap {abs(closed - dense) / abs(dense):.3e}")
    assert abs(closed - dense) <= 1e-10 * abs(dense)
    # the weights are in the comparison: the unweighted dense loss is another number
    assert abs(closed - wref.loss_dense(csr.indptr, csr.indices, ua, U, V, a0, lam_u, lam_v)) > 1e-4 * abs(dense)


def test_reference_with_unit_weights_is_the_unweighted_reference():
    m, n, k = 40, 30, 8
    _, csr, csc = _sides(m, n, 300, 1)
    ua, ia = iref.weights(csr.vals, ALPHA), iref.weights(csc.vals, ALPHA)
    args = (csr.indptr, csr.indices, ua, csc.indptr, csc.indices, ia, (m, n), k, 3, 0.7, 0.3, 0.4, 9)
    U, V, losses = iref.fit(*args)
    U1, V1, losses1 = wref.fit(*args)
    assert np.array_equal(U, U1) and np.array_equal(V, V1) and np.array_equal(losses, losses1)
    one_p, one_q = np.ones(m, np.float32), np.ones(n, np.float32)
    U2, V2, losses2 = wref.fit(*args, p=one_p, q=one_q)
    np.testing.assert_allclose(U2, U, rtol=0, atol=1e-12)
    np.testing.assert_allclose(losses2, losses, rtol=1e-12)


def test_reference_loss_does_not_increase():
    m, n, k = 60, 40, 8
    _, csr, csc = _sides(m, n, 500, 4)
    ua, ia = iref.weights(csr.vals, ALPHA), iref.weights(csc.vals, ALPHA)
    p, q = _random_weights(m, 31, zeros=2), wref.popularity_weights(np.diff(csc.indptr), 0.5)
    for store_f32 in (False, True):
        _, _, losses = wref.fit(csr.indptr, csr.indices, ua, csc.indptr, csc.indices, ia, (m, n), k, 6, 1.0, 0.5, 0.5, 3,
                                p=p, q=q, store_f32=store_f32)
        assert losses.shape == (6,) and (np.diff(losses) <= 0).all()


# ---------------------------------------------------------------------------------------------------------
# popularity weights
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [wref.popularity_weights, implicit_mod.popularity_weights])
def test_popularity_weights(weights):
    counts = np.array([0, 1, 1, 4, 9, 100, 0, 2500, 3], dtype=np.int64)
    for eta in (0.25, 0.5, 1.0, 2.0):
        q = weights(counts, eta)
        assert q.dtype == np.float32 and q.shape == counts.shape
        assert abs(q.astype(np.float64).mean() - 1.0) <= 2.0 ** -23        # one fp32 rounding (2^-24) per value
        assert not q[counts == 0].any() and (q[counts > 0] > 0).all()
        order = np.argsort(counts, kind="stable")
        assert (np.diff(q[order]) >= 0).all()                                         # monotone in the counts
        assert q[1] == q[2]
        f = counts.astype(np.float64) ** eta
        assert np.array_equal(q, (counts.size * f / f.sum()).astype(np.float32))
    assert np.array_equal(weights(counts, 0.0), np.ones(counts.size, np.float32))      # 0^0 = 1: uniform
    assert np.array_equal(weights(np.zeros(5, np.int64), 0.5), np.ones(5, np.float32))  # no entries at all
    assert weights(np.zeros(0, np.int64), 0.5).shape == (0,)


# ---------------------------------------------------------------------------------------------------------
# the engine on the stand-in
# ---------------------------------------------------------------------------------------------------------
M, N, K, ITERS, A0, LAM = 120, 80, 12, 4, 0.6, 0.5
WEIGHTINGS = ("popularity", "arrays", "user_only")


def _weighting(name, csc):
    """(ImplicitConfig keywords, p, q as the reference takes them)."""
    if name == "popularity":
        return dict(item_weight="popularity", popularity_exponent=0.75), None, wref.popularity_weights(
            np.diff(csc.indptr), 0.75)
    if name == "arrays":
        p, q = _random_weights(M, 41, zeros=4), _random_weights(N, 42, zeros=3)
        return dict(user_weight=p.astype(np.float64), item_weight=list(q)), p, q
    p = _random_weights(M, 43)
    return dict(user_weight=p), p, None


@pytest.fixture(scope="module")
def data():
    return _sides(M, N, 1500, 11)


@pytest.fixture(scope="module", params=WEIGHTINGS)
def fitted(request, data):
    coo, csr, csc = data
    kw, p, q = _weighting(request.param, csc)
    icfg = ImplicitConfig(alpha=ALPHA, unobserved_weight=A0, **kw)
    model = ImplicitALS(_cfg(K, ITERS, LAM, LAM, random_state=7), icfg, backend=WeightedImplicitNumpyBackend(),
                        device="cpu")
    model.fit_coo(*coo, (M, N), tol=None, verbose=0)
    ua, ia = iref.weights(csr.vals, ALPHA), iref.weights(csc.vals, ALPHA)
    trace = []
    U, V, losses = wref.fit(csr.indptr, csr.indices, ua, csc.indptr, csc.indices, ia, (M, N), K, ITERS, A0, LAM, LAM, 7,
                            p=p, q=q, trace=trace)
    return model, (U, V, losses, trace), p, q


def _loss_summed_as_the_engine_sums(ua, U, xb, V, lam_u):
    """The reference's closed-form loss of one iteration, sum_obs t - sum x.b - 1e-10 |V|^2 + lambda_u |U|^2, from the
    reference's own terms, each sum taken the way `_ImplicitEngine.loss_step` and the stand-in's `sumsq` take it (torch
    on the [rows, ld] fp32 tables) - `implicit_ref.loss_closed` adds the same terms with numpy's sums, whose last bit
    may differ."""
    import torch
    ld = layout.padded_k(K)

    def sumsq(X):
        P = torch.zeros(X.shape[0], ld, dtype=torch.float32)
        P[:, :K] = torch.from_numpy(X.astype(np.float32))
        return float((P.double() ** 2).sum())
    sum_t = float(ua.size + torch.from_numpy(ua).to(torch.float64).sum().item())
    return float(sum_t - torch.from_numpy(xb).sum() - wref.EPS * sumsq(V) + lam_u * sumsq(U))


def test_fit_equals_the_weighted_reference(fitted, data):
    """The stand-in and the reference run the same numpy text on the same fp32-rounded operands: U, V and the loss of
    every iteration agree in every bit (the loss with the reference's terms summed in the engine's order)."""
    model, (U, V, losses, trace), _, _ = fitted
    _, csr, _ = data
    assert np.array_equal(model.U, U) and np.array_equal(model.V, V)
    loss = np.asarray(model.history["loss"])
    assert loss.shape == (ITERS,)
    ua = iref.weights(csr.vals, ALPHA)
    exact = np.array([_loss_summed_as_the_engine_sums(ua, Ui, xb, Vi, LAM) for Ui, xb, Vi in trace])
    assert np.array_equal(loss, exact)
    # and numpy's sums of the same terms (implicit_ref.loss_closed) agree to the rounding of a sum: relative 1e-14
    assert np.max(np.abs(loss - losses) / np.abs(losses)) <= 1e-14
    assert (np.diff(loss) <= 0).all()


def test_weights_change_the_fit(fitted, data):
    model, _, _, _ = fitted
    coo, _, _ = data
    plain = ImplicitALS(_cfg(K, ITERS, LAM, LAM, random_state=7), ImplicitConfig(alpha=ALPHA, unobserved_weight=A0),
                        backend=ImplicitNumpyBackend(), device="cpu").fit_coo(*coo, (M, N), tol=None, verbose=0)
    assert np.max(np.abs(plain.U - model.U)) > 1e-3 * np.max(np.abs(plain.U))


def test_missing_weights_returns_what_the_fit_used(fitted):
    model, _, p, q = fitted
    mp, mq = model.missing_weights()
    assert mp.dtype == mq.dtype == np.float32 and mp.shape == (M,) and mq.shape == (N,)
    assert np.array_equal(mp, np.ones(M, np.float32) if p is None else p)
    assert np.array_equal(mq, np.ones(N, np.float32) if q is None else q)


def test_popularity_counts_come_from_tensor_sides_too(data):
    """`fit_csr` with torch tensors (how a caller hands over device-resident sides): the same q as from numpy sides."""
    import torch
    _, csr, csc = data
    icfg = ImplicitConfig(alpha=ALPHA, item_weight="popularity")
    model = ImplicitALS(_cfg(4, 1), icfg, backend=WeightedImplicitNumpyBackend(), device="cpu")
    sides = [tuple(torch.from_numpy(x) for x in (s.indptr, s.indices, s.vals)) for s in (csr, csc)]
    model.fit_csr(sides[0], sides[1], (M, N), tol=None, verbose=0)
    assert np.array_equal(model.missing_weights()[1], wref.popularity_weights(np.diff(csc.indptr), 0.5))


def test_missing_weights_of_an_unweighted_model_are_ones(data):
    coo, _, _ = data
    model = ImplicitALS(_cfg(4, 1), ImplicitConfig(alpha=ALPHA), backend=ImplicitNumpyBackend(), device="cpu")
    with pytest.raises(RuntimeError):
        model.missing_weights()
    model.fit_coo(*coo, (M, N), tol=None, verbose=0)
    p, q = model.missing_weights()
    assert np.array_equal(p, np.ones(M, np.float32)) and np.array_equal(q, np.ones(N, np.float32))


class _Recording(WeightedImplicitNumpyBackend):
    """Records the keywords of every Gram and row-solve call."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def table_gram(self, *args, **kw):
        self.calls.append(("table_gram", len(args), tuple(sorted(kw))))
        return super().table_gram(*args, **kw)

    def implicit_row_solve(self, **kw):
        self.calls.append(("implicit_row_solve", 0, tuple(sorted(kw))))
        return super().implicit_row_solve(**kw)


def _row_of(csr, u):
    s = slice(csr.indptr[u], csr.indptr[u + 1])
    R = np.full((1, N), np.nan)
    R[0, csr.indices[s]] = csr.vals[s]
    return R


def test_an_unweighted_model_makes_no_call_with_the_new_keywords(data):
    """Fit and fold-in of a model without weights: positional Gram arguments and keyword sets exactly as before the
    options existed (tests/implicit_cpu_backend.py, whose methods do not take `w` / `g_scale_row`, keeps working)."""
    coo, csr, _ = data
    be = _Recording()
    model = ImplicitALS(_cfg(6, 2), ImplicitConfig(alpha=ALPHA), backend=be, device="cpu")
    model.fit_coo(*coo, (M, N), tol=None, verbose=0)
    model.fold_in(_row_of(csr, 3))
    solve_kw = tuple(sorted(("k", "ld", "side", "F", "zero_row", "G", "g_scale", "lam", "lam_row", "X_out", "xb_out",
                             "status", "tasks")))
    assert {c for c in be.calls if c[0] == "table_gram"} == {("table_gram", 4, ())}
    assert {c for c in be.calls if c[0] == "implicit_row_solve"} == {("implicit_row_solve", 0, solve_kw)}
    assert len(be.calls) == 2 * 2 * 2 + 2


def test_a_weighted_model_passes_each_keyword_only_where_its_weights_are_set(data):
    coo, csr, _ = data
    be = _Recording()
    model = ImplicitALS(_cfg(6, 1), ImplicitConfig(alpha=ALPHA, user_weight=_random_weights(M, 5)), backend=be,
                        device="cpu")
    model.fit_coo(*coo, (M, N), tol=None, verbose=0)
    model.fold_in(_row_of(csr, 3))
    kinds = [(name, "w" in kw, "g_scale_row" in kw) for name, _, kw in be.calls]
    # U-step: Gram of V unweighted (q unset), rows scaled by p; V-step: Gram of U weighted by p, rows unscaled;
    # fold-in: a new user has p = 1 and q is unset
    assert kinds == [("table_gram", False, False), ("implicit_row_solve", False, True),
                     ("table_gram", True, False), ("implicit_row_solve", False, False),
                     ("table_gram", False, False), ("implicit_row_solve", False, False)]


# ---------------------------------------------------------------------------------------------------------
# fold-in
# ---------------------------------------------------------------------------------------------------------
def test_fold_in_is_a_user_half_step_with_unit_user_weight(fitted, data):
    """A training user's own row, folded in: the reference U-step row against the fitted V with G_q and p = 1 (not the
    user's own p_u: a new user has none)."""
    model, _, p, q = fitted
    _, csr, _ = data
    users = np.array([0, 3, 50, M - 1])
    R_new = np.concatenate([_row_of(csr, u) for u in users])
    Un, bn = model.fold_in(R_new)
    lens = [csr.indptr[u + 1] - csr.indptr[u] for u in users]
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = np.concatenate([csr.indices[csr.indptr[u]:csr.indptr[u + 1]] for u in users])
    a = iref.weights(np.concatenate([csr.vals[csr.indptr[u]:csr.indptr[u + 1]] for u in users]), ALPHA)
    X, _ = wref.half_step(ptr, idx, a, model.V, A0, LAM, w_table=q, w_rows=None)
    assert np.max(np.abs(Un - X)) <= 2.0 ** -23 * np.max(np.abs(X)) and not bn.any()
    if q is not None:       # the weighted Gram is what was used: the unweighted one gives another row
        X1, _ = wref.half_step(ptr, idx, a, model.V, A0, LAM)
        assert np.max(np.abs(Un - X1)) > 1e-3 * np.max(np.abs(X))
    items, _ = model.recommend_new(R_new[:2], N=5)
    assert not np.intersect1d(items[0], csr.indices[csr.indptr[0]:csr.indptr[1]]).size


# ---------------------------------------------------------------------------------------------------------
# validation
# ---------------------------------------------------------------------------------------------------------
def _model(icfg):
    return ImplicitALS(_cfg(4, 1), icfg, backend=WeightedImplicitNumpyBackend(), device="cpu")


@pytest.mark.parametrize("kw", [dict(item_weight="inverse"), dict(item_weight=""), dict(popularity_exponent=-0.5),
                                dict(popularity_exponent=np.nan), dict(popularity_exponent=np.inf),
                                dict(item_weight="popularity", popularity_exponent=-1.0)])
def test_bad_weight_options_raise_in_the_constructor(kw):
    with pytest.raises(ValueError):
        _model(ImplicitConfig(**kw))


def _bad(size, value):
    w = np.ones(size)
    w[size // 2] = value
    return w


@pytest.mark.parametrize("kw", [dict(item_weight=np.ones(N + 1)), dict(item_weight=np.ones(N - 1)),
                                dict(item_weight=np.ones((N, 1))), dict(user_weight=np.ones(M + 1)),
                                dict(user_weight=np.ones(N)), dict(item_weight=_bad(N, -1e-3)),
                                dict(item_weight=_bad(N, np.nan)), dict(item_weight=_bad(N, np.inf)),
                                dict(user_weight=_bad(M, -1.0)), dict(user_weight=_bad(M, np.nan)),
                                dict(user_weight=_bad(M, np.inf)), dict(user_weight=_bad(M, 1e300))])
def test_bad_weight_arrays_raise_at_fit(kw, data):
    coo, _, _ = data
    model = _model(ImplicitConfig(alpha=ALPHA, **kw))            # the length is only known at fit
    with pytest.raises(ValueError):
        model.fit_coo(*coo, (M, N), tol=None, verbose=0)


def test_zero_weights_are_accepted(data):
    """p = q = 0 takes the all-entries term out: every row solves its own entries with lambda alone."""
    coo, csr, csc = data
    model = _model(ImplicitConfig(alpha=ALPHA, user_weight=np.zeros(M), item_weight=np.zeros(N)))
    model.fit_coo(*coo, (M, N), tol=None, verbose=0)
    ua, ia = iref.weights(csr.vals, ALPHA), iref.weights(csc.vals, ALPHA)
    U, V, _ = iref.fit(csr.indptr, csr.indices, ua, csc.indptr, csc.indices, ia, (M, N), 4, 1, 0.0, 0.5, 0.5, 42)
    np.testing.assert_allclose(model.U, U, rtol=0, atol=1e-6 * np.max(np.abs(U)))
    np.testing.assert_allclose(model.V, V, rtol=0, atol=1e-6 * np.max(np.abs(V)))
