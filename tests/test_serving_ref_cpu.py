"""tests/serving_ref.py validated without a device: top-N and rank counts against brute-force statements of the
order, the two fold-ins against the half-steps of the oracle (oracle/als_oracle.py) applied to one new row or column,
the closed-form fixed point against the bordered (k + 1)-order system of include/als_hip.h, and the algebra the
contract of als_explain rests on."""
import numpy as np
import pytest

from oracle.als_oracle import EPS, OracleALS, OracleConfig, ratings_from_coo
from tests import serving_ref as ref


# ------------------------------------------------------------------------------------------ top-N, ranks
def _brute_top(P, seen, ok, N):
    """Dense oracle: the row with seen and disallowed columns masked, (score desc, id asc)."""
    keep = ok & ~np.isnan(P)
    keep[list(seen)] = False
    items = np.nonzero(keep)[0]
    return items[np.lexsort((items, -P[items]))][:N]


def _brute_rank(P, seen, u, t):
    """(rank, candidates) of item t for user u from the dense predictions, the seen items masked."""
    cand = ~np.isnan(P[u])
    cand[list(seen)] = False
    j = np.arange(P.shape[1])
    return int((cand & ((P[u] > P[u, t]) | ((P[u] == P[u, t]) & (j < t)))).sum()), int(cand.sum())


def _pairwise_top(row, seen, ok, N):
    """The order stated item by item, no sort key arithmetic: a precedes b when it scores higher, or equally with
    the lower id."""
    cand = [i for i in range(row.size) if ok[i] and i not in seen and row[i] == row[i]]
    ahead = {i: sum(1 for j in cand if row[j] > row[i] or (row[j] == row[i] and j < i)) for i in cand}
    return sorted(cand, key=ahead.get)[:N]


@pytest.fixture(scope="module")
def scores():
    """[12, 70] fp32: small integers (many ties), a NaN column, a NaN entry; seen rows; an allow mask."""
    rng = np.random.default_rng(0)
    P = rng.integers(-3, 4, size=(12, 70)).astype(np.float32)
    P[:, 5] = np.nan
    P[3, 40] = np.nan
    seen = [np.sort(rng.permutation(70)[: rng.integers(0, 30)]) for _ in range(12)]
    seen[0] = np.zeros(0, np.int64)
    seen[1] = np.setdiff1d(np.arange(70), [2, 5, 69])                    # all but three, one of them NaN
    return P, seen, rng.random(70) < 0.6


@pytest.mark.parametrize("masked", [False, True])
def test_topn_equals_the_brute_force_orders(scores, masked):
    P, seen, ok = scores
    allowed = ok if masked else None
    every = np.ones(70, bool)
    for N in (1, 7, 128):
        tv, ti, tc = ref.topn_batch(P, seen, allowed, N)
        assert tv.dtype == np.float32 and ti.dtype == np.int32 and tc.dtype == np.int32
        for u in range(12):
            want = _brute_top(P[u], seen[u], ok if masked else every, N)
            assert want.tolist() == _pairwise_top(P[u], set(seen[u].tolist()), ok if masked else every, N)
            v, i, c = ref.topn(P[u], seen[u], allowed, N)
            assert c == want.size == tc[u] and (i == want).all() and (v == P[u, want]).all()
            assert (ti[u, :c] == want).all() and (ti[u, c:] == -1).all()
            assert (tv[u, :c] == P[u, want]).all() and np.isneginf(tv[u, c:]).all()
    assert ref.topn_batch(P, seen, None, 10)[2][1] == 2                   # the NaN item is no candidate
    assert ref.topn(P[0], (), np.zeros(70, bool), 5)[2] == 0


@pytest.mark.parametrize("masked", [False, True])
def test_rank_counts_equal_the_brute_force_counts(scores, masked):
    P, seen, ok = scores
    Pm = P.copy()
    if masked:
        Pm[:, ~ok] = np.nan                                               # a disallowed item is no candidate either
    targets = np.arange(70)
    for u in range(12):
        t_score, above, n_cand = ref.rank_counts(P[u], seen[u], ok if masked else None, targets)
        assert above.dtype == np.int32
        for t in targets:
            if np.isnan(P[u, t]):
                assert above[t] == -1 and np.isnan(t_score[t])
                continue
            Pt = Pm.copy()
            Pt[u, t] = P[u, t]                                            # the target keeps its own score
            assert above[t] == _brute_rank(Pt, seen[u], u, t)[0]
            assert t_score[t] == P[u, t]
        assert n_cand == _brute_rank(Pm, seen[u], u, 0)[1]
        # position p of the list <-> rank p
        _, items, c = ref.topn(P[u], seen[u], ok if masked else None, 128)
        assert (ref.rank_counts(P[u], seen[u], ok if masked else None, items)[1] == np.arange(c)).all()
    q_ptr = np.array([0, 3, 3] + [5] * 10)
    q_items = np.array([4, 5, 4, 69, 0])
    sc, ab, nc = ref.rank_counts_batch(P, seen, None, q_ptr, q_items)
    assert ab[1] == -1 and ab[0] == ab[2] and nc[1] == 2 and sc.dtype == np.float32 and nc.dtype == np.int32


def test_bitmap_round_trip():
    rng = np.random.default_rng(1)
    for n in (1, 31, 32, 33, 70):
        mask = rng.random(n) < 0.5
        mask[n - 1] = True
        words = ref.bitmap_numpy(mask)
        assert words.size == (n + 31) // 32
        assert (ref.unpack_bitmap(words, n) == mask).all()
        assert (ref.unpack_bitmap(words.view(np.int32), n) == mask).all()


# ------------------------------------------------------------------------------------------ user fold-in
USER_CASES = [(3, 5.0), (12, 1e-2), (40, 0.5)]                            # the fixtures of tests/test_fold_in_cpu.py
K_USER, N_USER, LAM_BU = 8, 60, 2.0


def _user_case(n_rated, lam_u):
    rng = np.random.default_rng(n_rated)
    cols = np.sort(rng.permutation(N_USER)[:n_rated])
    vals = rng.integers(1, 11, n_rated) * 0.5
    rt = ratings_from_coo(np.zeros(n_rated, np.int64), cols, vals, (1, N_USER))
    o = OracleALS(OracleConfig(n_factors=K_USER, n_iters=1, lambda_u=lam_u, lambda_v=1.0, lambda_bu=LAM_BU,
                               lambda_bi=1.0))
    Z = rng.normal(size=(N_USER, K_USER))
    o.mu, o.b_i = 3.1, rng.normal(scale=0.3, size=N_USER)
    o.U, o.b_u = np.zeros((1, K_USER)), np.zeros(1)
    return o, rt, Z, cols, vals


@pytest.mark.parametrize("n_rated,lam_u", USER_CASES)
def test_fold_in_user_equals_the_user_half_step_applied_T_times(n_rated, lam_u):
    o, rt, Z, cols, vals = _user_case(n_rated, lam_u)
    want = {}
    for T in range(1, 6):
        o.user_step(rt, Z)
        want[T] = (o.U[0].copy(), o.b_u[0])
    for T in (1, 2, 5):
        u, b = ref.fold_in_user(Z, o.b_i, o.mu, lam_u, LAM_BU, cols, vals, K_USER, T)
        np.testing.assert_allclose(u, want[T][0], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(b, want[T][1], rtol=1e-10, atol=1e-12)
    for T in (0, 1, 4):                                                   # the empty row
        u, b = ref.fold_in_user(Z, o.b_i, o.mu, lam_u, LAM_BU, cols[:0], vals[:0], K_USER, T)
        assert (u == 0).all() and u.shape == (K_USER,) and b == 0.0


@pytest.mark.parametrize("n_rated,lam_u", USER_CASES)
def test_fold_in_user_converges_to_its_fixed_point(n_rated, lam_u):
    """The recurrence contracts by h.q / d < 1; on these fixtures 200 alternations are within 1e-9 of the limit."""
    o, _, Z, cols, vals = _user_case(n_rated, lam_u)
    u0, b0 = ref.fold_in_user(Z, o.b_i, o.mu, lam_u, LAM_BU, cols, vals, K_USER, 0)
    u, b = ref.fold_in_user(Z, o.b_i, o.mu, lam_u, LAM_BU, cols, vals, K_USER, 200)
    assert np.abs(u - u0).max() <= 1e-9 * max(1.0, np.abs(u0).max())
    assert abs(b - b0) <= 1e-9 * max(1.0, abs(b0))


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("n_rated,lam_u", USER_CASES)
def test_fold_in_user_fixed_point_equals_the_bordered_solve(n_rated, lam_u):
    o, _, Z, cols, vals = _user_case(n_rated, lam_u)
    u, b = ref.fold_in_user(Z, o.b_i, o.mu, lam_u, LAM_BU, cols, vals, K_USER, 0)
    x, bb = ref.bordered_fixed_point(*ref.user_system(Z, o.b_i, o.mu, lam_u, LAM_BU, cols, vals, K_USER)[:5])
    assert _rel(u, x) <= 1e-12 and _rel(b, bb) <= 1e-12


# ------------------------------------------------------------------------------------------ item fold-in
def _item_case(pop_reg, alpha, n_rated):
    k, m, n = 6, 50, 20                                  # n fitted items + the new column n
    rng = np.random.default_rng(n_rated + int(alpha * 10) + (pop_reg is not None))
    raters = np.sort(rng.permutation(m)[:n_rated])
    vals = rng.integers(1, 11, n_rated) * 0.5
    rt = ratings_from_coo(raters, np.full(n_rated, n), vals, (m, n + 1))
    o = OracleALS(OracleConfig(n_factors=k, n_iters=1, lambda_u=1.0, lambda_v=3.0, pop_reg_mode=pop_reg,
                               lambda_bu=1.0, lambda_bi=2.0, alpha=alpha, sim={"feature_name": "x", "topk": 5}))
    o.U, o.b_u, o.mu = rng.normal(size=(m, k)), rng.normal(scale=0.3, size=m), 3.2
    o.V = np.vstack([rng.normal(size=(n, k)), np.zeros((1, k))])
    o.b_i = np.zeros(n + 1)
    nb_idx = np.array([2, 5, 11, 17])
    nb_val = np.array([0.9, 0.4, 0.7, 0.05])
    ptr = np.zeros(n + 2, np.int64)
    ptr[n + 1] = nb_idx.size
    o.S_csr, o.use_graph = (ptr, nb_idx, nb_val), alpha > 0
    o.D = np.zeros(n + 1)
    o.D[n] = nb_val.sum()
    o.lambda_v_i = o.item_reg(np.full(n + 1, float(n_rated)))
    o.lambda_bi_i = np.full(n + 1, o.lambda_bi)
    args = (o.U, o.b_u, o.mu, o.V[:n], raters, vals, nb_idx, nb_val, 3.0, pop_reg is not None, 2.0, alpha)
    return o, rt, args, k, n, raters, vals, nb_idx, nb_val


@pytest.mark.parametrize("pop_reg", [None, "inverse_sqrt"])
@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("n_rated", [4, 30])
def test_recurrence_and_fixed_point_equal_the_item_half_step(pop_reg, alpha, n_rated):
    """T applications of OracleALS.item_step to a new column (its graph row, lambda_v_i and lambda_bi_i set as the
    fit would) equal the recurrence, and their limit is the bordered solve."""
    o, rt, args, k, n, raters, vals, nb_idx, nb_val = _item_case(pop_reg, alpha, n_rated)
    for T in range(1, 6):
        o.item_step(rt, cols=[n])
        v, b = ref.fold_in_item(*args, T)
        np.testing.assert_allclose(v, o.V[n], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(b, o.b_i[n], rtol=1e-10, atol=1e-12)
    v, b = ref.fold_in_item(*args, 0)
    lam = o.lambda_v_i[n] + EPS + alpha * o.D[n]
    Us = o.U[raters]
    M = np.block([[Us.T @ Us + lam * np.eye(k), Us.sum(axis=0)[:, None]],
                  [Us.sum(axis=0)[None, :], np.array([[n_rated + 2.0 + EPS]])]])
    rhs = np.append(Us.T @ (vals - o.mu - o.b_u[raters]) + alpha * (nb_val @ o.V[nb_idx]),
                    (vals - o.mu - o.b_u[raters]).sum())
    x = np.linalg.solve(M, rhs)
    np.testing.assert_allclose(v, x[:k], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(b, x[k], rtol=1e-10, atol=1e-12)
    for _ in range(300):
        o.item_step(rt, cols=[n])
    np.testing.assert_allclose(o.V[n], x[:k], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(o.b_i[n], x[k], rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize("pop_reg", [None, "inverse_sqrt"])
@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("n_rated", [4, 30])
def test_fold_in_item_fixed_point_equals_the_bordered_solve(pop_reg, alpha, n_rated):
    args = _item_case(pop_reg, alpha, n_rated)[2]
    v, b = ref.fold_in_item(*args, 0)
    x, bb = ref.bordered_fixed_point(*ref.item_system(*args))
    assert _rel(v, x) <= 1e-12 and _rel(b, bb) <= 1e-12


# ------------------------------------------------------------------------------------------ explain
@pytest.mark.parametrize("T", [None, 1, 3])
@pytest.mark.parametrize("lam_u", [5.0, 1e-4])
@pytest.mark.parametrize("k", [8, 64])
def test_contributions_sum_to_the_half_step_users_latent_score(k, lam_u, T):
    """(u, b_u) from OracleALS.user_step iterated T times (None: the bordered solve); with bprev the bias u was
    solved with, sum_j (z_i^T A^-1 z_j)(r_j - mu - b_i[j] - bprev) = u.z_i and 0 < z_i^T A^-1 z_i <= |z_i|^2 / lambda.
    Both sides are float64 solves against A, so they differ by a few cond(A) * 2^-52 (measured when the feature was
    specified: 2e-15 at lambda_u = 5, 2e-11 at lambda_u = 1e-4 with cond(A) ~ 1e5); the bound is 100 cond(A) 2^-52."""
    n = 6 * k
    rng = np.random.default_rng(k + (0 if T is None else T))
    Z = (rng.standard_normal((n, k)) * 0.3).astype(np.float32).astype(np.float64)
    b_i = (rng.standard_normal(n) * 0.2).astype(np.float32).astype(np.float64)
    mu, lam_bu = 3.4, 3.0
    lam = lam_u + EPS
    for nr in (0, 1, k // 2, k, 5 * k):
        cols = np.sort(rng.permutation(n)[:nr])
        vals = rng.integers(1, 11, nr) * 0.5
        targets = rng.permutation(n)[:6]
        if nr == 0:                                           # no ratings: u = 0, leverage |z_i|^2 / lambda
            for i in targets:
                assert np.isclose(Z[i] @ np.linalg.solve(lam * np.eye(k), Z[i]), Z[i] @ Z[i] / lam, rtol=1e-14)
            continue
        Zs = Z[cols]
        res = vals - mu - b_i[cols]
        A = Zs.T @ Zs + lam * np.eye(k)
        if T is None:
            h = Zs.sum(axis=0)
            Mb = np.block([[A, h[:, None]], [h[None, :], np.array([[nr + lam_bu + EPS]])]])
            x = np.linalg.solve(Mb, np.append(Zs.T @ res, res.sum()))
            u, bprev = x[:k], x[k]
        else:
            o = OracleALS(OracleConfig(n_factors=k, n_iters=1, lambda_u=lam_u, lambda_v=1.0, lambda_bu=lam_bu,
                                       lambda_bi=1.0))
            o.mu, o.b_i = mu, b_i
            o.U, o.b_u = np.zeros((1, k)), np.zeros(1)
            rt = ratings_from_coo(np.zeros(nr, np.int64), cols, vals, (1, n))
            for _ in range(T):
                bprev = o.b_u[0]
                o.user_step(rt, Z)
            u = o.U[0]
        rho = res - bprev
        bound = 100 * np.linalg.cond(A) * 2.0 ** -52
        for i in targets:
            w = np.linalg.solve(A, Z[i])
            contrib = (Zs @ w) * rho
            assert abs(contrib.sum() - u @ Z[i]) <= bound * max(1.0, abs(u @ Z[i])), (nr, i)
            lev = w @ Z[i]
            assert 0 < lev <= Z[i] @ Z[i] / lam * (1 + bound)


@pytest.mark.parametrize("T", [None, 1, 3])
@pytest.mark.parametrize("lam_u", [5.0, 1e-4])
@pytest.mark.parametrize("k", [8, 64])
def test_explain_fixed_point_equals_the_bordered_solve_and_its_parts_agree(k, lam_u, T):
    """On the data of the test above (T only seeds it): b_u and latent of the fixed point against the bordered solve,
    to 1e-12 at lambda_u = 5.  At lambda_u = 1e-4 cond(A) reaches 1e5 and two float64 solves of one system differ by
    cond(A) 2^-52 whichever is taken (observed 3.9e-11), so the bound there is that test's 100 cond(A) 2^-52."""
    n = 6 * k
    rng = np.random.default_rng(k + (0 if T is None else T))
    Z = (rng.standard_normal((n, k)) * 0.3).astype(np.float32).astype(np.float64)
    b_i = (rng.standard_normal(n) * 0.2).astype(np.float32).astype(np.float64)
    mu, lam_bu = 3.4, 3.0
    for nr in (0, 1, k // 2, k, 5 * k):
        cols = np.sort(rng.permutation(n)[:nr]).astype(np.int32)
        vals = rng.integers(1, 11, nr) * 0.5
        targets = rng.permutation(n)[:6]
        row = ref.explain_row(Z, b_i, mu, lam_u, lam_bu, cols, vals, k, 0, targets)
        if nr == 0:
            assert row["b_u"] == 0.0 and (row["latent"] == 0).all() and row["contrib"].shape == (6, 0)
            continue
        x, bb = ref.bordered_fixed_point(*ref.user_system(Z, b_i, mu, lam_u, lam_bu, cols, vals, k)[:5])
        bound = 1e-12 if lam_u == 5.0 else 100 * row["cond"] * 2.0 ** -52
        assert _rel(row["b_u"], bb) <= bound and _rel(row["latent"], Z[targets] @ x) <= bound, (nr, row["cond"])
        assert row["b_u"] == ref.fold_in_user(Z, b_i, mu, lam_u, lam_bu, cols, vals, k, 0)[1]    # one fixed point
        for largest, T_pair in ((True, 0), (False, 2)):
            e = ref.explain_pair(Z, b_i, mu, lam_u, lam_bu, cols, vals, k, T_pair, int(targets[1]), 5, largest)
            one = ref.explain_row(Z, b_i, mu, lam_u, lam_bu, cols, vals, k, T_pair, targets[1:2])
            assert e["b_u"] == one["b_u"] and e["score"] == mu + e["b_u"] + b_i[targets[1]] + e["latent"]
            pos = np.searchsorted(cols, e["items"])
            assert (e["contributions"] == one["contrib"][0][pos]).all()
            assert (e["weights"] == one["weights"][0][pos]).all()
            step = np.diff(e["contributions"].astype(np.float32))
            assert e["items"].size == min(5, nr) and ((step <= 0) if largest else (step >= 0)).all()
