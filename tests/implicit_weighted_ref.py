"""fp64 numpy definitions of the implicit-feedback model with rank-one weights p_u q_i on the unobserved entries
(ImplicitConfig.user_weight / item_weight), written from its formulas on top of
tests/implicit_ref.py - the reference of the weighted CPU stand-in and of the GPU kernel and fit tests.

    loss = a0 sum_all p_u q_i (u.v)^2 + sum_obs [a (u.v)^2 - 2 t (u.v) + t] + lambda_u |U|^2 + lambda_v |V|^2
    U-step, user u:  A = (a0 p_u) G_q + sum_t a_t v_t v_t^T + (lambda_u + 1e-10) I,   G_q = sum_i q_i v_i v_i^T
    V-step, item i:  A = (a0 q_i) G_p + sum_t a_t u_t u_t^T + (lambda_v + 1e-10) I,   G_p = sum_u p_u u_u u_u^T
    b = sum_t t_t f_t and x = A^-1 b as in the unweighted model; p = q = 1 is that model.

p and q are the fp32 values the device holds, widened to fp64 here.
"""
import numpy as np

from tests import implicit_ref as iref

EPS = iref.EPS
loss_closed = iref.loss_closed          # holds unchanged: A x = b for every item row after the V-step


def table_gram(F, w=None):
    """sum_r w_r f_r f_r^T (w None: every w_r = 1), symmetric bit for bit (the lower triangle mirrored)."""
    F = np.asarray(F, dtype=np.float64)
    if w is None:
        return iref.table_gram(F)
    G = (F * np.asarray(w, dtype=np.float64)[:, None]).T @ F
    return np.tril(G) + np.tril(G, -1).T


def popularity_weights(counts, exponent):
    """q_i = n f_i^eta / sum_j f_j^eta in fp64, rounded once to fp32 (mean 1); 0^0 = 1; all ones without entries."""
    f = np.asarray(counts, dtype=np.float64)
    w = f ** float(exponent)
    total = w.sum()
    if not total > 0:
        return np.ones(f.size, dtype=np.float32)
    return ((f.size * w) / total).astype(np.float32)


def half_step(ptr, idx, a, F, a0, lam, w_table=None, w_rows=None, t=None):
    """All rows of one orientation against the table F [ncols, k], whose rows weigh w_table in the Gram; row r takes
    that Gram times a0 w_rows[r].  Returns (X [nrows, k], xb [nrows] = x.b per row)."""
    F = np.asarray(F, dtype=np.float64)
    G = table_gram(F, w_table)
    nrows, k = ptr.size - 1, F.shape[1]
    X, xb = np.zeros((nrows, k)), np.zeros(nrows)
    a64 = np.asarray(a, dtype=np.float64)
    t64 = 1.0 + a64 if t is None else np.asarray(t, dtype=np.float64)
    for r in range(nrows):
        s = slice(ptr[r], ptr[r + 1])
        scale = a0 if w_rows is None else a0 * float(w_rows[r])
        X[r], b = iref.row_solve(F[idx[s]], a64[s], t64[s], scale * G, lam)
        xb[r] = X[r] @ b
    return X, xb


def loss_dense(uptr, uidx, a, U, V, a0, lam_u, lam_v, p=None, q=None):
    """The objective with a0 sum_all p_u q_i (u.v)^2 evaluated literally on the dense m x n product."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    p = np.ones(U.shape[0]) if p is None else np.asarray(p, dtype=np.float64)
    q = np.ones(V.shape[0]) if q is None else np.asarray(q, dtype=np.float64)
    P = U @ V.T
    rest = iref.loss_dense(uptr, uidx, a, U, V, 0.0, lam_u, lam_v)       # the observed and the lambda terms
    return a0 * np.sum(p[:, None] * q[None, :] * P * P) + rest


def fit(uptr, uidx, ua, iptr, iidx, ia, shape, k, n_iters, a0, lam_u, lam_v, seed, p=None, q=None, store_f32=True,
        trace=None):
    """`implicit_ref.fit` with the weights: n_iters iterations (U-step, V-step, closed-form loss) from the seed's draws,
    U and V rounded to fp32 after every half-step when store_f32.  Returns (U, V, losses).  trace: a list that
    receives (U, xb, V) of every iteration - the terms of that iteration's closed-form loss."""
    m, n = shape
    U, V = iref.init_tables(m, n, k, seed)

    def store(X):
        return X.astype(np.float32).astype(np.float64) if store_f32 else X
    U, V = store(U), store(V)
    losses = []
    for _ in range(n_iters):
        U = store(half_step(uptr, uidx, ua, V, a0, lam_u, w_table=q, w_rows=p)[0])
        X, xb = half_step(iptr, iidx, ia, U, a0, lam_v, w_table=p, w_rows=q)
        V = store(X)
        losses.append(loss_closed(ia, xb, U, V, lam_u))
        if trace is not None:
            trace.append((U, xb, V))
    return U, V, np.asarray(losses)
