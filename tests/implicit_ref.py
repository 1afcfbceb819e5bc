"""fp64 numpy definitions of the implicit-feedback model (ImplicitALS), written from its formulas - the reference of
the CPU stand-in and of the GPU kernel and fit tests.

    a = alpha r ("linear") | alpha log1p(r / eps) ("log"),  t = 1 + a
    loss = a0 sum_all (u.v)^2 + sum_obs [a (u.v)^2 - 2 t (u.v) + t] + lambda_u |U|^2 + lambda_v |V|^2
    half-step, per row:  A = a0 F^T F + sum_t a_t f_t f_t^T + (lambda + 1e-10) I,  b = sum_t t_t f_t,  x = A^-1 b
"""
import numpy as np

EPS = 1e-10
SCALE_FACTOR = 0.1


def weights(r, alpha, confidence="linear", eps=1.0):
    """The confidence weights a as the device stores them: evaluated in fp64, rounded once to fp32."""
    r = np.asarray(r, dtype=np.float64)
    a = alpha * (r if confidence == "linear" else np.log1p(r / eps))
    return a.astype(np.float32)


def table_gram(F):
    F = np.asarray(F, dtype=np.float64)
    return F.T @ F


def row_solve(Fr, a, t, G, lam):
    """x of one row: Fr [n_r, k] the gathered rows, a / t [n_r] the weights, G [k, k] the (scaled) all-entries Gram.
    Returns (x, b); a row without entries has x = 0."""
    k = G.shape[0]
    Fr = np.asarray(Fr, dtype=np.float64).reshape(-1, k)
    a, t = np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64)
    b = Fr.T @ t
    if Fr.shape[0] == 0:
        return np.zeros(k), b
    A = G + (Fr * a[:, None]).T @ Fr + (lam + EPS) * np.eye(k)
    L = np.linalg.cholesky(A)
    return np.linalg.solve(L.T, np.linalg.solve(L, b)), b


def half_step(ptr, idx, a, F, a0, lam, t=None):
    """All rows of one orientation against the table F [ncols, k]: (X [nrows, k], xb [nrows] = x.b per row)."""
    F = np.asarray(F, dtype=np.float64)
    G = a0 * table_gram(F)
    nrows, k = ptr.size - 1, F.shape[1]
    X, xb = np.zeros((nrows, k)), np.zeros(nrows)
    a64 = np.asarray(a, dtype=np.float64)
    t64 = 1.0 + a64 if t is None else np.asarray(t, dtype=np.float64)
    for r in range(nrows):
        s = slice(ptr[r], ptr[r + 1])
        X[r], b = row_solve(F[idx[s]], a64[s], t64[s], G, lam)
        xb[r] = X[r] @ b
    return X, xb


def loss_direct(uptr, uidx, a, U, V, a0, lam_u, lam_v):
    """The objective evaluated term by term; the all-entries term through the two Grams (tr(U^T U V^T V))."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    t = 1.0 + a
    rows = np.repeat(np.arange(uptr.size - 1), np.diff(uptr))
    p = np.einsum("ij,ij->i", U[rows], V[uidx])
    return (a0 * np.sum((U.T @ U) * (V.T @ V)) + np.sum(a * p * p - 2.0 * t * p + t)
            + lam_u * np.sum(U * U) + lam_v * np.sum(V * V))


def loss_dense(uptr, uidx, a, U, V, a0, lam_u, lam_v):
    """The objective with sum_all evaluated literally over the dense m x n matrix (small shapes only)."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    P = U @ V.T
    total = a0 * np.sum(P * P)
    for u in range(uptr.size - 1):
        for e in range(uptr[u], uptr[u + 1]):
            p, ae = P[u, uidx[e]], float(a[e])
            total += ae * p * p - 2.0 * (1.0 + ae) * p + (1.0 + ae)
    return total + lam_u * np.sum(U * U) + lam_v * np.sum(V * V)


def loss_closed(a, xb, U, V, lam_u):
    """The objective right after a V-step: sum_obs t - sum_i x_i.b_i - 1e-10 |V|^2 + lambda_u |U|^2.  A x = b for every
    item row, so the G, weighted and lambda_v terms add up to x.b less the 1e-10 that A carries on its diagonal beside
    lambda_v.  xb: the V-step's x.b per item; U: the table that V-step saw; V: its result."""
    U, V = np.asarray(U, dtype=np.float64), np.asarray(V, dtype=np.float64)
    return float(np.sum(1.0 + np.asarray(a, dtype=np.float64)) - np.sum(xb) - EPS * np.sum(V * V)
                 + lam_u * np.sum(U * U))


def init_tables(m, n, k, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(scale=SCALE_FACTOR, size=(m, k)), rng.normal(scale=SCALE_FACTOR, size=(n, k))


def fit(uptr, uidx, ua, iptr, iidx, ia, shape, k, n_iters, a0, lam_u, lam_v, seed, store_f32=True):
    """n_iters iterations (U-step, V-step, closed-form loss) from the seed's draws.  ua / ia: the weights in CSR / CSC
    order.  store_f32: U and V are rounded to fp32 after every half-step (and at the start) - the arithmetic the device
    performs.  Returns (U, V, losses)."""
    m, n = shape
    U, V = init_tables(m, n, k, seed)

    def store(X):
        return X.astype(np.float32).astype(np.float64) if store_f32 else X
    U, V = store(U), store(V)
    losses = []
    for _ in range(n_iters):
        U = store(half_step(uptr, uidx, ua, V, a0, lam_u)[0])
        X, xb = half_step(iptr, iidx, ia, U, a0, lam_v)
        V = store(X)
        losses.append(loss_closed(ia, xb, U, V, lam_u))
    return U, V, np.asarray(losses)


def zipf_counts(m, n, nnz_target, seed, max_count=19):
    """Zipf-ish rows: COO (rows, cols, integer counts 1 ... max_count) without duplicates."""
    rng = np.random.default_rng(seed)
    pu = 1.0 / np.arange(1, m + 1) ** 0.8
    pi = 1.0 / np.arange(1, n + 1) ** 0.8
    r = rng.choice(m, size=2 * nnz_target, p=pu / pu.sum())
    c = rng.choice(n, size=2 * nnz_target, p=pi / pi.sum())
    key = np.unique(r.astype(np.int64) * n + c)
    key = rng.permutation(key)[:nnz_target]
    key.sort()
    return key // n, key % n, rng.integers(1, max_count + 1, size=key.size).astype(np.float32)


# ---- the Gram image of als_table_gram_f64 (include/als_hip.h): lower 16 x 16 blocks in perm space ---------------
def _perm_cols(k):
    """(ld, col[p]: the factor column at perm position p)."""
    ld = (k + 15) // 16 * 16
    kb = ld // 16
    p = np.arange(ld)
    return ld, kb * (p & 15) + (p >> 4)


def gram_image(G, k):
    """The k x k matrix G as the kernels lay it out: block (I, K), K <= I, at 256 (I (I + 1) / 2 + K), row-major
    inside a block, positions of padding columns zero."""
    ld, col = _perm_cols(k)
    kb = ld // 16
    Gp = np.zeros((ld, ld))
    real = col < k
    Gp[np.ix_(real, real)] = np.asarray(G, dtype=np.float64)[np.ix_(col[real], col[real])]
    img = np.zeros(kb * (kb + 1) // 2 * 256)
    for I in range(kb):
        for K in range(I + 1):
            o = 256 * (I * (I + 1) // 2 + K)
            img[o:o + 256] = Gp[16 * I:16 * I + 16, 16 * K:16 * K + 16].reshape(-1)
    return img


def gram_from_image(img, k):
    """Inverse of `gram_image` (lower blocks mirrored): (G [k, k], the padding part of the image as a flat array)."""
    ld, col = _perm_cols(k)
    kb = ld // 16
    img = np.asarray(img, dtype=np.float64)
    Gp = np.zeros((ld, ld))
    for I in range(kb):
        for K in range(I + 1):
            o = 256 * (I * (I + 1) // 2 + K)
            B = img[o:o + 256].reshape(16, 16)
            Gp[16 * I:16 * I + 16, 16 * K:16 * K + 16] = B
            if K < I:
                Gp[16 * K:16 * K + 16, 16 * I:16 * I + 16] = B.T
    inv = np.empty(k, dtype=np.int64)
    real = col < k
    inv[col[real]] = np.nonzero(real)[0]
    pad = ~real
    padding = np.concatenate([Gp[pad].reshape(-1), Gp[:, pad].reshape(-1)])
    return Gp[np.ix_(inv, inv)], padding
