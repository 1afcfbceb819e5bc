"""The contracts of the serving kernels, once, in float64 numpy: als_recommend_topk[_masked] (`topn`),
als_rank_count[_masked] (`rank_counts`), als_fold_in (`fold_in_user`), als_fold_in_items (`fold_in_item`) and
als_explain (`explain_row`, `explain_pair`), as include/als_hip.h documents them.

Both suites read this text: tests/cpu_backend.py adapts it to the engine's backend interface (the stand-in the host
orchestration is tested on), and the tests/test_gpu_*.py modules of these kernels hold the kernels to it.  It is
validated without a device by tests/test_serving_ref_cpu.py.  No torch, no product import.

Parameters (lambdas, alpha) are taken as given: a caller that checks a kernel passes them fp32-rounded, as the kernel
reads them.  The fixed point of the two fold-ins is the closed form b = (s - h.p) / (d - h.q) of the bordered
(k + 1)-order system (`bordered_fixed_point` solves that system directly; the CPU test asserts they agree)."""
import numpy as np

EPS = 1e-10


# ------------------------------------------------------------------------------------------ bitmaps
def bitmap_numpy(mask):
    """The C ABI's definition, item by item: bit i & 31 of word i >> 5, uint32 words, ceil(n / 32) of them."""
    words = np.zeros((mask.size + 31) // 32, dtype=np.uint32)
    for i in np.nonzero(mask)[0]:
        words[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return words


def unpack_bitmap(words, n):
    """bool [n] from the words of `bitmap_numpy` (any 32-bit integer dtype)."""
    words = np.ascontiguousarray(words).view(np.uint32)
    assert words.size == (n + 31) // 32
    i = np.arange(n)
    return ((words[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


# ------------------------------------------------------------------------------------------ top-N, ranks
def candidates(scores_row, seen, allowed):
    """bool [n]: not seen, allowed (None: every item) and not NaN."""
    cand = ~np.isnan(scores_row)
    if allowed is not None:
        cand &= allowed
    cand[np.asarray(seen, dtype=np.int64)] = False
    return cand


def topn(scores_row, seen, allowed, N):
    """(values, items, count): the first N candidates in the stable order (score descending, item ascending)."""
    items = np.nonzero(candidates(scores_row, seen, allowed))[0]
    items = items[np.lexsort((items, -scores_row[items]))[:N]]
    return scores_row[items], items, items.size


def topn_batch(scores, seen_rows, allowed, N):
    """What the kernels write for a batch: values [B, N] padded with -inf (dtype of `scores`), items [B, N] int32
    padded with -1, counts [B] int32."""
    B = scores.shape[0]
    tv = np.full((B, N), -np.inf, scores.dtype)
    ti = np.full((B, N), -1, np.int32)
    tc = np.zeros(B, np.int32)
    for b in range(B):
        v, i, c = topn(scores[b], seen_rows[b], allowed, N)
        tv[b, :c], ti[b, :c], tc[b] = v, i, c
    return tv, ti, tc


def rank_counts(scores_row, seen, allowed, targets):
    """(t_score [T], above [T], n_cand): above[p] = candidates that precede target p in (score descending, item
    ascending), -1 for a NaN target score; a seen or disallowed target gets the position it would take."""
    cand = candidates(scores_row, seen, allowed)
    j = np.arange(scores_row.size)
    targets = np.asarray(targets, dtype=np.int64)
    above = np.zeros(targets.size, np.int32)
    for p, t in enumerate(targets):
        s = scores_row[t]
        above[p] = -1 if np.isnan(s) else (cand & ((scores_row > s) | ((scores_row == s) & (j < t)))).sum()
    return scores_row[targets], above, int(cand.sum())


def rank_counts_batch(scores, seen_rows, allowed, q_ptr, q_items):
    """`rank_counts` of every batch row over its targets q_items[q_ptr[b]: q_ptr[b + 1]]: (t_score [T], above [T]
    int32, n_cand [B] int32)."""
    B = scores.shape[0]
    sc = np.zeros(len(q_items), scores.dtype)
    ab = np.zeros(len(q_items), np.int32)
    nc = np.zeros(B, np.int32)
    for b in range(B):
        s = slice(q_ptr[b], q_ptr[b + 1])
        sc[s], ab[s], nc[b] = rank_counts(scores[b], seen_rows[b], allowed, q_items[s])
    return sc, ab, nc


# ------------------------------------------------------------------------------------------ the half-step of one row
def _alternate(A, g, h, s, d, T):
    """(p, q, b, bprev) of the row's normal equations A x = g - b h, b = (s - h.x) / d, with p = A^-1 g and
    q = A^-1 h: T >= 1 alternations from b = 0 (bprev: the bias the last x was solved with), T == 0 the fixed point
    (b = bprev)."""
    p, q = np.linalg.solve(A, g), np.linalg.solve(A, h)
    if T == 0:
        b = (s - h @ p) / (d - h @ q)
        return p, q, b, b
    b = bprev = 0.0
    for _ in range(T):
        bprev, b = b, (s - h @ p + b * (h @ q)) / d
    return p, q, b, bprev


def bordered_fixed_point(A, g, h, s, d):
    """(x, b) of the bordered (k + 1)-order system [[A, h], [h^T, d]] (x; b) = (g; s) of include/als_hip.h."""
    k = g.size
    M = np.block([[A, h[:, None]], [h[None, :], np.array([[d]])]])
    x = np.linalg.solve(M, np.append(g, s))
    return x[:k], x[k]


def user_system(Z, b_i, mu, lam_u, lam_bu, idx, vals, k):
    """(A, g, h, s, d, Zs, res) of a new user's row: idx its rated items, vals their ratings."""
    Zs = Z[idx, :k].astype(np.float64)
    res = vals.astype(np.float64) - mu - b_i[idx].astype(np.float64)
    A = Zs.T @ Zs + (lam_u + EPS) * np.eye(k)
    return A, Zs.T @ res, Zs.sum(axis=0), res.sum(), idx.size + lam_bu + EPS, Zs, res


def fold_in_user(Z, b_i, mu, lam_u, lam_bu, idx, vals, k, T):
    """(u, b) of als_fold_in for one row: T >= 1 alternations of the user half-step from b = 0, T == 0 their fixed
    point; zeros for the empty row."""
    if idx.size == 0:
        return np.zeros(k), 0.0
    A, g, h, s, d, _, _ = user_system(Z, b_i, mu, lam_u, lam_bu, idx, vals, k)
    p, q, b, bprev = _alternate(A, g, h, s, d, T)
    return p - bprev * q, b


def item_system(U, b_u, mu, V, raters, r, nb_idx, nb_val, lam_v, pop_reg, lam_bi, alpha):
    """(A, g, h, s, d) of a new item's column: raters / r its ratings, nb_idx / nb_val its graph row."""
    k = V.shape[1]
    n_i = raters.size
    nb_val = nb_val.astype(np.float64)
    lv = lam_v / np.sqrt(n_i + 1.0) if pop_reg else lam_v
    lam = lv + EPS + alpha * nb_val.sum()
    Us = U[raters, :k].astype(np.float64)
    res = r.astype(np.float64) - mu - b_u[raters].astype(np.float64)
    A = Us.T @ Us + lam * np.eye(k)
    g = Us.T @ res + alpha * (nb_val @ V[nb_idx].astype(np.float64))
    return A, g, Us.sum(axis=0), res.sum(), n_i + lam_bi + EPS


def fold_in_item(U, b_u, mu, V, raters, r, nb_idx, nb_val, lam_v, pop_reg, lam_bi, alpha, T):
    """(v, b) of als_fold_in_items for one item (V: the fitted items' [n, k] table): T >= 1 alternations of the
    item half-step from b = 0, T == 0 their fixed point.  Without ratings h = 0 and b = 0 for every T."""
    A, g, h, s, d = item_system(U, b_u, mu, V, raters, r, nb_idx, nb_val, lam_v, pop_reg, lam_bi, alpha)
    p, q, b, bprev = _alternate(A, g, h, s, d, T)
    return p - bprev * q, b


def explain_row(Z, b_i, mu, lam_u, lam_bu, idx, vals, k, T, targets):
    """The contract of als_explain for one row and its targets [t]: b_u, cond(A), and per target score, latent,
    leverage and, over all of the row's ratings in the order of idx, the `weights` and `contrib` vectors [t, nr]."""
    A, g, h, s, d, Zs, res = user_system(Z, b_i, mu, lam_u, lam_bu, idx, vals, k)
    b = bprev = 0.0
    if idx.size:
        _, _, b, bprev = _alternate(A, g, h, s, d, T)
    Zt = Z[targets, :k].astype(np.float64)
    Wt = np.linalg.solve(A, Zt.T).T
    weights = Wt @ Zs.T
    contrib = weights * (res - bprev)[None, :]
    latent = contrib.sum(axis=1)
    return dict(b_u=b, weights=weights, contrib=contrib, latent=latent, leverage=(Wt * Zt).sum(axis=1),
                score=mu + b + b_i[targets].astype(np.float64) + latent, cond=np.linalg.cond(A))


def explain_pair(Z, b_i, mu, lam_u, lam_bu, idx, vals, k, T, target, M, largest):
    """`explain_row` for one target, with what the kernel lists: the first M rated items by (float32(contribution)
    descending - ascending with largest=False -, item ascending), their contributions and weights."""
    e = explain_row(Z, b_i, mu, lam_u, lam_bu, idx, vals, k, T, np.array([target]))
    contrib, weight = e["contrib"][0], e["weights"][0]
    key = (contrib if largest else -contrib).astype(np.float32) + np.float32(0.0)
    order = np.lexsort((idx, -key))[:M]
    return dict(score=float(e["score"][0]), latent=float(e["latent"][0]), leverage=float(e["leverage"][0]),
                b_u=e["b_u"], items=idx[order], contributions=contrib[order], weights=weight[order])
