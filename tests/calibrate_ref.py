"""The float64 numpy definition of calibrated top-N: category tables and profiles, the smoothed
KL divergence of a list from a target, and the greedy genre-proportional re-ranking of a candidate pool.  Shared by
test_calibrate_cpu.py (as the arithmetic of the stand-in backend) and test_gpu_calibrate.py (as the reference of the
kernels).  The relevance and the end-of-list rule are section 18's (tests/mmr_ref.py)."""
import numpy as np

from tests.mmr_ref import list_len, relevance


def normalise(a: np.ndarray) -> np.ndarray:
    """Rows divided by their sums in float64 (an all-zero row stays zero), rounded once to float32: float64 [rows, ncat]
    holding the fp32 values the kernels read."""
    a = np.asarray(a, dtype=np.float64)
    s = a.sum(axis=1, keepdims=True)
    return np.divide(a, s, out=np.zeros_like(a), where=s > 0).astype(np.float32).astype(np.float64)


def has_category(C: np.ndarray) -> np.ndarray:
    return (np.asarray(C) > 0).any(axis=1)


def profile(C: np.ndarray, indptr: np.ndarray, indices: np.ndarray, rows=None) -> np.ndarray:
    """float64 [B, ncat]: (sum of C_i over the CSR row) / (its items with a category), zeros when there is none.
    `rows`: the CSR row of every batch row (None: row b)."""
    C = np.asarray(C, dtype=np.float64)
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows)
    has = has_category(C)
    out = np.zeros((len(rows), C.shape[1]))
    for b, r in enumerate(rows):
        ids = np.asarray(indices[indptr[r]: indptr[r + 1]], dtype=np.int64)
        cnt = int(has[ids].sum())
        if cnt:
            out[b] = C[ids].sum(axis=0) / cnt
    return out


def kl(p: np.ndarray, q: np.ndarray, alpha: float) -> float:
    """sum over p_c > 0 of p_c ln(p_c / ((1 - alpha) q_c + alpha p_c))."""
    m = p > 0
    if not m.any():
        return 0.0
    qt = (1.0 - alpha) * q[m] + alpha * p[m]
    return float(np.sum(p[m] * (np.log2(p[m]) - np.log2(qt))) * np.log(2.0))


def state(Cp: np.ndarray, picks):
    """(S float64 [ncat], cnt): the sum of the picked rows in pick order and the number of them with a category."""
    S = np.zeros(Cp.shape[1])
    cnt = 0
    for j in picks:
        S = S + Cp[j]
        cnt += int((Cp[j] > 0).any())
    return S, cnt


def state_kl(p: np.ndarray, S: np.ndarray, cnt: int, alpha: float) -> float:
    return kl(p, S / cnt if cnt else np.zeros_like(S), alpha)


def objectives(rel: np.ndarray, Cp: np.ndarray, p: np.ndarray, chosen, lam: float, alpha: float) -> np.ndarray:
    """(1 - lam) rel_j - lam KL(p || list so far plus j) for every pool position."""
    S, cnt = state(Cp, chosen)
    m = p > 0
    if not m.any() or rel.size == 0:
        return (1.0 - lam) * rel
    cj = (cnt + has_category(Cp))[:, None].astype(np.float64)
    q = np.divide(S[m] + Cp[:, m], cj, out=np.zeros((rel.size, int(m.sum()))), where=cj > 0)
    qt = (1.0 - alpha) * q + alpha * p[m]
    return (1.0 - lam) * rel - lam * (np.sum(p[m] * (np.log2(p[m]) - np.log2(qt)), axis=1) * np.log(2.0))


def greedy(rel: np.ndarray, Cp: np.ndarray, p: np.ndarray, lam: float, alpha: float, N: int) -> list:
    """Pool positions in pick order; ties to the lower position."""
    chosen = []
    for _ in range(min(N, rel.size)):
        obj = objectives(rel, Cp, p, chosen, lam, alpha)
        obj[chosen] = -np.inf
        chosen.append(int(np.argmax(obj)))                # the first of equal maxima
    return chosen


def rerank(C: np.ndarray, n: int, P: np.ndarray, cand_val: np.ndarray, cand_idx: np.ndarray, lam: float,
           alpha: float, N: int):
    """als_calibrated_rerank in float64 (lam and alpha as the fp32 values the kernel receives): (top_val float32
    [B, N], top_idx int32 [B, N], top_cnt int32 [B], kl float64 [B], picks: list of position lists)."""
    lam, alpha = float(np.float32(lam)), float(np.float32(alpha))
    C, P = np.asarray(C, dtype=np.float64), np.asarray(P, dtype=np.float64)
    B = cand_idx.shape[0]
    tv = np.full((B, N), -np.inf, np.float32)
    ti = np.full((B, N), -1, np.int32)
    tc = np.zeros(B, np.int32)
    out_kl = np.zeros(B)
    picks = []
    for b in range(B):
        M = list_len(cand_idx[b], n)
        ids = cand_idx[b, :M]
        Cp = C[ids]
        p = greedy(relevance(cand_val[b, :M]), Cp, P[b], lam, alpha, N)
        tv[b, : len(p)] = cand_val[b, p]
        ti[b, : len(p)] = ids[p]
        tc[b] = len(p)
        out_kl[b] = state_kl(P[b], *state(Cp, p), alpha)
        picks.append(p)
    return tv, ti, tc, out_kl, picks


def list_miscalibration(C: np.ndarray, n: int, P: np.ndarray, lists: np.ndarray, alpha: float) -> np.ndarray:
    alpha = float(np.float32(alpha))
    C, P = np.asarray(C, dtype=np.float64), np.asarray(P, dtype=np.float64)
    out = np.zeros(lists.shape[0])
    for b in range(lists.shape[0]):
        ids = lists[b, : list_len(lists[b], n)]
        out[b] = state_kl(P[b], *state(C[ids], range(ids.size)), alpha)
    return out


# ------------------------------------------------------------------------------------------ synthetic sets
def synthetic(n: int, B: int, ncat: int, seed: int, max_hist: int = 39, uncategorised: float = 0.05):
    """The synthetic set of the tests: a multi-hot matrix [n, ncat] - every item 1 .. 3 categories drawn from a
    1 / rank distribution, `uncategorised` of the items none - and histories of 0 .. max_hist distinct items as a
    CSR (indptr int64 [B + 1], indices int32); row 0 is empty, row 1 (when the set has one) holds only items without
    a category."""
    rng = np.random.default_rng(seed)
    w = 1.0 / np.arange(1, ncat + 1)
    w /= w.sum()
    G = np.zeros((n, ncat))
    for i in range(n):
        G[i, rng.choice(ncat, size=min(ncat, int(rng.integers(1, 4))), replace=False, p=w)] = 1.0
    none = rng.random(n) < uncategorised
    none[:2] = True
    G[none] = 0.0
    lens = rng.integers(0, max_hist + 1, size=B)
    lens[0] = 0
    hist = [np.sort(rng.choice(n, size=int(L), replace=False)) for L in lens]
    if B > 1:
        hist[1] = np.nonzero(none)[0][:5]
    indptr = np.zeros(B + 1, np.int64)
    indptr[1:] = np.cumsum([h.size for h in hist])
    indices = np.concatenate(hist).astype(np.int32)
    return G, indptr, indices
