"""The float64 numpy definition of diversified top-N: cosine similarity inside a candidate
pool, min-max relevance, greedy maximal marginal relevance and intra-list diversity.  Shared by
test_diversify_cpu.py (as the arithmetic of the stand-in backend) and test_gpu_diversify.py (as the reference of
the kernels)."""
import numpy as np


def list_len(ids, n: int) -> int:
    """A list ends at the first -1, at the first id outside [0, n), or at its full width."""
    bad = np.nonzero((np.asarray(ids) < 0) | (np.asarray(ids) >= n))[0]
    return int(bad[0]) if bad.size else len(ids)


def similarities(Zp: np.ndarray) -> np.ndarray:
    """sim(j, l) = G_jl / sqrt(G_jj G_ll) of the rows of Zp, 0 when either norm is 0."""
    Zp = np.asarray(Zp, dtype=np.float64)
    G = Zp @ Zp.T
    d = np.sqrt(np.diag(G))
    with np.errstate(divide="ignore", invalid="ignore"):
        S = G / np.outer(d, d)
    S[(d == 0)[:, None] | (d == 0)[None, :]] = 0.0
    return S


def relevance(s: np.ndarray) -> np.ndarray:
    """(s - s_min) / (s_max - s_min); zeros when the range is 0 or not finite."""
    s = np.asarray(s, dtype=np.float64)
    if s.size == 0:
        return s
    with np.errstate(invalid="ignore", over="ignore"):
        rng = s.max() - s.min()
    if not np.isfinite(rng) or rng == 0:
        return np.zeros_like(s)
    return (s - s.min()) / rng


def objectives(rel: np.ndarray, S: np.ndarray, chosen, lam: float) -> np.ndarray:
    """(1 - lam) rel_j - lam max_{l chosen} sim(j, l) for every pool position (the max over no item is 0)."""
    pen = S[:, list(chosen)].max(axis=1) if len(chosen) else np.zeros(rel.size)
    return (1.0 - lam) * rel - lam * pen


def greedy(rel: np.ndarray, S: np.ndarray, lam: float, N: int) -> list:
    """Pool positions in pick order; ties to the lower position."""
    chosen = []
    for _ in range(min(N, rel.size)):
        obj = objectives(rel, S, chosen, lam)
        obj[chosen] = -np.inf
        chosen.append(int(np.argmax(obj)))                # the first of equal maxima
    return chosen


def ild(S: np.ndarray, picks) -> float:
    """Mean of 1 - sim over the unordered pairs of `picks`; NaN for fewer than two."""
    p = list(picks)
    if len(p) < 2:
        return float("nan")
    iu = np.triu_indices(len(p), 1)
    return float(np.mean(1.0 - S[np.ix_(p, p)][iu]))


def rerank(Z: np.ndarray, n: int, cand_val: np.ndarray, cand_idx: np.ndarray, lam: float, N: int):
    """als_mmr_rerank in float64: (top_val float32 [B, N], top_idx int32 [B, N], top_cnt int32 [B],
    ild float64 [B], picks: list of position lists)."""
    B = cand_idx.shape[0]
    tv = np.full((B, N), -np.inf, np.float32)
    ti = np.full((B, N), -1, np.int32)
    tc = np.zeros(B, np.int32)
    out_ild = np.full(B, np.nan)
    picks = []
    for b in range(B):
        M = list_len(cand_idx[b], n)
        ids = cand_idx[b, :M]
        S = similarities(Z[ids])
        p = greedy(relevance(cand_val[b, :M]), S, lam, N)
        tv[b, : len(p)] = cand_val[b, p]
        ti[b, : len(p)] = ids[p]
        tc[b] = len(p)
        out_ild[b] = ild(S, p)
        picks.append(p)
    return tv, ti, tc, out_ild, picks


def list_diversity(Z: np.ndarray, n: int, lists: np.ndarray) -> np.ndarray:
    out = np.full(lists.shape[0], np.nan)
    for b in range(lists.shape[0]):
        ids = lists[b, : list_len(lists[b], n)]
        out[b] = ild(similarities(Z[ids]), range(ids.size))
    return out
