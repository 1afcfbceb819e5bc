"""The definition of ALS.recommend_quota and the contract of als_recommend_topk_quota (include/als_hip.h), in numpy,
read by both suites.

`greedy_capped` IS the definition: one scan of a row's candidates in recommend's order.  `stream_model` is what the
kernel does with them - chunks of 32 candidates against a threshold, a survivor buffer, capped compactions, per-slice
lists folded left under the same filter - on plain (score, item) pairs; the CPU suite holds it against `greedy_capped`,
which is the streaming argument of DESIGN.md section 30 as an executable check.  `QuotaNumpyBackend` adapts the
definition to the engine's backend interface, as tests/capacity_ref.py does for the capacity calls."""
import numpy as np
import torch

from tests.cpu_backend import NumpyBackend
from tests.serving_ref import candidates, unpack_bitmap


def _label(groups, ngroups, i):
    g = int(groups[i])
    return g if 0 <= g < ngroups else -1


# ------------------------------------------------------------------------------------------ the definition
def greedy_capped(scores_row, seen, allowed, groups, cap, N):
    """(values, items, count) of one row: its candidates (`serving_ref.candidates`) scanned in (score descending, item
    ascending); a candidate is taken iff fewer than cap[g] taken items share its group g (a label outside [0, len(cap)):
    no group, never capped); the scan stops after N taken items."""
    cap = np.asarray(cap, np.int64)
    items = np.nonzero(candidates(scores_row, seen, allowed))[0]
    items = items[np.lexsort((items, -(scores_row[items] + 0.0)))]         # -0.0 == +0.0 in the order
    used = np.zeros(cap.size, np.int64)
    taken = []
    for i in items:
        if len(taken) == N:
            break
        g = _label(groups, cap.size, i)
        if g < 0:
            taken.append(i)
        elif used[g] < cap[g]:
            used[g] += 1
            taken.append(i)
    taken = np.asarray(taken, np.int64)
    return scores_row[taken], taken, taken.size


def greedy_capped_batch(scores, seen_rows, allowed, groups, cap, N):
    """What the kernel writes for a batch: values [B, N] padded with -inf (dtype of `scores`), items [B, N] int32 padded
    with -1, counts [B] int32."""
    B = scores.shape[0]
    tv = np.full((B, N), -np.inf, scores.dtype)
    ti = np.full((B, N), -1, np.int32)
    tc = np.zeros(B, np.int32)
    for b in range(B):
        v, i, c = greedy_capped(scores[b], seen_rows[b], allowed, groups, cap, N)
        tv[b, :c], ti[b, :c], tc[b] = v, i, c
    return tv, ti, tc


def n_eff(allowed, groups, cap, N):
    """The host clamp: min(N, #allowed items without a group + sum_g min(cap[g], #allowed items of g))."""
    cap = np.asarray(cap, np.int64)
    ok = np.ones(len(groups), bool) if allowed is None else allowed
    lab = np.array([_label(groups, cap.size, i) for i in range(len(groups))])
    room = int((ok & (lab < 0)).sum())
    for g in range(cap.size):
        room += min(int(cap[g]), int((ok & (lab == g)).sum()))
    return min(N, room)


# ------------------------------------------------------------------------------------------ the streaming model
def _capped_filter(pairs, groups, cap, N):
    """pairs: (score, item) tuples; sorted by (score descending, item ascending), a pair kept iff fewer than cap better
    pairs of its group are in the sorted set, cut after N kept pairs."""
    pairs = sorted(pairs, key=lambda p: (-p[0], p[1]))
    seen_of = {}
    kept = []
    for s, i in pairs:
        g = _label(groups, len(cap), i)
        if g >= 0:
            r = seen_of.get(g, 0)
            seen_of[g] = r + 1
            if r >= cap[g]:
                continue
        kept.append((s, i))
        if len(kept) == N:
            break
    return kept


def _before(a, b):
    """pair a precedes pair b in the order (score descending, item ascending)"""
    return a[0] > b[0] or (a[0] == b[0] and a[1] < b[1])


def stream_model(scores_row, order, groups, cap, N, nslices=1, chunk=32, buf=96, limit=64):
    """The kernel's selection on one row, on (score, item) pairs: the items `order` (candidates only, in arrival order)
    are cut into `nslices` contiguous parts; each part is walked in chunks of `chunk`: a candidate that precedes the
    threshold (the N-th kept pair; none while fewer than N are kept) goes to the buffer, and when the buffer holds more
    than `limit` after a chunk, list + buffer are compacted by `_capped_filter`.  The parts' lists are folded left, the
    filter after every fold.  Returns the list of (score, item)."""
    assert chunk <= buf - limit and N <= buf
    order = list(order)
    per = -(-len(order) // nslices) if order else 0
    per = -(-per // chunk) * chunk                                          # slices are whole chunks
    compactions = 0
    lists = []
    for s in range(nslices):
        part = order[s * per: (s + 1) * per]
        lst, pend = [], []
        for c0 in range(0, len(part), chunk):
            thr = lst[N - 1] if len(lst) == N else None
            for i in part[c0: c0 + chunk]:
                p = (float(scores_row[i]) + 0.0, int(i))
                if thr is None or _before(p, thr):
                    pend.append(p)
            assert len(pend) <= buf
            if len(pend) > limit:
                lst, pend = _capped_filter(lst + pend, groups, cap, N), []
                compactions += 1
        if pend:
            lst = _capped_filter(lst + pend, groups, cap, N)
            compactions += 1
        lists.append(lst)
    out = lists[0]
    for lst in lists[1:]:
        out = _capped_filter(out + lst, groups, cap, N)
    return out, compactions


# ------------------------------------------------------------------------------------------ the stand-in
class QuotaNumpyBackend(NumpyBackend):
    """NumpyBackend with als_recommend_topk_quota; `calls` records one tuple per call."""

    def recommend_topk_quota(self, *, k, ld, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow, item_group,
                             group_cap, topn, top_val, top_idx, top_cnt):
        assert item_group.dtype == torch.int32 and item_group.numel() == n and group_cap.dtype == torch.int32
        assert top_val.shape[1] == topn and top_idx.shape[1] == topn
        self.calls.append(("recommend_topk_quota", users.numel(), topn))
        S, seen = self._serving_rows(users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx)
        ok = None if allow is None else unpack_bitmap(allow.numpy(), n)
        lists = greedy_capped_batch(S, seen, ok, item_group.numpy(), group_cap.numpy(), topn)
        for out, a in zip((top_val, top_idx, top_cnt), lists):
            out[: a.shape[0]] = torch.from_numpy(a)
