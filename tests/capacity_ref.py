"""The definition of ALS.recommend_capacity and the contracts of als_recommend_topk_priced and als_capacity_settle
(include/als_hip.h), in numpy, read by both suites.

`greedy` IS the definition: the sorted scan over all candidate pairs.  `priced_topn` and `settle` are the two kernel
contracts, item by item; `rounds_model` runs the threshold rounds on them (what the host loop of serving.py does over a
backend), which the CPU suite holds against `greedy`.  `CapacityNumpyBackend` adapts the two contracts to the engine's
backend interface, as tests/eligible_ref.py does for the eligibility calls."""
import numpy as np
import torch

from tests.cpu_backend import NumpyBackend
from tests.serving_ref import candidates, unpack_bitmap


# ------------------------------------------------------------------------------------------ keys
def enc_f32(s):
    """topk::enc_f32 on a float32 array: uint64 values < 2^32 whose integer order is the float order, -0.0 on +0.0."""
    b = (np.asarray(s, np.float32) + np.float32(0.0)).view(np.uint32).astype(np.uint64)
    return np.where(b & np.uint64(0x80000000), b ^ np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def make_key(s, idx):
    """topk::make_key: (enc(s) << 32) | (0xFFFFFFFF - idx), uint64."""
    return (enc_f32(s) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(idx).astype(np.uint64))


# ------------------------------------------------------------------------------------------ the definition
def greedy(scores, seen_rows, allowed, capacity, N):
    """The capped lists of a batch: scores [B, n] (row b = batch row b), seen_rows[b] the seen items of row b, allowed
    bool [n] or None, capacity int [n].  One scan over the candidate pairs in (score descending, row ascending, item
    ascending); -> (items int64 [B, N] padded -1, values [B, N] padded -inf, fill int64 [n])."""
    B, n = scores.shape
    capacity = np.asarray(capacity, np.int64)
    cand = np.stack([candidates(scores[b], seen_rows[b], allowed) for b in range(B)]) & (capacity > 0)[None, :]
    bb, ii = np.nonzero(cand)
    ss = scores[bb, ii] + 0.0                                              # -0.0 == +0.0 in the order
    order = np.lexsort((ii, bb, -ss))
    items = np.full((B, N), -1, np.int64)
    vals = np.full((B, N), -np.inf, scores.dtype)
    held = np.zeros(B, np.int64)
    fill = np.zeros(n, np.int64)
    for p in order:
        b, i = bb[p], ii[p]
        if held[b] < N and fill[i] < capacity[i]:
            items[b, held[b]], vals[b, held[b]] = i, scores[b, i]
            held[b] += 1
            fill[i] += 1
    return items, vals, fill


# ------------------------------------------------------------------------------------------ the kernel contracts
def priced_topn(scores, seen_rows, allowed, row_ids, floor_key, N):
    """als_recommend_topk_priced: scores float32 [R, n] of the launched rows, row_ids [R] their batch rows, floor_key
    uint64 [n].  Row r takes item i only if it is a candidate of the masked call and make_key(score, row_ids[r]) >=
    floor_key[i]; order (score descending, item ascending).  -> (values [R, N] -inf padded, items int32 [R, N] -1
    padded, counts int32 [R])."""
    R, n = scores.shape
    tv = np.full((R, N), -np.inf, scores.dtype)
    ti = np.full((R, N), -1, np.int32)
    tc = np.zeros(R, np.int32)
    for r in range(R):
        ok = candidates(scores[r], seen_rows[r], allowed) & (make_key(scores[r], np.full(n, row_ids[r])) >= floor_key)
        it = np.nonzero(ok)[0]
        it = it[np.lexsort((it, -(scores[r, it] + 0.0)))[:N]]
        tv[r, :it.size], ti[r, :it.size], tc[r] = scores[r, it], it, it.size
    return tv, ti, tc


def settle(top_idx, top_val, capacity, floor_key):
    """als_capacity_settle on the whole batch's lists (list row = batch row; an id outside [0, n) is an empty slot):
    -> (floor_key uint64 [n], fill int32 [n], dirty int32 [B], n_over).  An item named more often than its capacity
    gets the capacity-th largest item-side key of its entries as its floor (capacity 0: ~0); a row is dirty when one of
    its entries has a key below the new floor of its item."""
    B, N = top_idx.shape
    n = capacity.size
    floor_key = floor_key.copy()
    keys = [[] for _ in range(n)]
    for b in range(B):
        for t in range(N):
            i = top_idx[b, t]
            if 0 <= i < n:
                keys[i].append(int(make_key(top_val[b, t], b)))
    fill = np.zeros(n, np.int32)
    n_over = 0
    for i in range(n):
        c = max(int(capacity[i]), 0)
        fill[i] = min(len(keys[i]), c)
        if len(keys[i]) > c:
            n_over += 1
            floor_key[i] = sorted(keys[i], reverse=True)[c - 1] if c else 0xFFFFFFFFFFFFFFFF
    dirty = np.zeros(B, np.int32)
    for b in range(B):
        for t in range(N):
            i = top_idx[b, t]
            if 0 <= i < n and int(make_key(top_val[b, t], b)) < int(floor_key[i]):
                dirty[b] = 1
    return floor_key, fill, dirty, n_over


def rounds_model(scores, seen_rows, allowed, capacity, N, dirty_only=True):
    """The threshold rounds on the two contracts above: -> (items [B, N], values [B, N], fill, rounds, walked rows)."""
    B, n = scores.shape
    capacity = np.asarray(capacity, np.int32)
    ok = (capacity > 0) if allowed is None else (allowed & (capacity > 0))
    floor = np.zeros(n, np.uint64)
    tv = np.full((B, N), -np.inf, scores.dtype)
    ti = np.full((B, N), -1, np.int32)
    work = np.arange(B)
    rounds = walked = 0
    while True:
        tv[work], ti[work], _ = priced_topn(scores[work], [seen_rows[b] for b in work], ok, work, floor, N)
        walked += work.size
        floor, fill, dirty, n_over = settle(ti, tv, capacity, floor)
        if n_over == 0:
            return ti.astype(np.int64), tv, fill.astype(np.int64), rounds, walked
        rounds += 1
        work = np.nonzero(dirty)[0] if dirty_only else np.arange(B)


# ------------------------------------------------------------------------------------------ the stand-in
def _u64(t):
    return t.numpy().view(np.uint64)


class CapacityNumpyBackend(NumpyBackend):
    """NumpyBackend with the two capacity entry points; `calls` records one tuple per call."""

    def recommend_topk_priced(self, *, k, ld, users, row_ids, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow,
                              floor_key, topn, top_val, top_idx, top_cnt):
        assert row_ids.dtype == torch.int32 and row_ids.numel() == users.numel()
        assert floor_key.dtype == torch.int64 and floor_key.numel() == n
        self.calls.append(("recommend_topk_priced", users.numel()))
        S, seen = self._serving_rows(users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx)
        ok = None if allow is None else unpack_bitmap(allow.numpy(), n)
        lists = priced_topn(S, seen, ok, row_ids.numpy(), _u64(floor_key), topn)
        for out, a in zip((top_val, top_idx, top_cnt), lists):
            out[: a.shape[0]] = torch.from_numpy(a)

    def capacity_settle(self, *, n, top_idx, top_val, capacity, floor_key, fill, dirty, n_over):
        assert top_idx.dtype == torch.int32 and top_val.dtype == torch.float32 and capacity.dtype == torch.int32
        self.calls.append(("capacity_settle", top_idx.shape[0]))
        fl, fi, di, no = settle(top_idx.numpy(), top_val.numpy(), capacity.numpy(), _u64(floor_key))
        floor_key.copy_(torch.from_numpy(fl.view(np.int64)))
        fill.copy_(torch.from_numpy(fi))
        dirty.copy_(torch.from_numpy(di))
        n_over[0] = no
