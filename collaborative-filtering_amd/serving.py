"""Serving a fitted model: the device side of `ALS.predict*`, `recommend*`, `rank_of*`, `explain*`, `fold_in`,
`fold_in_items`, `recommend*_diverse`, `list_diversity`, `similar_items` / `similar_users`, `recommend_users`,
`recommend_group`, `recommend*_explore`, `recommend*_calibrated`, `category_profile`, `list_miscalibration` and
`recommend*_deep`, the per-user eligibility calls (`eligibility`, `recommend*_eligible`, `rank_of_eligible`), the
capped batch lists (`recommend*_capacity`) and the lists under per-group caps (`recommend*_quota`).

`_Serving` is the part of the engine (engine._Engine inherits it) that reads the fit's device state - `U V Z b_u b_i
mu W64 csr` and the shapes - and never changes it.  Every call is local to the calling rank: after the all-gathers
of the fit every rank holds the full tables and the training CSR, so nothing here issues a collective.  The
arithmetic is in the HIP kernels behind the backend (`self.be`); what lives here is the host orchestration: which
Z a call scores against, REC_BATCH chunking, grouping pairs by user, and bringing results back in the caller's
order.  Arguments arrive validated (validate.py, through the `ALS` facade).
"""
from __future__ import annotations

import logging
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np
import torch

from . import layout

RECOMMEND_MAX_N = 128   # ALS_TOPK_MAX: longest list of ALS.recommend
RECOMMEND_DEEP_MAX_N = 1024     # ALS_TOPK_DEEP_MAX: longest list of ALS.recommend_deep
ELIGIBILITY_MAX_BYTES = 1 << 30     # largest eligibility table ALS.eligibility builds (4 S ceil(n / 32) bytes)
# most list slots B N of ALS.recommend_capacity: the batch's lists stay on the device across the rounds (8 B N bytes,
# and as much again for the key buckets of als_capacity_settle, which indexes them with 32-bit offsets)
CAPACITY_MAX_PAIRS = 1 << 26

logger = logging.getLogger(__name__)


@dataclass
class FoldedItems:
    """Items outside the fit, placed by `ALS.fold_in_items`; folded item b is item n + b in `ALS.recommend`.

    V, Z: float64 [B, k], the fp32 device values (Z = V + sum_f X_new,f W_f, what predictions use); b_i: float64
    [B].  graph: the graph rows used, (ptr int64 [B+1], idx int32 fitted item ids, val float32), or None without a
    graph.  ratings: the ratings CSR (ptr int64 [B+1], idx int32 user ids ascending, val float32)."""
    V: np.ndarray
    b_i: np.ndarray
    Z: np.ndarray
    graph: Optional[tuple]
    ratings: tuple

    @property
    def n_items(self) -> int:
        return int(self.b_i.shape[0])


@dataclass
class ItemEligibility:
    """Per-segment item eligibility, made by `ALS.eligibility` and resident on the device: `table` int32
    [n_segments, ceil(n_items / 32)], row s the allow bitmap of segment s (`pack_bitmap`'s layout).  The
    `*_eligible` calls take it with one segment id per batch row."""
    table: torch.Tensor
    n_segments: int
    n_items: int

    def allowed(self, segments: np.ndarray, items: np.ndarray) -> np.ndarray:
        """bool [P]: item items[p] is eligible in segment segments[p] (read from the device table)."""
        s = torch.from_numpy(np.asarray(segments, dtype=np.int64)).to(self.table.device)
        i = torch.from_numpy(np.asarray(items, dtype=np.int64)).to(self.table.device)
        return (((self.table[s, i >> 5].to(torch.int64) >> (i & 31)) & 1) != 0).cpu().numpy()


@dataclass
class CapacityInfo:
    """What `ALS.recommend_capacity(..., return_info=True)` adds to the lists.  rounds: the settle passes that found an
    over-demanded item (0: the uncapped lists were feasible); walked_rows: the rows scored over all rounds (B in round
    0, then the dirty rows only); fill int64 [n_total]: how many lists hold each item (<= capacity); cutoff float64
    [n_total]: the score of the worst holder of a full item (fill == capacity > 0), NaN where the item is not full."""
    rounds: int
    walked_rows: int
    fill: np.ndarray
    cutoff: np.ndarray


def quota_plan(allowed: Optional[np.ndarray], labels: np.ndarray, caps: np.ndarray, N: int):
    """What the caps of `recommend_quota` leave of a call's catalogue: (allowed, N_eff).  `allowed`: bool [n] or None
    (every item), returned with the items of the groups of cap 0 cleared (they go into the allow bitmap; None when
    nothing is blocked).  N_eff = min(N, #allowed items without a group + sum over the groups of min(cap, #allowed
    items of the group)): no list can hold more, and a list that long fills, so the walk's threshold works."""
    grouped = labels >= 0
    closed = np.zeros(labels.size, dtype=bool)
    closed[grouped] = caps[labels[grouped]] == 0
    if closed.any():
        allowed = ~closed if allowed is None else allowed & ~closed
    open_ = grouped if allowed is None else grouped & allowed
    sizes = np.bincount(labels[open_], minlength=caps.size).astype(np.int64)
    free = int((~grouped).sum() if allowed is None else (allowed & ~grouped).sum())
    return allowed, min(N, free + int(np.minimum(sizes, caps.astype(np.int64)).sum()))


@dataclass
class Explanation:
    """What `ALS.explain` / `explain_new` return for P (row, target) pairs, all float64 / int64 host arrays.

    score, latent, leverage, b_u: [P] - the half-step user's score mu + b_u + b_i[i] + latent, its latent part
    u.z_i (the sum of ALL the row's contributions), z_i^T A^-1 z_i, and the user bias.  items [P, M] (-1 padded),
    contributions, weights [P, M] (0 padded): the M strongest rated items with contribution = weight * (r_j - mu -
    b_i[j] - b) and weight = z_i^T A^-1 z_j.  counts [P] = min(M, ratings of the row)."""
    score: np.ndarray
    latent: np.ndarray
    leverage: np.ndarray
    b_u: np.ndarray
    items: np.ndarray
    contributions: np.ndarray
    weights: np.ndarray
    counts: np.ndarray

    @staticmethod
    def empty(M: int) -> "Explanation":
        z = lambda *sh: np.empty(sh, dtype=np.float64)                  # noqa: E731
        return Explanation(z(0), z(0), z(0), z(0), np.empty((0, M), dtype=np.int64), z(0, M), z(0, M),
                           np.empty(0, dtype=np.int64))


def concat_features(features, names) -> np.ndarray:
    """The feature matrices of `names` side by side, float32 [rows, sum of widths]: the X of als_compose_z."""
    return np.concatenate([np.asarray(features[f], dtype=np.float32) for f in names], axis=1)


def pack_bitmap(mask: torch.Tensor) -> torch.Tensor:
    """The allow bitmap of als_recommend_topk_masked / als_rank_count_masked from a bool tensor [n] (any device):
    int32 [ceil(n / 32)], item i = bit i & 31 of word i >> 5 (bit 31 is the sign bit), the bits beyond n zero."""
    n = mask.numel()
    nw = (n + 31) // 32
    bits = torch.zeros(nw * 32, dtype=torch.int64, device=mask.device)
    bits[:n] = mask
    words = (bits.view(nw, 32) << torch.arange(32, dtype=torch.int64, device=mask.device)).sum(dim=1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def pack_words(bits: np.ndarray) -> np.ndarray:
    """bool [R, A] (host) -> int32 [R, ceil(A / 32)] holding uint32 words: bit a of a row is bit a & 31 of word a >> 5,
    the bits beyond A zero - the rows of an eligibility table (A = n items: `pack_bitmap`'s layout) and the attribute
    words of als_eligibility_bitmaps."""
    R, A = bits.shape
    by = np.zeros((R, (A + 31) // 32 * 4), dtype=np.uint8)
    by[:, : (A + 7) // 8] = np.packbits(bits, axis=1, bitorder="little")
    return by.view("<u4").astype(np.uint32).view(np.int32)


def cursor_keys(after_items: np.ndarray, after_scores: np.ndarray) -> np.ndarray:
    """The cursor keys of als_recommend_deep (include/als_hip.h) for the entries (after_items [B], after_scores [B]):
    (enc(float32(score)) << 32) | (0xFFFFFFFF - item) as int64 bit patterns; item -1 - the padding of an exhausted
    list - gives key 0, below which no candidate lies."""
    bits = (after_scores.astype(np.float32) + np.float32(0.0)).view(np.uint32).astype(np.uint64)      # -0.0 -> +0.0
    enc = np.where(bits & np.uint64(0x80000000), bits ^ np.uint64(0xFFFFFFFF), bits | np.uint64(0x80000000))
    low = np.uint64(0xFFFFFFFF) - np.maximum(after_items, 0).astype(np.uint64)
    key = np.where(after_items < 0, np.uint64(0), (enc << np.uint64(32)) | low)
    return key.astype(np.uint64).view(np.int64)


def _raise_unless_solved(status: torch.Tensor, what: str, row_name=lambda r: f"row {r}") -> None:
    """`status` is the one-word result of a solve kernel: 0, or 1 + the first row whose system failed."""
    bad = int(status.item())
    if bad:
        raise np.linalg.LinAlgError(f"{what} normal equations of {row_name(bad - 1)} are not positive definite")


class _Serving:
    """Read-only calls on the device state of a fit; see the module docstring for what `self` has to hold."""

    # rows per als_recommend_topk / als_rank_count / als_explain call: bounds the outputs and the item-slice
    # workspace.  Looked up through the instance at call time (tests shrink it to cross chunk boundaries).
    REC_BATCH = 1 << 16
    GRAPH_ROWS_MAX_D = 160      # sim feature width the top-k kernel takes (its k)
    # rows per als_row_whitener / als_explore_topk call: W costs 4 ld^2 bytes per row, so the chunk is what
    # EXPLORE_W_BYTES hold (4096 rows at k = 64, 655 at k = 160), at most REC_BATCH; EXPLORE_BATCH overrides (tests)
    EXPLORE_W_BYTES = 64 << 20
    EXPLORE_BATCH: Optional[int] = None
    # rows per als_recommend_deep call: at most DEEP_BATCH (and REC_BATCH), halved until the call's workspace - 8 nb
    # (128 S + NL + S) + 64 bytes, S <= 64 slices, a running list of NL <= 1024 keys, so at most 74 240 B per row - is
    # within DEEP_WS_BYTES.  Few slices (many users, short lists) allow large calls, which the walk rewards
    DEEP_BATCH = 1 << 16
    DEEP_WS_BYTES = 512 << 20

    # ------------------------------------------------------------- helpers
    def _concat_w(self, names, dims, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The fp32 projection matrix of the features `names` (widths `dims`), rows stacked as concat_features
        stacks columns: [sum(dims), ld] with zero padding columns; into `out` when given."""
        if out is None:
            out = torch.zeros(sum(dims), self.ld, dtype=torch.float32, device=self.dev)
        off = 0
        for f, d in zip(names, dims):
            out[off:off + d, : self.k] = self.W64[f].to(torch.float32)
            off += d
        return out

    def _compose_for(self, features, features_of_fit: bool = False):
        """Z for `features` as passed to predict (scripts/als.py:568-572): composed from whatever is passed.
        `features_of_fit`: the caller vouches that these are the unchanged arrays of the fit (sweep.SweepDriver,
        which owns them) - the fit's own Z = V + sum_f X_f W_f is then current and nothing is uploaded.  (Round 2
        inferred that from object identity, which says nothing about the contents and can be recycled.)"""
        names = [f for f in features if f in self.W64]
        if not names:
            return self.V
        if features_of_fit and self.iters_run > 0 and names == self.feat_names:
            return self.Z
        X = torch.from_numpy(concat_features(features, names)).to(self.dev)
        Z = torch.empty_like(self.V)
        self.be.compose_z(self.V, X, self._concat_w(names, [features[f].shape[1] for f in names]), Z)
        return Z

    def _item_side(self, Z) -> dict:
        """The fitted item tables as the scoring kernels name them."""
        return dict(k=self.k, ld=self.ld, n=self.n, Z=Z, b_i=self.b_i, mu=self.mu)

    def _csr_dev(self, ptr, idx, val):
        """A CSR triple (host arrays or device tensors) on the device; `idx` / `val` are one-element buffers when
        no row has an entry: the library wants valid pointers."""
        if len(idx) == 0:
            idx, val = np.zeros(1, np.int32), np.zeros(1, np.float32)
        return tuple(a if torch.is_tensor(a) else torch.from_numpy(a).to(self.dev) for a in (ptr, idx, val))

    def allow_bitmap(self, filters, n_total: int) -> Optional[torch.Tensor]:
        """Device bitmap (`pack_bitmap`) of a validated (items, filter_items) pair (validate.item_filters) over
        n_total items: `items` minus `filter_items`, scattered and packed on the device, once per call.  None for
        None: the unfiltered path."""
        if filters is None:
            return None
        allow, block = filters
        mask = torch.ones(n_total, dtype=torch.bool, device=self.dev)
        for a, keep in ((allow, True), (block, False)):
            if a is None:
                continue
            a = torch.from_numpy(a).to(self.dev)
            if a.dtype != torch.bool:                                    # ids -> mask (duplicates write the same value)
                a = torch.zeros(n_total, dtype=torch.bool, device=self.dev).index_fill_(0, a, True)
            mask = a if keep else mask & ~a
        return pack_bitmap(mask)

    def _fitted_rows(self, users: torch.Tensor, exclude_seen: bool):
        """Chunk source of the drivers below for users of the fit: the ids index the resident tables, the seen
        items are the training CSR."""
        seen_ptr = seen_idx = None
        if exclude_seen and self.nnz > 0:
            seen_ptr, seen_idx = self.csr.indptr, self.csr.indices
        return lambda b0, nb: (users[b0: b0 + nb], self.U, self.b_u, seen_ptr, seen_idx)

    def _side(self, features, folded: Optional["FoldedItems"] = None) -> dict:
        """The item tables a call scores against: the fitted items with the Z of `predict`, followed with `folded`
        by the folded ones (`_joint_side`)."""
        return self._item_side(self._compose_for(features)) if folded is None else self._joint_side(features, folded)

    def _catalogue(self, users_t: torch.Tensor, features, exclude_seen: bool, folded: Optional["FoldedItems"] = None):
        """(side, rows) of a call for users of the fit: the item tables of `_side` and the chunk source that goes
        with them - `_fitted_rows`, or `_joint_rows` over the joint catalogue."""
        if folded is None:
            return self._side(features), self._fitted_rows(users_t, exclude_seen)
        return self._side(features, folded), self._joint_rows(users_t, exclude_seen, folded)

    def _table_rows(self, B: int, U, b_u, seen=None):
        """Chunk source for a table made for the call (batch row b = table row b): the chunk is addressed as rows
        0 .. nb of the tables advanced to b0.  `seen` = (host indptr, device indptr, device indices) or None."""
        users = torch.arange(min(B, self.REC_BATCH), dtype=torch.int32, device=self.dev)

        def rows(b0, nb):
            seen_ptr = seen_idx = None
            if seen is not None and seen[0][b0 + nb] > seen[0][b0]:
                # views: row b of the chunk reads ptr_d[b0 + b]; the offsets stay absolute into idx_d
                seen_ptr, seen_idx = seen[1][b0: b0 + nb + 1], seen[2]
            return users[:nb], U[b0:], b_u[b0:], seen_ptr, seen_idx
        return rows

    # ------------------------------------------------------- chunked drivers
    @staticmethod
    def _chunks(B: int, step: int):
        """(b0, nb) of the chunks of B batch rows, `step` rows each but the last."""
        for b0 in range(0, B, step):
            yield b0, min(step, B - b0)

    def _topn_out(self, nb: int, N: int):
        """The outputs of a top-N call over nb rows on the device: (top_val fp32 [nb, N], top_idx int32 [nb, N],
        top_cnt int32 [nb])."""
        return (torch.empty(nb, N, dtype=torch.float32, device=self.dev),
                torch.empty(nb, N, dtype=torch.int32, device=self.dev),
                torch.empty(nb, dtype=torch.int32, device=self.dev))

    def _collect(self, B: int, step: int, specs, call) -> tuple:
        """call(b0, nb) -> one device tensor [nb, ...] per entry of `specs` = ((trailing shape, host dtype), ...) for
        every chunk of `_chunks(B, step)`; returns the host arrays [B, ...], copied chunk by chunk - nothing of B rows
        exists on the device."""
        outs = tuple(np.empty((B, *shape), dtype=dtype) for shape, dtype in specs)
        for b0, nb in self._chunks(B, step):
            for out, t in zip(outs, call(b0, nb)):
                out[b0: b0 + nb] = t.cpu().numpy()
        return outs

    def _collect_topn(self, B: int, N: int, step: int, call, extra=()) -> tuple:
        """`_collect` of a top-N call: call(b0, nb, top_val, top_idx, top_cnt) fills the `_topn_out` of the chunk and
        returns further device tensors [nb, ...] of the trailing shapes `extra` (or None).  Returns host (ids int64
        [B, N], values float64 [B, N], and the extras as float64)."""
        def chunk(b0, nb):
            tv, ti, tc = self._topn_out(nb, N)
            return (ti, tv, *(call(b0, nb, tv, ti, tc) or ()))
        specs = (((N,), np.int64), ((N,), np.float64), *((shape, np.float64) for shape in extra))
        return self._collect(B, step, specs, chunk)

    def _restricted(self, name: str, allow, seg, b0: int, nb: int, **kw):
        """The backend call `name` over the catalogue the chunk [b0, b0 + nb) may see: `name`_segmented with seg =
        (eligibility table, row_seg int32 [B] on the device), `name`_masked with the bitmap `allow`, else `name`."""
        if seg is not None:
            getattr(self.be, name + "_segmented")(seg_allow=seg[0], row_seg=seg[1][b0: b0 + nb], **kw)
        elif allow is not None:
            getattr(self.be, name + "_masked")(allow=allow, **kw)
        else:
            getattr(self.be, name)(**kw)

    def _topk_chunks(self, B: int, N: int, rows, items: dict, on_device: bool = False, filters=None, seg=None):
        """als_recommend_topk over B batch rows in REC_BATCH chunks.  rows(b0, nb) -> (users int32 [nb], U, b_u,
        seen_ptr, seen_idx) of chunk [b0, b0 + nb); `items`: the item tables (k, ld, n, Z, b_i, mu); `filters`: the
        validated (items, filter_items) pair of the call - its bitmap (`allow_bitmap`) is made once and every chunk
        goes through als_recommend_topk_masked; `seg` instead: als_recommend_topk_segmented (`_restricted`).  Returns
        host (items int64 [B, N], scores float64 [B, N]), copied chunk by chunk, or with `on_device` the kernel's own
        (top_val fp32 [B, N], top_idx int32 [B, N])."""
        allow = self.allow_bitmap(filters, items["n"])

        def call(b0, nb, tv, ti, tc):
            users, U, b_u, seen_ptr, seen_idx = rows(b0, nb)
            self._restricted("recommend_topk", allow, seg, b0, nb, users=users, U=U, b_u=b_u, seen_ptr=seen_ptr,
                             seen_idx=seen_idx, topn=N, top_val=tv, top_idx=ti, top_cnt=tc, **items)
        if not on_device:
            return self._collect_topn(B, N, self.REC_BATCH, call)
        top_val, top_idx, top_cnt = self._topn_out(B, N)
        for b0, nb in self._chunks(B, self.REC_BATCH):
            call(b0, nb, top_val[b0:], top_idx[b0:], top_cnt[b0:])
        return top_val, top_idx

    def _rank_chunks(self, rows, t_ptr: torch.Tensor, t_ptr_h: np.ndarray, q_items: torch.Tensor, items: dict,
                     filters=None, seg=None):
        """als_rank_count over the batch rows of the prefix sum `t_ptr` (device; `t_ptr_h` its host copy) in
        REC_BATCH chunks: row b's targets are q_items[t_ptr[b]:t_ptr[b + 1]]; `rows`, `items`, `filters` and `seg` as
        in `_topk_chunks` (als_rank_count_masked, als_rank_count_segmented).
        Returns device (above int32 [P], n_cand int32 [rows], score fp32 [P])."""
        B, P = t_ptr_h.size - 1, q_items.numel()
        allow = self.allow_bitmap(filters, items["n"])
        above = torch.empty(P, dtype=torch.int32, device=self.dev)
        score = torch.empty(P, dtype=torch.float32, device=self.dev)
        ncand = torch.empty(B, dtype=torch.int32, device=self.dev)
        for b0, nb in self._chunks(B, self.REC_BATCH):
            users, U, b_u, seen_ptr, seen_idx = rows(b0, nb)
            t0, t1 = int(t_ptr_h[b0]), int(t_ptr_h[b0 + nb])
            self._restricted("rank_count", allow, seg, b0, nb, U=U, b_u=b_u, seen_ptr=seen_ptr, seen_idx=seen_idx,
                             q_users=users, q_ptr=(t_ptr[b0: b0 + nb + 1] - t0).contiguous(), q_items=q_items[t0:t1],
                             t_score=score[t0:t1], above=above[t0:t1], n_cand=ncand[b0: b0 + nb], **items)
        return above, ncand, score

    def _group_by_user(self, us: torch.Tensor):
        """Pairs grouped by user on the device: (order, inv, uniq, counts, ptr, ptr_h) - `order` sorts the pairs by
        user (stable), `inv` undoes it, `uniq` are the distinct users ascending with `counts` pairs each, `ptr`
        (device) / `ptr_h` (host) the prefix sum of the counts."""
        order = torch.sort(us.to(torch.int64), stable=True).indices
        uniq, counts = torch.unique_consecutive(us[order], return_counts=True)
        ptr = torch.zeros(uniq.numel() + 1, dtype=torch.int64, device=self.dev)
        torch.cumsum(counts, 0, out=ptr[1:])
        inv = torch.empty_like(order)
        inv[order] = torch.arange(order.numel(), device=order.device)
        return order, inv, uniq.contiguous(), counts, ptr, ptr.cpu().numpy()

    # ------------------------------------------------------------- predict
    def predict_dense(self, features) -> np.ndarray:
        Z = self._compose_for(features)
        out = torch.empty(self.m, self.n, dtype=torch.float32, device=self.dev)
        self.be.predict_dense(k=self.k, ld=self.ld, m=self.m, n=self.n, U=self.U, Z=Z, b_u=self.b_u,
                              b_i=self.b_i, mu=self.mu, out=out)
        return out.cpu().numpy().astype(np.float64)

    def predict_at(self, flat_idx: np.ndarray, features) -> np.ndarray:
        u, i = np.divmod(flat_idx, self.n)
        us = torch.from_numpy(u.astype(np.int32)).to(self.dev)
        is_ = torch.from_numpy(i.astype(np.int32)).to(self.dev)
        return self.predict_pairs(us, is_, features).cpu().numpy().astype(np.float64)

    def predict_pairs(self, us: torch.Tensor, is_: torch.Tensor, features, features_of_fit: bool = False) -> torch.Tensor:
        """Predictions at (user, item) index tensors already on the device (int32); fp32 device tensor."""
        Z = self._compose_for(features, features_of_fit)
        out = torch.empty(us.numel(), dtype=torch.float32, device=self.dev)
        self.be.predict_at(k=self.k, ld=self.ld, us=us, is_=is_, U=self.U, Z=Z, b_u=self.b_u,
                           b_i=self.b_i, mu=self.mu, out=out)
        return out

    # ----------------------------------------------------- users of the fit
    def recommend(self, users_t: torch.Tensor, N: int, features, exclude_seen: bool, filters=None):
        """Top-N items of the users in `users_t` (int32, device): (items int64 [B, N], scores float64 [B, N]),
        unused slots -1 / -inf.  Z is composed as in `predict`; the seen items are the training CSR of this fit.
        `filters`: here and below the validated (items, filter_items) pair of the call, or None."""
        side, rows = self._catalogue(users_t, features, exclude_seen)
        return self._topk_chunks(users_t.numel(), N, rows, side, filters=filters)

    def _rank_outputs(self, above, ncand_rows, counts, score, inv=None):
        rank = above.to(torch.int64)
        cand = torch.repeat_interleave(ncand_rows.to(torch.int64), counts)
        if inv is not None:
            rank, cand, score = rank[inv], cand[inv], score[inv]
        return rank.cpu().numpy(), cand.cpu().numpy(), score.cpu().numpy()

    def rank_of(self, us: torch.Tensor, is_: torch.Tensor, features, exclude_seen: bool, filters=None):
        """Ranks of the pairs (us[p], is_[p]) (int32, device): the pairs are grouped by user on the device, every
        user of a REC_BATCH chunk is scored once (als_rank_count), and the outputs go back to the pairs' order:
        (rank int64 [P], n_candidates int64 [P], scores float32 [P]).  Z and the seen items as in `recommend`."""
        return self._rank_pairs(us, is_, features, exclude_seen, filters=filters)

    def _rank_pairs(self, us, is_, features, exclude_seen: bool, folded=None, filters=None, elig=None, pair_seg=None):
        """`rank_of` / `rank_of_eligible`: with `elig` the segment of a user's row is that of its first pair."""
        order, inv, uniq, counts, ptr, ptr_h = self._group_by_user(us)
        seg = None if elig is None else (elig.table, pair_seg[order][ptr[:-1]].contiguous())
        side, rows = self._catalogue(uniq, features, exclude_seen, folded)
        above, ncand, score = self._rank_chunks(rows, ptr, ptr_h, is_[order].contiguous(), side, filters, seg)
        return self._rank_outputs(above, ncand, counts, score, inv)

    def explain(self, us: torch.Tensor, is_: torch.Tensor, M: int, features, n_sweeps: int, largest: bool):
        """Explanations of the pairs (us[p], is_[p]) (int32, device), the rows read from the resident training CSR:
        the pairs are grouped by user on the device (as `rank_of`), every distinct user of a REC_BATCH chunk is
        factorised once (als_explain, `rows` = the users), and the outputs go back to the pairs' order."""
        Z = self._compose_for(features)
        order, inv, uniq, counts, ptr, ptr_h = self._group_by_user(us)
        out = self._explain_rows((self.csr.indptr, self.csr.indices, self.csr.vals), uniq, ptr, ptr_h,
                                 is_[order].contiguous(), Z, M, n_sweeps, largest, lambda w: f"user {int(uniq[w])}")
        return self._explanation(*out[:3], torch.repeat_interleave(out[3], counts), *out[4:], inv=inv)

    def seen_pairs(self, us: torch.Tensor, is_: torch.Tensor) -> np.ndarray:
        """bool [P]: (us[p], is_[p]) (int64, device) is an entry of the training CSR (a binary search per pair)."""
        if self.nnz == 0:
            return np.zeros(us.numel(), dtype=bool)
        ptr, idx = self.csr.indptr, self.csr.indices
        lo, hi = ptr[us].clone(), ptr[us + 1].clone()
        end = hi.clone()
        while bool((lo < hi).any()):                                     # first entry >= the item
            act, mid = lo < hi, (lo + hi) >> 1
            below = act & (idx[mid.clamp(max=idx.numel() - 1)] < is_)
            lo, hi = torch.where(below, mid + 1, lo), torch.where(act & ~below, mid, hi)
        found = (lo < end) & (idx[lo.clamp(max=idx.numel() - 1)] == is_)
        return found.cpu().numpy()

    # -------------------------------------------------- users outside the fit
    def _fold_in_dev(self, indptr: np.ndarray, indices: np.ndarray, vals: np.ndarray, Z, n_sweeps: int):
        """Folded factors (fp32 [B, ld], zero padding columns) and biases (fp32 [B]) on the device, with the
        device CSR they were computed from (one als_fold_in launch)."""
        md = self.model
        B = indptr.size - 1
        ptr_d, idx_d, val_d = self._csr_dev(indptr, indices, vals)
        U = torch.empty(B, self.ld, dtype=torch.float32, device=self.dev)
        b = torch.empty(B, dtype=torch.float32, device=self.dev)
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.be.fold_in(k=self.k, ld=self.ld, indptr=ptr_d, indices=idx_d, vals=val_d, n=self.n, Z=Z, b_i=self.b_i,
                        mu=self.mu, lam_u=md.lambda_u, lam_bu=md.lambda_bu, n_sweeps=n_sweeps, U_out=U, b_u_out=b,
                        status=status)
        _raise_unless_solved(status, "fold-in")
        return U, b, ptr_d, idx_d

    def _new_catalogue(self, indptr: np.ndarray, indices, vals, features, n_sweeps: int, exclude_seen: bool):
        """`_catalogue` for rows outside the fit: fold in against the Z of `predict`, then the chunk source of the
        folded table - batch row b = new row b, the given ratings as the seen CSR.  Returns (side, rows, and the
        device row pointers and indices of the ratings)."""
        Z = self._compose_for(features)
        U, b, ptr_d, idx_d = self._fold_in_dev(indptr, indices, vals, Z, n_sweeps)
        rows = self._table_rows(indptr.size - 1, U, b, (indptr, ptr_d, idx_d) if exclude_seen else None)
        return self._item_side(Z), rows, ptr_d, idx_d

    def fold_in(self, indptr, indices, vals, features, n_sweeps: int):
        """Factors / biases of new users (host CSR, rows sorted) against this fit's item side: device fp32
        ([B, ld], [B]).  Z is composed as in `predict`."""
        U, b, _, _ = self._fold_in_dev(indptr, indices, vals, self._compose_for(features), n_sweeps)
        return U, b

    def recommend_new(self, indptr, indices, vals, N: int, features, n_sweeps: int, exclude_seen: bool,
                      filters=None):
        """Fold in, then als_recommend_topk on the folded table in REC_BATCH chunks: (items int64 [B, N], scores
        float64 [B, N])."""
        side, rows, *_ = self._new_catalogue(indptr, indices, vals, features, n_sweeps, exclude_seen)
        return self._topk_chunks(indptr.size - 1, N, rows, side, filters=filters)

    def rank_of_new(self, indptr, indices, vals, tptr: np.ndarray, titems: np.ndarray, features, n_sweeps: int,
                    exclude_seen: bool, filters=None):
        """Fold in, then als_rank_count on the folded table (as `recommend_new` composes it) for the targets
        titems[tptr[b]:tptr[b + 1]], in REC_BATCH chunks."""
        side, rows, *_ = self._new_catalogue(indptr, indices, vals, features, n_sweeps, exclude_seen)
        tptr_d = torch.from_numpy(tptr).to(self.dev)
        above, ncand, score = self._rank_chunks(rows, tptr_d, tptr, torch.from_numpy(titems).to(self.dev), side,
                                                filters)
        return self._rank_outputs(above, ncand, tptr_d[1:] - tptr_d[:-1], score)

    def explain_new(self, indptr, indices, vals, tptr: np.ndarray, titems: np.ndarray, M: int, features,
                    n_sweeps: int, largest: bool):
        """Explanations for new rows (host CSR, rows sorted), targets titems[tptr[b]:tptr[b + 1]] of row b."""
        Z = self._compose_for(features)
        tptr_d = torch.from_numpy(tptr).to(self.dev)
        out = self._explain_rows((indptr, indices, vals), None, tptr_d, tptr, torch.from_numpy(titems).to(self.dev),
                                 Z, M, n_sweeps, largest, lambda w: f"row {w}")
        return self._explanation(*out[:3], torch.repeat_interleave(out[3], tptr_d[1:] - tptr_d[:-1]), *out[4:])

    def _explain_rows(self, csr, rows_d, tptr_d, tptr_h: np.ndarray, q_items, Z, M: int, n_sweeps: int,
                      largest: bool, row_name):
        """als_explain over W work rows in REC_BATCH chunks.  rows_d (int32 [W]) names the row of `csr` (a triple,
        host or device) of every work row; None: work row w is CSR row w.  Targets q_items[tptr[w]:tptr[w + 1]].
        Returns the device outputs in target order and b_u per work row.  row_name(w): how an error names work
        row w."""
        md = self.model
        W, P = tptr_h.size - 1, q_items.numel()
        f64 = dict(dtype=torch.float64, device=self.dev)
        score, latent, lev = (torch.empty(P, **f64) for _ in range(3))
        top_item = torch.empty(P, M, dtype=torch.int32, device=self.dev)
        top_c, top_w = torch.empty(P, M, **f64), torch.empty(P, M, **f64)
        top_cnt = torch.empty(P, dtype=torch.int32, device=self.dev)
        b_u = torch.empty(W, **f64)
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        ptr_d, idx_d, val_d = self._csr_dev(*csr)
        for b0, nb in self._chunks(W, self.REC_BATCH):
            t0, t1 = int(tptr_h[b0]), int(tptr_h[b0 + nb])
            if t1 == t0:
                b_u[b0: b0 + nb] = float("nan")                          # rows without targets: never read
                continue
            # views: without rows_d work row w of the chunk reads ptr_d[b0 + w]; the offsets stay absolute
            self.be.explain(k=self.k, ld=self.ld, indptr=ptr_d if rows_d is not None else ptr_d[b0: b0 + nb + 1],
                            indices=idx_d, vals=val_d, rows=None if rows_d is None else rows_d[b0: b0 + nb],
                            n=self.n, Z=Z, b_i=self.b_i, mu=self.mu, lam_u=md.lambda_u, lam_bu=md.lambda_bu,
                            n_sweeps=n_sweeps, t_ptr=(tptr_d[b0: b0 + nb + 1] - t0).contiguous(),
                            t_items=q_items[t0:t1], topm=M, largest=largest, score=score[t0:t1],
                            latent=latent[t0:t1], leverage=lev[t0:t1], top_item=top_item[t0:t1],
                            top_contrib=top_c[t0:t1], top_weight=top_w[t0:t1], top_cnt=top_cnt[t0:t1],
                            b_u_out=b_u[b0: b0 + nb], status=status)
            _raise_unless_solved(status, "fold-in", lambda r: row_name(b0 + r))
        return score, latent, lev, b_u, top_item, top_c, top_w, top_cnt

    @staticmethod
    def _explanation(score, latent, lev, b_u_t, top_item, top_c, top_w, top_cnt, inv=None) -> "Explanation":
        outs = [score, latent, lev, b_u_t, top_item.to(torch.int64), top_c, top_w, top_cnt.to(torch.int64)]
        if inv is not None:
            outs = [o[inv] for o in outs]
        return Explanation(*(o.cpu().numpy() for o in outs))

    # ----------------------------------------------------------- new items
    def graph_rows_new(self, X_new: np.ndarray, X_fit) -> tuple:
        """Graph rows of new items against the fitted ones: top-`sim.topk` fp32 cosines
        under (similarity descending, index ascending), positive entries only, as device CSR (ptr int64, idx
        int32, val float32).  als_recommend_topk with k = d, U = normalised new rows, Z = normalised fitted rows,
        zero biases and mu = 0 computes exactly that; topk None / > 128 or d > 160 take the blocked torch
        formulation (same contract)."""
        md = self.model
        eps, topk = md.S_eps, md.S_topk
        Xn_new = layout.normalize_rows_f32(X_new, eps, self.dev)
        Xn_fit = layout.normalize_rows_f32(X_fit, eps, self.dev)
        B, d = Xn_new.shape
        if topk is None or topk > RECOMMEND_MAX_N or d > self.GRAPH_ROWS_MAX_D or d < 1:
            logger.warning("graph rows of new items: top-k %s / %d feature columns are outside what the top-k "
                           "kernel takes (top-k <= %d, d <= %d); using the blocked torch formulation", topk, d,
                           RECOMMEND_MAX_N, self.GRAPH_ROWS_MAX_D)
            return layout.similarity_rows_torch(Xn_new, Xn_fit, topk)
        ldd = layout.padded_k(d)
        Un = torch.zeros(B, ldd, dtype=torch.float32, device=self.dev)
        Un[:, :d] = Xn_new
        Zn = torch.zeros(self.n, ldd, dtype=torch.float32, device=self.dev)
        Zn[:, :d] = Xn_fit
        zu = torch.zeros(B, dtype=torch.float32, device=self.dev)
        side = dict(k=d, ld=ldd, n=self.n, Z=Zn, b_i=torch.zeros(self.n, dtype=torch.float32, device=self.dev),
                    mu=torch.zeros(1, dtype=torch.float64, device=self.dev))
        return layout.rows_from_topk(*self._topk_chunks(B, topk, self._table_rows(B, Un, zu), side, on_device=True))

    def fold_in_items(self, indptr, indices, vals, S, X_new: Dict[str, np.ndarray], n_sweeps: int):
        """Factors / biases of new items (host ratings CSR by user id, rows sorted; device graph rows S or None)
        against this fit's user side and V (one als_fold_in_items launch), and their Z = V + X_new W
        (als_compose_z): device fp32 ([B, ld], [B], [B, ld])."""
        md = self.model
        B = indptr.size - 1
        ptr_d, idx_d, val_d = self._csr_dev(indptr, indices, vals)
        if S is not None:
            S = self._csr_dev(*S)
        V = torch.empty(B, self.ld, dtype=torch.float32, device=self.dev)
        b = torch.empty(B, dtype=torch.float32, device=self.dev)
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.be.fold_in_items(k=self.k, ld=self.ld, indptr=ptr_d, indices=idx_d, vals=val_d, m=self.m, U=self.U,
                              b_u=self.b_u, mu=self.mu, S=S, n=self.n, V=self.V, lam_v=md.lambda_v,
                              pop_reg=bool(md.pop_reg_mode), lam_bi=md.lambda_bi,
                              alpha=md.alpha if S is not None else 0.0, n_sweeps=n_sweeps, V_out=V, b_i_out=b,
                              status=status)
        _raise_unless_solved(status, "item fold-in")
        if not self.feat_names:
            return V, b, V
        X = torch.from_numpy(concat_features(X_new, self.feat_names)).to(self.dev)
        Z = torch.empty_like(V)
        self.be.compose_z(V, X, self._concat_w(self.feat_names, self.feat_dims), Z)
        return V, b, Z

    def _folded_dev(self, folded: "FoldedItems"):
        """Z [B, ld] and b_i [B] of folded items back on the device (exact: they are fp32 values)."""
        B = folded.n_items
        Z = torch.zeros(B, self.ld, dtype=torch.float32, device=self.dev)
        Z[:, : self.k] = torch.from_numpy(folded.Z.astype(np.float32)).to(self.dev)
        return Z, torch.from_numpy(folded.b_i.astype(np.float32)).to(self.dev)

    def predict_new_items(self, us: torch.Tensor, folded: "FoldedItems") -> torch.Tensor:
        """Scores of the folded items for users `us` (int64, device): als_predict_dense on the gathered user rows,
        fp32 [len(us), B]."""
        Z, b_new = self._folded_dev(folded)
        out = torch.empty(us.numel(), folded.n_items, dtype=torch.float32, device=self.dev)
        self.be.predict_dense(k=self.k, ld=self.ld, m=us.numel(), n=folded.n_items, U=self.U.index_select(0, us),
                              Z=Z, b_u=self.b_u.index_select(0, us), b_i=b_new, mu=self.mu, out=out)
        return out

    def _joint_side(self, features, folded: "FoldedItems") -> dict:
        """The item tables of the n fitted items followed by the folded ones (ids n + b)."""
        Z_new, b_new = self._folded_dev(folded)
        return dict(k=self.k, ld=self.ld, n=self.n + folded.n_items, Z=torch.cat([self._compose_for(features), Z_new]),
                    b_i=torch.cat([self.b_i, b_new]), mu=self.mu)

    def _joint_rows(self, users_t: torch.Tensor, exclude_seen: bool, folded: "FoldedItems"):
        """Chunk source over the joint catalogue: the batch's user rows are gathered (batch row r = user
        users_t[r]) and their seen lists are the training row followed by the folded items they rated - ascending,
        as the new ids come last."""
        pairs = self._folded_rater_pairs(folded) if exclude_seen else None

        def rows(b0, nb):
            us = users_t[b0: b0 + nb].to(torch.int64)
            seen_ptr, seen_idx = self._merged_seen(us, *pairs) if exclude_seen else (None, None)
            return (torch.arange(nb, dtype=torch.int32, device=self.dev), self.U.index_select(0, us),
                    self.b_u.index_select(0, us), seen_ptr, seen_idx)
        return rows

    def _folded_rater_pairs(self, folded: Optional["FoldedItems"]):
        """The raters of the folded items, transposed: device (user int64, item n + b int32) pairs sorted by user,
        then item - what `_merged_seen` appends to the training rows.  No pairs without `folded`."""
        if folded is None:
            return (torch.empty(0, dtype=torch.int64, device=self.dev),
                    torch.empty(0, dtype=torch.int32, device=self.dev))
        rp, ri = folded.ratings[0], folded.ratings[1]
        new_u = ri.astype(np.int64)
        new_i = self.n + np.repeat(np.arange(folded.n_items, dtype=np.int64), np.diff(rp))
        o = np.lexsort((new_i, new_u))
        return torch.from_numpy(new_u[o]).to(self.dev), torch.from_numpy(new_i[o].astype(np.int32)).to(self.dev)

    def recommend_with_items(self, users_t: torch.Tensor, N: int, features, exclude_seen: bool,
                             folded: "FoldedItems", filters=None):
        """`recommend` over the n fitted items and the folded ones (ids n + b): one als_recommend_topk on the
        concatenated Z / b_i tables (`_joint_side`) with the gathered user rows and merged seen lists of
        `_joint_rows`.  The bitmap of `filters` spans the n + B ids of the concatenated table."""
        side, rows = self._catalogue(users_t, features, exclude_seen, folded)
        return self._topk_chunks(users_t.numel(), N, rows, side, filters=filters)

    # ----------------------------------------------------------- eligibility
    def eligibility_table(self, kind: str, payload, filters, n_total: int) -> "ItemEligibility":
        """The resident table of `ALS.eligibility` from validate.eligibility_inputs' (kind, payload).  "masks": bool
        [S, n_total] with the call's filters already ANDed in, packed on the host (`pack_words`), one upload.  "tags":
        the packed tags and rules go up and als_eligibility_bitmaps writes the table with the bitmap of `filters` (the
        validated (items, filter_items) pair or None) as its base, so nothing S x n exists on the host."""
        W = (n_total + 31) // 32
        if kind == "masks":
            return ItemEligibility(torch.from_numpy(pack_words(payload)).to(self.dev), payload.shape[0], n_total)
        tags, *rules = payload
        S = next(r for r in rules if r is not None).shape[0]
        up = lambda a: None if a is None else torch.from_numpy(a).to(self.dev)      # noqa: E731
        table = torch.empty(S, W, dtype=torch.int32, device=self.dev)
        self.be.eligibility_bitmaps(n=n_total, item_tags=up(tags), need_all=up(rules[0]), need_any=up(rules[1]),
                                    forbid=up(rules[2]), base_allow=self.allow_bitmap(filters, n_total), out=table)
        return ItemEligibility(table, S, n_total)

    def recommend_eligible(self, users_t: torch.Tensor, N: int, features, exclude_seen: bool, elig, row_seg,
                           folded: Optional["FoldedItems"] = None):
        """`recommend` (or `recommend_with_items` with `folded`) with the catalogue of batch row b restricted to row
        row_seg[b] (int32 [B], device) of the table `elig`: als_recommend_topk_segmented in REC_BATCH chunks."""
        side, rows = self._catalogue(users_t, features, exclude_seen, folded)
        return self._topk_chunks(users_t.numel(), N, rows, side, seg=(elig.table, row_seg))

    def recommend_new_eligible(self, indptr, indices, vals, N: int, features, n_sweeps: int, exclude_seen: bool,
                               elig, row_seg):
        """Fold in, then als_recommend_topk_segmented on the folded table, as `recommend_new`."""
        side, rows, *_ = self._new_catalogue(indptr, indices, vals, features, n_sweeps, exclude_seen)
        return self._topk_chunks(indptr.size - 1, N, rows, side, seg=(elig.table, row_seg))

    def rank_of_eligible(self, us: torch.Tensor, is_: torch.Tensor, features, exclude_seen: bool, elig, pair_seg,
                         folded: Optional["FoldedItems"] = None):
        """`rank_of` among the items eligible for each pair's segment (pair_seg int32 [P], device; the pairs of a
        user agree on it - the facade checked): grouped by user as `rank_of`, the segment of a user's row that of
        its first pair, als_rank_count_segmented in REC_BATCH chunks."""
        return self._rank_pairs(us, is_, features, exclude_seen, folded, elig=elig, pair_seg=pair_seg)

    # --------------------------------------------------------- exposure caps
    def _capacity_rounds(self, B: int, N: int, pick, items: dict, filters, capacity: np.ndarray, max_rounds):
        """The threshold rounds of `recommend_capacity` over B batch rows.  pick(ix) -> (users
        int32, U, b_u, seen_ptr, seen_idx) of the batch rows `ix` (int64, device, ascending): unlike the chunk sources
        of `_topk_chunks` it serves any subset, since the rounds after the first walk the dirty rows only.  `items`,
        `filters` as in `_topk_chunks`, the items of capacity 0 already blocked by `filters`
        (validate.capacity_filters); `capacity` int32 [n] (host).  The lists stay on the device; the host reads one
        int per round.  Returns host (items int64 [B, N], scores float64 [B, N],
        CapacityInfo)."""
        n = items["n"]
        if B * N > CAPACITY_MAX_PAIRS:
            raise ValueError(f"recommend_capacity keeps the batch's lists on the device: {B} rows x N = {N} is above "
                             f"CAPACITY_MAX_PAIRS = {CAPACITY_MAX_PAIRS} slots - split the batch (and its capacities)")
        allow = self.allow_bitmap(filters, n)
        cap = torch.from_numpy(capacity).to(self.dev)
        floor = torch.zeros(n, dtype=torch.int64, device=self.dev)          # the bits of the 64-bit floors
        fill = torch.empty(n, dtype=torch.int32, device=self.dev)
        dirty = torch.empty(B, dtype=torch.int32, device=self.dev)
        n_over = torch.empty(1, dtype=torch.int32, device=self.dev)
        top_val, top_idx, top_cnt = self._topn_out(B, N)

        def walk(ix, tv, ti, tc):
            users, U, b_u, seen_ptr, seen_idx = pick(ix)
            self.be.recommend_topk_priced(users=users, row_ids=ix.to(torch.int32), U=U, b_u=b_u, seen_ptr=seen_ptr,
                                          seen_idx=seen_idx, allow=allow, floor_key=floor, topn=N, top_val=tv,
                                          top_idx=ti, top_cnt=tc, **items)

        work, rounds, walked = None, 0, 0                                    # None: every row (round 0)
        while True:
            W = B if work is None else work.numel()
            for b0, nb in self._chunks(W, self.REC_BATCH):
                if work is None:
                    walk(torch.arange(b0, b0 + nb, dtype=torch.int64, device=self.dev), top_val[b0: b0 + nb],
                         top_idx[b0: b0 + nb], top_cnt[b0: b0 + nb])
                else:
                    ix = work[b0: b0 + nb]
                    tv, ti, tc = self._topn_out(nb, N)
                    walk(ix, tv, ti, tc)
                    top_val[ix], top_idx[ix] = tv, ti
            walked += W
            self.be.capacity_settle(n=n, top_idx=top_idx, top_val=top_val, capacity=cap, floor_key=floor, fill=fill,
                                    dirty=dirty, n_over=n_over)
            if int(n_over.item()) == 0:                                      # the round's only synchronisation
                break
            rounds += 1
            if max_rounds is not None and rounds > max_rounds:
                raise RuntimeError(f"recommend_capacity: items were still over-demanded after max_rounds = "
                                   f"{max_rounds} rounds")
            work = torch.nonzero(dirty).flatten()
        # the worst holder of every item, then NaN where the item is not full
        held = top_idx >= 0
        worst = torch.full((n,), float("inf"), dtype=torch.float32, device=self.dev)
        worst.scatter_reduce_(0, top_idx[held].to(torch.int64), top_val[held], "amin")
        cutoff = torch.where((fill == cap) & (cap > 0), worst.to(torch.float64), float("nan"))
        info = CapacityInfo(rounds, walked, fill.to(torch.int64).cpu().numpy(), cutoff.cpu().numpy())
        return top_idx.to(torch.int64).cpu().numpy(), top_val.to(torch.float64).cpu().numpy(), info

    def recommend_capacity(self, users_t: torch.Tensor, N: int, features, exclude_seen: bool, capacity: np.ndarray,
                           folded: Optional["FoldedItems"] = None, filters=None, max_rounds=None):
        """`recommend` (or `recommend_with_items` with `folded`) under per-item caps: `_capacity_rounds` with batch row
        b = user users_t[b]."""
        side = self._side(features, folded)
        if folded is None:
            seen_ptr = seen_idx = None
            if exclude_seen and self.nnz > 0:
                seen_ptr, seen_idx = self.csr.indptr, self.csr.indices

            def pick(ix):
                return users_t[ix], self.U, self.b_u, seen_ptr, seen_idx
        else:
            pairs = self._folded_rater_pairs(folded) if exclude_seen else None

            def pick(ix):                                                    # as `_joint_rows`, for any subset
                us = users_t[ix].to(torch.int64)
                seen_ptr, seen_idx = self._merged_seen(us, *pairs) if exclude_seen else (None, None)
                return (torch.arange(ix.numel(), dtype=torch.int32, device=self.dev), self.U.index_select(0, us),
                        self.b_u.index_select(0, us), seen_ptr, seen_idx)
        return self._capacity_rounds(users_t.numel(), N, pick, side, filters, capacity, max_rounds)

    def recommend_new_capacity(self, indptr, indices, vals, N: int, features, n_sweeps: int, exclude_seen: bool,
                               capacity: np.ndarray, filters=None, max_rounds=None):
        """Fold in, then `_capacity_rounds` on the folded table: batch row b = table row b, the given ratings as the
        seen CSR."""
        Z = self._compose_for(features)
        U, b, ptr_d, idx_d = self._fold_in_dev(indptr, indices, vals, Z, n_sweeps)
        seen = (ptr_d, idx_d) if exclude_seen and indptr[-1] > 0 else (None, None)
        return self._capacity_rounds(indptr.size - 1, N, lambda ix: (ix.to(torch.int32), U, b, *seen),
                                     self._item_side(Z), filters, capacity, max_rounds)

    # ----------------------------------------------------------- group quotas
    def _quota_chunks(self, B: int, N: int, rows, items: dict, allowed, labels: np.ndarray, caps: np.ndarray):
        """als_recommend_topk_quota over B batch rows in REC_BATCH chunks; `rows`, `items` as in
        `_topk_chunks`, `allowed` the call's filters as one host mask (bool [n]) or None, `labels` int32 [n] / `caps`
        int32 [G] from validate.item_groups, uploaded once.  The kernel is called with N_eff = `quota_plan`'s clamp - the
        longest list the caps allow - so that every list fills and the walk's threshold works; the columns N_eff ... N
        hold -1 / -inf, as they would anyway.  Returns host (items int64 [B, N], scores float64 [B, N])."""
        allowed, n_eff = quota_plan(allowed, labels, caps, N)
        out_i, out_v = np.full((B, N), -1, dtype=np.int64), np.full((B, N), -np.inf, dtype=np.float64)
        if n_eff == 0:
            return out_i, out_v
        allow = self.allow_bitmap(None if allowed is None else (allowed, None), items["n"])
        item_group, group_cap = torch.from_numpy(labels).to(self.dev), torch.from_numpy(caps).to(self.dev)

        def call(b0, nb, tv, ti, tc):
            users, U, b_u, seen_ptr, seen_idx = rows(b0, nb)
            self.be.recommend_topk_quota(users=users, U=U, b_u=b_u, seen_ptr=seen_ptr, seen_idx=seen_idx, allow=allow,
                                         item_group=item_group, group_cap=group_cap, topn=n_eff, top_val=tv,
                                         top_idx=ti, top_cnt=tc, **items)
        out_i[:, :n_eff], out_v[:, :n_eff] = self._collect_topn(B, n_eff, self.REC_BATCH, call)
        return out_i, out_v

    def recommend_quota(self, users_t: torch.Tensor, N: int, features, exclude_seen: bool, labels: np.ndarray,
                        caps: np.ndarray, folded: Optional["FoldedItems"] = None, allowed=None):
        """`recommend` (or `recommend_with_items` with `folded`) with at most caps[g] items of group g in a list."""
        side, rows = self._catalogue(users_t, features, exclude_seen, folded)
        return self._quota_chunks(users_t.numel(), N, rows, side, allowed, labels, caps)

    def recommend_new_quota(self, indptr, indices, vals, N: int, features, n_sweeps: int, exclude_seen: bool,
                            labels: np.ndarray, caps: np.ndarray, allowed=None):
        """Fold in, then `_quota_chunks` on the folded table, as `recommend_new`."""
        side, rows, *_ = self._new_catalogue(indptr, indices, vals, features, n_sweeps, exclude_seen)
        return self._quota_chunks(indptr.size - 1, N, rows, side, allowed, labels, caps)

    # ------------------------------------------------------------ deep lists
    def _deep_chunks(self, B: int, N: int, rows, items: dict, filters, after):
        """als_recommend_deep over B batch rows in chunks (DEEP_BATCH, DEEP_WS_BYTES); `rows`, `items`, `filters` as
        in `_topk_chunks`, `after` the validated (after_items int64 [B], after_scores float64 [B]) cursor or None.
        Returns host (items int64 [B, N], scores float64 [B, N]), copied chunk by chunk."""
        allow = self.allow_bitmap(filters, items["n"])
        keys = None if after is None else torch.from_numpy(cursor_keys(*after)).to(self.dev)
        step = min(B, self.DEEP_BATCH, self.REC_BATCH)     # the chunk sources are sized for REC_BATCH rows at most
        while step > 1 and self.be.recommend_deep_workspace_bytes(step, items["n"], N) > self.DEEP_WS_BYTES:
            step = (step + 1) // 2

        def call(b0, nb, tv, ti, tc):
            users, U, b_u, seen_ptr, seen_idx = rows(b0, nb)
            self.be.recommend_deep(users=users, U=U, b_u=b_u, seen_ptr=seen_ptr, seen_idx=seen_idx, allow=allow,
                                   after_key=None if keys is None else keys[b0: b0 + nb], topn=N, top_val=tv,
                                   top_idx=ti, top_cnt=tc, **items)
        return self._collect_topn(B, N, step, call)

    def recommend_deep(self, users_t: torch.Tensor, N: int, features, exclude_seen: bool,
                       folded: Optional["FoldedItems"] = None, filters=None, after=None):
        """`recommend` (or `recommend_with_items` with `folded`) for N up to RECOMMEND_DEEP_MAX_N, below the cursor
        `after` when given: als_recommend_deep in the chunks of `_deep_chunks`."""
        side, rows = self._catalogue(users_t, features, exclude_seen, folded)
        return self._deep_chunks(users_t.numel(), N, rows, side, filters, after)

    def recommend_new_deep(self, indptr, indices, vals, N: int, features, n_sweeps: int, exclude_seen: bool,
                           filters=None, after=None):
        """Fold in, then als_recommend_deep on the folded table, as `recommend_new`."""
        side, rows, *_ = self._new_catalogue(indptr, indices, vals, features, n_sweeps, exclude_seen)
        return self._deep_chunks(indptr.size - 1, N, rows, side, filters, after)

    # ------------------------------------------------------------ diversity
    def _pool_chunks(self, B: int, N: int, pool: int, rows, items: dict, filters, with_stat: bool, rerank):
        """The pool - `_topk_chunks` with N = pool, kept on the device - re-ranked in REC_BATCH chunks by
        rerank(b0, nb, cand_val, cand_idx, top_val, top_idx, top_cnt, stat): the chunk's pool rows, its [nb, N] outputs
        and `stat`, a fp32 [nb] per-list statistic the kernel writes (None without `with_stat`).  Only the [B, N]
        results come back: (items int64, scores float64, and the statistic float64 [B] or None)."""
        pool_val, pool_idx = self._topk_chunks(B, pool, rows, items, on_device=True, filters=filters)

        def call(b0, nb, tv, ti, tc):
            stat = torch.empty(nb, dtype=torch.float32, device=self.dev) if with_stat else None
            rerank(b0, nb, pool_val[b0: b0 + nb], pool_idx[b0: b0 + nb], tv, ti, tc, stat)
            return (stat,) if with_stat else ()
        out = self._collect_topn(B, N, self.REC_BATCH, call, extra=((),) if with_stat else ())
        return out if with_stat else (*out, None)

    def _rerank_chunks(self, B: int, N: int, pool: int, lam: float, rows, items: dict, filters, with_ild: bool):
        """`_pool_chunks` with als_mmr_rerank against the Z the pool was scored with: (items int64, scores float64,
        and ild float64 [B] or None)."""
        def rerank(b0, nb, cand_val, cand_idx, tv, ti, tc, ild):
            self.be.mmr_rerank(k=items["k"], ld=items["ld"], n=items["n"], Z=items["Z"], cand_val=cand_val,
                               cand_idx=cand_idx, lam=lam, topn=N, top_val=tv, top_idx=ti, top_cnt=tc, top_ild=ild)
        return self._pool_chunks(B, N, pool, rows, items, filters, with_ild, rerank)

    def recommend_diverse(self, users_t: torch.Tensor, N: int, pool: int, lam: float, features, exclude_seen: bool,
                          folded: Optional["FoldedItems"] = None, filters=None, with_ild: bool = False):
        """`recommend(N=pool)` (or `recommend_with_items` with `folded`) on the device, then the MMR re-rank."""
        side, rows = self._catalogue(users_t, features, exclude_seen, folded)
        return self._rerank_chunks(users_t.numel(), N, pool, lam, rows, side, filters, with_ild)

    def recommend_new_diverse(self, indptr, indices, vals, N: int, pool: int, lam: float, features, n_sweeps: int,
                              exclude_seen: bool, filters=None, with_ild: bool = False):
        """`recommend_new(N=pool)` on the device, then the MMR re-rank."""
        side, rows, *_ = self._new_catalogue(indptr, indices, vals, features, n_sweeps, exclude_seen)
        return self._rerank_chunks(indptr.size - 1, N, pool, lam, rows, side, filters, with_ild)

    def list_diversity(self, lists: torch.Tensor, features, folded: Optional["FoldedItems"] = None) -> np.ndarray:
        """ILD float64 [B] of the id lists `lists` (int32 [B, L], -1 padded, device): als_list_diversity in
        REC_BATCH chunks against the Z of `recommend` (the joint table with `folded`)."""
        side = self._side(features, folded)

        def call(b0, nb):
            ild = torch.empty(nb, dtype=torch.float32, device=self.dev)
            self.be.list_diversity(k=side["k"], ld=side["ld"], n=side["n"], Z=side["Z"], idx=lists[b0: b0 + nb],
                                   ild=ild)
            return (ild,)
        return self._collect(lists.shape[0], self.REC_BATCH, (((), np.float64),), call)[0]

    # ---------------------------------------------------------- calibration
    def _fitted_history(self, users_t: torch.Tensor):
        """History source of the calibration drivers for users of the fit: hist(b0, nb) -> (indptr, indices, rows)
        of als_category_profile - the training CSR, batch row b = its row users_t[b]."""
        ptr, idx, _ = self._csr_dev(self.csr.indptr, self.csr.indices, self.csr.vals)
        return lambda b0, nb: (ptr, idx, users_t[b0: b0 + nb])

    @staticmethod
    def _table_history(ptr_d: torch.Tensor, idx_d: torch.Tensor):
        """History source for a CSR made for the call (batch row b = its row b): a view of the row pointers, the
        offsets stay absolute."""
        return lambda b0, nb: (ptr_d[b0: b0 + nb + 1], idx_d, None)

    def _profile_chunk(self, C: torch.Tensor, ncat: int, hist, b0: int, nb: int) -> torch.Tensor:
        """als_category_profile of the batch rows [b0, b0 + nb): fp32 [nb, ldc] on the device."""
        P = torch.empty(nb, C.shape[1], dtype=torch.float32, device=self.dev)
        indptr, indices, rows = hist(b0, nb)
        self.be.category_profile(ncat=ncat, indptr=indptr, indices=indices, rows=rows, n=C.shape[0], C=C, P_out=P)
        return P

    def _calibrate_chunks(self, B: int, N: int, pool: int, lam: float, alpha: float, rows, items: dict, filters,
                          table: np.ndarray, ncat: int, hist, target: Optional[np.ndarray], with_kl: bool):
        """`_pool_chunks` with als_calibrated_rerank over the category table `table` (validate.category_table of the
        catalogue scored, uploaded once): per chunk the targets are the rows of `target` (validate.target_rows) or,
        without one, the profiles of the histories `hist` (als_category_profile).  Returns (items int64, scores
        float64, and the lists' miscalibration float64 [B] or None)."""
        C = torch.from_numpy(table).to(self.dev)
        T = None if target is None else torch.from_numpy(target).to(self.dev)

        def rerank(b0, nb, cand_val, cand_idx, tv, ti, tc, kl):
            P = T[b0: b0 + nb] if T is not None else self._profile_chunk(C, ncat, hist, b0, nb)
            self.be.calibrated_rerank(ncat=ncat, n=items["n"], C=C, P=P, cand_val=cand_val, cand_idx=cand_idx,
                                      lam=lam, alpha=alpha, topn=N, top_val=tv, top_idx=ti, top_cnt=tc, top_kl=kl)
        return self._pool_chunks(B, N, pool, rows, items, filters, with_kl, rerank)

    def recommend_calibrated(self, users_t: torch.Tensor, N: int, pool: int, lam: float, alpha: float,
                             table: np.ndarray, ncat: int, target, features, exclude_seen: bool,
                             folded: Optional["FoldedItems"] = None, filters=None, with_kl: bool = False):
        """`recommend(N=pool)` (or `recommend_with_items` with `folded`) on the device, then the calibrated re-rank
        towards the profile of the user's training row (or `target`)."""
        side, rows = self._catalogue(users_t, features, exclude_seen, folded)
        return self._calibrate_chunks(users_t.numel(), N, pool, lam, alpha, rows, side, filters, table, ncat,
                                      self._fitted_history(users_t), target, with_kl)

    def recommend_new_calibrated(self, indptr, indices, vals, N: int, pool: int, lam: float, alpha: float,
                                 table: np.ndarray, ncat: int, target, features, n_sweeps: int, exclude_seen: bool,
                                 filters=None, with_kl: bool = False):
        """`recommend_new(N=pool)` on the device, then the calibrated re-rank towards the profile of the given
        ratings (or `target`)."""
        side, rows, ptr_d, idx_d = self._new_catalogue(indptr, indices, vals, features, n_sweeps, exclude_seen)
        return self._calibrate_chunks(indptr.size - 1, N, pool, lam, alpha, rows, side, filters, table, ncat,
                                      self._table_history(ptr_d, idx_d), target, with_kl)

    def category_profile(self, users_t: torch.Tensor, table: np.ndarray, ncat: int) -> np.ndarray:
        """float64 [B, ncat]: the category profiles of the training rows of `users_t` (int32, device),
        als_category_profile in REC_BATCH chunks."""
        C = torch.from_numpy(table).to(self.dev)
        hist = self._fitted_history(users_t)
        return self._collect(users_t.numel(), self.REC_BATCH, (((ncat,), np.float64),),
                             lambda b0, nb: (self._profile_chunk(C, ncat, hist, b0, nb)[:, :ncat],))[0]

    def list_miscalibration(self, lists: torch.Tensor, table: np.ndarray, ncat: int, alpha: float,
                            users_t: Optional[torch.Tensor], target: Optional[np.ndarray]) -> np.ndarray:
        """Miscalibration float64 [B] of the id lists `lists` (int32 [B, L], -1 padded, device) against the profiles
        of the users `users_t` or the rows of `target`: als_list_miscalibration in REC_BATCH chunks."""
        C = torch.from_numpy(table).to(self.dev)
        T = None if target is None else torch.from_numpy(target).to(self.dev)
        hist = None if users_t is None else self._fitted_history(users_t)

        def call(b0, nb):
            P = T[b0: b0 + nb] if T is not None else self._profile_chunk(C, ncat, hist, b0, nb)
            kl = torch.empty(nb, dtype=torch.float32, device=self.dev)
            self.be.list_miscalibration(ncat=ncat, n=C.shape[0], C=C, P=P, idx=lists[b0: b0 + nb], alpha=alpha, kl=kl)
            return (kl,)
        return self._collect(lists.shape[0], self.REC_BATCH, (((), np.float64),), call)[0]

    # ----------------------------------------------------------- neighbours
    def _similar_chunks(self, T: torch.Tensor, ids: torch.Tensor, N: int, filters=None):
        """The N rows of the table T [rows, ld] most similar (cosine) to each of its rows `ids` (int32, device), a row
        never its own neighbour: one als_row_inv_norms launch over T per call (nothing is kept between calls, so a
        refit or other features cannot meet stale norms), then als_similar_topk in REC_BATCH chunks.  `filters`: as
        in `_topk_chunks`, over the rows of T.  Returns host (ids int64 [B, N], sims float64 [B, N]), unused
        slots -1 / -inf."""
        B, rows = ids.numel(), T.shape[0]
        allow = self.allow_bitmap(filters, rows)
        inv = torch.empty(rows, dtype=torch.float32, device=self.dev)
        self.be.row_inv_norms(k=self.k, ld=self.ld, T=T, inv_norm=inv)

        def call(b0, nb, tv, ti, tc):
            q = ids[b0: b0 + nb]
            self.be.similar_topk(k=self.k, ld=self.ld, q_ids=q, Q=T, q_inv=inv, self_ids=q, n=rows, T=T, t_inv=inv,
                                 allow=allow, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)
        return self._collect_topn(B, N, self.REC_BATCH, call)

    def similar_items(self, items_t: torch.Tensor, N: int, features, filters=None):
        """Nearest items of the items `items_t` (int32, device) by the cosine of their rows of Z, composed as in
        `list_diversity`; `filters` restricts the neighbours, not the queries."""
        return self._similar_chunks(self._compose_for(features), items_t, N, filters)

    def similar_users(self, users_t: torch.Tensor, N: int):
        """Nearest users of the users `users_t` (int32, device) by the cosine of their rows of U."""
        return self._similar_chunks(self.U, users_t, N)

    # ------------------------------------------------------------- audience
    def _rater_rows(self, folded: Optional["FoldedItems"]):
        """The rater CSR als_audience_topk excludes by, indexed by item id: the training CSC, followed with `folded`
        by the rows of its ratings (item n + b = row n + b) - one indptr with the second part's offsets shifted, one
        index array, built on the device.  (None, None) when no item has a rater."""
        ptr, idx, total = self.csc.indptr, self.csc.indices, self.nnz
        if folded is not None:
            fptr = torch.from_numpy(np.asarray(folded.ratings[0], dtype=np.int64)).to(self.dev)
            fidx = torch.from_numpy(np.asarray(folded.ratings[1], dtype=np.int32)).to(self.dev)
            ptr = torch.cat([ptr, fptr[1:] + self.nnz])
            idx = torch.cat([idx[: self.nnz], fidx])
            total += int(fidx.numel())
        if total == 0:
            return None, None
        return ptr, idx

    def recommend_users(self, items_t: torch.Tensor, N: int, features, exclude_seen: bool,
                        folded: Optional["FoldedItems"] = None, filters=None):
        """Top-N users of the items `items_t` (int32, device; ids >= n are the folded items of `folded`): (users
        int64 [B, N], scores float64 [B, N]), unused slots -1 / -inf - als_audience_topk in REC_BATCH chunks.  The
        query table is the Z of `predict` (the joint table of `_joint_side` with `folded`), the raters left out are
        `_rater_rows`; `filters`: the validated user allow / block pair of the call over the m users, or None."""
        side = self._side(features, folded)
        seen_ptr, seen_idx = self._rater_rows(folded) if exclude_seen else (None, None)
        allow = self.allow_bitmap(filters, self.m)

        def call(b0, nb, tv, ti, tc):
            self.be.audience_topk(k=self.k, ld=self.ld, q_ids=items_t[b0: b0 + nb], Q=side["Z"], q_bias=side["b_i"],
                                  m=self.m, U=self.U, b_u=self.b_u, mu=self.mu, seen_ptr=seen_ptr, seen_idx=seen_idx,
                                  allow=allow, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)
        return self._collect_topn(items_t.numel(), N, self.REC_BATCH, call)

    # --------------------------------------------------------------- groups
    def _group_seen(self, members: torch.Tensor, ptr: torch.Tensor, n_total: int, new_u: torch.Tensor,
                    new_i: torch.Tensor):
        """Seen CSR by batch group (device): the union of the members' seen rows - an item any member has seen is
        out.  `members` int32, group b = members[ptr[b]:ptr[b + 1]]; the members' rows are gathered as `_merged_seen`
        gathers them (training row, then the folded items of the pairs new_u / new_i), keyed by (group, item),
        sorted, repeats dropped, counted.  (None, None) when no member has seen anything."""
        mptr, midx = self._merged_seen(members.to(torch.int64), new_u, new_i)
        if mptr is None:
            return None, None
        nb = ptr.numel() - 1
        group_of_member = torch.repeat_interleave(torch.arange(nb, device=self.dev), ptr[1:] - ptr[:-1])
        group = torch.repeat_interleave(group_of_member, mptr[1:] - mptr[:-1])
        key = torch.unique(group * n_total + midx[: group.numel()].to(torch.int64))      # ascending, distinct
        group = torch.div(key, n_total, rounding_mode="floor")
        out_ptr = torch.zeros(nb + 1, dtype=torch.int64, device=self.dev)
        torch.cumsum(torch.bincount(group, minlength=nb), 0, out=out_ptr[1:])
        return out_ptr, (key - group * n_total).to(torch.int32)

    def recommend_group(self, g_ptr: np.ndarray, g_users: np.ndarray, N: int, aggregate: str, features,
                        exclude_seen: bool, folded: Optional["FoldedItems"] = None, filters=None):
        """Top-N items of the groups g_users[g_ptr[b]:g_ptr[b + 1]] (validate.user_groups: host int64 / int32) under
        `aggregate`: (items int64 [G, N], scores float64 [G, N]), unused slots -1 / -inf - als_group_topk in REC_BATCH
        chunks of groups.  The item tables are the Z of `predict` (the joint table of `_joint_side` with `folded`);
        the members index the resident U / b_u; per chunk the seen rows of the groups are `_group_seen`; `filters`:
        the validated item allow / block pair of the call over the catalogue scored, or None."""
        side = self._side(features, folded)
        allow = self.allow_bitmap(filters, side["n"])
        sizes = np.diff(g_ptr)
        ptr_d = torch.from_numpy(g_ptr).to(self.dev)
        users_d = torch.from_numpy(g_users).to(self.dev)
        new_u, new_i = self._folded_rater_pairs(folded if exclude_seen else None)

        def call(b0, nb, tv, ti, tc):
            p0, p1 = int(g_ptr[b0]), int(g_ptr[b0 + nb])
            ptr = (ptr_d[b0: b0 + nb + 1] - p0).contiguous()
            members = users_d[p0:p1]
            seen_ptr = seen_idx = None
            if exclude_seen and (self.nnz > 0 or new_u.numel() > 0):
                seen_ptr, seen_idx = self._group_seen(members, ptr, side["n"], new_u, new_i)
            self.be.group_topk(g_ptr=ptr, g_users=members, max_members=int(sizes[b0: b0 + nb].max()), U=self.U,
                               b_u=self.b_u, seen_ptr=seen_ptr, seen_idx=seen_idx, allow=allow, aggregate=aggregate,
                               topn=N, top_val=tv, top_idx=ti, top_cnt=tc, **side)
        return self._collect_topn(g_ptr.size - 1, N, self.REC_BATCH, call)

    def _merged_seen(self, us: torch.Tensor, new_u: torch.Tensor, new_i: torch.Tensor):
        """Seen CSR of batch rows r = user us[r] (device): the user's training row, then the folded items
        (ids >= n) they rated, taken from the (user, item)-sorted pairs new_u / new_i."""
        ptr, idx = self.csr.indptr, self.csr.indices
        beg_f = ptr[us]
        cnt_f = ptr[us + 1] - beg_f
        beg_n = torch.searchsorted(new_u, us)
        cnt_n = torch.searchsorted(new_u, us, right=True) - beg_n
        cnt = cnt_f + cnt_n
        out_ptr = torch.zeros(us.numel() + 1, dtype=torch.int64, device=self.dev)
        out_ptr[1:] = torch.cumsum(cnt, 0)
        total = int(out_ptr[-1])
        out_idx = torch.empty(max(total, 1), dtype=torch.int32, device=self.dev)
        rows = torch.arange(us.numel(), device=self.dev)
        for beg, c, skip, src in ((beg_f, cnt_f, None, idx), (beg_n, cnt_n, cnt_f, new_i)):
            tot = int(c.sum())
            if tot == 0:
                continue
            r = torch.repeat_interleave(rows, c)
            first = torch.cumsum(c, 0) - c                       # position of each row's first entry in this part
            off = torch.arange(tot, device=self.dev) - first[r]
            dst = out_ptr[r] + off + (skip[r] if skip is not None else 0)
            out_idx[dst] = src[beg[r] + off]
        if total == 0:
            return None, None
        return out_ptr, out_idx

    # ----------------------------------------------------------- exploration
    @staticmethod
    def thompson_table(U: torch.Tensor, W: torch.Tensor, eps: torch.Tensor, beta: float) -> torch.Tensor:
        """One posterior sample per row: u + beta W^T eps (fp32 [B, ld]; U [B, ld], W [B, ld, ld] the whiteners,
        eps [B, ld] standard normal, zero in the padding columns) - cov(W^T eps) = W^T W = A^-1."""
        return U + beta * torch.bmm(W.transpose(1, 2), eps.unsqueeze(2)).squeeze(2)

    def _explore_chunks(self, B: int, N: int, beta: float, eps, rows, table_rows, wrows, items: dict, filters,
                        row_name):
        """als_row_whitener + als_explore_topk over B batch rows in chunks of `EXPLORE_BATCH` rows.  rows(b0, nb) as in
        `_topk_chunks` (the seen CSR by USER ID), as are `items` and `filters`; wrows(b0, nb) -> (indptr, indices,
        rows) of the whitener's work rows; `eps` (fp32 [B, ld], device) switches to Thompson sampling: table_rows(b0,
        nb) -> (U, b_u, seen_ptr, seen_idx) gathered by BATCH ROW, the sampled table of `thompson_table` goes through
        als_recommend_topk and the leverages of the returned items are formed from W in torch.  Returns host (items
        int64, keys float64, leverage float64), each [B, N], unused slots -1 / -inf / 0."""
        md, ld = self.model, self.ld
        allow = self.allow_bitmap(filters, items["n"])
        cb = min(self.REC_BATCH, self.EXPLORE_BATCH or max(1, self.EXPLORE_W_BYTES // (4 * ld * ld)))
        W = torch.empty(min(B, cb), ld, ld, dtype=torch.float32, device=self.dev)
        status = torch.zeros(1, dtype=torch.int32, device=self.dev)

        def call(b0, nb, tv, ti, tc):
            indptr, indices, wr = wrows(b0, nb)
            self.be.row_whitener(k=self.k, ld=ld, indptr=indptr, indices=indices, rows=wr, n=self.n, Z=items["Z"],
                                 lam_u=md.lambda_u, W_out=W, status=status)
            _raise_unless_solved(status, "explore", lambda r: row_name(b0 + r))
            if eps is None:
                tl = torch.empty(nb, N, dtype=torch.float32, device=self.dev)
                users, U, b_u, seen_ptr, seen_idx = rows(b0, nb)
                self.be.explore_topk(users=users, U=U, b_u=b_u, W=W, beta=beta, seen_ptr=seen_ptr, seen_idx=seen_idx,
                                     allow=allow, topn=N, top_val=tv, top_idx=ti, top_cnt=tc, top_lev=tl, **items)
                return (tl,)
            U, b_u, seen_ptr, seen_idx = table_rows(b0, nb)
            self._restricted("recommend_topk", allow, None, b0, nb,
                             users=torch.arange(nb, dtype=torch.int32, device=self.dev),
                             U=self.thompson_table(U[:nb], W[:nb], eps[b0: b0 + nb], beta).contiguous(), b_u=b_u,
                             seen_ptr=seen_ptr, seen_idx=seen_idx, topn=N, top_val=tv, top_idx=ti, top_cnt=tc, **items)
            y = torch.bmm(items["Z"][ti.clamp(min=0).to(torch.int64)], W[:nb].transpose(1, 2))         # [nb, N, ld]
            return (torch.where(ti >= 0, (y * y).sum(dim=2), torch.zeros((), device=self.dev)),)
        return self._collect_topn(B, N, cb, call, extra=((N,),))

    def _thompson_eps(self, B: int, seed) -> Optional[torch.Tensor]:
        """default_rng(seed).standard_normal((B, k)) as fp32 on the device, zero padded to ld; None without a seed."""
        if seed is None:
            return None
        eps = np.zeros((B, self.ld), dtype=np.float32)
        eps[:, : self.k] = np.random.default_rng(seed).standard_normal((B, self.k)).astype(np.float32)
        return torch.from_numpy(eps).to(self.dev)

    def recommend_explore(self, users_t: torch.Tensor, N: int, beta: float, seed, features, exclude_seen: bool,
                          filters=None):
        """Top-N of the users in `users_t` (int32, device) by score + beta * sigma, sigma^2 the leverage of the item
        under the user's training row; `seed` not None: one Thompson sample per batch row instead.  See
        `_explore_chunks` for the return."""
        Z = self._compose_for(features)
        B = users_t.numel()
        ptr_d, idx_d, _ = self._csr_dev(self.csr.indptr, self.csr.indices, self.csr.vals)
        with_seen = exclude_seen and self.nnz > 0
        no_pairs = self._folded_rater_pairs(None)

        def table_rows(b0, nb):
            us = users_t[b0: b0 + nb].to(torch.int64)
            seen = self._merged_seen(us, *no_pairs) if with_seen else (None, None)
            return (self.U.index_select(0, us), self.b_u.index_select(0, us), *seen)
        return self._explore_chunks(B, N, beta, self._thompson_eps(B, seed), self._fitted_rows(users_t, exclude_seen),
                                    table_rows, lambda b0, nb: (ptr_d, idx_d, users_t[b0: b0 + nb]),
                                    self._item_side(Z), filters,
                                    lambda w: f"user {int(users_t[w])}")

    def recommend_new_explore(self, indptr, indices, vals, N: int, beta: float, seed, features, n_sweeps: int,
                              exclude_seen: bool, filters=None):
        """`recommend_explore` for rows outside the fit (host CSR, rows sorted): fold in, whiten the same rows, rank."""
        B = indptr.size - 1
        side, rows, ptr_d, idx_d = self._new_catalogue(indptr, indices, vals, features, n_sweeps, exclude_seen)
        return self._explore_chunks(B, N, beta, self._thompson_eps(B, seed), rows, lambda b0, nb: rows(b0, nb)[1:],
                                    lambda b0, nb: (ptr_d[b0: b0 + nb + 1], idx_d, None), side,
                                    filters, lambda w: f"row {w}")
