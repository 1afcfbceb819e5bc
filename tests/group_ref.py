"""The contract of als_group_topk (include/als_hip.h) in numpy, and the stand-in backend that serves it to the engine
on the CPU.

`group_scores` folds the members' fp32 scores of every item into the group's: numpy's min / max, which PROPAGATE a NaN
(so an item with a NaN member score is a NaN and `serving_ref.candidates` drops it, whatever the other members say),
or the fp64 sum of the fp32 scores divided by the group size in fp64 and rounded once to fp32.  `group_topn` takes the
member scores as given - on the GPU the rows als_predict_dense writes, which the kernel's member scores equal bitwise -
and selects with serving_ref.topn_batch, so the order rule (score descending, item id ascending, NaN never a
candidate) is written once.  numpy adds the fp64 sum in an order of its own; the sum is exact, and so the same in any
order, when the nonzero member scores of an item lie within a factor 2^17 of each other (24-bit values, at most 64 of
them, a 53-bit accumulator) - the tests that compare a mean with == keep their inputs inside that band.
`GroupNumpyBackend` forms the member scores with the stand-in's own `predict_dense`."""
import numpy as np
import torch

from tests import serving_ref as ref
from tests.audience_ref import AudienceNumpyBackend

AGGREGATES = ("mean", "min", "max")


def group_scores(member_scores_f32, aggregate):
    """fp32 [n]: the group score of every item from the members' scores fp32 [g, n]."""
    s = np.asarray(member_scores_f32)
    assert s.dtype == np.float32 and s.ndim == 2 and s.shape[0] >= 1
    if aggregate == "min":
        return s.min(axis=0)
    if aggregate == "max":
        return s.max(axis=0)
    assert aggregate == "mean"
    with np.errstate(invalid="ignore"):                     # +inf and -inf members: a NaN, and no candidate
        return (s.astype(np.float64).sum(axis=0) / s.shape[0]).astype(np.float32)


def group_topn(member_scores, seen_rows, allowed, N, aggregate):
    """What als_group_topk writes for a batch: (values float32 [G, N] padded with -inf, items int32 [G, N] padded with
    -1, counts int32 [G]).  member_scores: per group the fp32 scores [g, n] of its members (g == 0: an empty list);
    seen_rows: per group the item ids left out; allowed: bool [n] or None."""
    n = None
    for s in member_scores:
        n = np.asarray(s).shape[1]
    rows = [group_scores(s, aggregate) if np.asarray(s).shape[0] else np.full(n, np.nan, np.float32)
            for s in member_scores]
    return ref.topn_batch(np.stack(rows), seen_rows, allowed, N)


def seen_rows(seen_ptr, seen_idx, G):
    """Row b of the per-group seen CSR for every batch group (empty rows when the CSR is None)."""
    if seen_ptr is None:
        return [np.zeros(0, np.int64) for _ in range(G)]
    return [np.asarray(seen_idx[seen_ptr[b]: seen_ptr[b + 1]], dtype=np.int64) for b in range(G)]


class GroupNumpyBackend(AudienceNumpyBackend):
    """AudienceNumpyBackend with `group_topk`: the member scores are rows of the stand-in's predict_dense over (all
    users, all items)."""

    def group_topk(self, *, k, ld, g_ptr, g_users, max_members, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow,
                   aggregate, topn, top_val, top_idx, top_cnt):
        G = g_ptr.numel() - 1
        self.calls.append(("group_topk", G, Z.data_ptr(), n, None if seen_ptr is None else seen_ptr.numel(),
                           None if allow is None else allow.data_ptr(), int(max_members), aggregate))
        ptr, users = g_ptr.numpy(), g_users.numpy().astype(np.int64)
        assert ptr[0] == 0 and (np.diff(ptr) <= max_members).all() and max_members <= 64
        if seen_ptr is not None:
            sp, si = seen_ptr.numpy(), seen_idx.numpy()
            assert sp.size == G + 1                         # indexed by batch group, ascending and distinct per row
            assert all((np.diff(si[sp[b]: sp[b + 1]]) > 0).all() for b in range(G))
        m = U.shape[0]
        dense = torch.empty(m, n, dtype=torch.float32)
        self.predict_dense(k=k, ld=ld, m=m, n=n, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, out=dense)
        S = dense.numpy()
        member_scores = [S[users[ptr[b]: ptr[b + 1]]] for b in range(G)]
        ok = None if allow is None else ref.unpack_bitmap(allow.numpy(), n)
        seen = seen_rows(None if seen_ptr is None else seen_ptr.numpy(),
                         None if seen_idx is None else seen_idx.numpy(), G)
        for dst, a in zip((top_val, top_idx, top_cnt), group_topn(member_scores, seen, ok, topn, aggregate)):
            dst[: a.shape[0]] = torch.from_numpy(a)
