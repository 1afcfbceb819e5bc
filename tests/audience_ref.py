"""The contract of als_audience_topk (include/als_hip.h) in numpy, and the stand-in backend that serves it to the
engine on the CPU.

`audience_topn` takes the fp32 scores as given - on the GPU the columns als_predict_dense writes, which the kernel's
scores equal bitwise - and selects with serving_ref.topn_batch, so the order rule (score descending, user id
ascending, NaN never a candidate) is written once.  `AudienceNumpyBackend` forms the scores with the stand-in's own
`predict_dense`, so the bias association ((dot + mu) + b_u) + b_i has a single definition; it also carries a
`fold_in_items` (serving_ref.fold_in_item row by row), which the stand-in lacked and the audience of a folded item
needs.  tests/cpu_backend.py and tests/similar_ref.py are not touched."""
import numpy as np
import torch

from tests import serving_ref as ref
from tests.similar_ref import SimilarNumpyBackend


def audience_topn(scores_f32, rater_rows, allowed, N):
    """What als_audience_topk writes for a batch: (values float32 [B, N] padded with -inf, users int32 [B, N] padded
    with -1, counts int32 [B]).  scores_f32 [B, m]: row b holds the scores of all m users for the item of batch row b;
    rater_rows: per batch row the user ids left out; allowed: bool [m] or None."""
    scores = np.asarray(scores_f32)
    assert scores.dtype == np.float32
    return ref.topn_batch(scores, rater_rows, allowed, N)


def rater_rows(q_ids, seen_ptr, seen_idx):
    """Row q_ids[b] of the rater CSR for every batch row (empty rows when the CSR is None)."""
    none = np.zeros(0, np.int64)
    if seen_ptr is None:
        return [none for _ in q_ids]
    return [np.asarray(seen_idx[seen_ptr[i]: seen_ptr[i + 1]], dtype=np.int64) for i in q_ids]


class AudienceNumpyBackend(SimilarNumpyBackend):
    """SimilarNumpyBackend with `audience_topk`: the scores are the stand-in's predict_dense over (all users, the
    distinct query items), transposed."""

    def fold_in_items(self, *, k, ld, indptr, indices, vals, m, U, b_u, mu, S, n, V, lam_v, pop_reg, lam_bi, alpha,
                      n_sweeps, V_out, b_i_out, status):
        """als_fold_in_items by serving_ref.fold_in_item, row by row (the stand-in of cpu_backend.py has none; the
        audience of a folded item needs one)."""
        ptr = indptr.numpy()
        Uh, buh, Vh, muh = U.numpy(), b_u.numpy(), V.numpy()[:n, :k], float(mu.item())
        V_out.zero_()
        none_i, none_v = np.zeros(0, np.int64), np.zeros(0, np.float32)
        for b in range(ptr.size - 1):
            s = slice(ptr[b], ptr[b + 1])
            nb_i, nb_v = none_i, none_v
            if S is not None:
                g = slice(int(S[0][b]), int(S[0][b + 1]))
                nb_i, nb_v = S[1][g].numpy().astype(np.int64), S[2][g].numpy()
            v, bi = ref.fold_in_item(Uh, buh, muh, Vh, indices[s].numpy().astype(np.int64), vals[s].numpy(), nb_i,
                                     nb_v, float(lam_v), bool(pop_reg), float(lam_bi), float(alpha), int(n_sweeps))
            V_out[b, :k] = torch.from_numpy(v.astype(np.float32))
            b_i_out[b] = float(np.float32(bi))

    def audience_topk(self, *, k, ld, q_ids, Q, q_bias, m, U, b_u, mu, seen_ptr, seen_idx, allow, topn, top_val,
                      top_idx, top_cnt):
        self.calls.append(("audience_topk", q_ids.numel(), Q.data_ptr(), Q.shape[0],
                           None if seen_ptr is None else seen_ptr.numel(), None if allow is None else allow.data_ptr()))
        q = q_ids.long()
        rows = Q.shape[0]
        dense = torch.empty(m, rows, dtype=torch.float32)
        self.predict_dense(k=k, ld=ld, m=m, n=rows, U=U, Z=Q, b_u=b_u, b_i=q_bias, mu=mu, out=dense)
        S = np.ascontiguousarray(dense.numpy().T[q.numpy()])
        ok = None if allow is None else ref.unpack_bitmap(allow.numpy(), m)
        seen = rater_rows(q.tolist(), None if seen_ptr is None else seen_ptr.numpy(),
                          None if seen_idx is None else seen_idx.numpy())
        for dst, a in zip((top_val, top_idx, top_cnt), audience_topn(S, seen, ok, topn)):
            dst[: a.shape[0]] = torch.from_numpy(a)
