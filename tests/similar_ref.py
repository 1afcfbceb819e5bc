"""The contract of als_row_inv_norms / als_similar_topk (include/als_hip.h) in numpy, and the stand-in backend that
serves it to the engine on the CPU.

`inv_norms` is float64 throughout.  `similar_topn` takes the fp32 dot products as given - on the GPU the rows
als_predict_dense writes for zero biases and mu = 0, which the kernel's dots equal bitwise - forms
(d * q_inv) * t_inv in np.float32, the kernel's association, and selects with serving_ref.topn_batch, so the order
rule (similarity descending, id ascending, NaN never a candidate) is written once.  tests/cpu_backend.py is not
touched: `SimilarNumpyBackend` adds the two methods to it."""
import numpy as np
import torch

from tests import serving_ref as ref
from tests.cpu_backend import NumpyBackend


def inv_norms(T):
    """float64 [rows]: 1 / sqrt(sum_c T[r][c]^2) in float64; 0 for an all-zero row, NaN for a row with a non-finite
    entry."""
    T = np.asarray(T, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = (T * T).sum(axis=1)
        inv = 1.0 / np.sqrt(s)
    inv[s == 0] = 0.0
    inv[~np.isfinite(s)] = np.nan
    return inv


def similarities(dots_f32, q_inv, t_inv):
    """float32 [B, n]: (dots[b, j] * q_inv[b]) * t_inv[j], every product rounded to float32."""
    d = np.asarray(dots_f32, dtype=np.float32)
    iq = np.asarray(q_inv, dtype=np.float32)[:, None]
    ij = np.asarray(t_inv, dtype=np.float32)[None, :]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        sim = (d * iq) * ij
    assert sim.dtype == np.float32
    return sim


def similar_topn(dots_f32, q_inv, t_inv, self_ids, allow, N):
    """What als_similar_topk writes for a batch: (values float32 [B, N] padded with -inf, ids int32 [B, N] padded
    with -1, counts int32 [B]).  dots_f32 [B, n]; q_inv [B]: the inverse norm of every batch row's query; t_inv [n];
    self_ids [B] (None or -1: nothing excluded); allow: bool [n] or None."""
    sim = similarities(dots_f32, q_inv, t_inv)
    B = sim.shape[0]
    self_ids = np.full(B, -1) if self_ids is None else np.asarray(self_ids)
    own = [np.empty(0, np.int64) if s < 0 else np.array([s], np.int64) for s in self_ids]
    return ref.topn_batch(sim, own, allow, N)


class SimilarNumpyBackend(NumpyBackend):
    """NumpyBackend with `row_inv_norms` / `similar_topk`: adapters from the engine's tensors to the functions above.
    The dots are float64 products rounded to float32 (the CPU stand-in of the matrix-core chain)."""

    def row_inv_norms(self, *, k, ld, T, inv_norm):
        self.calls.append(("row_inv_norms", T.shape[0], T.data_ptr()))
        inv_norm[: T.shape[0]] = torch.from_numpy(inv_norms(T.detach().numpy()).astype(np.float32))

    def similar_topk(self, *, k, ld, q_ids, Q, q_inv, self_ids, n, T, t_inv, allow, topn, top_val, top_idx, top_cnt):
        self.calls.append(("similar_topk", q_ids.numel(), None if allow is None else allow.data_ptr()))
        q = q_ids.long()
        dots = (Q[q].double() @ T[:n].double().T).float().numpy()
        ok = None if allow is None else ref.unpack_bitmap(allow.numpy(), n)
        own = None if self_ids is None else self_ids.numpy()
        out = similar_topn(dots, q_inv[q].numpy(), t_inv[:n].numpy(), own, ok, topn)
        for dst, a in zip((top_val, top_idx, top_cnt), out):
            dst[: a.shape[0]] = torch.from_numpy(a)
