"""The contract of als_row_whitener / als_explore_topk (include/als_hip.h) in float64 numpy, the error bounds the GPU
tests hold the kernels to, and the stand-in backend that serves both calls to the engine on the CPU.

`whitener` is L^-1 for one row, L the lower Cholesky factor of A = Z_S^T Z_S + lam I in the natural column order.
`explore_keys` takes the fp32 base scores as given - on the GPU the row als_predict_dense writes, which the kernel's
base equals bitwise - and returns, per item, the exact leverage |L^-1 z_i|^2, sigma, key and the bounds:

  tau_lev = 2 (k + 4) 2^-24 |y|_2 |a|_2,  y = L^-1 z_i,  a = |W| |z_i|,  W = float32(L^-1):
            every entry of W z_i is off by at most (k + 1) 2^-24 a_r (the rounding of W, a k-term fp32 dot product
            in any order), the squares and their sum add at most three more roundings of that size;
  tau_sig = sqrt(lev + tau_lev) - sqrt(max(lev - tau_lev, 0)): sigma over the interval of the leverage;
  tau_s   = |beta| tau_sig + 4 2^-24 (|base| + |beta| sigma): the three fp32 roundings of the key.

`whitener_residual_bound`: W = L^-1 + E with |E| <= 2^-24 |L^-1|, so W A W^T - I = E L + (E L)^T + E A E^T and
|E L| <= 2^-24 |L^-1| |L| entry by entry; every entry of |L^-1| |L| is at most cond_2(A)^(1/2).  The fp64 errors of
the factorisation (cond_2(A) 2^-53) are added with a factor 64 k.

`ExploreNumpyBackend`: the stand-in forms W in fp64 and rounds it, the leverage as float32 of the fp64 |W z|^2, and
the key with numpy float32 arithmetic, as the header states it; selection is serving_ref.topn_batch's."""
import numpy as np
import torch

from tests import serving_ref as ref
from tests.group_ref import GroupNumpyBackend

EPS = ref.EPS
U24 = 2.0 ** -24


def whitener(Z, S, lam, k):
    """float64 [k, k]: L^-1, L L^T = Z[S, :k]^T Z[S, :k] + lam I (lam includes the 1e-10)."""
    Zs = np.asarray(Z)[np.asarray(S, dtype=np.int64), :k].astype(np.float64)
    A = Zs.T @ Zs + lam * np.eye(k)
    L = np.linalg.cholesky(A)
    return np.tril(np.linalg.solve(L, np.eye(k))), A, L


def key_f32(base, beta, lev):
    """The kernel's key from its own fp32 leverage: sqrt, product, sum, each rounded to float32."""
    base, lev = np.asarray(base, np.float32), np.asarray(lev, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return (base + (np.float32(beta) * np.sqrt(lev)).astype(np.float32)).astype(np.float32)


def explore_keys(base_f32, Z, Winv, beta, k):
    """dict of float64 [n] arrays for one row: lev, sigma, key (exact, from the fp32 base as given) and the bounds
    tau_lev, tau_s of the module docstring."""
    Zk = np.asarray(Z)[:, :k].astype(np.float64)
    Y = Zk @ Winv.T                                                     # [n, k]: y_i = L^-1 z_i
    a = np.abs(Zk) @ np.abs(Winv.astype(np.float32).astype(np.float64)).T
    lev = (Y * Y).sum(axis=1)
    sigma = np.sqrt(lev)
    base = np.asarray(base_f32).astype(np.float64)
    tau_lev = 2.0 * (k + 4) * U24 * np.sqrt(lev) * np.sqrt((a * a).sum(axis=1))
    tau_sig = np.sqrt(lev + tau_lev) - np.sqrt(np.maximum(lev - tau_lev, 0.0))
    tau_s = abs(beta) * tau_sig + 4.0 * U24 * (np.abs(base) + abs(beta) * sigma)
    return dict(lev=lev, sigma=sigma, key=base + beta * sigma, tau_lev=tau_lev, tau_s=tau_s)


def whitener_residual_bound(A, L, Winv):
    """The bound on max |W A W^T - I| for W = float32(L^-1) formed in fp64 (module docstring)."""
    k = A.shape[0]
    M = np.abs(Winv) @ np.abs(L)
    first = U24 * (M + M.T).max()
    second = U24 * U24 * (np.abs(Winv) @ np.abs(A) @ np.abs(Winv).T).max()
    return first + second + 64.0 * k * 2.0 ** -53 * np.linalg.cond(A)


class ExploreNumpyBackend(GroupNumpyBackend):
    """GroupNumpyBackend with `row_whitener` and `explore_topk`."""

    def row_whitener(self, *, k, ld, indptr, indices, rows, n, Z, lam_u, W_out, status):
        ptr, idx = indptr.numpy(), indices.numpy()
        nrows = ptr.size - 1 if rows is None else rows.numel()
        self.calls.append(("row_whitener", nrows, Z.data_ptr()))
        assert W_out.shape[0] >= nrows and tuple(W_out.shape[1:]) == (ld, ld)
        lam = float(np.float32(lam_u)) + EPS
        for w in range(nrows):
            r = w if rows is None else int(rows[w])
            S = idx[ptr[r]: ptr[r + 1]]
            assert (np.diff(S) > 0).all()
            Winv, _, _ = whitener(Z.numpy(), S, lam, k)
            W_out[w].zero_()
            W_out[w, :k, :k] = torch.from_numpy(Winv.astype(np.float32))

    def explore_topk(self, *, k, ld, users, n, U, Z, b_u, b_i, mu, W, beta, seen_ptr, seen_idx, allow, topn, top_val,
                     top_idx, top_cnt, top_lev):
        B = users.numel()
        self.calls.append(("explore_topk", B, Z.data_ptr(), float(beta), None if allow is None else allow.data_ptr()))
        assert np.isfinite(beta) and W.shape[0] >= B
        S, seen = self._serving_rows(users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx)
        Zk = Z[:n].numpy().astype(np.float64)
        keys = np.empty_like(S)
        levs = np.empty_like(S)
        for b in range(B):
            y = Zk @ W[b].numpy().astype(np.float64).T
            levs[b] = (y * y).sum(axis=1).astype(np.float32)
            keys[b] = key_f32(S[b], beta, levs[b])
        ok = None if allow is None else ref.unpack_bitmap(allow.numpy(), n)
        tv, ti, tc = ref.topn_batch(keys, seen, ok, topn)
        tl = np.where(ti >= 0, np.take_along_axis(levs, np.maximum(ti, 0).astype(np.int64), axis=1), np.float32(0))
        for out, a in zip((top_val, top_idx, top_cnt, top_lev), (tv, ti, tc, tl.astype(np.float32))):
            out[: a.shape[0]] = torch.from_numpy(a)
