"""Plumbing shared by the GPU test modules (tests/test_gpu_*.py): the device environment, fixture builders, uploads,
launch wrappers of the serving kernels and small comparison helpers.  No test module imports another test module.

The builders draw from numpy generators seeded by their `seed` argument in a fixed call order; the tests' inputs are
those streams, so the order of the draws is part of each builder's contract."""
import ctypes as C
import os
from typing import Any, NamedTuple

import numpy as np
import pytest


class Env(NamedTuple):
    torch: Any
    layout: Any
    side_dev: Any
    tasks_dev: Any
    be: Any
    dev: Any

    @property
    def short(self):
        """(torch, layout, be, dev): what the tests of the serving kernels use."""
        return self.torch, self.layout, self.be, self.dev


def env(gram="f16x2"):
    """The device environment; fails the test when there is no device.  gram: "f16x2", "f32", or "f64" for
    ALS_GRAM_F64 (row_solve_f64.hip).  The backend's solve_dtype is fixed ("float32" unless gram is "f64"): it only
    steers als_row_solve, so the tests of every other kernel take the default."""
    solve_dtype = "float64" if gram == "f64" else "float32"
    gram = "f16x2" if gram == "f64" else gram
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no ROCm device is visible")
    from collaborative_filtering_amd import layout
    from collaborative_filtering_amd.als import _side_to_dev, _tasks_to_dev
    from collaborative_filtering_amd.backend import HipBackend
    dev = torch.device("cuda", 0)
    return Env(torch, layout, _side_to_dev, _tasks_to_dev, HipBackend(dev, gram=gram, solve_dtype=solve_dtype), dev)


def record_margins(key, worst):
    """ALS_RECORD_MARGINS=<file>: append the observed errors of a kernel test (the tolerances are set from them)."""
    path = os.environ.get("ALS_RECORD_MARGINS")
    if path:
        import json
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[key] = worst
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


# ------------------------------------------------------------------------------------------ comparisons, pointers
def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def same_bits(a, b):
    a, b = (x.numpy() if hasattr(x, "numpy") else x for x in (a, b))
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def ratio(got, exp, bound, what):
    """max |got - exp| / bound where bound > 0 (exactly zero error required elsewhere), in float64, or in long double
    when the reference is."""
    dt = np.result_type(np.asarray(exp).dtype, np.float64)
    err = np.abs(np.asarray(got, dtype=dt) - np.asarray(exp, dtype=dt))
    bound = np.asarray(bound, dtype=dt)
    assert np.isfinite(err).all(), what
    pos = bound > 0
    assert not err[~pos].any(), f"{what}: non-zero where every term is zero"
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


def assert_same(got, exp, nan_equal=False):
    """Tuples of arrays, element by element with ==; nan_equal: a NaN on both sides is equal too."""
    for g, e in zip(got, exp):
        assert g.shape == e.shape
        same = (g == e) | ((g != g) & (e != e)) if nan_equal else g == e
        assert same.all(), (np.argwhere(~same)[:5], g[~same][:5], e[~same][:5])


# ------------------------------------------------------------------------------------------ host fixtures, uploads
def upload(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def random_side(layout, nrows, ncols, lens, seed):
    rng = np.random.default_rng(seed)
    indptr = np.zeros(nrows + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    idx = np.concatenate([np.sort(rng.choice(ncols, size=l, replace=False)) for l in lens]).astype(np.int32) \
        if sum(lens) else np.zeros(0, np.int32)
    vals = (np.round(rng.uniform(0.5, 5.0, size=idx.size) * 2) / 2).astype(np.float32)
    return layout.SparseSide(nrows, ncols, indptr, idx, vals)


def pad(A, ld, extra_rows=0):
    out = np.zeros((A.shape[0] + extra_rows, ld), dtype=np.float32)
    out[: A.shape[0], : A.shape[1]] = A
    return out


def factors(torch, layout, dev, m, n, k, seed, integer=False):
    """U [m, ld], Z [n, ld] (padding columns zero), biases, mu - fp32 / fp64 device tensors."""
    ld = layout.padded_k(k)
    rng = np.random.default_rng(seed)
    if integer:                                  # small integers: many exactly equal scores
        U = np.zeros((m, ld), np.float32)
        Z = np.zeros((n, ld), np.float32)
        U[:, :k] = rng.integers(-2, 3, size=(m, k))
        Z[:, :k] = rng.integers(-2, 3, size=(n, k))
        Z[1::3] = Z[0::3][: Z[1::3].shape[0]]    # duplicated item rows
        bu = rng.integers(-1, 2, size=m).astype(np.float32)
        bi = np.zeros(n, np.float32)
        mu = 0.0
    else:
        U = np.zeros((m, ld), np.float32)
        Z = np.zeros((n, ld), np.float32)
        U[:, :k] = rng.normal(size=(m, k))
        Z[:, :k] = rng.normal(size=(n, k))
        bu = rng.normal(scale=0.3, size=m).astype(np.float32)
        bi = rng.normal(scale=0.3, size=n).astype(np.float32)
        mu = 3.5
    return dict(k=k, ld=ld, U=upload(U, dev), Z=upload(Z, dev), b_u=upload(bu, dev), b_i=upload(bi, dev),
                mu=torch.tensor([mu], dtype=torch.float64, device=dev))


def seen_csr(m, n, seed, density=0.05):
    """Seen rows by user id: user 0 sees nothing, user 1 all but 3 items, user 2 more than 3000 (when n allows),
    the others a random subset."""
    rng = np.random.default_rng(seed)
    rows = []
    for u in range(m):
        if u == 0:
            s = np.empty(0, np.int64)
        elif u == 1:
            s = np.sort(rng.permutation(n)[: max(n - 3, 0)])
        elif u == 2 and n > 3500:
            s = np.sort(rng.permutation(n)[: 3200])
        else:
            s = np.nonzero(rng.random(n) < density)[0]
        rows.append(s)
    ptr_ = np.zeros(m + 1, np.int64)
    ptr_[1:] = np.cumsum([len(s) for s in rows])
    idx = np.concatenate(rows).astype(np.int32) if ptr_[-1] else np.zeros(0, np.int32)
    return ptr_, idx, rows


def item_table(torch, layout, dev, n, k, seed, scale=0.5, mu=3.5):
    """Z [n, ld] (padding columns zero) and b_i, on the host (Z, b_i) and on the device (Zd, bid), and mud = [mu]."""
    ld = layout.padded_k(k)
    rng = np.random.default_rng(seed)
    Z = np.zeros((n, ld), np.float32)
    Z[:, :k] = rng.normal(scale=scale, size=(n, k))
    bi = rng.normal(scale=0.3, size=n).astype(np.float32)
    return dict(ld=ld, Z=Z, b_i=bi, Zd=upload(Z, dev), bid=upload(bi, dev),
                mud=torch.tensor([mu], dtype=torch.float64, device=dev))


def csr_rows(lengths, ncols, seed, weights=False):
    """CSR rows of the given lengths with sorted distinct columns; values are ratings on the half-star grid, or
    (weights=True) uniform graph weights in [0.05, 1)."""
    rng = np.random.default_rng(seed)
    cols = [np.sort(rng.permutation(ncols)[:L]) for L in lengths]
    indptr = np.zeros(len(lengths) + 1, np.int64)
    indptr[1:] = np.cumsum(lengths)
    indices = np.concatenate(cols).astype(np.int32) if indptr[-1] else np.zeros(0, np.int32)
    if weights:
        vals = rng.uniform(0.05, 1.0, size=indices.size).astype(np.float32)
    else:
        vals = (rng.integers(1, 11, size=indices.size) * 0.5).astype(np.float32)
    return indptr, indices, vals


# ------------------------------------------------------------------------------------------ launches
class GsSweep:
    """One case of tests/gs_sweep_ref.py on the device, ready to be swept: the by-products come from als_row_solve in
    factor mode (f64: as doubles, from the fp64 kernel), V and the biases hold the case's values on entry, `kw` is what
    be.gs_level / gs_levels / gs_dataflow take (`stat`: with the fused residual statistics)."""

    def __init__(self, E, case, f64=False, stat=True):
        torch, dev, be = E.torch, E.dev, E.be
        k, ld, n = case.k, case.ld, case.n
        ft = torch.float64 if f64 else torch.float32
        side = E.layout.SparseSide(n, case.m, case.indptr, case.indices, case.vals)
        t = E.layout.build_row_tasks(side.indptr)
        sd = E.side_dev(side, dev)
        self.factor = torch.zeros(n * ld * ld, dtype=ft, device=dev)
        rhs, cs = torch.zeros(n, ld, dtype=ft, device=dev), torch.zeros(n, ld, dtype=ft, device=dev)
        sumr, sumr2 = torch.zeros(n, dtype=ft, device=dev), torch.zeros(n, dtype=ft, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(max(t.nslots, 1) * be.slot_bytes(k, f64) // 4, dtype=torch.float32, device=dev)
        be.row_solve(k=k, ld=ld, side=sd, F=upload(pad(case.U, ld, 1), dev), zero_row=case.m,
                     bias_self=upload(case.b_i, dev), bias_other=upload(case.b_u, dev),
                     mu=torch.tensor([case.mu], dtype=torch.float64, device=dev), lam=0.0,
                     lam_row=upload(case.lam_row, dev), lam_b=case.lam_b, lam_b_row=None, rhs_extra=None,
                     diag_extra=upload(case.diag_extra, dev), X_out=None, bias_out=None, gram_out=None,
                     factor_out=self.factor, rhs_out=rhs, colsum_out=cs, sumr_out=sumr, sumr2_out=sumr2,
                     status=status, tasks=E.tasks_dev(t, dev), workspace=ws, f64=f64)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        self.torch, self.be, self.case = torch, be, case
        self.V, self.bias = upload(case.V_pad(), dev), upload(case.b_i.copy(), dev)
        self.stat = torch.full((n, 2), 7.0, dtype=torch.float32, device=dev) if stat else None
        self.items = upload(case.sched.items, dev)
        self.offsets = np.ascontiguousarray(case.sched.offsets, dtype=np.int64)
        self.wait = upload(case.wait, dev)
        self.kw = dict(k=k, ld=ld, S_ptr=upload(case.S_ptr, dev), S_idx=upload(case.S_idx, dev),
                       S_val=upload(case.S_val, dev), alpha=case.alpha, factor=self.factor, rhs=rhs, colsum=cs,
                       sumr=sumr, indptr=sd.indptr, lam_b=case.lam_b, lam_b_row=None, V=self.V, bias=self.bias)
        if stat:
            self.kw.update(sumr2=sumr2, lambda_eff=upload(case.lambda_eff, dev), stat_out=self.stat)
        if f64:
            self.kw["f64"] = True

    def levels(self):
        self.be.gs_levels(offsets=self.offsets, items=self.items, **self.kw)
        return self.fetch()

    def level_by_level(self):
        for lo, hi in zip(self.offsets[:-1], self.offsets[1:]):
            self.be.gs_level(items=self.items[int(lo): int(hi)], **self.kw)
        return self.fetch()

    def dataflow(self, publish, nondep=None):
        """The whole schedule in its own order; -> (V, bias, stat) after asserting that no wait timed out."""
        err = self.torch.zeros(1, dtype=self.torch.int32, device=self.V.device)
        self.be.gs_dataflow(items=self.items, S_idx_wait=self.wait, publish=publish, err=err, nondep=nondep, **self.kw)
        out = self.fetch()
        assert int(err.item()) == 0, "a dependency wait of the dataflow sweep timed out"
        return out

    def fetch(self):
        self.torch.cuda.synchronize()
        return (self.V.cpu().numpy(), self.bias.cpu().numpy(), None if self.stat is None else self.stat.cpu().numpy())


def predict_dense(torch, be, f, m, n, dev):
    """als_predict_dense on the first m users and n items of `factors`."""
    out = torch.empty(m, n, dtype=torch.float32, device=dev)
    be.predict_dense(k=f["k"], ld=f["ld"], m=m, n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"], mu=f["mu"],
                     out=out)
    return out.cpu().numpy()


def _opt(a, dev):
    return None if a is None else upload(a, dev)


def run_topk(torch, be, f, users, n, seen_ptr, seen_idx, N, dev, allow=None):
    """als_recommend_topk, or (allow: the device bitmap) als_recommend_topk_masked -> numpy (values, items, counts)."""
    us = upload(np.asarray(users, np.int32), dev)
    B = us.numel()
    tv = torch.empty(B, N, dtype=torch.float32, device=dev)
    ti = torch.empty(B, N, dtype=torch.int32, device=dev)
    tc = torch.empty(B, dtype=torch.int32, device=dev)
    kw = dict(k=f["k"], ld=f["ld"], users=us, n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"], mu=f["mu"],
              seen_ptr=_opt(seen_ptr, dev), seen_idx=_opt(seen_idx, dev), topn=N, top_val=tv, top_idx=ti, top_cnt=tc)
    if allow is None:
        be.recommend_topk(**kw)
    else:
        be.recommend_topk_masked(allow=allow, **kw)
    return tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()


def run_rank(torch, be, f, users, n, seen_ptr, seen_idx, q_ptr, q_items, dev, allow=None):
    """als_rank_count, or (allow: the device bitmap) als_rank_count_masked, into buffers that start from 7 ->
    numpy (t_score, above, n_cand)."""
    t = lambda a, dt: upload(np.asarray(a, dt), dev)        # noqa: E731
    nq, nt = len(users), len(q_items)
    sc = torch.full((max(nt, 1),), 7.0, dtype=torch.float32, device=dev)
    ab = torch.full((max(nt, 1),), 7, dtype=torch.int32, device=dev)
    nc = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    kw = dict(k=f["k"], ld=f["ld"], n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"], mu=f["mu"],
              seen_ptr=None if seen_ptr is None else t(seen_ptr, np.int64),
              seen_idx=None if seen_idx is None else t(seen_idx, np.int32), q_users=t(users, np.int32),
              q_ptr=t(q_ptr, np.int64), q_items=t(q_items, np.int32)[:nt], t_score=sc[:nt], above=ab[:nt], n_cand=nc)
    if allow is None:
        be.rank_count(**kw)
    else:
        be.rank_count_masked(allow=allow, **kw)
    return sc[:nt].cpu().numpy(), ab[:nt].cpu().numpy(), nc.cpu().numpy()
