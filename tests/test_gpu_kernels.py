"""T3 (GPU): each C-ABI entry point against numpy on random CSR, incl. degenerate
rows (nnz = 1, < k, >> k, > ALS_SPLIT_CHUNK so the split/finish path runs) and
k in {1, 16, 32, 50, 64, 128}.  Calls go through ctypes -> libals_hip.so.  The W-step entry points
(als_w_normal_equations, als_item_stats, als_item_stats_f64) have their own file, tests/test_gpu_w_step.py, with
its reference in tests/w_step_ref.py (validated without a device by tests/test_w_step_ref_cpu.py)."""
import numpy as np
import pytest

from tests.gpu_common import env, pad, random_side, record_margins

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("gram", ["f16x2", "f32", "f64"])
@pytest.mark.parametrize("k", [1, 16, 32, 50, 64, 80, 96, 112, 128, 160])
def test_row_solve_against_numpy(k, gram):
    torch, layout, side_dev, tasks_dev, be, dev = env(gram)
    # Tolerances at about 10x the error observed on the MI355X over all k and row lengths of this test
    # (profiles/r03_kernel_test_margins.json, written by this test under ALS_RECORD_MARGINS=<file>), relative to
    # max|x| of the row / max|G|: fp32 solve x observed 6.8e-6 (f16x2) / 2.8e-6 (f32), bias 1.5e-7, Gram 7.3e-7
    # (f16x2) / 3.0e-6 (f32: the f32-MFMA chain is the less accurate one on the 8200-rating row); fp64 mode: the
    # fp32 rounding of the stored x and Gram, 5.7e-8.  (Round 2 had rtol 2e-3 / atol 2e-4 here: a two-digit
    # regression would have passed.)
    xr, xa, ba, gr, ga = (0.0, 6e-7, 6e-7, 0.0, 6e-7) if gram == "f64" else (0.0, 6e-5, 2e-6, 0.0, 2.5e-5)
    gram_name = gram
    worst = {"x": 0.0, "bias": 0.0, "gram": 0.0}
    ncols = 9000
    lens = [1, 2, 0, k // 2 + 1, k, 3 * k + 5, 700, 0, 4096, 4097, 8200 + k, 33, 64, 65, 5]
    nrows = len(lens)
    side = random_side(layout, nrows, ncols, lens, seed=k)
    rng = np.random.default_rng(100 + k)
    ld = layout.padded_k(k)
    F = rng.normal(scale=0.3, size=(ncols, k))
    b_self = rng.normal(scale=0.2, size=nrows)
    b_other = rng.normal(scale=0.2, size=ncols)
    lam_row = rng.uniform(0.5, 4.0, size=nrows)
    rhs_extra = rng.normal(scale=0.5, size=(nrows, k))
    diag_extra = rng.uniform(0.0, 2.0, size=nrows)
    mu, lam_b = 3.3, 1.7
    t = layout.build_row_tasks(side.indptr)
    assert t.nslots > 0 and t.long_rows.shape[0] == 2        # split path is exercised
    sd, td = side_dev(side, dev), tasks_dev(t, dev)
    f32 = torch.float32
    X_out = torch.full((nrows, ld), 7.0, dtype=f32, device=dev)
    bias_out = torch.full((nrows,), 7.0, dtype=f32, device=dev)
    gram = torch.zeros(nrows, ld, ld, dtype=f32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(t.nslots * be.slot_bytes(k) // 4, dtype=f32, device=dev)
    be.row_solve(k=k, ld=ld, side=sd, F=torch.from_numpy(pad(F, ld, 1)).to(dev), zero_row=ncols,
                 bias_self=torch.from_numpy(b_self.astype(np.float32)).to(dev),
                 bias_other=torch.from_numpy(b_other.astype(np.float32)).to(dev),
                 mu=torch.tensor([mu], dtype=torch.float64, device=dev), lam=0.0,
                 lam_row=torch.from_numpy(lam_row.astype(np.float32)).to(dev), lam_b=lam_b, lam_b_row=None,
                 rhs_extra=torch.from_numpy(pad(rhs_extra, ld)).to(dev),
                 diag_extra=torch.from_numpy(diag_extra.astype(np.float32)).to(dev),
                 X_out=X_out, bias_out=bias_out, gram_out=gram, factor_out=None, rhs_out=None,
                 colsum_out=None, sumr_out=None, status=status, tasks=td, workspace=ws)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    X = X_out.cpu().numpy().astype(np.float64)
    bias = bias_out.cpu().numpy().astype(np.float64)
    G = gram.cpu().numpy().astype(np.float64)
    pos = layout.perm_of_col(k)[:k]
    F32 = F.astype(np.float32).astype(np.float64)
    for r in range(nrows):
        lo, hi = side.indptr[r], side.indptr[r + 1]
        if hi == lo:                                          # untouched, as in the reference
            assert np.all(X[r] == 7.0) and bias[r] == 7.0
            continue
        idx = side.indices[lo:hi]
        Fr = F32[idx]
        vals = side.vals[lo:hi].astype(np.float64)
        rr = vals - (mu + float(np.float32(b_self[r])) + b_other.astype(np.float32)[idx].astype(np.float64))
        A = Fr.T @ Fr + (float(np.float32(lam_row[r])) + 1e-10 + float(np.float32(diag_extra[r]))) * np.eye(k)
        b = Fr.T @ rr + rhs_extra.astype(np.float32)[r].astype(np.float64)
        x = np.linalg.solve(A, b)
        scale = max(np.max(np.abs(x)), 1e-6)
        worst["x"] = max(worst["x"], float(np.max(np.abs(X[r, :k] - x)) / scale))
        np.testing.assert_allclose(X[r, :k], x, rtol=xr, atol=xa * scale, err_msg=f"row {r} nnz {hi - lo}")
        assert np.all(X[r, k:] == 0.0)
        bref = np.sum(vals - Fr @ x - mu - b_other.astype(np.float32)[idx]) / ((hi - lo) + lam_b + 1e-10)
        worst["bias"] = max(worst["bias"], abs(bias[r] - bref) / max(1.0, abs(bref)))
        assert abs(bias[r] - bref) <= ba * max(1.0, abs(bref)), (r, bias[r], bref)
        Gr = G[r][np.ix_(pos, pos)]
        blk = pos // 16
        lower_block = blk[:, None] >= blk[None, :]            # documented valid region
        ref = Fr.T @ Fr
        worst["gram"] = max(worst["gram"], float(np.max(np.abs(Gr - ref)[lower_block]) / max(np.max(np.abs(ref)), 1e-6)))
        np.testing.assert_allclose(Gr[lower_block], ref[lower_block], rtol=gr,
                                   atol=ga * max(np.max(np.abs(ref)), 1e-6))
    record_margins(f"row_solve k={k} {gram_name}", worst)


@pytest.mark.parametrize("k", [50, 64, 120, 128])
def test_row_solve_presplit_operands_equal_the_in_kernel_split(k):
    """als_row_solve_params::F_planes (k = 49 ... 64 and 113 ... 128): the Gram from pre-split fp16 operands is the in-kernel split's
    Gram BIT FOR BIT (same terms, same products, same order); the right-hand side and the column sums come from the
    matrix cores instead of the vector unit, so x and the bias agree to rounding (every row class: 1 rating, < k, k,
    long, split rows with partial slots, empty rows untouched)."""
    torch, layout, side_dev, tasks_dev, _, dev = env()
    from collaborative_filtering_amd.backend import HipBackend
    ncols = 9000
    lens = [1, 2, 0, k // 2 + 1, k, 3 * k + 5, 700, 0, 4096, 4097, 8200 + k, 33, 64, 65, 5, 511, 513]
    nrows = len(lens)
    side = random_side(layout, nrows, ncols, lens, seed=7 * k)
    rng = np.random.default_rng(9 + k)
    ld = layout.padded_k(k)
    F = rng.normal(scale=0.3, size=(ncols, k)) * 10.0 ** rng.uniform(-2, 0, size=(ncols, 1))      # two decades of row norms
    b_self, b_other = rng.normal(scale=0.2, size=nrows), rng.normal(scale=0.2, size=ncols)
    t = layout.build_row_tasks(side.indptr)
    sd, td = side_dev(side, dev), tasks_dev(t, dev)
    f32 = torch.float32
    out = {}
    for label, planes in (("split", 0), ("planes", HipBackend.PLANES_MAX_FLOATS)):
        be = HipBackend(dev, solve_dtype="float32")
        be.planes_max_floats = be.planes_max_floats_k128 = planes          # (k = 128: off by default, exercised here)
        X_out = torch.full((nrows, ld), 7.0, dtype=f32, device=dev)
        bias_out = torch.full((nrows,), 7.0, dtype=f32, device=dev)
        gram = torch.zeros(nrows, ld, ld, dtype=f32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        ws = torch.empty(t.nslots * be.slot_bytes(k) // 4, dtype=f32, device=dev)
        tt = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)       # noqa: E731
        be.row_solve(k=k, ld=ld, side=sd, F=tt(pad(F, ld, 1)), zero_row=ncols, bias_self=tt(b_self), bias_other=tt(b_other),
                     mu=torch.tensor([3.3], dtype=torch.float64, device=dev), lam=2.5, lam_row=None, lam_b=1.7,
                     lam_b_row=None, rhs_extra=None, diag_extra=None, X_out=X_out, bias_out=bias_out, gram_out=gram,
                     factor_out=None, rhs_out=None, colsum_out=None, sumr_out=None, status=status, tasks=td, workspace=ws)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        assert (len(be._planes) > 0) == (planes > 0)
        out[label] = (X_out.cpu().numpy(), bias_out.cpu().numpy(), gram.cpu().numpy())
    np.testing.assert_array_equal(out["split"][2], out["planes"][2])                     # the Gram: bit for bit
    xs, xp = out["split"][0].astype(np.float64), out["planes"][0].astype(np.float64)
    scale = np.maximum(np.max(np.abs(xs), axis=1, keepdims=True), 1e-6)
    assert np.max(np.abs(xs - xp) / scale) <= 2e-5
    np.testing.assert_allclose(out["split"][1], out["planes"][1], rtol=0, atol=2e-6)
    empty = np.diff(side.indptr) == 0
    assert np.all(out["planes"][0][empty] == 7.0) and np.all(out["planes"][1][empty] == 7.0)


@pytest.mark.parametrize("k", [16, 50, 64, 128])
def test_row_solve_f64_small_lambda(k):
    """ALS_GRAM_F64 at lambda = 1e-4 with rows shorter than k (cond ~ 1/lambda, where the fp32 kernels lose the
    null-space components): the fp64 kernel returns numpy's float64 solution up to the fp32 rounding of the
    stored x, and the closed-form residual statistics equal the directly evaluated sums."""
    torch, layout, side_dev, tasks_dev, be, dev = env("f64")
    ncols = 5000
    lens = [1, 3, k // 2 + 1, max(k - 1, 1), k, k + 7, 300, 4100, 17, 2]
    nrows = len(lens)
    side = random_side(layout, nrows, ncols, lens, seed=900 + k)
    rng = np.random.default_rng(950 + k)
    ld = layout.padded_k(k)
    F = rng.normal(scale=0.3, size=(ncols, k)).astype(np.float32)
    b_self = rng.normal(scale=0.2, size=nrows).astype(np.float32)
    b_other = rng.normal(scale=0.2, size=ncols).astype(np.float32)
    mu, lam, lam_b = 3.3, 1e-4, 1.7
    t = layout.build_row_tasks(side.indptr)
    sd, td = side_dev(side, dev), tasks_dev(t, dev)
    f32 = torch.float32
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    X_out = torch.zeros(nrows, ld, dtype=f32, device=dev)
    bias_out = torch.zeros(nrows, dtype=f32, device=dev)
    stat = torch.zeros(nrows, 2, dtype=f32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(t.nslots, 1) * be.slot_bytes(k) // 4, dtype=f32, device=dev)
    be.row_solve(k=k, ld=ld, side=sd, F=tt(pad(F, ld, 1)), zero_row=ncols, bias_self=tt(b_self), bias_other=tt(b_other),
                 mu=torch.tensor([mu], dtype=torch.float64, device=dev), lam=lam, lam_row=None, lam_b=lam_b,
                 lam_b_row=None, rhs_extra=None, diag_extra=None, X_out=X_out, bias_out=bias_out, gram_out=None,
                 factor_out=None, rhs_out=None, colsum_out=None, sumr_out=None, status=status, tasks=td, workspace=ws,
                 stat_out=stat)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    X = X_out.cpu().numpy().astype(np.float64)
    bias = bias_out.cpu().numpy().astype(np.float64)
    st = stat.cpu().numpy().astype(np.float64)
    F64 = F.astype(np.float64)
    for r in range(nrows):
        lo, hi = side.indptr[r], side.indptr[r + 1]
        idx = side.indices[lo:hi]
        Fr = F64[idx]
        vals = side.vals[lo:hi].astype(np.float64)
        rho = vals - mu - b_other[idx].astype(np.float64)
        A = Fr.T @ Fr + (np.float32(lam).astype(np.float64) + 1e-10) * np.eye(k)
        x = np.linalg.solve(A, Fr.T @ (rho - np.float64(b_self[r])))
        scale = max(np.max(np.abs(x)), 1e-6)
        np.testing.assert_allclose(X[r, :k], x, rtol=5e-6, atol=5e-6 * scale, err_msg=f"row {r} nnz {hi - lo}")
        bref = np.sum(rho - Fr @ x) / ((hi - lo) + lam_b + 1e-10)
        assert abs(bias[r] - bref) <= 2e-6 * max(1.0, abs(bref)), (r, bias[r], bref)
        d = rho - Fr @ x - bref
        assert abs(st[r, 0] - d.sum()) <= 1e-5 * max(1.0, np.abs(rho).sum())
        assert abs(st[r, 1] - (d * d).sum()) <= 1e-5 * max(1e-3, (d * d).sum()) + 1e-9 * (rho * rho).sum()


@pytest.mark.parametrize("gram", ["f16x2", "f64"])
@pytest.mark.parametrize("k", [16, 64, 80, 96, 128, 160])
def test_factor_mode_and_gs_level(k, gram):
    """factor-only als_row_solve + als_gs_sweep on one level == direct solve with the graph term."""
    torch, layout, side_dev, tasks_dev, be, dev = env(gram)
    ncols, nrows = 6000, 40
    rng = np.random.default_rng(7 + k)
    lens = list(rng.integers(1, 300, size=nrows))
    lens[3] = 5000
    side = random_side(layout, nrows, ncols, lens, seed=3 * k)
    ld = layout.padded_k(k)
    F = rng.normal(scale=0.3, size=(ncols, k)).astype(np.float32)
    Vold = rng.normal(scale=0.3, size=(nrows, k)).astype(np.float32)
    b_self = rng.normal(scale=0.2, size=nrows).astype(np.float32)
    b_other = rng.normal(scale=0.2, size=ncols).astype(np.float32)
    lam_row = rng.uniform(0.5, 4.0, size=nrows).astype(np.float32)
    mu, lam_b, alpha = 3.1, 2.2, 0.7
    # a graph whose rows only reference items that are NOT swept in this level (items 20..39)
    sweep = np.arange(0, 20, dtype=np.int32)
    S_ptr = np.zeros(nrows + 1, dtype=np.int64)
    S_idx, S_val = [], []
    for i in range(nrows):
        nb = rng.choice(np.arange(20, 40), size=rng.integers(0, 9), replace=False)
        S_idx.append(np.sort(nb))
        S_val.append(rng.uniform(0.1, 1.0, size=nb.size))
        S_ptr[i + 1] = S_ptr[i] + nb.size
    S_idx = np.concatenate(S_idx).astype(np.int32)
    S_val = np.concatenate(S_val).astype(np.float32)
    D = np.array([S_val[S_ptr[i]:S_ptr[i + 1]].sum() for i in range(nrows)], dtype=np.float32)
    t = layout.build_row_tasks(side.indptr)
    sd, td = side_dev(side, dev), tasks_dev(t, dev)
    f32 = torch.float32
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    factor = torch.zeros(nrows * ld * ld, dtype=f32, device=dev)
    rhs = torch.zeros(nrows, ld, dtype=f32, device=dev)
    cs = torch.zeros(nrows, ld, dtype=f32, device=dev)
    sumr = torch.zeros(nrows, dtype=f32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(t.nslots, 1) * be.slot_bytes(k) // 4, dtype=f32, device=dev)
    mu_t = torch.tensor([mu], dtype=torch.float64, device=dev)
    be.row_solve(k=k, ld=ld, side=sd, F=tt(pad(F, ld, 1)), zero_row=ncols, bias_self=tt(b_self), bias_other=tt(b_other),
                 mu=mu_t, lam=0.0, lam_row=tt(lam_row), lam_b=lam_b, lam_b_row=None, rhs_extra=None,
                 diag_extra=tt(alpha * D), X_out=None, bias_out=None, gram_out=None, factor_out=factor,
                 rhs_out=rhs, colsum_out=cs, sumr_out=sumr, status=status, tasks=td, workspace=ws)
    V = tt(pad(Vold, ld))
    bias = tt(b_self.copy())
    be.gs_level(k=k, ld=ld, items=tt(sweep), S_ptr=tt(S_ptr), S_idx=tt(S_idx), S_val=tt(S_val),
                alpha=alpha, factor=factor, rhs=rhs, colsum=cs, sumr=sumr, indptr=sd.indptr,
                lam_b=lam_b, lam_b_row=None, V=V, bias=bias)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    Vn = V.cpu().numpy().astype(np.float64)
    bn = bias.cpu().numpy().astype(np.float64)
    F64 = F.astype(np.float64)
    for i in range(nrows):
        if i >= 20:
            np.testing.assert_array_equal(Vn[i, :k], Vold[i])        # not swept
            continue
        lo, hi = side.indptr[i], side.indptr[i + 1]
        idx = side.indices[lo:hi]
        Fr = F64[idx]
        vals = side.vals[lo:hi].astype(np.float64)
        rr = vals - (mu + b_self[i] + b_other[idx])
        A = Fr.T @ Fr + (lam_row[i] + 1e-10 + alpha * D[i]) * np.eye(k)
        sl = slice(S_ptr[i], S_ptr[i + 1])
        b = Fr.T @ rr + alpha * (S_val[sl].astype(np.float64) @ Vold[S_idx[sl]].astype(np.float64))
        x = np.linalg.solve(A, b)
        np.testing.assert_allclose(Vn[i, :k], x, rtol=0, atol=1e-4 * max(np.max(np.abs(x)), 1e-6))      # ~10x observed
        bref = np.sum(vals - Fr @ x - mu - b_other[idx]) / ((hi - lo) + lam_b + 1e-10)
        assert abs(bn[i] - bref) <= 2e-5 * max(1.0, abs(bref))


@pytest.mark.parametrize("k", [1, 16, 50, 64, 96, 128, 160])
def test_stats_predict_compose(k):
    torch, layout, side_dev, tasks_dev, be, dev = env()
    m, n = 300, 500
    rng = np.random.default_rng(5 + k)
    lens = list(rng.integers(0, 120, size=m))
    lens[7] = 0
    lens[11] = 450
    side = random_side(layout, m, n, lens, seed=k + 1)
    ld = layout.padded_k(k)
    U = rng.normal(scale=0.3, size=(m, k)).astype(np.float32)
    V = rng.normal(scale=0.3, size=(n, k)).astype(np.float32)
    X = rng.normal(size=(n, 7)).astype(np.float32)
    W = rng.normal(scale=0.2, size=(7, k)).astype(np.float32)
    b_u = rng.normal(scale=0.2, size=m).astype(np.float32)
    b_i = rng.normal(scale=0.2, size=n).astype(np.float32)
    mu = 3.4
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    Ud, Vd = tt(pad(U, ld)), tt(pad(V, ld))
    Zd = torch.empty_like(Vd)
    be.compose_z(Vd, tt(X), tt(pad(W, ld)), Zd)
    Zref = V.astype(np.float64) + X.astype(np.float64) @ W.astype(np.float64)
    Z = Zd.cpu().numpy()
    np.testing.assert_allclose(Z[:, :k], Zref, rtol=1e-5, atol=1e-6)
    assert np.all(Z[:, k:] == 0)
    t = layout.build_row_tasks(side.indptr)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    mu_t = torch.tensor([mu], dtype=torch.float64, device=dev)
    be.residual_stats(k=k, ld=ld, side=side_dev(side, dev), U=Ud, Z=Zd, b_u=tt(b_u), b_i=tt(b_i),
                      mu=mu_t, tasks=tasks_dev(t, dev), out=out)
    ru = np.repeat(np.arange(m), np.diff(side.indptr))
    ri = side.indices
    Z64 = Z[:, :k].astype(np.float64)
    d = side.vals - (np.sum(U[ru].astype(np.float64) * Z64[ri], axis=1) + b_u[ru] + b_i[ri] + mu)
    got = out.cpu().numpy()
    assert abs(got[0] - d.sum()) <= 1e-4 * max(1.0, abs(d.sum())) + 1e-3
    assert abs(got[1] - (d ** 2).sum()) <= 1e-5 * (d ** 2).sum()
    ss = torch.zeros(1, dtype=torch.float64, device=dev)
    be.sumsq(Ud, ss)
    assert abs(ss.item() - (U.astype(np.float64) ** 2).sum()) <= 1e-9 * (U.astype(np.float64) ** 2).sum() + 1e-12
    # predictions
    flat = rng.choice(m * n, size=1001, replace=False)
    uu, ii = np.divmod(flat, n)
    outp = torch.empty(flat.size, dtype=torch.float32, device=dev)
    be.predict_at(k=k, ld=ld, us=tt(uu.astype(np.int32)), is_=tt(ii.astype(np.int32)), U=Ud, Z=Zd,
                  b_u=tt(b_u), b_i=tt(b_i), mu=mu_t, out=outp)
    pref = np.sum(U[uu].astype(np.float64) * Z64[ii], axis=1) + mu + b_u[uu] + b_i[ii]
    np.testing.assert_allclose(outp.cpu().numpy(), pref, atol=2e-5, rtol=1e-5)
    dense = torch.empty(m, n, dtype=torch.float32, device=dev)
    be.predict_dense(k=k, ld=ld, m=m, n=n, U=Ud, Z=Zd, b_u=tt(b_u), b_i=tt(b_i), mu=mu_t, out=dense)
    dref = U.astype(np.float64) @ Z64.T + mu + b_u[:, None] + b_i[None, :]
    np.testing.assert_allclose(dense.cpu().numpy(), dref, atol=2e-5, rtol=1e-5)


def test_bad_arguments_are_rejected():
    torch, layout, side_dev, tasks_dev, be, dev = env()
    import ctypes as C
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    assert lib.als_padded_k(0) == -2 and lib.als_padded_k(161) == -2 and lib.als_padded_k(50) == 64
    p = _hip.RowSolveParams()
    p.k, p.ld = 64, 48                       # ld does not match k
    assert lib.als_row_solve(C.byref(p), None) == -1
    assert lib.als_row_solve(None, None) == -1
    assert lib.als_spd_solve_workspace_bytes(0) == 0 and lib.als_spd_solve_workspace_bytes(8129) == 0
    assert lib.als_spd_solve_f64(0, None, 0, None, 0.0, None, None, None, None) == -1


def _spd_system(N, seed, cond=1e4):
    rng = np.random.default_rng(seed)
    B = rng.normal(size=(N, max(N // 2, 1)))
    A = B @ B.T + np.diag(rng.uniform(1.0 / cond, 1.0, size=N)) * N       # SPD, moderately conditioned
    A = 0.5 * (A + A.T)
    return A, rng.normal(size=N)


@pytest.mark.parametrize("N", [1, 7, 50, 64, 65, 128, 200, 950, 1216, 2432])
def test_spd_solve_against_numpy(N):
    """als_spd_solve_f64 (the W-step's cholesky_solve, scripts/als.py:497-500) against numpy fp64:
    relative error of x at fp64 level scaled by the condition number, residual at rounding level,
    bitwise reproducible, inputs untouched."""
    torch, layout, side_dev, tasks_dev, be, dev = env()
    A, b = _spd_system(N, seed=N)
    lam = 0.75
    ref = np.linalg.solve(A + lam * np.eye(N), b)
    At, bt = torch.from_numpy(A).to(dev), torch.from_numpy(b).to(dev)
    status = torch.full((1,), 7, dtype=torch.int32, device=dev)
    x1 = be.spd_solve(At, bt, lam, status)
    assert int(status.item()) == 0
    x2 = be.spd_solve(At, bt, lam, status)
    assert torch.equal(x1, x2)
    assert np.array_equal(At.cpu().numpy(), A) and np.array_equal(bt.cpu().numpy(), b)
    x = x1.cpu().numpy()
    cond = np.linalg.cond(A + lam * np.eye(N))
    assert np.linalg.norm(x - ref) <= 50 * cond * np.finfo(np.float64).eps * np.linalg.norm(ref)
    res = (A + lam * np.eye(N)) @ x - b
    assert np.linalg.norm(res) <= 1e-12 * (np.linalg.norm(A) * np.linalg.norm(x) + np.linalg.norm(b))


def test_spd_solve_reports_indefinite_matrices():
    torch, layout, side_dev, tasks_dev, be, dev = env()
    N = 130
    A, b = _spd_system(N, seed=3)
    A[100, 100] = -5.0                                   # pivot 100 (or an earlier one) turns non-positive
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    be.spd_solve(torch.from_numpy(A).to(dev), torch.from_numpy(b).to(dev), 0.0, status)
    assert 1 <= int(status.item()) <= 101
    A2 = np.zeros((3, 3))
    be.spd_solve(torch.from_numpy(A2).to(dev), torch.zeros(3, dtype=torch.float64, device=dev), 0.0, status)
    assert int(status.item()) == 1


@pytest.mark.parametrize("k", [20, 32, 48, 50, 64, 65, 80, 96, 112, 128, 150, 160])
def test_dual_form_short_rows_against_numpy_and_the_primal_kernel(k):
    """Plain solve at k > 64: whole rows of at most 64 ratings (the tail of the task list) are solved in the
    dual form (n x n system); longer rows and split rows stay primal.  Every row against numpy fp64, the
    closed-form bias and residual sums against their definitions, and the dual rows against the primal kernel
    (ndual_tail = 0) on the same input."""
    torch, layout, side_dev, tasks_dev, be, dev = env("f16x2")
    ncols = 5000
    lens = [1, 2, 0, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100, 4097 + 40, 64, 7, 300, 66, 79, 80, 81, 95,
            96, 97]
    nrows = len(lens)
    side = random_side(layout, nrows, ncols, lens, seed=3 * k)
    rng = np.random.default_rng(7 + k)
    ld = layout.padded_k(k)
    F = rng.normal(scale=0.3, size=(ncols, k))
    b_self = rng.normal(scale=0.2, size=nrows).astype(np.float32)
    b_other = rng.normal(scale=0.2, size=ncols).astype(np.float32)
    lam_row = rng.uniform(0.5, 4.0, size=nrows).astype(np.float32)
    mu, lam_b = 3.3, 1.7
    # the engine uses the dual form above k = 64 (layout.dual_max_len); the kernel also takes rows whose
    # 16-rating blocks are fewer than k/16 at smaller k - exercised here as well
    dl = 64 if k > 64 else 16 * (layout.padded_k(k) // 16 - 1)
    assert layout.dual_max_len(k) == (64 if k > 64 else 0)
    dm = layout.dual_mid_len(k)                               # 96 above k = 96: rows of 65 ... 96 ratings
    t = layout.build_row_tasks(side.indptr, dual_len=dl, mid_len=dm)
    n_short = sum(1 for l in lens if 0 < l <= dl)
    assert t.ndual == n_short and t.nslots == 2 and t.nmid == sum(1 for l in lens if dl < l <= dm)
    sd = side_dev(side, dev)
    f32 = torch.float32
    Fd = torch.from_numpy(pad(F, ld, 1)).to(dev)
    ws = torch.empty(t.nslots * be.slot_bytes(k) // 4, dtype=f32, device=dev)

    def run(tasks):
        X = torch.full((nrows, ld), 7.0, dtype=f32, device=dev)
        bias = torch.from_numpy(b_self.copy()).to(dev)
        stat = torch.zeros(nrows, 2, dtype=f32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        be.row_solve(k=k, ld=ld, side=sd, F=Fd, zero_row=ncols, bias_self=bias,
                     bias_other=torch.from_numpy(b_other).to(dev),
                     mu=torch.tensor([mu], dtype=torch.float64, device=dev), lam=0.0,
                     lam_row=torch.from_numpy(lam_row).to(dev), lam_b=lam_b, lam_b_row=None,
                     rhs_extra=None, diag_extra=None, X_out=X, bias_out=bias, gram_out=None, factor_out=None,
                     rhs_out=None, colsum_out=None, sumr_out=None, status=status, tasks=tasks, workspace=ws,
                     stat_out=stat)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        return X.cpu().numpy().astype(np.float64), bias.cpu().numpy().astype(np.float64), stat.cpu().numpy().astype(np.float64)

    td = tasks_dev(t, dev)
    Xd, bd, sd_ = run(td)
    td.ndual = td.nmid = 0                                    # same tasks, everything primal
    Xp, bp, sp = run(td)
    F32 = F.astype(np.float32).astype(np.float64)
    for r in range(nrows):
        lo, hi = side.indptr[r], side.indptr[r + 1]
        if hi == lo:
            assert np.all(Xd[r] == 7.0) and bd[r] == b_self[r]
            continue
        idx = side.indices[lo:hi]
        Fr = F32[idx]
        vals = side.vals[lo:hi].astype(np.float64)
        rb = vals - mu - b_other[idx]
        A = Fr.T @ Fr + (lam_row[r] + 1e-10) * np.eye(k)
        x = np.linalg.solve(A, Fr.T @ (rb - b_self[r]))
        scale = max(np.max(np.abs(x)), 1e-6)
        for X, tag in ((Xd, "dual"), (Xp, "primal")):
            np.testing.assert_allclose(X[r, :k], x, rtol=0, atol=1e-4 * scale, err_msg=f"{tag} row {r} nnz {hi - lo}")
            assert np.all(X[r, k:] == 0.0)
        bref = np.sum(rb - Fr @ x) / ((hi - lo) + lam_b + 1e-10)
        d = rb - Fr @ x - bref
        for b_, s_, tag in ((bd, sd_, "dual"), (bp, sp, "primal")):
            assert abs(b_[r] - bref) <= 2e-5 * max(1.0, abs(bref)), (tag, r)
            assert abs(s_[r, 0] - d.sum()) <= 2e-4 * max(1.0, np.abs(d).sum()), (tag, r, s_[r, 0], d.sum())
            assert abs(s_[r, 1] - (d * d).sum()) <= 1e-3 * max(1.0, (d * d).sum()), (tag, r, s_[r, 1], (d * d).sum())
    # the two forms are different roundings of the same solution
    np.testing.assert_allclose(Xd, Xp, rtol=0, atol=1e-4 * np.abs(Xp).max())


def test_dual_classes_are_ignored_by_calls_with_byproducts():
    """Regression: a factor-only call (no X_out) whose task list carries dual classes (here: only the
    65...96 class, no short rows) must keep every row primal - the dual kernels write X_out."""
    torch, layout, side_dev, tasks_dev, be, dev = env("f16x2")
    k, ncols = 128, 3000
    lens = [70, 80, 96, 200, 90]
    nrows = len(lens)
    side = random_side(layout, nrows, ncols, lens, seed=5)
    rng = np.random.default_rng(6)
    ld = layout.padded_k(k)
    t = layout.build_row_tasks(side.indptr, dual_len=64, mid_len=96)
    assert t.ndual == 0 and t.nmid == 4
    f32 = torch.float32
    F = torch.from_numpy(pad(rng.normal(scale=0.3, size=(ncols, k)), ld, 1)).to(dev)
    factor = torch.zeros(nrows * ld * ld, dtype=f32, device=dev)
    rhs = torch.zeros(nrows, ld, dtype=f32, device=dev)
    cs = torch.zeros(nrows, ld, dtype=f32, device=dev)
    sumr = torch.zeros(nrows, dtype=f32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    be.row_solve(k=k, ld=ld, side=side_dev(side, dev), F=F, zero_row=ncols,
                 bias_self=torch.zeros(nrows, dtype=f32, device=dev), bias_other=torch.zeros(ncols, dtype=f32, device=dev),
                 mu=torch.tensor([3.0], dtype=torch.float64, device=dev), lam=2.0, lam_row=None, lam_b=1.0,
                 lam_b_row=None, rhs_extra=None, diag_extra=None, X_out=None, bias_out=None, gram_out=None,
                 factor_out=factor, rhs_out=rhs, colsum_out=cs, sumr_out=sumr, status=status,
                 tasks=tasks_dev(t, dev), workspace=None)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    M = factor.view(nrows, ld, ld).cpu().numpy()
    assert all(np.all(np.diag(M[r]) > 0) for r in range(nrows))         # every row was factorised (1/L_ii > 0)
    assert np.all(np.abs(rhs.cpu().numpy()).sum(axis=1) > 0)


def test_dual_and_primal_agree_on_random_shapes():
    """Seeded sweep over ranks and row-length mixes: the dual classes (<= 64 ratings; 65...96 above k = 96)
    and the primal kernel must agree row by row within the fp32 tolerance, including bias and residual sums."""
    torch, layout, side_dev, tasks_dev, be, dev = env("f16x2")
    rng = np.random.default_rng(2024)
    f32 = torch.float32
    for trial in range(12):
        k = int(rng.integers(65, 161))
        ncols = int(rng.integers(200, 3000))
        nrows = int(rng.integers(5, 60))
        lens = [int(x) for x in np.minimum(rng.integers(0, 130, size=nrows), ncols)]
        side = random_side(layout, nrows, ncols, lens, seed=1000 + trial)
        ld = layout.padded_k(k)
        t = layout.build_row_tasks(side.indptr, dual_len=64, mid_len=layout.dual_mid_len(k))
        Fd = torch.from_numpy(pad(rng.normal(scale=0.3, size=(ncols, k)), ld, 1)).to(dev)
        b_self = torch.from_numpy(rng.normal(scale=0.2, size=nrows).astype(np.float32)).to(dev)
        b_other = torch.from_numpy(rng.normal(scale=0.2, size=ncols).astype(np.float32)).to(dev)
        lam = float(rng.uniform(0.05, 5.0))
        sd = side_dev(side, dev)

        def run(tasks):
            X = torch.zeros(nrows, ld, dtype=f32, device=dev)
            bias = b_self.clone()
            stat = torch.zeros(nrows, 2, dtype=f32, device=dev)
            status = torch.zeros(1, dtype=torch.int32, device=dev)
            be.row_solve(k=k, ld=ld, side=sd, F=Fd, zero_row=ncols, bias_self=bias, bias_other=b_other,
                         mu=torch.tensor([3.1], dtype=torch.float64, device=dev), lam=lam, lam_row=None, lam_b=1.3,
                         lam_b_row=None, rhs_extra=None, diag_extra=None, X_out=X, bias_out=bias, gram_out=None,
                         factor_out=None, rhs_out=None, colsum_out=None, sumr_out=None, status=status, tasks=tasks,
                         workspace=None, stat_out=stat)
            torch.cuda.synchronize()
            assert int(status.item()) == 0
            return X.cpu().numpy(), bias.cpu().numpy(), stat.cpu().numpy()

        td = tasks_dev(t, dev)
        Xd, bd, sdl = run(td)
        td.ndual = td.nmid = 0
        Xp, bp, sp = run(td)
        scale = max(float(np.abs(Xp).max()), 1e-6)
        np.testing.assert_allclose(Xd, Xp, rtol=0, atol=5e-4 * scale, err_msg=f"trial {trial} k {k}")
        np.testing.assert_allclose(bd, bp, rtol=0, atol=3e-4)
        np.testing.assert_allclose(sdl, sp, rtol=2e-3, atol=2e-3)
