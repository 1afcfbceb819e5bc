"""Reference of the input-scale tests of als_row_solve (tests/test_gpu_row_scale.py), numpy only; validated without a
device by tests/test_row_scale_ref_cpu.py.

als_row_solve is linear in the ratings, the global mean, the biases and rhs_extra: multiply them by 2^p and x, the
bias and stat_out[:, 0] come back multiplied by 2^p, stat_out[:, 1] by 2^2p.  Everything here serves that statement:
one input for all kernel paths (`make_input`), its exact 2^p multiples (`scaled_inputs`), the fp64 solution at p = 0
(`solve_fp64`; the reference at scale p is 2^p times it, exactly), and the two pieces of the pre-split path that are
NOT scale-free by construction - the fp16 pair a residual is rounded to (`split_pair`) and the power-of-two scale
the caller gives it (`residual_scale`, the numpy statement of HipBackend.residual_scale)."""
from types import SimpleNamespace

import numpy as np

PS = (-24, -12, -6, 0, 6, 12, 17, 24)
NCOLS = 5000
MU = float(np.float32(3.3))             # the fp32 kernels read (float) mu: an fp32 value keeps every path on one input
LAM_B = 1.7
SMALL_ROWS = (5, 10)                    # rows (65 and 700 ratings) whose residuals are 2^-8 of the ordinary ones

F16 = np.finfo(np.float16)
F16_OVERFLOW = float(F16.max) + 2.0 ** (F16.maxexp - 2 - F16.nmant)  # 65520: what rounds to inf (half an ulp past max)
F16_HALF_SUBNORMAL = float(F16.smallest_subnormal) / 2.0            # 2^-25: absolute error of a subnormal low term
F16_U = float(F16.eps) / 2.0                                         # 2^-11: unit roundoff of a normal fp16


def lens(k):
    """The row classes of the existing kernel tests: 1, 2, empty, < k, 64 / 65 (chunk edge), k, 3k + 5, 511 / 513 /
    700 (the 512-rating flush of the f16x2 accumulators, where fold_planes_rhs runs mid-row), 4097 (split row)."""
    return [1, 2, 0, 33, 64, 65, k, 3 * k + 5, 511, 513, 700, 4097]


def make_input(k, extra=False, seed=0):
    """The one input of every path, fp32 host arrays: CSR rows of `lens(k)` over NCOLS columns, ratings on the
    half-star grid 0.5 ... 5.0 except SMALL_ROWS, F = normal(0.3) [NCOLS + 1, ld] with the zero row appended,
    lam_row in 0.5 ... 4, biases ~ N(0, 0.2); `extra`: with an rhs_extra ~ N(0, 0.5) [nrows, ld]."""
    L = lens(k)
    nrows, ld = len(L), 16 * ((k + 15) // 16)
    rng = np.random.default_rng(4000 + 31 * k + seed)
    indptr = np.zeros(nrows + 1, np.int64)
    indptr[1:] = np.cumsum(L)
    indices = np.concatenate([np.sort(rng.choice(NCOLS, size=n, replace=False)) for n in L]).astype(np.int32)
    vals = (np.round(rng.uniform(0.5, 5.0, size=indices.size) * 2) / 2).astype(np.float32)
    F = np.zeros((NCOLS + 1, ld), np.float32)
    F[:NCOLS, :k] = rng.normal(scale=0.3, size=(NCOLS, k))
    b_self = rng.normal(scale=0.2, size=nrows).astype(np.float32)
    b_other = rng.normal(scale=0.2, size=NCOLS).astype(np.float32)
    lam_row = rng.uniform(0.5, 4.0, size=nrows).astype(np.float32)
    for r in SMALL_ROWS:
        sl = slice(indptr[r], indptr[r + 1])
        noise = rng.normal(size=L[r])
        vals[sl] = (MU + np.float64(b_self[r]) + b_other[indices[sl]].astype(np.float64) + 2.0 ** -8 * noise)
    rhs_extra = None
    if extra:
        rhs_extra = np.zeros((nrows, ld), np.float32)
        rhs_extra[:, :k] = rng.normal(scale=0.5, size=(nrows, k))
    side = SimpleNamespace(nrows=nrows, ncols=NCOLS, indptr=indptr, indices=indices, vals=vals)
    return SimpleNamespace(k=k, ld=ld, nrows=nrows, side=side, F=F, b_self=b_self, b_other=b_other, lam_row=lam_row,
                           rhs_extra=rhs_extra, mu=MU, lam_b=LAM_B, lens=np.asarray(L))


def _times_pow2(a, p):
    """a * 2^p in fp32, asserted exact: every non-zero product a normal, finite fp32 number that divides back to the
    bits of a."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    s = np.float32(2.0 ** p)
    with np.errstate(over="ignore"):
        out = a * s
    nz = a != 0
    assert np.isfinite(out).all(), p
    assert (np.abs(out[nz]) >= np.finfo(np.float32).tiny).all(), p
    assert (out / s).tobytes() == a.tobytes(), p
    return out


def scaled_inputs(side, mu, b_self, b_other, rhs_extra, p):
    """(side, mu, b_self, b_other, rhs_extra) with the ratings, mu, both biases and rhs_extra times 2^p - exact in fp32
    (asserted), so the exact solution of the scaled problem is 2^p times the solution of the original."""
    mu32 = np.float32(mu)
    assert float(mu32) == float(mu), "mu must be an fp32 value"
    sside = SimpleNamespace(nrows=side.nrows, ncols=side.ncols, indptr=side.indptr, indices=side.indices,
                            vals=_times_pow2(side.vals, p))
    return (sside, float(_times_pow2(np.array([mu32]), p)[0]), _times_pow2(b_self, p), _times_pow2(b_other, p),
            None if rhs_extra is None else _times_pow2(rhs_extra, p))


def solve_fp64(inp):
    """Per row, in fp64 from the fp32 inputs, as tests/test_gpu_kernels.py::test_row_solve_against_numpy forms them:
    x = (F_r^T F_r + (lam_row + 1e-10) I)^-1 (F_r^T (vals - mu - b_other - b_self) + rhs_extra), the bias
    sum(vals - F_r x - mu - b_other) / (n + lam_b + 1e-10) and the residual sums (sum d, sum d^2) with the new x and
    bias.  Empty rows: None.  Also what the tolerances of the statistics are relative to (sum |d|, ...)."""
    k, side = inp.k, inp.side
    F64 = inp.F[:, :k].astype(np.float64)
    out = []
    for r in range(inp.nrows):
        lo, hi = side.indptr[r], side.indptr[r + 1]
        if hi == lo:
            out.append(None)
            continue
        idx = side.indices[lo:hi]
        Fr = F64[idx]
        rho = side.vals[lo:hi].astype(np.float64) - inp.mu - inp.b_other[idx].astype(np.float64)
        A = Fr.T @ Fr + (float(inp.lam_row[r]) + 1e-10) * np.eye(k)
        b = Fr.T @ (rho - float(inp.b_self[r]))
        if inp.rhs_extra is not None:
            b = b + inp.rhs_extra[r, :k].astype(np.float64)
        x = np.linalg.solve(A, b)
        bias = float(np.sum(rho - Fr @ x) / ((hi - lo) + inp.lam_b + 1e-10))
        d = rho - Fr @ x - bias
        out.append(dict(x=x, bias=bias, sd=float(d.sum()), sd2=float((d * d).sum()), d_abs=float(np.abs(d).sum()),
                        rho_abs=float(np.abs(rho).sum()), rho2=float((rho * rho).sum()), A=A, b=b, rho=rho, Fr=Fr))
    return out


def split_pair(r, s):
    """The two fp16 terms of the residuals r (fp32) as gram_accumulate forms them with residual scale s (a power of
    two): y = r s in fp32, h = fp16(y), l = fp16(y - h), both round-to-nearest-even.  -> (h, l) as float16.  (The kernel also adds what the fp32 subtraction that
    produced r dropped to the low term before rounding it; for an r given exactly, as here, that term is zero.)"""
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.asarray(r, np.float32) * np.float32(s)
        h = y.astype(np.float16)
        l = (y - h.astype(np.float32)).astype(np.float16)
    return h, l


def pair_value(h, l, s):
    """What the pair stands for, in fp64: (h + l) / s."""
    with np.errstate(invalid="ignore"):
        return (h.astype(np.float64) + l.astype(np.float64)) / float(s)


def pair_bound(y_abs):
    """Relative error bound of the pair of a scaled residual of magnitude y_abs > 0 that fp16 holds as a normal, finite
    number: h is within u |y| (u = 2^-11), the remainder y - h is exact in fp32, and l rounds it to within u of itself
    when it is a normal fp16 number, to within half the smallest subnormal (2^-25) when it is not:
    max(u^2, 2^-25 / |y|)."""
    return np.maximum(F16_U * F16_U, F16_HALF_SUBNORMAL / np.asarray(y_abs, np.float64))


def residual_scale(max_abs_val):
    """The backend's rule (HipBackend.residual_scale): the power of two that puts max_abs_val in [2^9, 2^10), clamped
    to 2^-126 ... 2^126 so that the scale and its inverse are normal fp32 numbers; 1.0 without a positive finite
    maximum."""
    v = float(max_abs_val)
    if not (0.0 < v < np.inf):
        return 1.0
    e = int(np.frexp(v)[1]) - 1                     # v in [2^e, 2^(e + 1))
    return float(np.ldexp(1.0, int(np.clip(9 - e, -126, 126))))
