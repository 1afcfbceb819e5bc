"""numpy-only inputs and references for the prediction, statistics and factor-scale entry points: als_predict_dense,
als_predict_at, als_compose_z (csrc/predict.hip), als_residual_stats, als_sumsq, als_sum_pairs, als_history_row
(csrc/stats.hip) and als_factor_scale (csrc/row_solve.hip).  Used by tests/test_gpu_stats_predict.py on the device and
validated without one by tests/test_stats_predict_ref_cpu.py.

Two kinds of input, as in tests/w_step_ref.py:

"exact"  factors are integers in [-3, 3]; ratings, mu and the biases of the statistics fixture are multiples of 1/8 with
         |.| <= 16.  A dot product is then an integer of at most 9 * 160, a residual d a multiple of 1/8 below 2^11,
         and every fp32 operation of a correct kernel is exact in any summation order; sum d and sum d^2 over 10^5
         ratings stay below 2^53 in units of 1/64, so the fp64 sums are exact too.  Comparisons are for equality.
         The PREDICTION fixture adds 2^-20-scale parts to its biases on purpose: the dot product is still exact, the
         epilogue is not, and the expected value is formed in np.float32 step by step as ((dot + float32(mu)) + b_u)
         + b_i - the association walk::score (csrc/catalogue_walk.hpp) promises.  `expected_predict_exact` can also
         form the other associations (ASSOCIATIONS) and a mu kept in double, so that the CPU test can show that the
         fixture tells them apart.
"real"   normal factors; every expected value comes in fp64 with its absolute-sum companion S (the same expression with
         every term replaced by its absolute value); rounding bounds are stated against S.  mu enters as float32(mu),
         the value the kernels are specified to use.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from collaborative_filtering_amd import layout

U32, U64 = 2.0 ** -24, 2.0 ** -53
KS = (1, 17, 33, 50, 65, 81, 100, 113, 129, 160)            # one per KB = ld / 16 = 1 ... 10
SENTINEL_ELEMS = 64

# ---- prediction ------------------------------------------------------------------------------------------------------
MU_EXACT = 3.375
# float32(MU_EXTRA) = 12.375 (the excess stays below half an ulp, 2^-21): a kernel that adds mu as a double gets
# another float wherever |dot + mu| < 8
MU_EXTRA = 12.375 + (2.0 ** -21 - 2.0 ** -40)
DENSE_MS = (1, 15, 16, 17, 33)
DENSE_NS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)
DENSE_SHAPE_KS = (33, 128)
AT_NPAIRS = (1, 3, 4, 5, 15, 16, 17, 1001, 131072 + 37)
ASSOCIATIONS = ("left", "mu_bu_first", "offset_first")       # "left" is the contract


def _pad(A, ld):
    out = np.zeros((A.shape[0], ld), dtype=np.float32)
    out[:, : A.shape[1]] = A
    return out


def exact_factors(rng, rows, k):
    return rng.integers(-3, 4, size=(rows, k)).astype(np.float32)


def eighths(rng, size, lim=16.0):
    """Multiples of 1/8 with |.| <= lim."""
    return (rng.integers(-int(lim * 8), int(lim * 8) + 1, size=size) / 8.0).astype(np.float32)


def mixed_biases(rng, size):
    """Mixed sign and magnitude: half of them 8 <= |b| < 16 with a part of a few 2^-20, the rest below 1 with an odd
    multiple of 2^-23 (bits that no sum with mu or a dot product keeps)."""
    big = rng.integers(64, 127, size=size) / 8.0 + rng.integers(-7, 8, size=size) * 2.0 ** -20
    small = rng.integers(1, 8, size=size) / 8.0 + (2 * rng.integers(-7, 8, size=size) + 1) * 2.0 ** -23
    b = np.where(rng.random(size) < 0.5, big, small) * rng.choice([-1.0, 1.0], size=size)
    out = b.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), b) and np.all(np.abs(out) < 16)
    return out


def tied_case(k):
    """(mu, fine unit, bound on the 1/8 part) of the "tied" biases: b_u = B_u + 5 units, b_i = B_i + 6 units, B a multiple
    of 1/8 of either sign.  dot + mu + B_u + B_i is a multiple of 1/8, so where the ulp of the score is 2, 4 or 8 units
    the association decides the result: adding b_u and then b_i rounds 5 and 6 units one after the other, adding
    b_u + b_i rounds 11 units at once, and mu + b_u loses bits of its own from |mu + b_u| >= 4 on.  The unit is 2^-22
    (an ulp of 2 ... 8 units: 8 <= |score| < 64, where most scores of k >= 17 lie), and 2^-24 with mu and B eight
    times smaller at k = 1, whose |dot| <= 9.  tests/test_stats_predict_ref_cpu.py measures the share of entries on
    which the ASSOCIATIONS differ."""
    return (0.375, 2.0 ** -24, 1.0) if k == 1 else (MU_EXACT, 2.0 ** -22, 4.0)


def tied_biases(rng, size, fine, unit, lim):
    b = rng.integers(-int(lim * 8) + 1, int(lim * 8), size=size) / 8.0 + fine * unit
    out = b.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), b)
    return out


def predict_inputs(k, m, n, kind, seed, mu=None, biases="tied"):
    """U [m, ld], Z [n, ld] (padding columns zero), b_u [m], b_i [n] float32 and mu (a Python float: the device double).
    Exact inputs take their biases from `tied_biases` (mu from `tied_case` unless given) or `mixed_biases`."""
    assert kind in ("exact", "real") and biases in ("tied", "mixed")
    rng = np.random.default_rng(seed)
    ld = layout.padded_k(k)
    if kind == "exact":
        U, Z = exact_factors(rng, m, k), exact_factors(rng, n, k)
        if biases == "tied":
            mu_k, unit, lim = tied_case(k)
            b_u, b_i = tied_biases(rng, m, 5, unit, lim), tied_biases(rng, n, 6, unit, lim)
        else:
            mu_k = MU_EXACT
            b_u, b_i = mixed_biases(rng, m), mixed_biases(rng, n)
        mu = mu_k if mu is None else mu
    else:
        U = rng.normal(scale=0.3, size=(m, k)).astype(np.float32)
        Z = rng.normal(scale=0.3, size=(n, k)).astype(np.float32)
        b_u = rng.normal(scale=0.2, size=m).astype(np.float32)
        b_i = rng.normal(scale=0.2, size=n).astype(np.float32)
        mu = 3.4 if mu is None else mu
    return SimpleNamespace(k=k, ld=ld, m=m, n=n, kind=kind, U=_pad(U, ld), Z=_pad(Z, ld), b_u=b_u, b_i=b_i, mu=float(mu))


def exact_dots(inp):
    """U Z^T of exact inputs as float32 [m, n], every entry an integer of at most 9 k."""
    d = inp.U[:, : inp.k].astype(np.int64) @ inp.Z[:, : inp.k].astype(np.int64).T
    assert np.max(np.abs(d), initial=0) <= 9 * inp.k
    return d.astype(np.float32)


def expected_predict_exact(inp, assoc="left", mu_double=False):
    """float32 [m, n]: ((dot + float32(mu)) + b_u) + b_i, every step rounded to float32.  assoc / mu_double: what a
    kernel that breaks the contract would write instead (for the CPU test of the fixture, never expected on the device)."""
    f32 = np.float32
    dot = exact_dots(inp)
    bu, bi = inp.b_u[:, None].astype(f32), inp.b_i[None, :].astype(f32)
    mu = f32(inp.mu)
    if mu_double:
        assert assoc == "left"
        first = (dot.astype(np.float64) + np.float64(inp.mu)).astype(f32)
        return ((first + bu).astype(f32) + bi).astype(f32)
    if assoc == "left":
        return (((dot + mu).astype(f32) + bu).astype(f32) + bi).astype(f32)
    if assoc == "mu_bu_first":                                   # dot + (mu + b_u) + b_i
        return ((dot + (mu + bu).astype(f32)).astype(f32) + bi).astype(f32)
    assert assoc == "offset_first"                               # dot + ((mu + b_u) + b_i)
    return (dot + ((mu + bu).astype(f32) + bi).astype(f32)).astype(f32)


def expected_predict_real(inp):
    """(P, S) float64 [m, n]: P = U Z^T + float32(mu) + b_u + b_i, S = |U| |Z|^T + |mu| + |b_u| + |b_i|."""
    U, Z = inp.U[:, : inp.k].astype(np.float64), inp.Z[:, : inp.k].astype(np.float64)
    mu = float(np.float32(inp.mu))
    bu, bi = inp.b_u.astype(np.float64)[:, None], inp.b_i.astype(np.float64)[None, :]
    return U @ Z.T + mu + bu + bi, np.abs(U) @ np.abs(Z).T + abs(mu) + np.abs(bu) + np.abs(bi)


def predict_pairs(m, n, npairs, seed):
    """(us, is) int32 with repeats; the corners u = 0, u = m - 1, i = 0, i = n - 1 are present from 4 pairs on."""
    rng = np.random.default_rng(seed)
    us = rng.integers(0, m, size=npairs).astype(np.int32)
    is_ = rng.integers(0, n, size=npairs).astype(np.int32)
    if npairs >= 4:
        us[:4], is_[:4] = [0, m - 1, 0, m - 1], [0, n - 1, n - 1, 0]
        us[-1], is_[-1] = us[0], is_[0]                          # a repeat that ends the list
    elif npairs == 3:
        us[:], is_[:] = [0, m - 1, 0], [n - 1, 0, n - 1]
    return us, is_


# ---- als_compose_z ---------------------------------------------------------------------------------------------------
COMPOSE_DS, COMPOSE_NS, COMPOSE_KS = (0, 1, 7), (1, 5, 300), (1, 50, 160)


def compose_inputs(k, n, D, kind, seed):
    rng = np.random.default_rng(seed)
    ld = layout.padded_k(k)
    if kind == "exact":
        V, X, W = exact_factors(rng, n, k), exact_factors(rng, n, D), exact_factors(rng, D, k)
    else:
        V = rng.normal(scale=0.3, size=(n, k)).astype(np.float32)
        X = rng.normal(size=(n, D)).astype(np.float32)
        W = rng.normal(scale=0.2, size=(D, k)).astype(np.float32)
    return SimpleNamespace(k=k, ld=ld, n=n, D=D, V=_pad(V, ld), X=X, W=_pad(W, ld))


def expected_compose(inp):
    """(Z, S) float64 [n, ld] over ALL ld columns: Z = V + X W, S = |V| + |X| |W|; both zero in the padding columns."""
    V, X, W = inp.V.astype(np.float64), inp.X.astype(np.float64), inp.W.astype(np.float64)
    return V + X @ W, np.abs(V) + np.abs(X) @ np.abs(W)


# ---- als_residual_stats ----------------------------------------------------------------------------------------------
STATS_NCOLS = 9000
MANY_ROWS, MANY_NCOLS = 1500, 64


def stats_lens(k):
    """Empty, 1, the tails len % 4 and len % 64, one short of / exactly / one over ALS_SPLIT_CHUNK, two and three segments."""
    return [0, 1, 2, 3, 4, 5, 63, 64, 65, 66, 67, 4095, 4096, 4097, 8192, 8193 + k]


def many_lens(seed=3):
    """1500 short rows, more than 1100 of them non-empty: more than 1024 tasks, more than 256 partials."""
    lens = np.random.default_rng(seed).integers(0, 9, size=MANY_ROWS)
    lens[::13] = 0
    return [int(x) for x in lens]


def stats_inputs(k, kind, lens, ncols, seed):
    rng = np.random.default_rng(seed)
    ld = layout.padded_k(k)
    m = len(lens)
    indptr = np.zeros(m + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = np.concatenate([np.sort(rng.choice(ncols, size=l, replace=False)) for l in lens] + [np.zeros(0, np.int64)])
    indices = indices.astype(np.int32)
    nnz = int(indptr[-1])
    if kind == "exact":
        U, Z = exact_factors(rng, m, k), exact_factors(rng, ncols, k)
        b_u, b_i, vals, mu = eighths(rng, m), eighths(rng, ncols), eighths(rng, nnz), -2.625
    else:
        U = rng.normal(scale=0.3, size=(m, k)).astype(np.float32)
        Z = rng.normal(scale=0.3, size=(ncols, k)).astype(np.float32)
        b_u = rng.normal(scale=0.2, size=m).astype(np.float32)
        b_i = rng.normal(scale=0.2, size=ncols).astype(np.float32)
        vals = (np.round(rng.uniform(0.5, 5.0, size=nnz) * 2) / 2).astype(np.float32)
        mu = 3.4
    return SimpleNamespace(k=k, ld=ld, m=m, ncols=ncols, kind=kind, nnz=nnz, indptr=indptr, indices=indices, vals=vals,
                           U=_pad(U, ld), Z=_pad(Z, ld), b_u=b_u, b_i=b_i, mu=float(mu))


def residuals(inp):
    """(d, S) float64 per rating: d = r - (U_u . Z_i + float32(mu) + b_u + b_i) and its absolute-sum companion."""
    ru = np.repeat(np.arange(inp.m), np.diff(inp.indptr))
    ri = inp.indices
    U, Z = inp.U[:, : inp.k].astype(np.float64), inp.Z[:, : inp.k].astype(np.float64)
    mu = float(np.float32(inp.mu))
    dot, adot = np.zeros(inp.nnz), np.zeros(inp.nnz)
    for s in range(0, inp.nnz, 8192):
        a, b = U[ru[s:s + 8192]], Z[ri[s:s + 8192]]
        dot[s:s + 8192], adot[s:s + 8192] = np.sum(a * b, axis=1), np.sum(np.abs(a * b), axis=1)
    v, bu, bi = inp.vals.astype(np.float64), inp.b_u.astype(np.float64)[ru], inp.b_i.astype(np.float64)[ri]
    return v - (dot + mu + bu + bi), np.abs(v) + adot + abs(mu) + np.abs(bu) + np.abs(bi)


def expected_stats(inp):
    """(sum d, sum d^2, bound on sum d, bound on sum d^2).  Exact inputs: the sums are exact (checked) and the bounds
    are not to be used.  Real inputs: with e_r = (ld + 3) u32 S_r the most a rating's fp32 residual can be off,
      |sum d|   <= sum e_r + nnz u64 sum (|d_r| + e_r)
      |sum d^2| <= sum e_r (2 |d_r| + e_r) + (nnz + 1) u64 sum (|d_r| + e_r)^2
    (the fp64 square rounds once, the fp64 sums add at most nnz - 1 times, in any order)."""
    d, S = residuals(inp)
    if inp.kind == "exact":
        d8 = d * 8.0
        assert np.array_equal(d8, np.rint(d8)) and np.max(np.abs(d), initial=0) < 2 ** 11
        i8 = d8.astype(np.int64)
        s0, s1 = int(i8.sum()), int((i8 * i8).sum())
        assert abs(s0) < 2 ** 53 and s1 < 2 ** 53
        return s0 / 8.0, s1 / 64.0, 0.0, 0.0
    e = (inp.ld + 3) * U32 * S
    ad = np.abs(d) + e
    b0 = e.sum() + inp.nnz * U64 * ad.sum()
    b1 = (e * (2 * np.abs(d) + e)).sum() + (inp.nnz + 1) * U64 * (ad * ad).sum()
    return float(np.sum(d)), float(np.sum(d * d)), float(b0), float(b1)


# ---- als_sumsq / als_sum_pairs / als_history_row ---------------------------------------------------------------------
SUMSQ_BLOCKS = 1024
SUMSQ_NS = (0, 1, 2, 3, 4, 5, 1023, 1027, 4 * 256 * SUMSQ_BLOCKS + 7)          # the last: above the block cap, n & 3 = 3
SUM_PAIRS_NS = (0, 1, 255, 256, 257, 256 * SUMSQ_BLOCKS + 3)
# (nU, nV, nb_u, nb_i): every residue mod 4, one array above the block cap, one of length 0
HISTORY_LENGTHS = ((4 * 256 * SUMSQ_BLOCKS + 11, 0, 301, 502), (1088, 4099, 301, 502))


def exact_vector(rng, n):
    return rng.integers(-3, 4, size=n).astype(np.float32)


def real_vector(rng, n):
    return rng.normal(scale=0.3, size=n).astype(np.float32)


def expected_sumsq(x):
    """(sum x^2 in fp64, the exact integer when x holds integers else None)."""
    x64 = x.astype(np.float64)
    exact = int((x.astype(np.int64) ** 2).sum()) if np.array_equal(x64, np.rint(x64)) else None
    return float(np.sum(x64 * x64)), exact


def expected_sum_pairs(x):
    """Column sums of x viewed as [npairs, 2]: (fp64 sums [2], absolute sums [2])."""
    p = x.astype(np.float64).reshape(-1, 2)
    return p.sum(axis=0), np.abs(p).sum(axis=0)


def expected_history_scalars(stats, nnz, mu):
    """(rmse, mu_new): the host's fp64 operations one by one - mean_d = s0 / nnz, mu + mean_d,
    sqrt(max(s1 / nnz - mean_d * mean_d, 0)); a NaN (nnz = 0) stays a NaN."""
    f = np.float64
    with np.errstate(all="ignore"):
        mean_d = f(stats[0]) / f(nnz)
        m = f(mu) + mean_d
        sq = mean_d * mean_d
        var = f(stats[1]) / f(nnz) - sq
        rmse = np.sqrt(f(0.0) if var < 0.0 else var)
    return rmse, m


# ---- als_factor_scale ------------------------------------------------------------------------------------------------
SCALE_NFLOATS = (0, 4, 4096, 4 * 1024 * 3 + 4, 4 * (4 * 512 * 256 + 5))
SCALE_J_MAX = 60


def expected_scale(F):
    """(scale[0], scale[1]) = (2^j, 2^-2j) float32, j = 14 - floor(log2 max|F|) clamped to [-60, 60]; max|F| = 0 (or
    a denormal) gives j = 60, a NaN / inf in F gives j = -60 (the clamps the kernel comment documents)."""
    F = np.asarray(F, dtype=np.float32)
    if F.size and not np.isfinite(F).all():
        j = -SCALE_J_MAX
    else:
        mx = float(np.max(np.abs(F))) if F.size else 0.0
        if mx == 0.0:
            j = SCALE_J_MAX
        else:
            _, e = np.frexp(mx)                                   # mx = mant 2^e, mant in [1/2, 1): floor(log2 mx) = e - 1
            j = int(min(max(14 - (int(e) - 1), -SCALE_J_MAX), SCALE_J_MAX))
    return np.float32(2.0 ** j), np.float32(2.0 ** (-2 * j))


def scale_geometry(nfloats):
    """(n4, grid, stride) of k_factor_scale: float4 count, workgroups, float4 stride between the unrolled slots."""
    n4 = nfloats // 4
    grid = min(512, max(1, (n4 + 1023) // 1024))
    return n4, grid, grid * 256


def scale_positions(nfloats):
    """Float positions for max|F|: the first and the last element and one in every unrolled slot u = 0 ... 3 of the
    final trip of the kernel's loop that holds data (different lanes of the float4)."""
    n4, _, stride = scale_geometry(nfloats)
    if n4 == 0:
        return []
    pos = {0, nfloats - 1}
    trip0 = (n4 - 1) // (4 * stride) * (4 * stride)               # first float4 of the final trip
    for u in range(4):
        lo, hi = trip0 + u * stride, min(trip0 + (u + 1) * stride, n4)
        if lo < hi:
            pos.add(4 * ((lo + hi) // 2) + u)
            pos.add(4 * (hi - 1) + (3 - u))
    return sorted(pos)


def scale_values():
    """name -> the float32 placed as max|F| (its background is scaled below it by `scale_background`)."""
    f32 = np.float32
    return {
        "negative": f32(-0.8125), "positive": f32(5.5), "pow2": f32(2.0 ** -3), "below_pow2": np.nextafter(f32(2.0 ** 4), f32(0)),
        "tiny": f32(1e-30), "huge": f32(1e30), "denormal": f32(3e-41), "zero": f32(0.0), "nan": f32(np.nan),
        "inf": f32(-np.inf),
    }


def scale_background(rng, nfloats, v):
    """nfloats float32 of mixed sign, all strictly below |v| in magnitude (zeros under a denormal or zero maximum;
    ordinary numbers under a NaN / inf)."""
    v = np.float32(v)
    if not np.isfinite(v):
        mag = 1.0
    elif abs(float(v)) < 2.0 ** -126:
        return np.zeros(nfloats, dtype=np.float32)
    else:
        mag = 2.0 ** (np.frexp(float(abs(v)))[1] - 1)            # 2^floor(log2 |v|) <= |v|
    base = rng.uniform(0.25, 0.5, size=nfloats) * rng.choice([-1.0, 1.0], size=nfloats)
    return (base * mag).astype(np.float32)
