"""numpy-only inputs and fp64 reference for the W-step kernels (csrc/w_step.hip): als_w_normal_equations phase 0
(k_w_item_vectors / k_w_item_vectors_f64), phase 1 (k_w_accumulate, k_w_reduce) and als_item_stats / als_item_stats_f64.

`build_inputs` makes the V-step by-products of n items from synthetic users (G_i = U_i^T U_i, rhs_i = U_i^T (rho - b_old),
colsum_i = U_i^T 1, sum rho, sum rho^2: formed in fp64, then rounded to the array's type) and lays them out the way
als_row_solve writes them: perm space (layout.perm_of_col), lower 16x16 blocks only.  What the contract says a kernel
must not read is NaN: every strictly upper block, and every row outside [item_begin, item_end) of every per-item array.

`expected_h`, `expected_ab`, `expected_stats` evaluate the documented formulas from the arrays actually handed to the
kernel (after rounding), in fp64 or np.longdouble, and return next to every value its absolute-sum companion S: the
same expression with every term replaced by its absolute value.  Rounding-error bounds are stated against S.

Two kinds of input: "exact" (small integers held in floats: every partial sum of every kernel is an integer below
2^24 (fp32) / 2^53 (fp64), so the expected result is exact whatever the summation order and the comparison is for
equality) and "real" (normal factors, binary / row-normalised / three-decade feature columns).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from collaborative_filtering_amd import layout

U32, U64 = 2.0 ** -24, 2.0 ** -53
TILE = 256          # items per tile of k_w_accumulate

# k -> how that k is run (tests/test_gpu_w_step.py).  Between them the rows cover: KB = ld/16 = 1 ... 10; padded k in
# several block counts; nchunks 1, 2, 3; chunks of exactly 256, exactly 257 and more than 512 items; an empty last
# chunk; a tile without / with only contributors; contributor counts of every class mod 4; a column whose only
# non-zero is the shard's last item; disjoint column supports; d = 1, 3, 20; feat_col0 > 0 and feat_index >= 1;
# 0 < item_begin < item_end < n; nfeat 1, 2, 3, 8 (tests/test_w_step_ref_cpu.py asserts this coverage).
# dims: columns per feature; feat: the feature phase 1 runs on; kinds: support pattern of its columns (build_x).
CASES = {
    1: dict(n=300, ib=7, ie=263, nchunks=1, dims=[1], feat=0, kinds=["full_empty"]),                 # one chunk of 256
    8: dict(n=700, ib=0, ie=700, nchunks=1, dims=[2, 3], feat=1, kinds=["full_empty", "even", "odd"]),    # 3 tiles
    16: dict(n=700, ib=3, ie=697, nchunks=2, dims=[20], feat=0, kinds=["full_empty", "even", "odd", "last"] + ["rand"] * 16),
    24: dict(n=520, ib=4, ie=518, nchunks=2, dims=[2, 2], feat=1, kinds=["full_empty", "last"]),    # KB = 2; 257 + 257
    40: dict(n=560, ib=20, ie=534, nchunks=2, dims=[1, 1, 1, 1, 1, 1, 3, 1], feat=6, kinds=["full_empty", "rand", "last"]),   # 257 + 257
    50: dict(n=800, ib=11, ie=782, nchunks=3, dims=[3, 1, 3], feat=2, kinds=["full_empty", "even", "last"]),  # 257 x 3
    64: dict(n=700, ib=5, ie=690, nchunks=2, dims=[3, 2], feat=0, kinds=["full_empty", "even", "odd"]),
    72: dict(n=700, ib=0, ie=650, nchunks=1, dims=[1, 3], feat=1, kinds=["dense", "rand", "last"]),
    96: dict(n=700, ib=33, ie=700, nchunks=3, dims=[2, 1], feat=1, kinds=["full_empty"]),
    100: dict(n=700, ib=1, ie=699, nchunks=2, dims=[3], feat=0, kinds=["full_empty", "odd", "even"]),
    128: dict(n=700, ib=64, ie=640, nchunks=1, dims=[1, 2, 3], feat=2, kinds=["full_empty", "even", "odd"]),   # 576: 3 tiles
    144: dict(n=530, ib=9, ie=523, nchunks=2, dims=[3, 3], feat=1, kinds=["rand", "full_empty", "last"]),
    150: dict(n=540, ib=2, ie=530, nchunks=2, dims=[1, 3], feat=1, kinds=["full_empty", "even", "odd"]),
    160: dict(n=530, ib=6, ie=520, nchunks=2, dims=[3, 1], feat=0, kinds=["full_empty", "odd", "last"]),
}
EXTRA_CASES = {
    # a shard shorter than nchunks * per: the last chunk is empty
    "short": dict(k=40, n=12, ib=2, ie=6, nchunks=3, dims=[3], feat=0, kinds=["dense", "even", "last"]),
    # the wrapper's own chunking (HipBackend.w_accumulate: 19 chunks of 258 items)
    "wrapper": dict(k=16, n=4900, ib=0, ie=4900, nchunks=19, dims=[20], feat=0,
                    kinds=["full_empty", "even", "odd", "last"] + ["rand"] * 16),
}


def chunk_tiles(ib, ie, nchunks):
    """[(chunk, tile_begin, tile_end)] in the order k_w_accumulate walks items [ib, ie)."""
    per = -(-(ie - ib) // nchunks)
    out = []
    for c in range(nchunks):
        cb, ce = ib + c * per, min(ie, ib + (c + 1) * per)
        out += [(c, t, min(ce, t + TILE)) for t in range(cb, ce, TILE)]
    return out


def tile_counts(X, ib, ie, nchunks, col0, d):
    """Contributing items (x_ia x_ia' != 0 in fp32, the kernel's test) of every (pair, tile): {(a, a2, tile_begin): count}."""
    out = {}
    for a in range(d):
        for a2 in range(a, d):
            w = X[:, col0 + a] * X[:, col0 + a2]
            for _, t0, t1 in chunk_tiles(ib, ie, nchunks):
                out[(a, a2, t0)] = int(np.count_nonzero(w[t0:t1]))
    return out


def build_x(rng, *, n, ib, ie, nchunks, dims, feat, kinds, kind):
    """Feature matrix X [n, D] float32.  exact: values 1 / 2; real: feature blocks cycle through binary, row-l2-normalised
    (non-dyadic) and row-l2-normalised with the last column replaced by one spanning three decades; the feature under
    test is never the binary one.  Zeros are structured: the other features are half empty, column c of the feature
    under test follows kinds[c]:
      full_empty  every item of the first tile, no item of the second, half of the rest
      even / odd  items of that parity (relative to item_begin) only: an even and an odd column never meet
      last        the shard's last item only
      rand        30 % of the items;  dense: all of them
    Rows outside the shard are NaN."""
    off = np.concatenate([[0], np.cumsum(dims)]).astype(np.int32)
    D = int(off[-1])
    if kind == "exact":
        val = rng.integers(1, 3, size=(n, D)).astype(np.float64)
    else:
        val = np.empty((n, D))
        for f, d in enumerate(dims):
            blk = rng.normal(size=(n, d))
            if f % 3 == 0 and f != feat:
                blk = np.ones((n, d))                                           # binary once masked
            else:
                blk /= np.linalg.norm(blk, axis=1, keepdims=True)
                if d == 1 or d >= 3:
                    blk[:, -1] = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-1.5, 1.5, size=n)
            val[:, off[f]:off[f + 1]] = blk
    mask = rng.random((n, D)) < 0.5
    j = np.arange(n) - ib
    tiles = chunk_tiles(ib, ie, nchunks)
    for c, kd in enumerate(kinds):
        col = off[feat] + c
        if kd == "full_empty":
            m = rng.random(n) < 0.5
            m[tiles[0][1]:tiles[0][2]] = True
            if len(tiles) > 1:
                m[tiles[1][1]:tiles[1][2]] = False
        elif kd in ("even", "odd"):
            m = (j % 2 == (kd == "odd")) & (rng.random(n) < 0.7)
        elif kd == "last":
            m = np.arange(n) == ie - 1
        elif kd == "rand":
            m = rng.random(n) < 0.3
        else:
            assert kd == "dense", kd
            m = np.ones(n, dtype=bool)
        mask[:, col] = m
    X = (val * mask).astype(np.float32)
    X[:ib] = np.nan
    X[ie:] = np.nan
    return X, off


def build_inputs(*, k, n, ib, ie, dims, feat, kinds, kind, f64, seed, nchunks=1, twin_scale=1.0):
    """Consistent inputs of all three entry points for n items, shard [ib, ie).  f64: gram / rhs / colsum / sumr / sumr2
    are doubles and W is [D, k] double; otherwise they are float32 and W is [D, ld] float32.  twin_scale: factor on
    the strictly upper triangle of every diagonal 16x16 block of the Gram (1.0: the transpose of the lower)."""
    assert kind in ("exact", "real") and 0 <= ib <= ie <= n
    rng = np.random.default_rng(seed)
    ld = layout.padded_k(k)
    pos = layout.perm_of_col(k)[:k]
    dt = np.float64 if f64 else np.float32
    f32 = np.float32
    X, off = build_x(rng, n=n, ib=ib, ie=ie, nchunks=nchunks, dims=dims, feat=feat, kinds=kinds, kind=kind)
    D = X.shape[1]
    if kind == "exact":
        assert D <= 24
        ni = rng.choice([0, 1, 2, 3, 6], size=n, p=[0.1, 0.2, 0.3, 0.2, 0.2])
        classes = [0, 1, 2, 6]
    else:
        classes = [0, 1, max(k // 2, 1), k + 3]                                 # none, one, fewer than k, more than k
        ni = rng.choice(classes + [2], size=n, p=[0.1, 0.2, 0.3, 0.1, 0.3])
    ni[ib:ib + len(classes)] = classes[: max(0, min(len(classes), ie - ib))]
    nmax = int(ni.max()) if n else 0
    users = np.arange(nmax)[None, :] < ni[:, None]                              # [n, nmax]
    if kind == "exact":
        U = rng.integers(-2, 3, size=(n, nmax, k)).astype(np.float64)
        rho = rng.integers(-3, 4, size=(n, nmax)).astype(np.float64)
        V = rng.integers(-2, 3, size=(n, k)).astype(np.float64)
        W = rng.integers(-1, 2, size=(D, k)).astype(np.float64)
        b_old = rng.integers(-2, 3, size=n).astype(np.float64)
        b_new = b_old + rng.integers(-1, 2, size=n)
    else:
        U = rng.normal(scale=0.3, size=(n, nmax, k))
        rho = rng.normal(size=(n, nmax))
        V = rng.normal(scale=0.3, size=(n, k))
        W = rng.normal(scale=0.3, size=(D, k))
        b_old = rng.normal(scale=0.3, size=n)
        b_new = b_old + rng.normal(scale=0.1, size=n)
    U *= users[:, :, None]
    rho *= users
    b_old, b_new = b_old.astype(f32), b_new.astype(f32)
    G = np.matmul(U.transpose(0, 2, 1), U)                                      # [n, k, k] fp64
    rhs = np.einsum("iuk,iu->ik", U, (rho - b_old.astype(np.float64)[:, None]) * users)
    colsum = U.sum(axis=1)
    sumr, sumr2 = rho.sum(axis=1), (rho * rho).sum(axis=1)

    blk = np.arange(ld) // 16
    r, c = np.arange(ld)[:, None], np.arange(ld)[None, :]
    gram = np.zeros((n, ld, ld), dtype=dt)
    gram[:, pos[:, None], pos[None, :]] = G.astype(dt)
    gram[:, (blk[:, None] == blk[None, :]) & (r < c)] *= dt(twin_scale)
    gram[:, blk[:, None] < blk[None, :]] = np.nan

    def perm_rows(a):
        out = np.zeros((n, ld), dtype=dt)
        out[:, pos] = a.astype(dt)
        return out

    def storage_rows(a, rows):
        out = np.zeros((rows, ld), dtype=f32)
        out[:, :k] = a.astype(f32)
        return out

    Vs = storage_rows(V, n)
    Wk = W.astype(dt)                                                            # what the kernel reads, [D, k]
    Xs = np.nan_to_num(X.astype(np.float64))
    Z = storage_rows(Vs[:, :k].astype(np.float64) + Xs @ Wk.astype(np.float64), n)
    inp = SimpleNamespace(
        k=k, ld=ld, n=n, ib=ib, ie=ie, nchunks=nchunks, dims=list(dims), feat=feat, kind=kind, f64=bool(f64), pos=pos,
        D=D, nfeat=len(dims), feat_off=off, X=X, gram=gram, rhs=perm_rows(rhs), colsum=perm_rows(colsum), V=Vs, Z=Z,
        b_new=b_new.copy(), b_old=b_old.copy(), sumr=sumr.astype(dt), sumr2=sumr2.astype(dt),
        W=Wk.copy() if f64 else storage_rows(W, D), ni=ni,
        indptr=np.concatenate([[0], np.cumsum(ni)]).astype(np.int64),
        users_U=U, users_rho=rho, users_mask=users)                             # the synthetic ratings themselves
    out = np.ones(n, dtype=bool)
    out[ib:ie] = False
    for a in (inp.gram, inp.rhs, inp.colsum, inp.V, inp.Z, inp.b_new, inp.b_old, inp.sumr, inp.sumr2):
        a[out] = np.nan
    if kind == "exact":
        check_exact_magnitudes(inp)
    return inp


def check_exact_magnitudes(inp):
    """The exact kind's promise: integers everywhere, every fp32 partial sum of phase 0 and of the statistics' G z
    below 2^24, every fp64 sum of phase 1 and of the statistics below 2^53."""
    sl = slice(inp.ib, inp.ie)
    m = inp.ie - inp.ib
    if m == 0:
        return
    k = inp.k
    arrays = dict(G=gram_storage(inp), rhs=inp.rhs[sl], colsum=inp.colsum[sl], V=inp.V[sl], Z=inp.Z[sl], X=inp.X[sl],
                  W=inp.W, b_new=inp.b_new[sl], b_old=inp.b_old[sl], sumr=inp.sumr[sl], sumr2=inp.sumr2[sl])
    mx = {}
    for name, a in arrays.items():
        a = np.asarray(a, dtype=np.float64)
        assert np.array_equal(a, np.rint(a)), name
        mx[name] = float(np.max(np.abs(a))) if a.size else 0.0
    db = float(np.max(np.abs(inp.b_new[sl].astype(np.float64) - inp.b_old[sl].astype(np.float64))))
    zmax = mx["V"] + inp.D * mx["X"] * mx["W"]                                  # |z| and, a fortiori, every |xw_f|
    assert mx["G"] <= 24 and mx["X"] <= 2 and db <= 1 and zmax <= 50 and mx["Z"] <= zmax
    gz = k * mx["G"] * zmax                                                      # <= 160 * 24 * 50
    h = mx["rhs"] + db * mx["colsum"] + 2 * gz
    assert h < 2 ** 24, h
    assert m * mx["X"] ** 2 * mx["G"] < 2 ** 53 and m * mx["X"] * h < 2 ** 53
    nmax = float(inp.ni.max())
    s2 = mx["sumr2"] + 2 * mx["b_new"] * mx["sumr"] + nmax * mx["b_new"] ** 2 \
        + 2 * k * zmax * (mx["rhs"] + db * mx["colsum"]) + k * zmax * gz
    assert s2 < 2 ** 53, s2


def gram_storage(inp):
    """Item Grams of the shard in storage column order, fp64 [ie - ib, k, k], decoded from the perm-space image the
    way the contract allows: lower blocks only, and inside a diagonal block the lower-triangle twin only."""
    Gp = inp.gram[inp.ib:inp.ie]
    r, c = np.arange(inp.ld)[:, None], np.arange(inp.ld)[None, :]
    sym = np.where(r >= c, Gp, Gp.transpose(0, 2, 1))
    return sym[:, inp.pos[:, None], inp.pos[None, :]].astype(np.float64)


def _matvecs(G, vecs, T):
    """G [m, k, k] float64 times vecs [m, k, nv] in type T, a few items at a time (T may be np.longdouble)."""
    out = np.empty(vecs.shape, dtype=T)
    step = 16 if T is not np.float64 else 4096
    for s in range(0, G.shape[0], step):
        out[s:s + step] = np.matmul(G[s:s + step].astype(T), vecs[s:s + step])
    return out


def expected_h(inp, wide=False):
    """Phase 0: h_{f,i} = rhs - (b_new - b_old) colsum - G z + G xw_f, z = V + sum_f xw_f (all features: the old W).
    Returns (H, S) of shape [nfeat, n, ld], perm space, padded positions 0, rows outside the shard NaN."""
    T = np.longdouble if wide else np.float64
    sl, k, pos = slice(inp.ib, inp.ie), inp.k, inp.pos
    m = inp.ie - inp.ib
    G = gram_storage(inp)
    X, W, V = inp.X[sl].astype(T), inp.W[:, :k].astype(T), inp.V[sl, :k].astype(T)
    rhs, colsum = inp.rhs[sl][:, pos].astype(T), inp.colsum[sl][:, pos].astype(T)
    db = (inp.b_new[sl].astype(T) - inp.b_old[sl].astype(T))[:, None]
    off = inp.feat_off
    xw = [X[:, off[f]:off[f + 1]] @ W[off[f]:off[f + 1]] for f in range(inp.nfeat)]
    axw = [np.abs(X[:, off[f]:off[f + 1]]) @ np.abs(W[off[f]:off[f + 1]]) for f in range(inp.nfeat)]
    z, az = V + sum(xw), np.abs(V) + sum(axw)
    prod = _matvecs(G, np.stack([z] + xw, axis=2), T)                           # G z, G xw_0, ...
    aprod = _matvecs(np.abs(G), np.stack([az] + axw, axis=2), T)
    H = np.full((inp.nfeat, inp.n, inp.ld), np.nan, dtype=T)
    S = np.full((inp.nfeat, inp.n, inp.ld), np.nan, dtype=T)
    H[:, sl], S[:, sl] = 0, 0
    for f in range(inp.nfeat):
        H[f, sl.start:sl.stop, pos] = (rhs - db * colsum - prod[:, :, 0] + prod[:, :, f + 1]).T
        S[f, sl.start:sl.stop, pos] = (np.abs(rhs) + np.abs(db * colsum) + aprod[:, :, 0] + aprod[:, :, f + 1]).T
    assert m == 0 or np.isfinite(H[:, sl]).all()
    return H, S


def expected_ab(inp, H_f, wide=False):
    """Phase 1 for feature inp.feat: A = sum_i (x_i x_i^T) (x) G_i, B = sum_i x_i (x) h_{f,i}, index a k + c (storage
    order), over the shard.  H_f [n, ld]: the h vectors phase 1 is given (what phase 0 wrote).  Returns (A, S_A, B, S_B)."""
    T = np.longdouble if wide else np.float64
    sl, k = slice(inp.ib, inp.ie), inp.k
    m = inp.ie - inp.ib
    d, c0 = inp.dims[inp.feat], int(inp.feat_off[inp.feat])
    G = gram_storage(inp).reshape(m, k * k)
    X = inp.X[sl, c0:c0 + d].astype(np.float64)
    P = (X[:, :, None] * X[:, None, :]).reshape(m, d * d)                       # exact: 24-bit factors

    def kron(p, g):
        return (p.T @ g).reshape(d, d, k, k).transpose(0, 2, 1, 3).reshape(d * k, d * k)

    A, SA = kron(P.astype(T), G.astype(T)), kron(np.abs(P), np.abs(G))
    Hs = np.asarray(H_f)[sl][:, inp.pos]
    B = (X.astype(T).T @ Hs.astype(T)).reshape(d * k)
    SB = (np.abs(X).T @ np.abs(Hs.astype(np.float64))).reshape(d * k)
    return A, SA, B, SB


def expected_stats(inp, wide=False):
    """Closed-form residual sums with z = inp.Z, as the kernels evaluate them from the by-products (rhs holds
    U^T (rho - b_old)):  sum d = sum rho - n b_new - z . (U^T 1);
    sum d^2 = (sum rho^2 - 2 b_new sum rho + n b_new^2) - 2 z . (rhs + (b_old - b_new) colsum) + z^T G z.
    Returns (stat, S) [n, 2], rows outside the shard NaN."""
    T = np.longdouble if wide else np.float64
    sl, k, pos = slice(inp.ib, inp.ie), inp.k, inp.pos
    G = gram_storage(inp)
    z = inp.Z[sl, :k].astype(T)
    rhs, colsum = inp.rhs[sl][:, pos].astype(T), inp.colsum[sl][:, pos].astype(T)
    b, bo = inp.b_new[sl].astype(T), inp.b_old[sl].astype(T)
    sr, sr2 = inp.sumr[sl].astype(T), inp.sumr2[sl].astype(T)
    cnt = np.diff(inp.indptr)[sl].astype(T)
    gz = _matvecs(G, z[:, :, None], T)[:, :, 0]
    agz = _matvecs(np.abs(G), np.abs(z)[:, :, None], T)[:, :, 0]
    zc, zr, zgz = (z * colsum).sum(1), (z * rhs).sum(1), (z * gz).sum(1)
    azc, azr, azgz = np.abs(z * colsum).sum(1), np.abs(z * rhs).sum(1), (np.abs(z) * agz).sum(1)
    stat = np.full((inp.n, 2), np.nan, dtype=T)
    S = np.full((inp.n, 2), np.nan, dtype=T)
    stat[sl, 0] = sr - cnt * b - zc
    S[sl, 0] = np.abs(sr) + cnt * np.abs(b) + azc
    stat[sl, 1] = (sr2 - 2 * b * sr + cnt * b * b) - 2 * (zr + (bo - b) * zc) + zgz
    S[sl, 1] = (sr2 + 2 * np.abs(b * sr) + cnt * b * b) + 2 * (azr + np.abs(bo - b) * azc) + azgz
    return stat, S
