"""numpy-only fixture and ISOLATED fp64 reference for the Gauss-Seidel Laplacian sweep (csrc/gs_sweep.hip: k_gs_level,
k_gs_level_f64, k_gs_dataflow in both forms, k_gs_nondep), shared by tests/test_gs_sweep_ref_cpu.py (which drives the
numpy stand-in, tests/cpu_backend.py, and wrong sweeps built on it) and tests/test_gpu_gs_sweep.py.

The sweep is the one stage whose correctness rests on ORDER: item i must see the rows of swept neighbours j < i as
solved in this sweep and every other neighbour's row as it was before.  `expected` therefore judges every item on its
own: from the raw ratings, the rows of the sweep's own output for the swept neighbours below it and the old rows for all
others, it computes in fp64 what that item should have produced.  An error does not travel down a chain, so the bound of
an item is the rounding of one solve; a row taken stale or too fresh is a jump of at least 20 bounds (`discrimination`).

Schedules and wait lists come from layout.build_level_schedule / layout.wait_edges only: a wait on a row that nobody
publishes would spin to the dataflow kernel's time limit, and no test goes there.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass

import numpy as np

from collaborative_filtering_amd import layout
from tests.gpu_common import record_margins

N_ITEMS, N_USERS = 192, 400
MU, ALPHA, LAMBDA_B, EPS = 3.1, 0.7, 2.2, 1e-10
# padded widths 16, 16, 32, 48, 64, 80, ... 160: every KB = ld / 16 from 1 to 10 (24 is there for KB = 2), a padded
# width in every rows-per-lane class (ld <= 64, <= 128, <= 160), WPW 4 / 2 / 1 of the level kernel
K_LIST = (5, 16, 24, 40, 64, 72, 96, 112, 128, 144, 150, 160)
SEED = 20

INACTIVE = (17, 90, 170, 191)       # no ratings: never swept, but neighbours of swept items on both sides
ISOLATED = 60                       # swept, no neighbour at all
CHAIN = (100, 146)                  # ids 100 - 101 - ... - 145 linked consecutively: at least 45 levels
HUB_LOW, HUB_HIGH = 0, 188          # >= 129 neighbours: none / at least 100 of them wait edges
DEG64, DEG65 = 150, 155             # exactly 64 / 65 neighbours (the kernels chunk neighbour lists by 64)

# The project's own numbers for the fp32 sweep kernels on row-solve by-products (test_factor_mode_and_gs_level), and
# the storage rounding of the fp64 level kernel (8 fp32 ulps of the row's largest element).  `stat1`, `stat2`:
# |stat - direct| <= c * B for sum d and sum d^2, B the absolute sum of the closed form's terms (`stat_bounds`); c is
# 10x the worst ratio observed on the MI355X, capped at the row-solve statistics test's 1e-5 (fp32) and at 1e-6 (fp64).
#   observed worst error / bound (V, bias) and error / B (statistics) over K_LIST (per k:
#   profiles/gs_sweep_kernel_test_margins.json, written by the GPU tests under ALS_RECORD_MARGINS=<file>):
#     level fp32        V 0.032   bias 0.0096   sum d 9.0e-6 B   sum d^2 1.3e-7 B   (statistics: ld <= 64 only)
#     level f64         V 0.076   bias 0.034    sum d 2.2e-7 B   sum d^2 3.7e-8 B
#     dataflow image    V 0.032   bias 0.011    sum d 9.0e-6 B   sum d^2 1.3e-7 B
#     dataflow stream   V 0.040   bias 0.011    sum d 5.6e-6 B   sum d^2 1.1e-7 B
# sum d of the fp32 paths sits at its cap: B1 holds |sum (r - mu - b_u)|, which knows nothing of the cancellation
# INSIDE that sum - the row solve forms each term in fp32 at the size of the rating (half an ulp of 5 = 2.4e-7 per
# rating, 34 ratings whose sum is 0.17: item 23 at k = 5, B1 = 0.36).  It is the by-product's rounding, not the sweep's.
TOL_FP32 = dict(v=1e-4, v_floor=1e-6, bias=2e-5, stat1=1e-5, stat2=1.5e-6)   # the cap (1.1x observed); ~10x observed
TOL_F64 = dict(v=1e-6, v_floor=0.0, bias=1e-6, stat1=1e-6, stat2=4e-7)       # the cap (~5x observed); ~10x observed


@dataclass
class Case:
    k: int
    ld: int
    n: int
    m: int
    indptr: np.ndarray        # ratings by item (CSC of the rating matrix): int64 [n + 1]
    indices: np.ndarray       # int32 user ids, ascending inside an item
    vals: np.ndarray          # float32, half-star grid
    U: np.ndarray             # float32 [m, k]
    V_old: np.ndarray         # float32 [n, k]
    b_u: np.ndarray           # float32 [m]
    b_i: np.ndarray           # float32 [n]: the item biases on entry (= the bias_self of the by-products)
    lam_row: np.ndarray       # float32 [n]
    S_ptr: np.ndarray
    S_idx: np.ndarray
    S_val: np.ndarray         # float32
    D: np.ndarray             # float64 row sums of S
    diag_extra: np.ndarray    # float32 alpha * D
    lambda_eff: np.ndarray    # float32, as engine.py forms it
    active: np.ndarray        # bool [n]
    sched: layout.LevelSchedule
    wait: np.ndarray          # layout.wait_edges
    mu: float = MU
    alpha: float = ALPHA
    lam_b: float = LAMBDA_B

    @property
    def swept(self):
        return self.sched.level >= 0

    def V_pad(self):
        out = np.zeros((self.n, self.ld), np.float32)
        out[:, : self.k] = self.V_old
        return out

    def with_v_old(self, V_old):
        return dataclasses.replace(self, V_old=np.ascontiguousarray(V_old, dtype=np.float32))


# ------------------------------------------------------------------------------------------------------ fixture
def _graph(rng):
    n = N_ITEMS
    W = np.zeros((n, n), np.float32)

    def link(i, j):
        if i != j and ISOLATED not in (i, j) and W[i, j] == 0:
            W[i, j] = W[j, i] = np.float32(rng.uniform(0.05, 1.0))

    for i in range(n):                                   # background of degree about 6
        for j in rng.choice(n, size=3, replace=False):
            if {i, int(j)} & {DEG64, DEG65, HUB_LOW, HUB_HIGH}:
                continue
            link(i, int(j))
    for i in range(CHAIN[0], CHAIN[1] - 1):
        link(i, i + 1)
    others = np.array([j for j in range(1, n) if j not in (DEG64, DEG65, HUB_HIGH)])
    for j in rng.choice(others, size=135, replace=False):
        link(HUB_LOW, int(j))
    below = np.array([j for j in range(1, HUB_HIGH) if j not in (DEG64, DEG65)])
    for j in rng.choice(below, size=150, replace=False):
        link(HUB_HIGH, int(j))
    for q in INACTIVE:                                   # inactive neighbours below and above swept items
        link(q, HUB_HIGH) if q < HUB_HIGH else link(q, HUB_HIGH - 1)
        link(q, max(q - 9, 1))
        link(q, HUB_LOW)
    link(HUB_HIGH, HUB_HIGH + 1)
    link(HUB_HIGH, HUB_HIGH + 2)
    # the exact-degree rows last, so that no later link changes them
    for item, deg, avoid in ((DEG64, 64, DEG65), (DEG65, 65, DEG64)):
        free = [j for j in range(n) if j not in (item, avoid, ISOLATED) and W[item, j] == 0]
        need = deg - int(np.count_nonzero(W[item]))
        assert 0 <= need <= len(free)
        for j in rng.choice(free, size=need, replace=False):
            link(item, int(j))
    assert np.array_equal(W, W.T) and not np.diag(W).any()
    assert ((W == 0) | ((W >= np.float32(0.05)) & (W < 1))).all()
    ptr, idx, val = layout.dense_graph_to_csr(W)
    return ptr, idx, val.astype(np.float32)


def chunk_profile(case):
    """Per 64-wide chunk of every swept row's neighbour list: (item, chunk number, wait flags of the chunk)."""
    out = []
    for i in np.nonzero(case.swept)[0]:
        w = case.wait[case.S_ptr[i]: case.S_ptr[i + 1]] < 0
        out += [(int(i), c // 64, w[c: c + 64]) for c in range(0, w.size, 64)]
    return out


def assert_fixture(case):
    """The conditions the tests of the sweep rest on (make_case asserts them itself)."""
    n, ptr, idx = case.n, case.S_ptr, case.S_idx
    deg = np.diff(ptr)
    lev, swept, active = case.sched.level, case.swept, case.active
    assert n == N_ITEMS and case.m == N_USERS
    nnz = np.diff(case.indptr)
    assert np.count_nonzero(nnz == 0) >= 3 and nnz.max() <= 40 and np.array_equal(active, nnz > 0)
    assert np.array_equal(swept, active)
    nwait = np.array([np.count_nonzero(case.wait[ptr[i]: ptr[i + 1]] < 0) for i in range(n)])
    assert deg[DEG64] == 64 and deg[DEG65] == 65 and swept[DEG64] and swept[DEG65]
    assert HUB_HIGH >= n - 8 and deg[HUB_HIGH] >= 129 and nwait[HUB_HIGH] >= 100
    assert deg[HUB_LOW] >= 129 and nwait[HUB_LOW] == 0 and swept[HUB_LOW]
    assert deg[ISOLATED] == 0 and swept[ISOLATED]
    chunks = chunk_profile(case)
    first = {(i, c): int(w.sum()) for i, c, w in chunks}
    assert any(nw > 16 and any(first.get((i, c2), 0) >= 1 for c2 in range(c + 1, 4)) for (i, c), nw in first.items())

    def interleaved(w):             # wait, non-wait, wait
        p = np.nonzero(w)[0]
        return p.size >= 2 and not w[p[0]: p[-1] + 1].all()
    assert any(interleaved(w) for _, _, w in chunks)
    rows = np.repeat(np.arange(n), deg)
    inact_nb = ~active[idx] & swept[rows]
    assert (inact_nb & (idx < rows)).any() and (inact_nb & (idx > rows)).any()
    assert all(ptr[i] < ptr[i + 1] and (i + 1) in idx[ptr[i]: ptr[i + 1]] for i in range(CHAIN[0], CHAIN[1] - 1))
    assert CHAIN[1] - CHAIN[0] >= 41 and swept[CHAIN[0]: CHAIN[1]].all()
    sizes = np.diff(case.sched.offsets)
    assert sizes.size >= 40 and (sizes == 1).any()
    assert ((sizes > 4) & (sizes % 4 != 0)).any() and ((sizes > 2) & (sizes % 2 == 1)).any()
    assert np.array_equal(case.V_pad()[:, case.k:], np.zeros((n, case.ld - case.k), np.float32))


def make_case(k, seed=SEED):
    """A small deterministic case: 192 items, 400 users.  The graph, the ratings' pattern and the schedule depend on
    `seed` alone; the factors and biases on (seed, k)."""
    rng = np.random.default_rng(seed)
    n, m = N_ITEMS, N_USERS
    S_ptr, S_idx, S_val = _graph(rng)
    lens = rng.integers(1, 41, size=n)
    lens[list(INACTIVE)] = 0
    lens[HUB_LOW], lens[DEG64], lens[ISOLATED] = 40, 1, 2
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(lens)
    indices = np.concatenate([np.sort(rng.choice(m, size=l, replace=False)) for l in lens]).astype(np.int32)
    vals = (rng.integers(1, 11, size=indices.size) * 0.5).astype(np.float32)
    rng = np.random.default_rng([seed, k])
    U = rng.normal(scale=0.3, size=(m, k)).astype(np.float32)
    V_old = rng.normal(size=(n, k)).astype(np.float32)
    b_u = rng.normal(scale=0.2, size=m).astype(np.float32)
    b_i = rng.normal(scale=0.2, size=n).astype(np.float32)
    lam_row = rng.uniform(0.5, 4.0, size=n).astype(np.float32)
    D = np.array([S_val[S_ptr[i]: S_ptr[i + 1]].astype(np.float64).sum() for i in range(n)])
    diag_extra = (ALPHA * D).astype(np.float32)
    lambda_eff = (lam_row + np.float32(EPS) + diag_extra).astype(np.float32)
    active = lens > 0
    sched = layout.build_level_schedule(S_ptr, S_idx, active)
    wait = layout.wait_edges(S_ptr, S_idx, sched.level)
    case = Case(k=k, ld=layout.padded_k(k), n=n, m=m, indptr=indptr, indices=indices, vals=vals, U=U, V_old=V_old,
                b_u=b_u, b_i=b_i, lam_row=lam_row, S_ptr=S_ptr, S_idx=S_idx, S_val=S_val, D=D, diag_extra=diag_extra,
                lambda_eff=lambda_eff, active=active, sched=sched, wait=wait)
    assert_fixture(case)
    return case


# ------------------------------------------------------------------------------------------------------ reference
def _item(case, i):
    """(U_r, base = r - mu - b_u, A) of item i in fp64 from the raw ratings."""
    lo, hi = case.indptr[i], case.indptr[i + 1]
    Ur = case.U[case.indices[lo:hi]].astype(np.float64)
    base = case.vals[lo:hi].astype(np.float64) - case.mu - case.b_u[case.indices[lo:hi]].astype(np.float64)
    lam = float(case.lam_row[i]) + EPS + float(case.diag_extra[i])
    return Ur, base, Ur.T @ Ur + lam * np.eye(case.k)


def _solve_item(case, i, Vsrc):
    """x_i, bias_i and the closed form's terms of item i given the neighbour rows `Vsrc` ([n, >= k], any float type)."""
    Ur, base, A = _item(case, i)
    sl = slice(case.S_ptr[i], case.S_ptr[i + 1])
    g = case.S_val[sl].astype(np.float64) @ Vsrc[case.S_idx[sl], : case.k].astype(np.float64)
    rhs = Ur.T @ (base - float(case.b_i[i]))
    b = rhs + case.alpha * g
    x = np.linalg.solve(A, b)
    cs = Ur.sum(axis=0)
    nnz = base.size
    bias = (base.sum() - cs @ x) / (nnz + case.lam_b + EPS)
    return x, bias, dict(sumr=base.sum(), sumr2=(base * base).sum(), nnz=nnz, csx=cs @ x, rhsx=rhs @ x, yy=b @ x,
                         lxx=float(case.lambda_eff[i]) * (x @ x), db=float(case.b_i[i]) - bias)


def expected(case, V_out):
    """The isolated reference: for every swept item what it should have computed from the rows it was given - the
    rows of `V_out` (the sweep's own fp32 output) for swept neighbours j < i, the rows of V_old for every other j.
    -> (x [n, k], bias [n], B1 [n], B2 [n]) in fp64; rows of unswept items are NaN.  B1, B2: `stat_bounds`."""
    n, k = case.n, case.k
    X, bias = np.full((n, k), np.nan), np.full(n, np.nan)
    B1, B2 = np.full(n, np.nan), np.full(n, np.nan)
    swept = case.swept
    for i in np.nonzero(swept)[0]:
        Vsrc = case.V_old.astype(np.float64)
        below = np.nonzero(swept[:i])[0]
        Vsrc[below] = V_out[below, :k]
        X[i], bias[i], t = _solve_item(case, i, Vsrc)
        B1[i], B2[i] = stat_bounds(t, bias[i])
    return X, bias, B1, B2


def stat_bounds(t, b):
    """Absolute sums of the terms of the closed form the kernels evaluate (csrc/gs_sweep.hip, "closed-form residual
    sums"): the statistics are differences of these, so their rounding error scales with them."""
    B1 = abs(t["sumr"]) + t["nnz"] * abs(b) + abs(t["csx"])
    B2 = (t["sumr2"] + 2 * abs(b * t["sumr"]) + t["nnz"] * b * b + 2 * abs(t["rhsx"]) + 2 * abs(t["db"] * t["csx"])
          + t["yy"] + t["lxx"])
    return B1, B2


def direct_stats(case, V_out, bias_out):
    """sum d and sum d^2 of d = r - mu - b_u - U_r x - b over the ratings of every swept item, x and b being the rows
    of V_out / bias_out: evaluated directly in fp64 -> [n, 2] (NaN for unswept items)."""
    out = np.full((case.n, 2), np.nan)
    for i in np.nonzero(case.swept)[0]:
        Ur, base, _ = _item(case, i)
        d = base - Ur @ V_out[i, : case.k].astype(np.float64) - float(bias_out[i])
        out[i] = d.sum(), (d * d).sum()
    return out


def reference_sweep(case):
    """The whole sweep in fp64 and index order (what the reference item loop does): V_new [n, k], bias [n]."""
    V = case.V_old.astype(np.float64)
    bias = case.b_i.astype(np.float64)
    for i in np.nonzero(case.swept)[0]:
        V[i], bias[i], _ = _solve_item(case, i, V)
    return V, bias


def v_tolerance(x, tol):
    return tol["v"] * np.maximum(np.max(np.abs(x), axis=-1), tol["v_floor"])


def check(case, V_out, bias_out, stat_out, tol, key=None):
    """The assertions shared by the CPU and the GPU tests on one sweep's outputs (V_out [n, ld] fp32, bias_out [n]
    fp32, stat_out [n, 2] fp32 or None); -> the worst error / bound ratios, also handed to record_margins(key)."""
    n, k, swept = case.n, case.k, case.swept
    V_out, bias_out = np.asarray(V_out), np.asarray(bias_out)
    assert V_out.shape == (n, case.ld) and V_out.dtype == np.float32 and bias_out.dtype == np.float32
    assert V_out[~swept].tobytes() == case.V_pad()[~swept].tobytes(), "unswept: a V row of an unswept item changed"
    assert bias_out[~swept].tobytes() == case.b_i[~swept].tobytes(), "unswept: a bias of an unswept item changed"
    assert not V_out[swept][:, k:].any(), "padding: non-zero padding column in a swept row"
    assert np.isfinite(V_out).all() and np.isfinite(bias_out).all(), "V: not finite"
    X, bias, B1, B2 = expected(case, V_out)
    sw = np.nonzero(swept)[0]
    ev = np.max(np.abs(V_out[sw, :k] - X[sw]), axis=1) / v_tolerance(X[sw], tol)
    eb = np.abs(bias_out[sw] - bias[sw]) / (tol["bias"] * np.maximum(1.0, np.abs(bias[sw])))
    worst = {"v": float(ev.max()), "bias": float(eb.max())}
    if stat_out is not None:
        st = np.asarray(stat_out, dtype=np.float64)
        direct = direct_stats(case, V_out, bias_out)
        assert st.shape == (n, 2) and np.isfinite(st[sw]).all(), "stat: not finite"
        e1 = np.abs(st[sw, 0] - direct[sw, 0]) / B1[sw]
        e2 = np.abs(st[sw, 1] - direct[sw, 1]) / B2[sw]
        worst["stat1"], worst["stat2"] = float(e1.max()), float(e2.max())
    if key:
        record_margins(key, worst)
    assert worst["v"] <= 1.0, f"V: item {sw[ev.argmax()]} (level {case.sched.level[sw[ev.argmax()]]}) off by " \
                              f"{ev.max():.3g} bounds"
    assert worst["bias"] <= 1.0, f"bias: item {sw[eb.argmax()]} off by {eb.max():.3g} bounds"
    if stat_out is not None:
        assert worst["stat1"] <= tol["stat1"], f"stat: sum d of item {sw[e1.argmax()]}: {e1.max():.3g} of B"
        assert worst["stat2"] <= tol["stat2"], f"stat: sum d^2 of item {sw[e2.argmax()]}: {e2.max():.3g} of B"
    return worst


# ------------------------------------------------------------------------------------------------------ discrimination
def discrimination(case, tol=TOL_FP32):
    """How far a wrong dependency moves an item, in V bounds of that item: for every wait edge (i, j) the row of j
    taken as before the sweep instead of as solved, for every edge to a swept j > i the row taken as solved instead of
    as before - |alpha S_ij A_i^-1 (V_new_j - V_old_j)|_inf / bound_i.  -> dict(stale=(min, i, j), fresh=(min, i, j))."""
    Vn, _ = reference_sweep(case)
    dV = Vn - case.V_old.astype(np.float64)
    bound = v_tolerance(Vn, tol)
    out = {"stale": (np.inf, -1, -1), "fresh": (np.inf, -1, -1)}
    for i in np.nonzero(case.swept)[0]:
        sl = slice(case.S_ptr[i], case.S_ptr[i + 1])
        if sl.start == sl.stop:
            continue
        _, _, A = _item(case, i)
        js = case.S_idx[sl]
        jump = np.max(np.abs(np.linalg.solve(A, (case.alpha * case.S_val[sl].astype(np.float64))[None, :] * dV[js].T)),
                      axis=0) / bound[i]
        is_wait = case.wait[sl] < 0
        for name, sel in (("stale", is_wait), ("fresh", ~is_wait & case.swept[js] & (js > i))):
            if sel.any():
                p = np.nonzero(sel)[0][np.argmin(jump[sel])]
                if jump[p] < out[name][0]:
                    out[name] = (float(jump[p]), int(i), int(js[p]))
    return out
