"""GPU: als_row_solve under a power-of-two scaling of its inputs, on every kernel path (reference and scale rule in
tests/row_scale_ref.py, validated without a device by tests/test_row_scale_ref_cpu.py).

The row solve is linear in the ratings, the global mean, the biases and rhs_extra.  At p = 0 every path is held to
the fp64 solution with the tolerances tests/test_gpu_kernels.py states for its mode; at every other p the outputs
must be the p = 0 outputs times 2^p (stat_out[:, 1]: 2^2p) BIT FOR BIT - the fp32 paths use fmas, adds and
power-of-two (un)scalings only - which carries the p = 0 accuracy to every scale without a tolerance.  The one place
that is not scale-free by construction is the fp16 residual pair of the pre-split path: it gets the caller's
power-of-two scale HipBackend.residual_scale(max |vals|), which follows the data.  Observed margins:
profiles/row_scale_margins.json (written under ALS_RECORD_MARGINS=<file>)."""
import functools

import numpy as np
import pytest

from tests import gpu_common as gc
from tests import row_scale_ref as R

pytestmark = pytest.mark.gpu

SENT = 7.0

# Tolerances at p = 0, cited from tests/test_gpu_kernels.py (x relative to max |x| of the row, bias to max(1, |bias|),
# stat (sum d, sum d^2) as (a0, r0, a1, r1, q1): |err0| <= a0 max(1, r0-quantity), |err1| <= a1 max(floor, sum d^2) + q1 sum rho^2):
#   fp32 primal kernels: test_row_solve_against_numpy (x 6e-5, bias 2e-6); statistics: the "primal" rows of
#     test_row_solve_dual_short_rows (2e-4 max(1, sum |d|), 1e-3 max(1, sum d^2));
#   dual classes: test_row_solve_dual_short_rows (x 1e-4, bias 2e-5, the same statistics);
#   fp64: test_row_solve_against_numpy[f64] (x 6e-7, bias 6e-7), statistics of test_row_solve_f64_small_lambda
#     (1e-5 max(1, sum |rho|), 1e-5 max(1e-3, sum d^2) + 1e-9 sum rho^2).
TOL_F32 = dict(x=6e-5, bias=2e-6, s0=2e-4, s0_of="d_abs", s1=1e-3, s1_floor=1.0, s1_rho2=0.0)
TOL_DUAL = dict(TOL_F32, x=1e-4, bias=2e-5)
TOL_F64 = dict(x=6e-7, bias=6e-7, s0=1e-5, s0_of="rho_abs", s1=1e-5, s1_floor=1e-3, s1_rho2=1e-9)
# the TOL of tests/test_gpu_parity.py (no test module imports another one)
PARITY_TOL = dict(hist=2e-6, norms=2e-6, test_rmse=1e-6, f_rtol=1e-4, f_atol=5e-5, bias=5e-6, mu=1e-6, pred=3e-4)

# id -> k, Gram mode, solve_dtype, pre-split operands ("on" / "off"), dual classes, rhs_extra, tolerances
PATHS = {
    "f32-k16": dict(k=16, gram="f32", dtype="float32", planes="off", dual=False, extra=True, tol=TOL_F32),
    "f32-k64": dict(k=64, gram="f32", dtype="float32", planes="off", dual=False, extra=False, tol=TOL_F32),
    "split-k50": dict(k=50, gram="f16x2", dtype="float32", planes="off", dual=False, extra=True, tol=TOL_F32),
    "split-k64": dict(k=64, gram="f16x2", dtype="float32", planes="off", dual=False, extra=False, tol=TOL_F32),
    "split-k128": dict(k=128, gram="f16x2", dtype="float32", planes="off", dual=False, extra=False, tol=TOL_F32),
    "planes-k50": dict(k=50, gram="f16x2", dtype="float32", planes="on", dual=False, extra=True, tol=TOL_F32),
    "planes-k64": dict(k=64, gram="f16x2", dtype="float32", planes="on", dual=False, extra=False, tol=TOL_F32),
    "planes-k128": dict(k=128, gram="f16x2", dtype="float32", planes="on", dual=False, extra=False, tol=TOL_F32),
    "dual-k80": dict(k=80, gram="f16x2", dtype="float32", planes="off", dual=True, extra=False, tol=TOL_DUAL),
    "dual-k128": dict(k=128, gram="f16x2", dtype="float32", planes="off", dual=True, extra=False, tol=TOL_DUAL),
    "f64-k64": dict(k=64, gram="f16x2", dtype="float64", planes="on", dual=False, extra=False, tol=TOL_F64),
    "auto-k64": dict(k=64, gram="f16x2", dtype="auto", planes="on", dual=False, extra=False, tol=TOL_F32),
    "refine-k64": dict(k=64, gram="f16x2", dtype="refine", planes="on", dual=False, extra=False, tol=TOL_F32),
}


def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no ROCm device is visible")
    return torch, torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def _input(k, extra):
    inp = R.make_input(k, extra=extra)
    return inp, R.solve_fp64(inp)


def _backend(cfg, dev):
    from collaborative_filtering_amd.backend import HipBackend
    be = HipBackend(dev, gram=cfg["gram"], solve_dtype=cfg["dtype"])
    on = cfg["planes"] == "on"
    be.planes_max_floats = HipBackend.PLANES_MAX_FLOATS if on else 0
    be.planes_max_floats_k128 = HipBackend.PLANES_MAX_FLOATS_K128 if on else 0        # (k = 128: off by default)
    return be


def _call(be, cfg, inp, p, b_other=None, gram_out=False, F=None):
    """One als_row_solve call on the input times 2^p (b_other / F: replacements, already scaled) -> dict of numpy
    arrays; every output starts from the sentinel and has one guard row."""
    torch, dev = _device()
    from collaborative_filtering_amd import layout
    from collaborative_filtering_amd.als import _side_to_dev, _tasks_to_dev
    k, ld, n = inp.k, inp.ld, inp.nrows
    assert ld == layout.padded_k(k)
    side, mu, bs, bo, ex = R.scaled_inputs(inp.side, inp.mu, inp.b_self, inp.b_other, inp.rhs_extra, p)
    if b_other is not None:
        bo = b_other
    if cfg["dual"]:
        t = layout.build_row_tasks(side.indptr, dual_len=64, mid_len=layout.dual_mid_len(k))
        assert t.ndual == 4 and t.nmid == (1 if k > 96 else 0)            # 1, 2, 33, 64 ratings; 65 above k = 96
    else:
        t = layout.build_row_tasks(side.indptr, dual_len=0)
        assert t.ndual == 0 and t.nmid == 0
    assert t.nslots == 2 and t.long_rows.shape[0] == 1                     # the 4097-rating row is split
    sd = _side_to_dev(layout.SparseSide(n, R.NCOLS, side.indptr, side.indices, side.vals), dev)
    f32 = torch.float32
    full = lambda *shape: torch.full(shape, SENT, dtype=f32, device=dev)                  # noqa: E731
    o = dict(X=full(n + 1, ld), bias=full(n + 1), stat=full(n + 1, 2), status=torch.zeros(1, dtype=torch.int32, device=dev))
    if gram_out:
        o["gram"] = torch.zeros(n, ld, ld, dtype=f32, device=dev)
    ws = torch.empty(t.nslots * be.slot_bytes(k) // 4, dtype=f32, device=dev)
    be.row_solve(k=k, ld=ld, side=sd, F=gc.upload(inp.F if F is None else F, dev), zero_row=R.NCOLS,
                 bias_self=gc.upload(bs, dev), bias_other=gc.upload(bo, dev),
                 mu=torch.tensor([mu], dtype=torch.float64, device=dev), lam=0.0, lam_row=gc.upload(inp.lam_row, dev),
                 lam_b=inp.lam_b, lam_b_row=None, rhs_extra=None if ex is None else gc.upload(ex, dev), diag_extra=None,
                 X_out=o["X"], bias_out=o["bias"], gram_out=o.get("gram"), factor_out=None, rhs_out=None,
                 colsum_out=None, sumr_out=None, status=o["status"], tasks=_tasks_to_dev(t, dev), workspace=ws,
                 stat_out=None if gram_out else o["stat"],
                 residual_scale=be.residual_scale(float(np.abs(side.vals).max())))
    torch.cuda.synchronize()
    res = {name: v.cpu().numpy() for name, v in o.items()}
    res["planes_used"] = len(be._planes) > 0
    if cfg["dtype"] in ("auto", "refine"):
        cnt = int(be._redo_count.item())
        assert 0 <= cnt <= n
        res["redo"] = sorted(be._redo_rows[n].cpu().numpy()[:cnt].tolist())
        assert len(set(res["redo"])) == cnt
    if cfg["dtype"] == "refine":
        cnt = int(be._fallback_count.item())
        res["fallback"] = sorted(be._fallback_rows[n].cpu().numpy()[:cnt].tolist())
        res["steps"] = be._refine_steps.cpu().numpy().copy()
    return res


@functools.lru_cache(maxsize=None)
def _run(path):
    """The path's outputs at every p of R.PS, one backend."""
    cfg = PATHS[path]
    _, dev = _device()
    inp, _ = _input(cfg["k"], cfg["extra"])
    assert R.residual_scale(5.0) == 128.0 and float(inp.side.vals.max()) == 5.0
    be = _backend(cfg, dev)
    return {p: _call(be, cfg, inp, p) for p in R.PS}


def _kernel_class(cfg, res):
    """Which kernel class ran, as the existing tests establish it."""
    planes = cfg["planes"] == "on" and cfg["gram"] == "f16x2" and cfg["dtype"] != "float64"
    assert res["planes_used"] == planes


def _untouched(inp, res):
    n, k = inp.nrows, inp.k
    empty = inp.lens == 0
    assert empty.sum() == 1
    assert np.all(res["X"][:n][empty] == SENT) and np.all(res["X"][n] == SENT)
    assert np.all(res["bias"][:n][empty] == SENT) and res["bias"][n] == SENT
    assert np.all(res["stat"][:n][empty] == SENT) and np.all(res["stat"][n] == SENT)
    assert np.all(res["X"][:n][~empty][:, k:] == 0.0)


def _margins_p0(inp, ref, res, tol):
    """Worst error / tolerance of x, the bias and the two residual sums over the non-empty rows (<= 1 passes)."""
    k = inp.k
    worst = dict(x=0.0, bias=0.0, stat0=0.0, stat1=0.0)
    for r, o in enumerate(ref):
        if o is None:
            continue
        scale = max(np.max(np.abs(o["x"])), 1e-6)
        worst["x"] = max(worst["x"], gc.ratio(res["X"][r, :k], o["x"], np.full(k, tol["x"] * scale), f"x row {r}"))
        worst["bias"] = max(worst["bias"], gc.ratio(res["bias"][r], o["bias"], tol["bias"] * max(1.0, abs(o["bias"])), f"bias row {r}"))
        worst["stat0"] = max(worst["stat0"], gc.ratio(res["stat"][r, 0], o["sd"], tol["s0"] * max(1.0, o[tol["s0_of"]]), f"stat0 row {r}"))
        b1 = tol["s1"] * max(tol["s1_floor"], o["sd2"]) + tol["s1_rho2"] * o["rho2"]
        worst["stat1"] = max(worst["stat1"], gc.ratio(res["stat"][r, 1], o["sd2"], b1, f"stat1 row {r}"))
    return worst


@pytest.mark.parametrize("path", sorted(PATHS))
def test_p0_against_fp64(path):
    """Assertion 1: the unscaled input against solve_fp64 with the tolerances the mode already has."""
    cfg = PATHS[path]
    inp, ref = _input(cfg["k"], cfg["extra"])
    res = _run(path)[0]
    assert int(res["status"][0]) == 0
    _kernel_class(cfg, res)
    _untouched(inp, res)
    worst = _margins_p0(inp, ref, res, cfg["tol"])
    print(f"row scale p=0 {path}: error / tolerance {worst}")
    gc.record_margins(f"p0 {path}", dict(worst, unit="error / tolerance"))
    assert max(worst.values()) <= 1.0, worst


def _scaled(a, p):
    """a * 2^p in fp32 - exact for what the tests scale (asserted: finite, and back to the same bits)."""
    s = np.float32(2.0 ** p)
    with np.errstate(over="ignore", under="ignore"):
        out = np.asarray(a, np.float32) * s
        assert np.isfinite(out).all() and (out / s).tobytes() == np.asarray(a, np.float32).tobytes()
    return out


@pytest.mark.parametrize("p", [p for p in R.PS if p != 0])
@pytest.mark.parametrize("path", sorted(PATHS))
def test_outputs_scale_bit_for_bit(path, p):
    """Assertion 2: X(p) == 2^p X(0), bias(p) == 2^p bias(0), stat(p)[:, 0] == 2^p stat(0)[:, 0],
    stat(p)[:, 1] == 2^2p stat(0)[:, 1], all bit for bit; status 0, padding zero, empty rows untouched; under
    solve_dtype "auto" / "refine" the same rows are redone (and fall back) at every p - the condition estimate and the
    cancellation test are ratios.  Every path of PATHS holds this (none needed the tolerance fallback of a path with an
    absolute constant: the 1e-10 sits on the matrix)."""
    cfg = PATHS[path]
    inp, _ = _input(cfg["k"], cfg["extra"])
    runs = _run(path)
    r0, rp = runs[0], runs[p]
    n = inp.nrows
    rows = inp.lens > 0
    bad = {}
    for name, got, want in (("X", rp["X"][:n][rows], _scaled(r0["X"][:n][rows], p)),
                            ("bias", rp["bias"][:n][rows], _scaled(r0["bias"][:n][rows], p)),
                            ("stat0", rp["stat"][:n][rows, 0], _scaled(r0["stat"][:n][rows, 0], p)),
                            ("stat1", rp["stat"][:n][rows, 1], _scaled(r0["stat"][:n][rows, 1], 2 * p))):
        if not gc.same_bits(np.ascontiguousarray(got), np.ascontiguousarray(want)):
            with np.errstate(invalid="ignore", divide="ignore"):
                g, w = got.astype(np.float64).reshape(rows.sum(), -1), want.astype(np.float64).reshape(rows.sum(), -1)
                rel = np.max(np.abs(g - w), axis=1) / np.maximum(np.max(np.abs(w), axis=1), 1e-300)
            bad[name] = {int(r): float(v) for r, v in zip(np.flatnonzero(rows), rel) if not v == 0.0}
    print(f"row scale {path} p={p}: rows off the 2^p image (relative to the row's max): {bad}, status {int(rp['status'][0])}")
    gc.record_margins(f"scaled {path} p={p}", {"rows_not_bit_exact": sum(len(v) for v in bad.values())})
    assert int(rp["status"][0]) == 0
    assert not bad, bad
    _kernel_class(cfg, rp)
    _untouched(inp, rp)
    for key in ("redo", "fallback"):
        if key in r0:
            assert rp[key] == r0[key], (key, rp[key], r0[key])
    if "steps" in r0:
        np.testing.assert_array_equal(rp["steps"], r0["steps"])


@pytest.mark.parametrize("factor", [100.0, 1000.0])
def test_presplit_overflow_is_never_silent(factor):
    """Assertion 4: bias_other = factor x the largest rating on the pre-split path (k = 64), ratings on the 2^12 scale.
    The per-call residual scale leaves 64 x of headroom (63.98 at the top of the binade; the largest rating here sits
    at 640 of 1024, so 100 x still fits and 1000 x does not).  Either x is the fp64 solution within the p = 0 tolerance
    or status != 0; status 0 with a wrong or non-finite x fails."""
    cfg = PATHS["planes-k64"]
    _, dev = _device()
    p = 12
    inp, _ = _input(64, False)
    vmax = float(inp.side.vals.max()) * 2.0 ** p
    bo = np.full(R.NCOLS, factor * vmax, np.float32)
    big = R.make_input(64)
    big.side, big.mu, big.b_self, _, _ = R.scaled_inputs(inp.side, inp.mu, inp.b_self, inp.b_other, None, p)
    big.b_other = bo
    ref = R.solve_fp64(big)
    res = _call(_backend(cfg, dev), cfg, inp, p, b_other=bo)
    _kernel_class(cfg, res)
    status = int(res["status"][0])
    worst = 0.0
    finite = True
    for r, o in enumerate(ref):
        if o is None:
            continue
        x = res["X"][r, :64].astype(np.float64)
        finite = finite and bool(np.isfinite(x).all())
        if finite:
            worst = max(worst, float(np.max(np.abs(x - o["x"])) / (cfg["tol"]["x"] * max(np.max(np.abs(o["x"])), 1e-6))))
    print(f"row scale overflow x{factor:g}: status {status}, x finite {finite}, error / tolerance {worst:.3g}")
    gc.record_margins(f"overflow x{factor:g}", {"status_nonzero": status != 0, "x_finite": finite,
                                                "x_error_over_tolerance": worst if finite else None})
    assert status != 0 or (finite and worst <= 1.0), (status, finite, worst)


@pytest.mark.parametrize("q", [0, 8, 13, 16])
@pytest.mark.parametrize("planes", ["off", "on"])
def test_factor_dynamic_range_contract(planes, q):
    """split2 (row_common.hpp): with S the power of two that puts M = max |F| of the whole table in [2^14, 2^15), an
    element f is held as h + l with |f S - h - l| <= 2^-23 |f S| while l is a normal fp16 number - every element within
    2^-14 of M - and to the absolute 2^-25 (half the smallest fp16 subnormal) otherwise: an element error of at most
    e = max(2^-23 |f|, 2^-25 / S) <= max(2^-23 |f|, 2^-39 M).  One row of F (the outlier) is 2^q times the others.
    Rows that gather it: the Gram tolerance of test_row_solve_against_numpy (2.5e-5) relative to max |G|.  Rows that
    do not: each product f_a f_b of their n ratings is off by at most (|f_a| + |f_b|) e + e^2, so
        |G - G_ref| <= 2.5e-5 max |G| (fp32 accumulation, as above) + n (2 t e_t + e_t^2),  t = max |F_row|,
        e_t = max(2^-23 t, 2^-39 M)
    - their own scale, not the outlier's: 2^-39 M is 2^-23 t at q = 16, so the small rows still keep about 22 bits."""
    cfg = dict(PATHS["planes-k64"], planes=planes)
    _, dev = _device()
    from collaborative_filtering_amd import layout
    k = 64
    inp, _ = _input(k, False)
    side = inp.side
    col = int(side.indices[side.indptr[10]])                    # a column of the 700-rating row
    F = inp.F.copy()
    F[col] *= np.float32(2.0 ** q)
    res = _call(_backend(cfg, dev), cfg, inp, 0, gram_out=True, F=F)
    # The Gram is what is checked.  Its error is relative to max |G|, which the outlier raises by 2^2q: from q = 13 on
    # that exceeds lambda + the small eigenvalues of the rows that gather it, their fp32 systems stop being positive
    # definite and status reports them (why solve_dtype "auto" exists) - those rows only, and gram_out is written
    # before the factorisation.
    gathers = [r for r in range(inp.nrows) if col in side.indices[side.indptr[r]: side.indptr[r + 1]]]
    status = int(res["status"][0])
    assert status == 0 or (q >= 13 and status - 1 in gathers), (status, gathers)
    _kernel_class(cfg, res)
    pos = layout.perm_of_col(k)[:k]
    blk = pos // 16
    lower = blk[:, None] >= blk[None, :]                         # the documented valid region of gram_out
    M = float(np.abs(F).max())
    F64 = F[:, :k].astype(np.float64)
    worst = {"gathering": 0.0, "others": 0.0}
    ngather = 0
    for r in range(inp.nrows):
        lo, hi = side.indptr[r], side.indptr[r + 1]
        if hi == lo:
            continue
        idx = side.indices[lo:hi]
        Fr = F64[idx]
        G = Fr.T @ Fr
        got = res["gram"][r].astype(np.float64)[np.ix_(pos, pos)]
        err = float(np.max(np.abs(got - G)[lower]))
        gmax = max(float(np.max(np.abs(G))), 1e-6)
        if col in idx:
            ngather += 1
            bound, key = 2.5e-5 * gmax, "gathering"
        else:
            t = float(np.abs(Fr).max())
            e = max(2.0 ** -23 * t, 2.0 ** -39 * M)
            bound, key = 2.5e-5 * gmax + (hi - lo) * (2.0 * t * e + e * e), "others"
        worst[key] = max(worst[key], err / bound)
    assert 1 <= ngather < int((inp.lens > 0).sum())
    print(f"row scale factor range planes={planes} q={q}: error / bound {worst}")
    gc.record_margins(f"factor range planes={planes} q={q}", dict(worst, unit="error / bound"))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("p", [-12, 0, 12, 17])
def test_fit_scales_with_the_ratings(p):
    """A whole fit of g7_k64 (k = 64: its U-step takes the pre-split path) with the ratings, lambda_u and lambda_v
    times 2^p, default solve_dtype, against OracleALS run live on the same input and configuration, within the TOL of
    tests/test_gpu_parity.py: absolute entries (history, biases, mu, predictions, fold RMSE) times 2^p, factor entries
    relative to max |ref| as they are.  p = 0 is that file's parity test."""
    _device()
    from oracle.als_oracle import OracleALS, ratings_from_coo
    from tests.common import Golden, model_for
    TOL = PARITY_TOL
    g = Golden("g7_k64")
    f = 2.0 ** p
    g.cfg["lambda_u"] *= f
    g.cfg["lambda_v"] *= f
    r, c, v = g.train
    v = v * f
    o = OracleALS(g.oracle_config()).fit(ratings_from_coo(r, c, v, (g.m, g.n)), {}, tol=None)
    m = model_for(g)
    m.fit_coo(r, c, v, (g.m, g.n), features=None, tol=None, verbose=0)
    be = m._eng.be
    assert len(be._planes) > 0 and m._eng.rs_kw["residual_scale"] == be.residual_scale(5.0 * f) == 128.0 / f
    fmax = lambda a: max(float(np.max(np.abs(a))), 1e-30)                                   # noqa: E731
    pred_m, pred_o = m.predict_at(g.val_flat(), None), o.predict_at(g.val_flat(), {})
    truth = g.val_truth() * f
    rmse = lambda pr: float(np.sqrt(np.mean((truth - pr) ** 2)))                           # noqa: E731
    worst = {
        "hist": float(np.max(np.abs(np.asarray(m.history["train_rmse"]) - np.asarray(o.history["train_rmse"])))) / (TOL["hist"] * f),
        "mu": abs(m.mu - o.mu) / (TOL["mu"] * f),
        "b_u": float(np.max(np.abs(m.b_u - o.b_u))) / (TOL["bias"] * f),
        "b_i": float(np.max(np.abs(m.b_i - o.b_i))) / (TOL["bias"] * f),
        "pred": float(np.max(np.abs(pred_m - pred_o))) / (TOL["pred"] * f),
        "test_rmse": abs(rmse(pred_m) - rmse(pred_o)) / (TOL["test_rmse"] * f),
        "U": float(np.max((np.abs(m.U - o.U) - TOL["f_rtol"] * np.abs(o.U)) / (TOL["f_atol"] * fmax(o.U)))),
        "V": float(np.max((np.abs(m.V - o.V) - TOL["f_rtol"] * np.abs(o.V)) / (TOL["f_atol"] * fmax(o.V)))),
    }
    print(f"row scale fit p={p}: error / tolerance {worst}")
    gc.record_margins(f"fit g7_k64 p={p}", dict(worst, unit="error / tolerance"))
    assert len(m.history["train_rmse"]) == len(o.history["train_rmse"])
    assert all(np.isfinite(x) for x in worst.values()) and max(worst.values()) <= 1.0, worst
