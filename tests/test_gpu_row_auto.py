"""T3 (GPU): the default precision path of als_row_solve, solve_dtype="auto" - the condition estimate
(row_needs_f64), the device-side redo list and k_row_redo_f64 - at kernel level, against tests/row_auto_ref.py
(validated without a device by tests/test_row_auto_ref_cpu.py).

A row redone in fp64 is MORE accurate, so a whole fit hides every mistake this path can make; here each part is pinned
on its own: the value of the estimate, which rows are flagged, that unflagged rows are bit for bit the fp32 kernel's,
that flagged rows are the fp64 kernel's (nothing carried over from the fp32 pass), and that the list restarts on every
call.  Every case runs the three backends on the same inputs; the calls are made once per configuration and shared
by the tests (`_run` is cached), the tasks are built as the engine builds them."""
import functools

import numpy as np
import pytest

from tests import row_auto_ref as R
from tests.gpu_common import record_margins

pytestmark = pytest.mark.gpu

SENT = 7.0                       # every output starts as this; the probe as PROBE
PROBE = -1.0
LIMIT_SEQ = (3e4, 30.0, 300.0)   # one backend, three calls: the list must restart growing AND shrinking
CASES = [(k, g, None) for k in R.KS for g in ("f16x2", "f32")] + [(50, "f16x2", 0), (64, "f16x2", 0)]
CASE_IDS = [f"k{k}-{g}" + ("" if p is None else "-noplanes") for k, g, p in CASES]
U24 = 2.0 ** -24

# |cond_probe - estimate| / estimate for the rows below 1e4: about 10x the deviation observed on the MI355X (5.9e-4,
# a pool row at an estimate of 2000 with the f32 Gram; profiles/row_auto_kernel_test_margins.json, "estimate ...");
# never above 0.25, or the guard band of the fixtures (factor 2 around every limit) would mean nothing
EST_TOL = 6e-3
assert EST_TOL <= 0.25
# worst error of an fp32 row / (max(estimate, 1) 2^-24) at the limit 300: 10x the observed value (55, the split pool
# row at an estimate of 100 with the f32 Gram, k = 128: relative error 3.3e-4; same file, "fp32 rows ...")
FP32_ERR_UNITS = 550.0


def _ref_gram(gram, factor=False):
    return "f32" if (factor or gram == "f32") else "f16x2"       # by-products or the f32 Gram: every row primal


@functools.lru_cache(maxsize=None)
def _run(k, gram, dtype, limits=(300.0,), planes=None, alias=False, stats=True, factor=False, overfit=False, rep=0):
    """One backend, one call per limit (fresh outputs each); a list of dicts of numpy arrays.  `rep` only separates
    cache entries (determinism)."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests selected (-m gpu) but no ROCm device is visible")
    from collaborative_filtering_amd import layout
    from collaborative_filtering_amd.als import _side_to_dev, _tasks_to_dev
    from collaborative_filtering_amd.backend import HipBackend
    dev = torch.device("cuda", 0)
    b = R.make_overfit_rows(k) if overfit else R.make_batch(k)
    be = HipBackend(dev, gram=gram, solve_dtype=dtype)
    if planes is not None:
        be.planes_max_floats = planes
    ld, n = layout.padded_k(k), b.nrows
    t = layout.build_row_tasks(b.side.indptr, dual_len=layout.dual_max_len(k), mid_len=layout.dual_mid_len(k))
    sd, td = _side_to_dev(b.side, dev), _tasks_to_dev(t, dev)
    f32 = torch.float32
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                      # noqa: E731
    full = lambda *shape: torch.full(shape, SENT, dtype=f32, device=dev)                  # noqa: E731
    F, b_other, lam_row = tt(b.F), tt(b.b_other), tt(b.lam_row)
    mu = torch.tensor([b.mu], dtype=torch.float64, device=dev)
    ws = torch.empty(max(t.nslots, 1) * be.slot_bytes(k) // 4, dtype=f32, device=dev)
    out = []
    for limit in limits:
        if dtype == "auto":
            be.cond_limit = float(limit)
            be.cond_probe = torch.full((n,), PROBE, dtype=f32, device=dev)
        bias_self = tt(b.b_self.copy())
        o = dict(status=torch.zeros(1, dtype=torch.int32, device=dev))
        if factor:          # one guard row behind every output
            o.update(factor=full((n + 1) * ld * ld), rhs=full(n + 1, ld), colsum=full(n + 1, ld), sumr=full(n + 1),
                     sumr2=full(n + 1))
        else:
            o.update(X=full(n + 1, ld), bias=bias_self if alias else full(n + 1))
            if stats:
                o["stat"] = full(n + 1, 2)
        be.row_solve(k=k, ld=ld, side=sd, F=F, zero_row=R.NCOLS, bias_self=bias_self, bias_other=b_other, mu=mu,
                     lam=0.0, lam_row=lam_row, lam_b=b.lam_b, lam_b_row=None, rhs_extra=None, diag_extra=None,
                     X_out=o.get("X"), bias_out=o.get("bias"), gram_out=None, factor_out=o.get("factor"),
                     rhs_out=o.get("rhs"), colsum_out=o.get("colsum"), sumr_out=o.get("sumr"), status=o["status"],
                     tasks=td, workspace=ws, sumr2_out=o.get("sumr2"), stat_out=o.get("stat"))
        torch.cuda.synchronize()
        res = {name: v.cpu().numpy() for name, v in o.items()}
        if dtype == "auto":
            res["cond"] = be.cond_probe.cpu().numpy()
            cnt = int(be._redo_count.item())
            assert 0 <= cnt <= n
            res["redo"] = be._redo_rows[n].cpu().numpy()[:cnt].tolist()
        if dtype != "float32":
            assert int(res["status"][0]) == 0
        res["planes_used"] = len(be._planes) > 0
        out.append(res)
    return out


def _auto_seq(k, gram, planes, limit):
    return _run(k, gram, "auto", limits=LIMIT_SEQ, planes=planes, stats=False)[LIMIT_SEQ.index(limit)]


def _untouched(b, res, alias=False):
    """Empty rows and the guard row keep their sentinels, the padding columns of written rows are zero."""
    n, k = b.nrows, b.k
    empty = np.flatnonzero(b.lens() == 0)
    if "X" in res:
        assert np.all(res["X"][empty] == SENT) and np.all(res["X"][n] == SENT)
        assert np.all(res["X"][:n][b.lens() > 0][:, k:] == 0.0)
        if alias:
            np.testing.assert_array_equal(res["bias"][empty], b.b_self[empty])
        else:
            assert np.all(res["bias"][empty] == SENT) and res["bias"][n] == SENT
        if "stat" in res:
            assert np.all(res["stat"][empty] == SENT) and np.all(res["stat"][n] == SENT)
    else:
        ld = res["rhs"].shape[1]
        fac = res["factor"].reshape(n + 1, ld, ld)
        for name in ("rhs", "colsum", "sumr", "sumr2"):
            assert np.all(res[name][empty] == SENT) and np.all(res[name][n] == SENT), name
        assert np.all(fac[empty] == SENT) and np.all(fac[n] == SENT)


@pytest.mark.parametrize("limit", R.LIMITS)
@pytest.mark.parametrize("k,gram,planes", CASES, ids=CASE_IDS)
def test_estimate_matches_reference(k, gram, planes, limit):
    """cond_out of every non-empty row against the documented estimate over the REAL pivots (row_auto_ref.estimate).
    Before the padded positions were left out of the max / min, k = 50 and 150 failed here: the padding's unit pivots
    turn the estimate of a row whose real pivots are large into (max L_ii)^2 - the rows of 4 k ... 8200 + k ratings of
    k = 50 (estimates 2 ... 5) were all listed at the limit 30."""
    b = R.make_batch(k)
    res = _auto_seq(k, gram, planes, limit)
    assert res["planes_used"] == (gram == "f16x2" and planes is None and k in (50, 64))
    worst = 0.0
    for r, ref in enumerate(b.reference(_ref_gram(gram))):
        got = float(res["cond"][r])
        if ref is None:
            assert got == PROBE
        elif ref["est"] < 1e4:
            dev = abs(got - ref["est"]) / ref["est"]
            worst = max(worst, dev)
            print(f"estimate k={k} {gram} row {r} {b.classes[r]}: device {got:.6g} reference {ref['est']:.6g}")
            assert dev <= EST_TOL, (r, b.classes[r], got, ref["est"])
        else:
            assert got > limit, (r, b.classes[r], got, ref["est"])           # inf: the fp32 factorisation broke down
    record_margins(f"estimate k={k} {gram} planes={planes} limit={limit:g}", {"rel_dev": worst, "tolerance": EST_TOL})


@pytest.mark.parametrize("k,gram,planes", CASES, ids=CASE_IDS)
def test_partition_is_the_reference_partition(k, gram, planes):
    """The redo list of each of three calls on ONE backend (limits 3e4, 30, 300) is exactly that limit's set: no
    duplicates, no empty rows, the exact count, and neither the union with nor a remnant of the call before - the
    counter is reset by k_factor_scale (f16x2 Gram) / k_reset_word (f32 Gram)."""
    b = R.make_batch(k)
    sets = []
    for limit in LIMIT_SEQ:
        res = _auto_seq(k, gram, planes, limit)
        want = b.flagged(limit, _ref_gram(gram))
        assert len(res["redo"]) == len(set(res["redo"])), res["redo"]
        assert set(res["redo"]) == want, (limit, sorted(res["redo"]), sorted(want))
        assert all(b.lens()[r] > 0 for r in res["redo"])
        _untouched(b, res)
        sets.append(want)
    assert sets[0] < sets[2] < sets[1]            # the three limits do cut the fixture differently


def _compare_fp64_row(b, r, ref, X, bias, stat, tag):
    """A row of the fp64 kernel against numpy at the tolerances of test_row_solve_f64_small_lambda."""
    k = b.k
    x = ref["x"]
    scale = max(np.max(np.abs(x)), 1e-6)
    np.testing.assert_allclose(X[r, :k].astype(np.float64), x, rtol=5e-6, atol=5e-6 * scale, err_msg=f"{tag} row {r} {b.classes[r]}")
    assert abs(float(bias[r]) - ref["bias"]) <= 2e-6 * max(1.0, abs(ref["bias"])), (tag, r, bias[r], ref["bias"])
    if stat is not None:
        assert abs(float(stat[r, 0]) - ref["sd"]) <= 1e-5 * max(1.0, ref["rho_abs"]), (tag, r, stat[r, 0], ref["sd"])
        assert abs(float(stat[r, 1]) - ref["sd2"]) <= 1e-5 * max(1e-3, ref["sd2"]) + 1e-9 * ref["rho2"], (tag, r, stat[r, 1], ref["sd2"])


def _flag_split(b, res, limit, gram):
    """(flagged, unflagged, either) with stat_out: the expected partition, the rows near the statistics threshold set
    aside and taken as the device lists them."""
    rg = _ref_gram(gram)
    rows = {r for r in range(b.nrows) if b.lens()[r] > 0}
    amb = b.stat_ambiguous(rg) - b.flagged(limit, rg)
    want = b.flagged(limit, rg, stats=True)
    got = set(res["redo"])
    assert len(res["redo"]) == len(got)
    assert got - amb == want - amb, (limit, sorted(got), sorted(want), sorted(amb))
    return got, rows - got


@pytest.mark.parametrize("alias", [False, True], ids=["", "alias"])
@pytest.mark.parametrize("limit", R.LIMITS)
@pytest.mark.parametrize("k,gram,planes", CASES, ids=CASE_IDS)
def test_unflagged_rows_are_the_fp32_rows_bitwise(k, gram, planes, limit, alias):
    """X, bias and stat_out of every unflagged row are bit for bit what solve_dtype="float32" writes on the same inputs
    (same binary, same arithmetic; the estimate only reads), with bias_out separate and aliasing bias_self."""
    b = R.make_batch(k)
    auto = _run(k, gram, "auto", limits=(limit,), planes=planes, alias=alias)[0]
    f32 = _run(k, gram, "float32", planes=planes, alias=alias)[0]
    _, unflagged = _flag_split(b, auto, limit, gram)
    assert unflagged
    rows = sorted(unflagged)
    for name in ("X", "bias", "stat"):
        np.testing.assert_array_equal(auto[name][rows], f32[name][rows], err_msg=name)
    _untouched(b, auto, alias)


@pytest.mark.parametrize("alias", [False, True], ids=["", "alias"])
@pytest.mark.parametrize("limit", R.LIMITS)
@pytest.mark.parametrize("k,gram,planes", CASES, ids=CASE_IDS)
def test_flagged_rows_are_the_fp64_rows(k, gram, planes, limit, alias):
    """Flagged rows of at most 4096 ratings are bit for bit the rows of solve_dtype="float64" (gram_passes_f64 and
    finish_row_f64 on the same operands - also the dual-form rows, which the redo solves in the primal form as the
    fp64 backend does); flagged split rows within 2 ulp(fp32) of max|x|, the redo summing them as one task; every
    flagged row against numpy at the fp64 test's tolerances, with the OLD bias when bias_out aliases bias_self."""
    b = R.make_batch(k)
    auto = _run(k, gram, "auto", limits=(limit,), planes=planes, alias=alias)[0]
    f64 = _run(k, "f16x2", "float64", alias=alias)[0]
    flagged, _ = _flag_split(b, auto, limit, gram)
    assert flagged
    ref = b.reference(_ref_gram(gram))
    for r in sorted(flagged):
        if b.lens()[r] <= 4096:
            for name in ("X", "bias", "stat"):
                np.testing.assert_array_equal(auto[name][r], f64[name][r], err_msg=f"{name} row {r} {b.classes[r]}")
        else:
            ulp = float(np.spacing(np.float32(np.max(np.abs(f64["X"][r])))))
            assert np.max(np.abs(auto["X"][r].astype(np.float64) - f64["X"][r])) <= 2 * ulp, (r, b.classes[r])
            assert abs(float(auto["bias"][r]) - float(f64["bias"][r])) <= 2 * float(np.spacing(np.float32(max(abs(f64["bias"][r]), 1.0))))
        _compare_fp64_row(b, r, ref[r], auto["X"], auto["bias"], auto["stat"], "auto")


@pytest.mark.parametrize("k,gram,planes", CASES, ids=CASE_IDS)
def test_fp32_rows_hold_the_documented_error(k, gram, planes):
    """The rows that stay fp32 at the limit 300 against numpy fp64: max|x - x_ref| / max|x_ref| in units of
    max(estimate, 1) 2^-24, and plainly (backend.py documents the latter)."""
    b = R.make_batch(k)
    auto = _run(k, gram, "auto", limits=(300.0,), planes=planes)[0]
    _, unflagged = _flag_split(b, auto, 300.0, gram)
    ref = b.reference(_ref_gram(gram))
    worst_units, worst_rel = 0.0, 0.0
    for r in sorted(unflagged):
        x = ref[r]["x"]
        rel = float(np.max(np.abs(auto["X"][r, :k] - x)) / max(np.max(np.abs(x)), 1e-6))
        units = rel / (max(ref[r]["est"], 1.0) * U24)
        print(f"fp32 row k={k} {gram} row {r} {b.classes[r]}: est {ref[r]['est']:.4g} rel err {rel:.3e} units {units:.1f}")
        worst_units, worst_rel = max(worst_units, units), max(worst_rel, rel)
    record_margins(f"fp32 rows k={k} {gram} planes={planes}", {"err_units": worst_units, "rel_err": worst_rel,
                                                                "tolerance_units": FP32_ERR_UNITS})
    assert worst_units <= FP32_ERR_UNITS


@pytest.mark.parametrize("gram", ["f16x2", "f32"])
@pytest.mark.parametrize("k", R.KS)
def test_statistics_flag_overfitted_rows(k, gram):
    """Well-conditioned rows whose ratings the model explains to 1e-3: with stat_out they are on the redo list although
    their estimate is far below the limit (sum d^2 < 1e-3 sum (rho - b)^2: the fp32 closed form has cancelled), and
    their stat_out is the directly evaluated fp64 sums; without stat_out nothing is listed."""
    b = R.make_overfit_rows(k)
    ref = b.reference(_ref_gram(gram))
    rows = {r for r in range(b.nrows) if ref[r] is not None}
    res = _run(k, gram, "auto", limits=(300.0,), overfit=True)[0]
    assert sorted(res["redo"]) == sorted(rows)
    for r in rows:
        assert 1.0 <= res["cond"][r] <= 30.0 and abs(res["cond"][r] - ref[r]["est"]) <= EST_TOL * ref[r]["est"]
        _compare_fp64_row(b, r, ref[r], res["X"], res["bias"], res["stat"], "overfit")
    _untouched(b, res)
    res = _run(k, gram, "auto", limits=(300.0,), overfit=True, stats=False)[0]
    assert res["redo"] == []
    _untouched(b, res)


def _l_error_units(M, L):
    """Worst deviation of the factor rebuilt from factor_out (lower triangle, reciprocal diagonal, perm space) from
    the fp64 Cholesky factor, in units of the fp32 storage rounding 2^-23 |L_ij| (+ 1e-9 max|L|)."""
    with np.errstate(all="ignore"):
        Lrec = np.tril(M, -1) + np.diag(1.0 / np.diag(M))
        tol = 2.0 ** -23 * np.abs(L) + 1e-9 * np.max(np.abs(L))
        u = np.abs(np.tril(Lrec) - L) / tol
    return float(np.max(np.where(np.isfinite(u), u, np.inf)))


@pytest.mark.parametrize("gram", ["f16x2", "f32"])
@pytest.mark.parametrize("k", [50, 64, 128])
def test_factor_mode_redo_overwrites_every_byproduct(k, gram):
    """Factor mode (factor_out + rhs_out, colsum_out, sumr_out, sumr2_out, no X_out): the fp32 kernel has written the
    four vectors before it decides, so the redo must overwrite them and the factor.  Flagged rows: L and the vectors
    are the fp64 ones to fp32 storage rounding - which an fp32-factored L misses by orders of magnitude (asserted on
    the float32 backend's output, so the test can tell the two apart).  Unflagged rows: bit for bit the fp32 rows."""
    b = R.make_batch(k)
    n, ld = b.nrows, R.layout.padded_k(k)
    auto = _run(k, gram, "auto", limits=(300.0,), factor=True)[0]
    f32 = _run(k, gram, "float32", factor=True)[0]
    ref = b.reference("f32")
    want = b.flagged(300.0, "f32")
    assert set(auto["redo"]) == want and len(auto["redo"]) == len(want)
    fa, ff = auto["factor"].reshape(n + 1, ld, ld), f32["factor"].reshape(n + 1, ld, ld)
    for r in range(n):
        if ref[r] is None:
            continue
        if r not in want:
            for name in ("rhs", "colsum", "sumr", "sumr2"):
                np.testing.assert_array_equal(auto[name][r], f32[name][r], err_msg=f"{name} row {r}")
            np.testing.assert_array_equal(fa[r], ff[r])
            continue
        L = ref[r]["L"]
        assert _l_error_units(fa[r].astype(np.float64), L) <= 1.0, (r, b.classes[r])
        assert not _l_error_units(ff[r].astype(np.float64), L) <= 30.0, (r, b.classes[r])
        np.testing.assert_allclose(fa[r], fa[r].T, rtol=0, atol=0)                       # the symmetric completion
        for name in ("rhs", "colsum"):
            v = ref[r][name]
            np.testing.assert_allclose(auto[name][r].astype(np.float64), v, rtol=2.0 ** -23, atol=1e-9 * np.max(np.abs(v)),
                                       err_msg=f"{name} row {r} {b.classes[r]}")
        for name in ("sumr", "sumr2"):
            assert abs(float(auto[name][r]) - ref[r][name]) <= 2.0 ** -23 * abs(ref[r][name]) + 1e-9 * ref[r]["rho2"] ** 0.5, (name, r)
    _untouched(b, auto)


@pytest.mark.parametrize("gram", ["f16x2", "f32"])
@pytest.mark.parametrize("k", [50, 128])
def test_auto_is_deterministic(k, gram):
    """Two runs on fresh backends: bitwise equal outputs and equal redo sets (the list order may differ)."""
    a = _run(k, gram, "auto", limits=(300.0,), alias=True, rep=1)[0]
    c = _run(k, gram, "auto", limits=(300.0,), alias=True, rep=2)[0]
    for name in ("X", "bias", "stat", "cond"):
        np.testing.assert_array_equal(a[name], c[name], err_msg=name)
    assert sorted(a["redo"]) == sorted(c["redo"]) and len(a["redo"]) > 2
