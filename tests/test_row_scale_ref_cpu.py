"""The reference of the row solve's input-scale tests (tests/row_scale_ref.py) without a device: the scaled inputs are
exact, the fp64 solution solves its system and is linear in them, and the fp16 pair of the pre-split path has the
range and precision the scale rule is built on - derived from np.finfo(np.float16), not measured."""
import numpy as np
import pytest

from tests import row_scale_ref as R

F16 = np.finfo(np.float16)


@pytest.mark.parametrize("k", [16, 50, 64, 80, 128])
def test_scaled_inputs_are_exact_multiples(k):
    inp = R.make_input(k, extra=True)
    assert list(np.diff(inp.side.indptr)) == R.lens(k) and inp.F.shape == (R.NCOLS + 1, inp.ld)
    assert not inp.F[R.NCOLS].any() and not inp.F[:, k:].any()
    for p in R.PS:      # (scaled_inputs asserts: normal, finite, divides back to the original bits)
        side, mu, bs, bo, ex = R.scaled_inputs(inp.side, inp.mu, inp.b_self, inp.b_other, inp.rhs_extra, p)
        assert side.vals.dtype == bs.dtype == bo.dtype == ex.dtype == np.float32
        assert mu == inp.mu * 2.0 ** p and float(np.float32(mu)) == mu
        np.testing.assert_array_equal(side.vals.astype(np.float64), inp.side.vals.astype(np.float64) * 2.0 ** p)
    with pytest.raises(AssertionError):         # 5.0 * 2^126 is not an fp32 number
        R.scaled_inputs(inp.side, inp.mu, inp.b_self, inp.b_other, None, 126)


def test_small_rows_have_small_residuals():
    inp = R.make_input(64)
    ref = R.solve_fp64(inp)
    small = max(np.abs(ref[r]["rho"] - float(inp.b_self[r])).max() for r in R.SMALL_ROWS)
    other = min(np.abs(ref[r]["rho"] - float(inp.b_self[r])).max() for r in range(inp.nrows)
                if ref[r] is not None and r not in R.SMALL_ROWS)
    assert small < 2.0 ** -8 * 6 and other > 0.25, (small, other)
    assert float(inp.side.vals.max()) == 5.0            # the small rows do not move the call's largest rating


@pytest.mark.parametrize("k,extra", [(16, True), (50, False), (64, False), (64, True)])
def test_solve_fp64_solves_and_is_linear(k, extra):
    """x solves its normal equations, the residual sums equal the closed forms the kernels use (DESIGN.md
    "Statistics"), and the solution of the 2^p-scaled input is 2^p times the solution at p = 0 to fp64 rounding - the
    1e-10 sits on the matrix, not on the right-hand side."""
    inp = R.make_input(k, extra=extra)
    ref = R.solve_fp64(inp)
    assert [r is None for r in ref] == [n == 0 for n in R.lens(k)]
    for r, o in enumerate(ref):
        if o is None:
            continue
        assert np.abs(o["A"] @ o["x"] - o["b"]).max() <= 1e-12 * max(np.abs(o["b"]).max(), 1e-30)
        n = len(o["rho"])
        s2 = ((o["rho"] - o["bias"]) ** 2).sum()
        Fx = o["Fr"] @ o["x"]
        closed = s2 - 2.0 * (Fx @ (o["rho"] - o["bias"])) + Fx @ Fx
        assert abs(o["sd2"] - closed) <= 1e-10 * max(s2, 1e-30)
        assert abs(o["sd"] - (o["rho"].sum() - n * o["bias"] - Fx.sum())) <= 1e-11 * o["rho_abs"]
    for p in (-24, 17):
        side, mu, bs, bo, ex = R.scaled_inputs(inp.side, inp.mu, inp.b_self, inp.b_other, inp.rhs_extra, p)
        sc = R.make_input(k, extra=extra)
        sc.side, sc.mu, sc.b_self, sc.b_other, sc.rhs_extra = side, mu, bs, bo, ex
        for o, q in zip(ref, R.solve_fp64(sc)):
            if o is None:
                assert q is None
                continue
            f = 2.0 ** p
            assert np.abs(q["x"] - f * o["x"]).max() <= 1e-11 * f * np.abs(o["x"]).max()
            assert abs(q["bias"] - f * o["bias"]) <= 1e-11 * f * max(abs(o["bias"]), o["rho_abs"] / len(o["rho"]))
            assert abs(q["sd2"] - f * f * o["sd2"]) <= 1e-9 * f * f * o["rho2"]


def _uniform_residuals(c):
    """The issue's sample: 4096 residuals uniform in +-2 c (fp32)."""
    return (np.random.default_rng(17).uniform(-2.0, 2.0, size=4096) * c).astype(np.float32)


def _rel_err(r, s):
    h, l = R.split_pair(r, s)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(R.pair_value(h, l, s) - r.astype(np.float64)) / np.abs(r.astype(np.float64))


def test_fp16_constants():
    assert R.F16_OVERFLOW == 65520.0 and R.F16_HALF_SUBNORMAL == 2.0 ** -25 and R.F16_U == 2.0 ** -11
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(65520.0).astype(np.float16))
        assert np.isfinite(np.nextafter(np.float32(65520.0), np.float32(0)).astype(np.float16))
    assert np.float32(2.0 ** -25).astype(np.float16) == 0 and np.nextafter(np.float32(2.0 ** -25), np.float32(1)).astype(np.float16) > 0


# rating scale c -> worst relative error of one residual of the sample with the UNSCALED pair (s = 1), as the issue's
# table states it (numpy emulation); None: inf / NaN
UNSCALED_TABLE = {2.0 ** -24: 1.0, 2.0 ** -12: 1.0, 2.0 ** -6: 2.2e-3, 1.0: 5.7e-6, 2.0 ** 12: 1.2e-7, 2.0 ** 17: None,
                  2.0 ** 24: None}


@pytest.mark.parametrize("c", sorted(UNSCALED_TABLE))
def test_unscaled_pair_table(c):
    """s = 1 - the path before it had a residual scale.  Every entry follows from the fp16 format: a residual below
    2^-25 rounds to (0, 0) (relative error exactly 1), one at or past 65520 to inf, and in between the pair is within
    max(2^-22, 2^-25 / |r|) (pair_bound) - full precision only where |r| >= 2^-3, whatever the ratings' scale."""
    r = _uniform_residuals(c)
    err = _rel_err(r, 1.0)
    a = np.abs(r.astype(np.float64))
    want = UNSCALED_TABLE[c]
    if want is None:
        assert (a >= R.F16_OVERFLOW).any() and not np.isfinite(err[a >= R.F16_OVERFLOW]).any()
        assert np.isfinite(err[a < R.F16_OVERFLOW]).all()
        return
    flushed = a < R.F16_HALF_SUBNORMAL
    assert (err[flushed] == 1.0).all()
    held = ~flushed
    assert (err[held] <= np.minimum(R.pair_bound(a[held]), 1.0)).all()
    worst = float(err.max())
    if c == 2.0 ** -24:         # 2 c = 2^-23: nothing above the two smallest subnormals - every pair is (0 | 2^-24 | 2^-23, 0)
        h, l = R.split_pair(r, 1.0)
        assert flushed.any() and worst == 1.0
        assert not l.any() and set(np.abs(h.astype(np.float64))) <= {0.0, 2.0 ** -24, 2.0 ** -23}
    else:
        # the sample's worst element is its smallest: the table's figure is 2^-25 / min |r| of the issue's draw, ours
        # differs by the draw - same order of magnitude, and never below the floor u^2 = 2^-22 = 2.4e-7 of a pair
        # (1.2e-7 in the table: the fp32 rounding of the residual itself, which the pair of a large residual reaches)
        assert want / 30.0 <= max(worst, 1.2e-7) <= want * 30.0, (c, worst, want)
        assert worst <= max(float(R.pair_bound(a[held].min())), R.F16_U ** 2)


@pytest.mark.parametrize("c", sorted(UNSCALED_TABLE))
def test_scaled_pair_precision_and_headroom(c):
    """With s = residual_scale(largest rating) - largest rating c * 5.0 here, as on the 0.5 ... 5 grid - the scaled
    largest rating lies in [2^9, 2^10).  From the format: a residual down to 2^-13 of the largest rating has
    |y| >= 2^-4, so its pair is within max(2^-22, 2^-25 / 2^-4) = 2^-21; one up to 64 times the largest rating has
    |y| < 2^16 and is finite as long as |y| < 65520, i.e. for every largest rating whose scaled value is below
    1023.75 - at the very top of the binade the headroom is 65520 / 1024 = 63.98."""
    vmax = np.float32(5.0 * c)
    s = R.residual_scale(vmax)
    assert 2.0 ** 9 <= float(vmax) * s < 2.0 ** 10
    r = _uniform_residuals(c)
    r = np.concatenate([r, [vmax, -vmax, vmax * np.float32(2.0 ** -13), vmax * np.float32(-2.0 ** -13)]]).astype(np.float32)
    a = np.abs(r.astype(np.float64))
    err = _rel_err(r, s)
    big = a >= 2.0 ** -13 * float(vmax)
    assert big.sum() > 4000 and (err[big] <= 2.0 ** -21).all(), float(err[big].max())
    assert (err[~big] <= R.pair_bound(a[~big] * s)).all()           # smaller ones: absolute, 2^-25 / s
    # headroom: 64 x the largest rating (mu and the biases on top of a rating) stays finite, 128 x does not
    top = np.array([64.0, -64.0, 63.98, 100.0], np.float32) * vmax
    h, l = R.split_pair(top, s)
    assert np.isfinite(h.astype(np.float64)).all() and np.isfinite(l.astype(np.float64)).all()
    assert (_rel_err(top, s) <= 2.0 ** -22).all()
    h, _ = R.split_pair(np.array([128.0], np.float32) * vmax, s)
    assert np.isinf(h).all()


def test_headroom_over_a_binade():
    """The headroom statement for every position of the largest rating inside its binade: 64 x is finite while the
    scaled maximum is below 65520 / 64 = 1023.75, 63.98 x always."""
    for m in np.concatenate([np.linspace(512.0, 1023.74, 300), [1023.75, 1023.99]]).astype(np.float32):
        s = R.residual_scale(m)
        assert s == 1.0
        h64, _ = R.split_pair(np.array([64.0 * float(m)], np.float32), s)
        assert np.isfinite(h64.astype(np.float64)).all() == (64.0 * float(m) < R.F16_OVERFLOW), m
        h, _ = R.split_pair(np.array([63.98 * float(m)], np.float32), s)
        assert np.isfinite(h.astype(np.float64)).all(), m


def test_residual_scale_rule():
    """An exact power of two; residual_scale(2^p v) == 2^-p residual_scale(v) for every p of the GPU tests (what makes
    the scaled pair - and with it every output - the same bits at every p); the backend's rule is this rule."""
    from collaborative_filtering_amd.backend import HipBackend
    vals = [5.0, 0.5, 4.99, 1.0, 3.3, 511.9, 512.0, 1023.99, 1024.0, 1e-3, 7e4, 2.0 ** -60, 2.0 ** 60]
    for v in vals:
        s = R.residual_scale(v)
        m, e = np.frexp(s)
        assert m == 0.5 and 2.0 ** 9 <= v * s < 2.0 ** 10, (v, s)
        assert s == HipBackend.residual_scale(v)
        for p in R.PS:
            assert R.residual_scale(v * 2.0 ** p) == s * 2.0 ** -p, (v, p)
    # the clamp keeps the scale and its inverse normal fp32 numbers; no ratings, or nonsense: 1
    for v, want in ((2.0 ** 140, 2.0 ** -126), (2.0 ** -140, 2.0 ** 126), (0.0, 1.0), (float("inf"), 1.0), (float("nan"), 1.0)):
        assert R.residual_scale(v) == want == HipBackend.residual_scale(v)
        assert np.float32(want) >= np.finfo(np.float32).tiny and np.float32(1.0 / want) >= np.finfo(np.float32).tiny
