"""The reference and the fixtures of tests/test_gpu_row_auto.py, checked without a device: the documented estimate is
the lower bound it claims to be, the fixtures keep their guard band around every limit the GPU tests use (so the
expected partition cannot depend on fp32 rounding), and the reference solutions solve their own equations."""
import numpy as np
import pytest

from tests import row_auto_ref as R

GRAMS = ("f16x2", "f32")
BAND = 2.0


@pytest.fixture(scope="module", params=R.KS)
def batch(request):
    return R.make_batch(request.param)


def _rows(batch, gram):
    return [(r, ref) for r, ref in enumerate(batch.reference(gram)) if ref is not None]


def test_fixture_has_every_row_class(batch):
    k, lens = batch.k, batch.lens()
    empty = np.flatnonzero(lens == 0)
    assert empty.size == 2 and empty[1] - empty[0] > 1
    for n in (1, k - 1, k, 4 * k - 1, 4 * k, 4 * k + 1, 700, 4097, 8200 + k):
        assert n in lens, n
    assert np.any((lens > k) & (lens < 4 * k - 1)) and np.any((lens > 0) & (lens < k))
    if k > 64:
        assert all(n in lens for n in (15, 16, 17, 48, 49, 64))
    if k > 96:
        assert all(n in lens for n in (65, 80, 81, 96))
    assert 20 <= batch.nrows <= 35
    # ratings 0.5 ... 5 in halves; the padding of F and its last row are zero
    assert np.all((batch.side.vals >= 0.5) & (batch.side.vals <= 5.0) & (batch.side.vals * 2 == np.round(batch.side.vals * 2)))
    assert np.all(batch.F[-1] == 0) and np.all(batch.F[:, k:] == 0) and batch.F.dtype == np.float32
    for r in range(batch.nrows):
        idx, _, _ = batch.row(r)
        assert np.all(np.diff(idx) > 0)
        if "pool" in batch.classes[r]:
            assert np.all(idx < R.NPOOL)


@pytest.mark.parametrize("gram", GRAMS)
def test_pivot_and_mean_terms_are_lower_bounds_of_cond2(batch, gram):
    for r, ref in _rows(batch, gram):
        assert ref["pivot"] <= ref["cond2"] * (1 + 1e-9), (r, batch.classes[r])
        assert ref["mean"] <= ref["cond2"] * (1 + 1e-9), (r, batch.classes[r])


@pytest.mark.parametrize("k", [1, 3, 16, 50, 64, 150])
def test_lower_bound_on_random_spd_matrices(k):
    rng = np.random.default_rng(40 + k)
    for trial in range(40):
        nnz = int(rng.integers(1, 6 * k + 2))
        Fr = rng.normal(size=(nnz, k)) * 10.0 ** rng.uniform(-2, 1, size=(1, k)) * 10.0 ** rng.uniform(-1, 1, size=(nnz, 1))
        lam = R.lam_of(10.0 ** rng.uniform(-4, 1))
        for dual in ((False, True) if nnz <= 96 else (False,)):
            e = R.estimate(Fr, lam, k, nnz, dual)
            c = R.cond2(Fr, lam, k, dual)
            assert e["pivot"] <= c * (1 + 1e-9) and e["mean"] <= c * (1 + 1e-9), (trial, dual, e, c)
            assert e["est"] >= 1.0


@pytest.mark.parametrize("gram", GRAMS)
def test_guard_band_and_partition_preconditions(batch, gram):
    k = batch.k
    rows = _rows(batch, gram)
    split = {r for r in range(batch.nrows) if batch.lens()[r] > 4096}
    assert len(split) >= 4
    for limit in R.LIMITS:
        for r, ref in rows:
            assert not (limit / BAND <= ref["est"] <= limit * BAND), (limit, r, batch.classes[r], ref["est"])
        flagged = batch.flagged(limit, gram)
        unflagged = {r for r, _ in rows} - flagged
        assert flagged and unflagged
        if k in (50, 64, 128):
            assert flagged & split and unflagged & split, limit
    # the statistics criterion: the rows near its threshold are few and short; the GPU tests that pass stat_out leave
    # them out of the expected partition (Batch.stat_ambiguous)
    amb = batch.stat_ambiguous(gram)
    assert len(amb) <= 4 and all(batch.lens()[r] < k for r in amb), [batch.classes[r] for r in amb]
    assert not (amb & split)


@pytest.mark.parametrize("gram", GRAMS)
def test_short_row_bound_switches_off_at_4k_ratings(batch, gram):
    ref = batch.reference(gram)
    c = {name: r for r, name in enumerate(batch.classes)}
    assert batch.lam_row[c["short_last"]] == batch.lam_row[c["long_first"]] == batch.lam_row[c["long_second"]]
    assert ref[c["short_last"]]["short"] > 600 and ref[c["short_last"]]["est"] == ref[c["short_last"]]["short"]
    for name in ("long_first", "long_second", "long_first_pool"):
        assert ref[c[name]]["short"] == 0.0
    assert ref[c["long_first"]]["est"] < 15 and ref[c["long_second"]]["est"] < 15
    # flagged by the pivot terms alone
    for name in ("pool_1e-3", "split_pool_hi", "long_first_pool"):
        assert ref[c[name]]["short"] == 0.0 and ref[c[name]]["est"] > 600


@pytest.mark.parametrize("gram", GRAMS)
def test_float32_cholesky_gives_the_same_partition(batch, gram):
    k = batch.k
    for r, ref in _rows(batch, gram):
        _, Fr, _ = batch.row(r)
        e32 = R.estimate(Fr, R.lam_of(batch.lam_row[r]), k, Fr.shape[0], ref["dual"], dtype=np.float32)["est"]
        for limit in R.LIMITS:
            assert (e32 > limit) == (ref["est"] > limit), (r, batch.classes[r], limit, e32, ref["est"])
        if ref["est"] < 1e4:
            assert abs(e32 - ref["est"]) < 0.25 * ref["est"], (r, batch.classes[r], e32, ref["est"])


@pytest.mark.parametrize("k", R.KS)
def test_overfit_rows_are_well_conditioned_and_cancel(k):
    b = R.make_overfit_rows(k)
    rows = _rows(b, "f16x2")
    assert len(rows) == 3
    for r, ref in rows:
        assert ref["est"] < 30 / BAND and not ref["dual"]
        assert ref["sd2"] < R.STAT_RATIO / 4 * ref["s2"], (r, ref["sd2"] / ref["s2"])


@pytest.mark.parametrize("gram", GRAMS)
def test_reference_solutions_satisfy_their_normal_equations(batch, gram):
    for r, ref in _rows(batch, gram):
        A, b, x = ref["A"], ref["b"], ref["x"]
        res = np.linalg.norm(A @ x - b)
        assert res <= 1e-12 * (np.linalg.norm(A, 2) * np.linalg.norm(x) + np.linalg.norm(b)), (r, batch.classes[r], res)
        # the bias is the stationary point of its own equation, and L L^T is the padded A
        idx, Fr, vals = batch.row(r)
        rho = vals - batch.mu - batch.b_other[idx].astype(np.float64)
        assert abs(ref["bias"] * (idx.size + batch.lam_b + R.EPS) - np.sum(rho - Fr @ x)) <= 1e-12 * np.abs(rho).sum()
        L = ref["L"]
        pos = R.layout.perm_of_col(batch.k)[: batch.k]
        np.testing.assert_allclose((L @ L.T)[np.ix_(pos, pos)], A, rtol=0, atol=1e-12 * np.abs(A).max())
