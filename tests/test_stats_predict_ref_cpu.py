"""The reference of tests/stats_predict_ref.py, validated without a device: exact-input expectations against rational
arithmetic, real-input expectations against math.fsum, the factor-scale rule against a brute-force search, the engine's
numpy stand-in (tests/cpu_backend.py) against the exact expectations, and the promises the fixtures make to
tests/test_gpu_stats_predict.py (split segments, more than 1024 tasks, association-sensitive entries, loop trips)."""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from collaborative_filtering_amd import layout
from tests import stats_predict_ref as ref
from tests.cpu_backend import NumpyBackend


def _round_f32(q):
    """Fraction -> the nearest float32, ties to even (q = 0 or a normal number)."""
    if q == 0:
        return np.float32(0.0)
    e = math.floor(math.log2(abs(q)))
    while Fraction(2) ** e > abs(q):
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(q):
        e += 1
    ulp = Fraction(2) ** (e - 23)
    t = q / ulp
    lo = math.floor(t)
    r = t - lo
    n = lo + 1 if (r > Fraction(1, 2) or (r == Fraction(1, 2) and lo % 2 == 1)) else lo
    return np.float32(float(n * ulp))


@pytest.mark.parametrize("biases", ["tied", "mixed"])
@pytest.mark.parametrize("k", [1, 17, 50])
def test_exact_prediction_equals_rational_arithmetic_rounded_step_by_step(k, biases):
    inp = ref.predict_inputs(k, 5, 7, "exact", seed=k, biases=biases, mu=ref.MU_EXTRA if biases == "mixed" else None)
    got = ref.expected_predict_exact(inp)
    mu = Fraction(float(np.float32(inp.mu)))
    for u in range(inp.m):
        for i in range(inp.n):
            dot = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(inp.U[u], inp.Z[i]))
            assert dot.denominator == 1
            s = _round_f32(dot + mu)
            s = _round_f32(Fraction(float(s)) + Fraction(float(inp.b_u[u])))
            s = _round_f32(Fraction(float(s)) + Fraction(float(inp.b_i[i])))
            assert s == got[u, i], (u, i)


@pytest.mark.parametrize("k", ref.KS)
def test_prediction_fixture_tells_the_associations_apart(k):
    """The shape every k runs on the device (m = 17, n = 257): on at least half of the entries the three associations
    of the epilogue do not all agree, and each wrong one differs from the contract on many entries; with MU_EXTRA a mu
    added in double differs as well, while float32(MU_EXTRA) is the plain 12.375."""
    inp = ref.predict_inputs(k, 17, 257, "exact", seed=k)
    left, a1, a2 = (ref.expected_predict_exact(inp, a) for a in ref.ASSOCIATIONS)
    assert np.mean((left != a1) | (left != a2) | (a1 != a2)) >= 0.5
    assert np.count_nonzero(left != a1) >= 100 and np.count_nonzero(left != a2) >= 100
    assert np.array_equal(ref.expected_predict_exact(inp, mu_double=True), left)          # mu is a float32 here
    ext = ref.predict_inputs(k, 17, 257, "exact", seed=k, mu=ref.MU_EXTRA, biases="mixed")
    assert float(np.float32(ext.mu)) == 12.375 and ext.mu != 12.375
    e = ref.expected_predict_exact(ext)
    assert np.count_nonzero(ref.expected_predict_exact(ext, mu_double=True) != e) >= 100
    assert all(np.count_nonzero(ref.expected_predict_exact(ext, a) != e) >= 50 for a in ref.ASSOCIATIONS[1:])


def test_real_prediction_and_residuals_equal_fsum():
    inp = ref.predict_inputs(50, 6, 9, "real", seed=3)
    P, S = ref.expected_predict_real(inp)
    mu = float(np.float32(inp.mu))
    for u in range(inp.m):
        for i in range(inp.n):
            terms = [float(a) * float(b) for a, b in zip(inp.U[u], inp.Z[i])] + [mu, float(inp.b_u[u]), float(inp.b_i[i])]
            assert abs(P[u, i] - math.fsum(terms)) <= 60 * ref.U64 * S[u, i]
            assert abs(S[u, i] - math.fsum(abs(t) for t in terms)) <= 60 * ref.U64 * S[u, i]
    st = ref.stats_inputs(33, "real", [0, 5, 70, 1], 200, seed=4)
    d, Sd = ref.residuals(st)
    ru = np.repeat(np.arange(st.m), np.diff(st.indptr))
    mu = float(np.float32(st.mu))
    exact = []
    for r, (u, i) in enumerate(zip(ru, st.indices)):
        terms = [float(st.vals[r]), -mu, -float(st.b_u[u]), -float(st.b_i[i])] + \
            [-float(a) * float(b) for a, b in zip(st.U[u], st.Z[i])]
        exact.append(math.fsum(terms))
        assert abs(d[r] - exact[-1]) <= 40 * ref.U64 * Sd[r]
    s0, s1, b0, b1 = ref.expected_stats(st)
    assert abs(s0 - math.fsum(exact)) <= 1e-12 and abs(s1 - math.fsum(x * x for x in exact)) <= 1e-12
    e = (st.ld + 3) * ref.U32 * Sd
    assert e.sum() < b0 <= 1.001 * e.sum() and 0 < b1 <= 1.001 * float((e * (2 * np.abs(d) + e)).sum())


def test_exact_statistics_equal_rational_arithmetic():
    st = ref.stats_inputs(17, "exact", [0, 1, 5, 64, 3], 80, seed=5)
    ru = np.repeat(np.arange(st.m), np.diff(st.indptr))
    s0 = s1 = Fraction(0)
    for r, (u, i) in enumerate(zip(ru, st.indices)):
        dot = sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(st.U[u], st.Z[i]))
        d = Fraction(float(st.vals[r])) - (dot + Fraction(st.mu) + Fraction(float(st.b_u[u])) + Fraction(float(st.b_i[i])))
        s0, s1 = s0 + d, s1 + d * d
    e0, e1, _, _ = ref.expected_stats(st)
    assert Fraction(e0) == s0 and Fraction(e1) == s1
    x = ref.exact_vector(np.random.default_rng(1), 1027)
    assert ref.expected_sumsq(x) == (float(sum(int(v) ** 2 for v in x)), sum(int(v) ** 2 for v in x))
    p = ref.eighths(np.random.default_rng(2), 2 * 257)
    sums, _ = ref.expected_sum_pairs(p)
    assert Fraction(sums[0]) == sum(Fraction(float(v)) for v in p[0::2])
    assert Fraction(sums[1]) == sum(Fraction(float(v)) for v in p[1::2])


def test_real_sums_equal_fsum_and_compose_equals_fsum():
    x = ref.real_vector(np.random.default_rng(6), 1027)
    s, exact = ref.expected_sumsq(x)
    assert exact is None and abs(s - math.fsum(float(v) ** 2 for v in x)) <= 1027 * ref.U64 * s
    c = ref.compose_inputs(50, 5, 7, "real", seed=7)
    Z, S = ref.expected_compose(c)
    for i in range(c.n):
        for col in range(c.ld):
            terms = [float(c.V[i, col])] + [float(c.X[i, a]) * float(c.W[a, col]) for a in range(c.D)]
            assert abs(Z[i, col] - math.fsum(terms)) <= 10 * ref.U64 * S[i, col]
    assert not Z[:, c.k:].any() and not S[:, c.k:].any()
    c0 = ref.compose_inputs(50, 5, 0, "exact", seed=8)
    assert np.array_equal(ref.expected_compose(c0)[0], c0.V)


def test_history_scalars_follow_the_host_arithmetic():
    rmse, m = ref.expected_history_scalars((-37.5, 912.25), 1000, 3.25)
    assert m == 3.25 + (-37.5 / 1000) and rmse == math.sqrt(912.25 / 1000 - (-37.5 / 1000) * (-37.5 / 1000))
    assert ref.expected_history_scalars((3.0, 0.0), 3, 0.0)[0] == 0.0          # negative variance clamps to 0
    assert np.isnan(ref.expected_history_scalars((0.0, 0.0), 0, 1.0)[0])
    assert np.isnan(ref.expected_history_scalars((2.0, 5.0), 0, 1.0)[0])


def _brute_force_j(mx):
    """The j in [-60, 60] with 2^j mx in [2^14, 2^15), else the clamp on the side mx falls off."""
    for j in range(-60, 61):
        if 2.0 ** 14 <= math.ldexp(mx, j) < 2.0 ** 15:
            return j
    return 60 if math.ldexp(mx, 60) < 2.0 ** 14 else -60


def test_factor_scale_rule_equals_a_brute_force_search():
    f32 = np.float32
    rng = np.random.default_rng(9)
    values = [float(v) for v in ref.scale_values().values() if np.isfinite(v) and v != 0]
    values += [float(f32(10.0 ** e)) for e in range(-36, 38, 3)] + [2.0 ** e for e in (-126, -47, -46, -45, 0, 73, 74, 75, 127)]
    values += [float(np.nextafter(f32(2.0 ** e), f32(0))) for e in (-45, 0, 74)]
    for v in values:
        F = ref.scale_background(rng, 64, f32(v))
        F[17] = -v
        j = _brute_force_j(abs(v))
        s0, s1 = ref.expected_scale(F)
        assert s0 == f32(2.0 ** j) and s1 == f32(2.0 ** (-2 * j)), v
        assert np.max(np.abs(F)) == abs(f32(v))
    assert ref.expected_scale(np.zeros(8, f32)) == (f32(2.0 ** 60), f32(2.0 ** -120))
    assert ref.expected_scale(np.zeros(0, f32)) == (f32(2.0 ** 60), f32(2.0 ** -120))
    for bad in (np.nan, np.inf, -np.inf):
        assert ref.expected_scale(np.array([1.0, bad, 3.0], f32)) == (f32(2.0 ** -60), f32(2.0 ** 120))
    assert ref.expected_scale(np.array([3e-41], f32))[0] == f32(2.0 ** 60)          # a denormal maximum


def test_factor_scale_positions_cover_the_unrolled_slots():
    """nfloats of the device cases: one workgroup / several; the last one runs a second trip with a partial tail; the
    positions hit every unrolled slot of the final trip that holds data, the first and the last element."""
    assert ref.scale_positions(0) == []
    assert ref.scale_positions(4) == [0, 3]
    n4, grid, stride = ref.scale_geometry(4 * 1024 * 3 + 4)
    assert (n4, grid, stride) == (3073, 4, 1024)
    slots = {(p // 4) // stride for p in ref.scale_positions(4 * 1024 * 3 + 4)}
    assert slots == {0, 1, 2, 3}
    big = ref.SCALE_NFLOATS[-1]
    n4, grid, stride = ref.scale_geometry(big)
    assert grid == 512 and n4 == 4 * stride + 5                     # second trip: 5 float4 in slot 0, slots 1 ... 3 empty
    pos = ref.scale_positions(big)
    assert pos[0] == 0 and pos[-1] == big - 1 and all(p == 0 or p // 4 >= 4 * stride for p in pos)
    for nf in ref.SCALE_NFLOATS:
        assert nf % 4 == 0 and all(0 <= p < nf for p in ref.scale_positions(nf))


def _side_and_tasks(st):
    side = SimpleNamespace(indptr=torch.from_numpy(st.indptr), indices=torch.from_numpy(st.indices),
                           vals=torch.from_numpy(st.vals))
    t = layout.build_row_tasks(st.indptr)
    return side, SimpleNamespace(tasks=torch.from_numpy(t.tasks), ntasks=t.tasks.shape[0]), t


@pytest.mark.parametrize("k", [1, 33, 160])
def test_numpy_stand_in_equals_the_exact_expectations(k):
    """tests/cpu_backend.py restates the contract for the CPU tests of the engine: on exact inputs it must give the
    very values the kernels are held to (predictions in the fp32 association of walk::score)."""
    be = NumpyBackend()
    tt = torch.from_numpy
    for biases, mu in (("tied", None), ("mixed", ref.MU_EXTRA)):
        inp = ref.predict_inputs(k, 17, 65, "exact", seed=k, mu=mu, biases=biases)
        exp = ref.expected_predict_exact(inp)
        mu_t = torch.tensor([inp.mu], dtype=torch.float64)
        dense = torch.zeros(inp.m, inp.n)
        be.predict_dense(k=k, ld=inp.ld, m=inp.m, n=inp.n, U=tt(inp.U), Z=tt(inp.Z), b_u=tt(inp.b_u), b_i=tt(inp.b_i),
                         mu=mu_t, out=dense)
        assert np.array_equal(dense.numpy(), exp)
        us, is_ = ref.predict_pairs(inp.m, inp.n, 1001, seed=k)
        at = torch.zeros(us.size)
        be.predict_at(k=k, ld=inp.ld, us=tt(us), is_=tt(is_), U=tt(inp.U), Z=tt(inp.Z), b_u=tt(inp.b_u), b_i=tt(inp.b_i),
                      mu=mu_t, out=at)
        assert np.array_equal(at.numpy(), exp[us, is_])
    st = ref.stats_inputs(k, "exact", [0, 1, 3, 64, 65, 300], 400, seed=k)
    side, tasks, _ = _side_and_tasks(st)
    out = torch.zeros(2, dtype=torch.float64)
    be.residual_stats(k=k, ld=st.ld, side=side, U=tt(st.U), Z=tt(st.Z), b_u=tt(st.b_u), b_i=tt(st.b_i),
                      mu=torch.tensor([st.mu], dtype=torch.float64), tasks=tasks, out=out)
    s0, s1, _, _ = ref.expected_stats(st)
    assert out[0].item() == s0 and out[1].item() == s1
    x = ref.exact_vector(np.random.default_rng(k), 1027)
    ss = torch.zeros(1, dtype=torch.float64)
    be.sumsq(tt(x), ss)
    assert ss.item() == ref.expected_sumsq(x)[1]
    p = ref.eighths(np.random.default_rng(k + 1), 2 * 257)
    sp = torch.zeros(2, dtype=torch.float64)
    be.sum_pairs(tt(p), sp)
    assert np.array_equal(sp.numpy(), ref.expected_sum_pairs(p)[0])


def test_pairs_hold_the_corners_and_repeats():
    m, n = 33, 300
    for npairs in ref.AT_NPAIRS:
        us, is_ = ref.predict_pairs(m, n, npairs, seed=npairs)
        assert us.size == npairs and us.min() >= 0 and us.max() < m and is_.min() >= 0 and is_.max() < n
        if npairs >= 3:
            assert 0 in us and m - 1 in us and 0 in is_ and n - 1 in is_
            assert len(set(zip(us.tolist(), is_.tolist()))) < npairs
    assert sum(1 for p in ref.AT_NPAIRS if p % 4) >= 5 and max(ref.AT_NPAIRS) > 8192 * 16      # a second grid-stride pass


@pytest.mark.parametrize("k", ref.KS)
def test_statistics_fixture_splits_rows_and_fills_the_final_reduction(k):
    """Preconditions of the device cases: the long rows of the statistics fixture give tasks with seg >= 1 (two and
    three segments), every tail class is present, and the many-row fixture gives more than 1024 tasks (more than 256
    partials: the strided part of the final reduction)."""
    lens = ref.stats_lens(k)
    assert max(lens) < ref.STATS_NCOLS
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    t = layout.build_row_tasks(indptr)
    segs = t.tasks[:, 1]
    assert segs.max() == 2 and np.count_nonzero(segs >= 1) == 4 and t.long_rows.shape[0] == 3
    assert {l % 4 for l in lens if l} == {0, 1, 2, 3} and {0, 1, 63} <= {l % 64 for l in lens}
    assert layout.SPLIT_CHUNK == 4096 and {4095, 4096, 4097} <= set(lens)
    many = ref.many_lens()
    nonempty = sum(1 for l in many if l)
    assert nonempty >= 1100 and 0 in many
    tm = layout.build_row_tasks(np.concatenate([[0], np.cumsum(many)]).astype(np.int64))
    assert tm.tasks.shape[0] == nonempty > 1024 and (tm.tasks.shape[0] + 3) // 4 > 256


def test_sum_fixtures_reach_the_tails_and_the_block_cap():
    assert {n & 3 for n in ref.SUMSQ_NS} == {0, 1, 2, 3}
    assert (max(ref.SUMSQ_NS) // 4 + 255) // 256 > ref.SUMSQ_BLOCKS and max(ref.SUMSQ_NS) & 3 == 3
    assert (max(ref.SUM_PAIRS_NS) + 255) // 256 > ref.SUMSQ_BLOCKS
    for lengths in ref.HISTORY_LENGTHS:
        assert len(lengths) == 4
    assert {n % 4 for n in ref.HISTORY_LENGTHS[0]} | {n % 4 for n in ref.HISTORY_LENGTHS[1]} == {0, 1, 2, 3}
    assert {n % 4 for n in ref.HISTORY_LENGTHS[1]} == {0, 1, 2, 3}
    assert 0 in ref.HISTORY_LENGTHS[0] and (ref.HISTORY_LENGTHS[0][0] // 4 + 255) // 256 > ref.SUMSQ_BLOCKS
    assert ref.HISTORY_LENGTHS[0][2:] == (301, 502)
