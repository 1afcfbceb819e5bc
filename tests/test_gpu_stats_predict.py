"""T3c (GPU): the prediction, statistics and factor-scale kernels on inputs of their own - als_predict_dense,
als_predict_at, als_compose_z (csrc/predict.hip), als_residual_stats, als_sumsq, als_sum_pairs, als_history_row
(csrc/stats.hip), als_factor_scale (csrc/row_solve.hip) - against tests/stats_predict_ref.py (validated on the CPU by
tests/test_stats_predict_ref_cpu.py).  Calls go through ctypes, so that the test owns every buffer: each output starts
from a sentinel and carries 64 sentinel elements behind its used part, which must be unchanged afterwards; inputs whose
length matters carry NaNs behind their end.

Widths: k in {1, 17, 33, 50, 65, 81, 100, 113, 129, 160}, one per template instance KB = ld / 16 = 1 ... 10.

Exact inputs (small integers, multiples of 1/8) are compared for EQUALITY.  For the predictions the dot product is exact
and the epilogue is not: the expected float is ((dot + float32(mu)) + b_u) + b_i rounded step by step, the association
walk::score promises, on biases chosen so that another association (or a mu added in double) gives another float on
most entries.

Real inputs are held to worst-case rounding bounds against the absolute-sum companion S of each value, u32 = 2^-24,
u64 = 2^-53, ld = padded k:
  prediction     |dp| <= (ld + 3) u32 S,  S = sum |u_j z_j| + |mu| + |b_u| + |b_i|.  A term of the dot product is rounded
                 once as a product (not at all under fma) and passes through at most ld - 1 fp32 additions whatever the
                 order (lanes, shuffles, MFMA chain); the epilogue adds three more roundings: ld + 3 in all.
  compose_z      |dz| <= D u32 S + u32 |z|,  S = |v| + sum |x_a w_a|: D fused multiply-adds, then the stored float.
                 D = 0 is a copy: equality.
  residual_stats per rating e_r = (ld + 3) u32 S_r (S_r includes |r|: the same ld + 3 roundings), then
                 |d sum d|   <= sum e_r + nnz u64 sum (|d_r| + e_r)
                 |d sum d^2| <= sum e_r (2 |d_r| + e_r) + (nnz + 1) u64 sum (|d_r| + e_r)^2
                 (float -> double is exact; the fp64 square rounds once; at most nnz - 1 fp64 additions in any order).
  sumsq          |ds| <= n u64 sum x^2 (the product of two floats is exact in double; at most n - 1 additions);
  sum_pairs      |ds| <= npairs u64 sum |x| per column.
These bounds cannot fail for a correct kernel.  Under ALS_RECORD_MARGINS=<file> every real-input test records its worst
observed error / bound ratio per k (kept as profiles/stats_predict_kernel_test_margins.json); the bounds are derived
and are not to be replaced by figures tuned to those ratios.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import stats_predict_ref as ref
from tests.gpu_common import env, ptr, ratio, record_margins, same_bits, upload

pytestmark = pytest.mark.gpu

GUARD = ref.SENTINEL_ELEMS
BADARG, BADK = -1, -2
U32, U64 = ref.U32, ref.U64


@functools.lru_cache(maxsize=None)
def _E():
    return env()


def _up(a):
    return upload(a, _E().dev)


def _up_tail(a):
    """a on the device with 16 NaNs behind it (a read past the end poisons the result; never a null pointer)."""
    return _up(np.concatenate([np.asarray(a, dtype=np.float32), np.full(16, np.nan, dtype=np.float32)]))


def _f64(*v):
    torch, dev = _E()[0], _E()[5]
    return torch.tensor(list(v), dtype=torch.float64, device=dev)


class _Out:
    """An output buffer of n elements that starts from a sentinel, with GUARD sentinel elements behind it."""

    def __init__(self, n, dtype="float32", sentinel=-777.25):
        torch, dev = _E()[0], _E()[5]
        self.n, self.sentinel = int(n), sentinel
        self.buf = torch.full((self.n + GUARD,), sentinel, dtype=getattr(torch, dtype), device=dev)

    @property
    def ptr(self):
        return ptr(self.buf)

    def get(self):
        """The used part as numpy, after checking that nothing behind it was written."""
        host = self.buf.cpu().numpy()
        assert np.all(host[self.n:] == self.sentinel), "written past the end of the output"
        return host[: self.n]

    def untouched(self):
        return bool(np.all(self.buf.cpu().numpy() == self.sentinel))


def _sync():
    _E()[0].cuda.synchronize()


# ---- predictions -----------------------------------------------------------------------------------------------------
def _predict_dev(inp):
    return dict(U=_up(inp.U), Z=_up(inp.Z), b_u=_up(inp.b_u), b_i=_up(inp.b_i), mu=_f64(inp.mu))


def _dense(inp, d, m, n):
    """als_predict_dense on the first m users and n items of inp."""
    be = _E()[4]
    out = _Out(m * n)
    rc = be.lib.als_predict_dense(inp.k, inp.ld, m, n, ptr(d["U"]), ptr(d["Z"]), ptr(d["b_u"]), ptr(d["b_i"]),
                                  ptr(d["mu"]), out.ptr, be._stream())
    assert rc == 0
    _sync()
    return out.get().reshape(m, n)


def _at(inp, d, us, is_):
    be = _E()[4]
    out = _Out(us.size)
    us_d, is_d = _up(us), _up(is_)                      # (held until the call has run)
    rc = be.lib.als_predict_at(inp.k, inp.ld, us.size, ptr(us_d), ptr(is_d), ptr(d["U"]), ptr(d["Z"]),
                               ptr(d["b_u"]), ptr(d["b_i"]), ptr(d["mu"]), out.ptr, be._stream())
    assert rc == 0
    _sync()
    return out.get()


@pytest.mark.parametrize("k", ref.KS)
def test_predict_dense_exact_every_width(k):
    """m = 17, n = 257 (a second row block of one row, a second workgroup of one column): bitwise the float32
    expectation, on the association-sensitive biases and with a mu that carries digits beyond float32."""
    for biases, mu in (("tied", None), ("mixed", ref.MU_EXTRA)):
        inp = ref.predict_inputs(k, 17, 257, "exact", seed=k, mu=mu, biases=biases)
        got = _dense(inp, _predict_dev(inp), inp.m, inp.n)
        exp = ref.expected_predict_exact(inp)
        assert np.array_equal(got, exp), (biases, int(np.count_nonzero(got != exp)))


@pytest.mark.parametrize("k", ref.DENSE_SHAPE_KS)
def test_predict_dense_exact_tile_edges(k):
    """Every m x n around the 16-row block, the 16-column tile, the 64-column wave and the 256-column workgroup."""
    M, N = max(ref.DENSE_MS), max(ref.DENSE_NS)
    inp = ref.predict_inputs(k, M, N, "exact", seed=7 * k, mu=ref.MU_EXTRA if k == 128 else None, biases="mixed")
    d = _predict_dev(inp)
    exp = ref.expected_predict_exact(inp)
    for m in ref.DENSE_MS:
        for n in ref.DENSE_NS:
            got = _dense(inp, d, m, n)
            assert np.array_equal(got, exp[:m, :n]), (m, n)


@pytest.mark.parametrize("k", ref.KS)
def test_predict_at_exact_every_width(k):
    """Pairs with repeats and the four corners, every tail npairs % 4, one pair, and a list long enough for a second
    pass of the grid-stride loop: bitwise the expectation and therefore what als_predict_dense writes."""
    inp = ref.predict_inputs(k, 33, 300, "exact", seed=100 + k)
    d = _predict_dev(inp)
    exp = ref.expected_predict_exact(inp)
    assert np.array_equal(_dense(inp, d, inp.m, inp.n), exp)
    for npairs in ref.AT_NPAIRS:
        us, is_ = ref.predict_pairs(inp.m, inp.n, npairs, seed=npairs)
        got = _at(inp, d, us, is_)
        assert np.array_equal(got, exp[us, is_]), npairs


def test_predict_at_without_pairs_is_a_no_op():
    inp = ref.predict_inputs(50, 5, 7, "exact", seed=1)
    d = _predict_dev(inp)
    be = _E()[4]
    out = _Out(4)
    idx = _up(np.zeros(4, np.int32))
    args = (ptr(d["U"]), ptr(d["Z"]), ptr(d["b_u"]), ptr(d["b_i"]), ptr(d["mu"]))
    assert be.lib.als_predict_at(inp.k, inp.ld, 0, ptr(idx), ptr(idx), *args, out.ptr, be._stream()) == 0
    assert be.lib.als_predict_at(inp.k, inp.ld, 0, None, None, *args, None, be._stream()) == 0
    _sync()
    assert out.untouched()


@pytest.mark.parametrize("k", ref.KS)
def test_predictions_real_inputs_within_the_derived_bound(k):
    inp = ref.predict_inputs(k, 33, 300, "real", seed=200 + k)
    d = _predict_dev(inp)
    P, S = ref.expected_predict_real(inp)
    bound = (inp.ld + 3) * U32 * S
    us, is_ = np.divmod(np.arange(inp.m * inp.n), inp.n)
    ratios = {"dense": ratio(_dense(inp, d, inp.m, inp.n), P, bound, "dense"),
              "at": ratio(_at(inp, d, us.astype(np.int32), is_.astype(np.int32)).reshape(inp.m, inp.n), P, bound, "at")}
    print(f"predict k={k}", ratios)
    record_margins(f"predict k={k}", ratios)
    assert all(r <= 1.0 for r in ratios.values()), ratios


# ---- als_compose_z ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", ref.COMPOSE_KS)
def test_compose_z(k):
    """D = 0 (X and W null: a copy), 1 and 7; n = 1, 5, 300: exact inputs equal, padding columns exactly zero; real
    inputs within D u32 S + u32 |z|."""
    be = _E()[4]
    worst = 0.0
    for D in ref.COMPOSE_DS:
        for n in ref.COMPOSE_NS:
            for kind in ("exact", "real"):
                inp = ref.compose_inputs(k, n, D, kind, seed=1000 * D + n + k)
                Z = _Out(n * inp.ld)
                V, X, W = _up(inp.V), (_up(inp.X) if D else None), (_up(inp.W) if D else None)
                rc = be.lib.als_compose_z(n, inp.ld, D, ptr(V), ptr(X), ptr(W), Z.ptr, be._stream())
                assert rc == 0
                _sync()
                got = Z.get().reshape(n, inp.ld)
                exp, S = ref.expected_compose(inp)
                assert not got[:, k:].any()
                if kind == "exact" or D == 0:
                    assert np.array_equal(got, exp.astype(np.float32)), (D, n, kind)
                else:
                    worst = max(worst, ratio(got, exp, D * U32 * S + U32 * np.abs(exp), f"compose D={D} n={n}"))
    print(f"compose_z k={k}", worst)
    record_margins(f"compose_z k={k}", {"Z": worst})
    assert worst <= 1.0


# ---- als_residual_stats ----------------------------------------------------------------------------------------------
def _stats_dev(inp):
    layout = _E()[1]
    t = layout.build_row_tasks(inp.indptr)
    return dict(indptr=_up(inp.indptr), indices=_up(inp.indices), vals=_up(inp.vals), U=_up(inp.U), Z=_up(inp.Z),
                b_u=_up(inp.b_u), b_i=_up(inp.b_i), mu=_f64(inp.mu), tasks=_up(t.tasks), ntasks=int(t.tasks.shape[0]))


def _stats(inp, d):
    """(out [2], partials) of one als_residual_stats call on fresh sentinel buffers."""
    be = _E()[4]
    nblk = (d["ntasks"] + 3) // 4
    partials, out = _Out(2 * nblk, "float64"), _Out(2, "float64")
    rc = be.lib.als_residual_stats(inp.k, inp.ld, ptr(d["indptr"]), ptr(d["indices"]), ptr(d["vals"]), ptr(d["U"]),
                                   ptr(d["Z"]), ptr(d["b_u"]), ptr(d["b_i"]), ptr(d["mu"]), ptr(d["tasks"]),
                                   d["ntasks"], partials.ptr, out.ptr, be._stream())
    assert rc == 0
    _sync()
    return out.get().copy(), partials.get().copy()


def _check_stats(inp, key):
    d = _stats_dev(inp)
    got, part = _stats(inp, d)
    again, part2 = _stats(inp, d)
    assert same_bits(got, again) and same_bits(part, part2), "not reproducible"
    s0, s1, b0, b1 = ref.expected_stats(inp)
    if inp.kind == "exact":
        assert got[0] == s0 and got[1] == s1, (got, s0, s1)
        return
    ratios = {"sum_d": float(abs(got[0] - s0) / b0), "sum_d2": float(abs(got[1] - s1) / b1)}
    print(key, ratios)
    record_margins(key, ratios)
    assert all(r <= 1.0 for r in ratios.values()), (ratios, got, s0, s1)


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("k", ref.KS)
def test_residual_stats_every_width_and_row_class(k, kind):
    """Rows that are empty, of every tail len % 4 and len % 64, of 4095 / 4096 / 4097 ratings and of two and three
    segments (t.seg > 0): exact inputs give the exact sums, real inputs stay within the derived bound, and a second call
    on fresh buffers repeats every bit."""
    inp = ref.stats_inputs(k, kind, ref.stats_lens(k), ref.STATS_NCOLS, seed=300 + k)
    _check_stats(inp, f"residual_stats k={k}")


@pytest.mark.parametrize("kind", ["exact", "real"])
def test_residual_stats_many_short_rows(kind):
    """More than 1024 tasks: more than 256 partials, so the strided part of the final reduction runs."""
    inp = ref.stats_inputs(50, kind, ref.many_lens(), ref.MANY_NCOLS, seed=11)
    _check_stats(inp, "residual_stats many rows k=50")


# ---- als_sumsq / als_sum_pairs ---------------------------------------------------------------------------------------
def _sumsq(x_dev, n):
    be = _E()[4]
    partials, out = _Out(be.lib.als_sumsq_partials(), "float64"), _Out(1, "float64")
    assert be.lib.als_sumsq(ptr(x_dev), n, partials.ptr, out.ptr, be._stream()) == 0
    _sync()
    partials.get()
    return out.get()[0]


def _sum_pairs(x_dev, npairs):
    be = _E()[4]
    partials, out = _Out(2 * be.lib.als_sumsq_partials(), "float64"), _Out(2, "float64")
    assert be.lib.als_sum_pairs(ptr(x_dev), npairs, partials.ptr, out.ptr, be._stream()) == 0
    _sync()
    partials.get()
    return out.get().copy()


def test_sumsq_tails_and_block_cap():
    worst = 0.0
    for n in ref.SUMSQ_NS:
        rng = np.random.default_rng(n)
        x = ref.exact_vector(rng, n)
        assert _sumsq(_up_tail(x), n) == float(ref.expected_sumsq(x)[1]), n
        x = ref.real_vector(rng, n)
        s, _ = ref.expected_sumsq(x)
        got = _sumsq(_up_tail(x), n)
        if n == 0:
            assert got == 0.0
        else:
            worst = max(worst, abs(got - s) / (n * U64 * s))
    print("sumsq", worst)
    record_margins("sumsq", {"sumsq": worst})
    assert worst <= 1.0


def test_sum_pairs_tails_and_block_cap():
    worst = 0.0
    for npairs in ref.SUM_PAIRS_NS:
        rng = np.random.default_rng(npairs)
        x = ref.eighths(rng, 2 * npairs)
        assert np.array_equal(_sum_pairs(_up_tail(x), npairs), ref.expected_sum_pairs(x)[0]), npairs
        x = ref.real_vector(rng, 2 * npairs)
        s, a = ref.expected_sum_pairs(x)
        got = _sum_pairs(_up_tail(x), npairs)
        if npairs == 0:
            assert not got.any()
        else:
            worst = max(worst, float(np.max(np.abs(got - s) / (npairs * U64 * a))))
    print("sum_pairs", worst)
    record_margins("sum_pairs", {"sum_pairs": worst})
    assert worst <= 1.0


# ---- als_history_row -------------------------------------------------------------------------------------------------
def _history(arrays_dev, lengths, stats, nnz, mu):
    be = _E()[4]
    partials, row, mu_t = _Out(4 * be.lib.als_sumsq_partials(), "float64"), _Out(6, "float64"), _Out(1, "float64")
    mu_t.buf[:1] = mu
    stats_d = _f64(*stats)
    args = []
    for x, n in zip(arrays_dev, lengths):
        args += [ptr(x), n]
    assert be.lib.als_history_row(*args, ptr(stats_d), nnz, mu_t.ptr, partials.ptr, row.ptr, be._stream()) == 0
    _sync()
    partials.get()
    return row.get().copy(), mu_t.get()[0]


@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", range(len(ref.HISTORY_LENGTHS)))
def test_history_row(case, kind):
    """Array lengths of every residue mod 4, one above the block cap and one empty: the RMSE, the new mu and row[5]
    are the host's fp64 operations bit for bit; every norm is sqrt of what als_sumsq returns for that array (the two
    paths of the engine agree), and on integer inputs sqrt of the exact sum; no ratings give a NaN RMSE."""
    lengths = ref.HISTORY_LENGTHS[case]
    rng = np.random.default_rng(40 + case)
    arrays = [(ref.exact_vector if kind == "exact" else ref.real_vector)(rng, n) for n in lengths]
    dev = [_up_tail(x) for x in arrays]
    norms = [np.sqrt(np.float64(_sumsq(x, n))) for x, n in zip(dev, lengths)]
    if kind == "exact":
        assert norms == [np.sqrt(np.float64(ref.expected_sumsq(x)[1])) for x in arrays]
    for stats, nnz, mu in (((-37.4321, 912.123), 1001, 3.3), ((5.0, 1.0), 7, -0.1), ((0.0, 0.0), 0, 1.5), ((2.0, 5.0), 0, 1.5)):
        row, mu_new = _history(dev, lengths, stats, nnz, mu)
        rmse, m = ref.expected_history_scalars(stats, nnz, mu)
        if nnz == 0:
            assert np.isnan(row[0]) and np.isnan(rmse)
        else:
            assert row[0] == rmse
        if np.isnan(m):
            assert np.isnan(row[5]) and np.isnan(mu_new)
        else:
            assert row[5] == m and mu_new == m, (row[5], mu_new, m)
        assert [row[1 + j] for j in range(4)] == norms, (row, norms)


# ---- als_factor_scale ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfloats", ref.SCALE_NFLOATS)
def test_factor_scale(nfloats):
    """max|F| at the first and the last element and in every unrolled slot of the loop's final trip, for every kind of
    maximum: scale[0 .. 1] bitwise the reference, the two work words zero again after every call - all calls reuse the
    same four words without re-zeroing - and nothing written behind them."""
    torch, dev, be = _E()[0], _E()[5], _E()[4]
    rng = np.random.default_rng(nfloats)
    sc = _Out(4, "float32")
    sc.buf[:4] = 0.0
    positions = ref.scale_positions(nfloats)

    def call(F_dev, F_host):
        assert be.lib.als_factor_scale(ptr(F_dev), nfloats, sc.ptr, be._stream()) == 0
        _sync()
        got = sc.get()
        assert not got[2:4].view(np.int32).any(), "work words not reset"
        s0, s1 = ref.expected_scale(F_host)
        assert got[0] == s0 and got[1] == s1, (got[:2], s0, s1)

    for name, v in ref.scale_values().items():
        host = ref.scale_background(rng, nfloats, v)
        F = _up_tail(host)
        if not positions or name == "zero":
            call(F, host)
            continue
        vt = _up(np.array([v], dtype=np.float32))
        for p in positions:
            keep = host[p]
            host[p] = v
            F[p:p + 1].copy_(vt)
            call(F, host)
            host[p] = keep
            F[p:p + 1].copy_(_up(np.array([keep], dtype=np.float32)))
        call(F, host)                                   # the background alone: another F on the same four words


# ---- rejected arguments ----------------------------------------------------------------------------------------------
def test_bad_arguments_are_rejected_before_any_launch():
    """Unaligned x, nfloats % 4 != 0, negative counts, ld != als_padded_k(k), k = 161: the documented status, and no
    output is written."""
    be = _E()[4]
    lib = be.lib
    x = _up(np.ones(1024, dtype=np.float32))
    idx = _up(np.zeros(16, dtype=np.int32))
    ptr64 = _up(np.zeros(16, dtype=np.int64))
    p, off4 = ptr(x), C.c_void_p(x.data_ptr() + 4)
    outs = [_Out(64, "float64") for _ in range(3)]
    o0, o1, o2 = (o.ptr for o in outs)
    fo = _Out(64)
    mu = _f64(3.0)
    assert lib.als_sumsq(off4, 8, o0, o1, None) == BADARG and lib.als_sumsq(p, -1, o0, o1, None) == BADARG
    assert lib.als_sum_pairs(off4, 8, o0, o1, None) == BADARG and lib.als_sum_pairs(p, -1, o0, o1, None) == BADARG
    for bad in (1, 2, 3, 7, -4):
        assert lib.als_factor_scale(p, bad, fo.ptr, None) == BADARG
    assert lib.als_factor_scale(off4, 8, fo.ptr, None) == BADARG
    pa = lambda k, ld, npairs: lib.als_predict_at(k, ld, npairs, ptr(idx), ptr(idx), p, p, p, p, ptr(mu), fo.ptr, None)  # noqa: E731
    assert pa(50, 48, 4) == BADARG and pa(50, 80, 4) == BADARG and pa(161, 176, 4) == BADK and pa(0, 0, 4) == BADK
    assert pa(50, 64, -1) == BADARG
    pd = lambda k, ld, m, n: lib.als_predict_dense(k, ld, m, n, p, p, p, p, ptr(mu), fo.ptr, None)  # noqa: E731
    assert pd(50, 48, 2, 2) == BADARG and pd(161, 176, 2, 2) == BADK
    assert pd(50, 64, -1, 2) == BADARG and pd(50, 64, 2, -1) == BADARG and pd(50, 64, 0, 2) == BADARG
    rs = lambda k, ld, nt: lib.als_residual_stats(k, ld, ptr(ptr64), ptr(idx), p, p, p, p, p, ptr(mu), ptr(idx), nt,  # noqa: E731
                                                 o0, o1, None)
    assert rs(50, 48, 1) == BADARG and rs(161, 176, 1) == BADK and rs(50, 64, -1) == BADARG and rs(50, 64, 0) == BADARG
    cz = lambda n, ld, D: lib.als_compose_z(n, ld, D, p, p, p, fo.ptr, None)  # noqa: E731
    assert cz(-1, 16, 1) == BADARG and cz(2, 0, 1) == BADARG and cz(2, 16, -1) == BADARG
    assert lib.als_compose_z(2, 16, 1, p, None, p, fo.ptr, None) == BADARG
    hr = lambda nU, nnz, U=p: lib.als_history_row(U, nU, p, 4, p, 4, p, 4, ptr(mu), nnz, o2, o0, o1, None)  # noqa: E731
    assert hr(-1, 5) == BADARG and hr(4, -1) == BADARG and hr(4, 5, off4) == BADARG
    _sync()
    assert all(o.untouched() for o in outs) and fo.untouched()
