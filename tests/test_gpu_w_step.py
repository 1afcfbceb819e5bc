"""T3b (GPU): the kernels of csrc/w_step.hip on inputs of their own - als_w_normal_equations phase 0 (k_w_item_vectors,
k_w_item_vectors_f64, gsym_matmul16), phase 1 (k_w_accumulate<KB, float / double>, k_w_reduce) and als_item_stats /
als_item_stats_f64 - against the fp64 / long double reference of tests/w_step_ref.py (validated on the CPU by
tests/test_w_step_ref_cpu.py).  Calls go through ctypes with _hip.WParams filled in here, so that the test decides
nchunks, the shard and the H plane; one case goes through HipBackend.w_item_vectors / w_accumulate unchanged.

Exact inputs (small integers) are compared for equality: any indexing, layout, compaction or tile error fails them.
Real inputs are held to worst-case rounding bounds against the absolute-sum companion S of each value, with
u32 = 2^-24, u64 = 2^-53, KP = padded k, D = feature columns, m = items of the shard:
  phase 0         |dH| <= (KP + D + 4) u S_H + u |H|         u = u32 (fp32 by-products) / u64 (f64)
  phase 1, B      |dB| <= (m + 2) u64 S_B                     (B from the H the device wrote: each phase on its own)
  phase 1, A      |dA| <= (m + 2) u64 S_A                     + u32 S_A in fp32 mode (its weight x_ia x_ia' is an fp32 product)
  statistics      |ds| <= (KP + 4) u S_s + u32 |s|           (the float store)
(m + 2: one rounding of a product, at most per - 1 additions inside a chunk and nchunks across, per + nchunks <= m + 1.)
These bounds cannot fail for a correct kernel.  Under ALS_RECORD_MARGINS=<file> every real-input test records its
observed error / bound ratios per k and mode (to be kept as profiles/w_step_kernel_test_margins.json); the bounds
are derived and are not to be replaced by figures tuned to those ratios.
"""
import ctypes as C

import numpy as np
import pytest

from tests import w_step_ref as ref
from tests.gpu_common import env as gpu_env, ptr, ratio, record_margins, same_bits, upload

pytestmark = pytest.mark.gpu

KS = sorted(ref.CASES)
U32, U64 = ref.U32, ref.U64


def _twin_scale(torch, dev, ld, dtype, s):
    """[ld, ld] factors: s on the strictly upper triangle of every diagonal 16x16 block, 1 elsewhere."""
    r = torch.arange(ld, device=dev)
    m = ((r[:, None] // 16) == (r[None, :] // 16)) & (r[:, None] < r[None, :])
    return torch.where(m, torch.tensor(s, dtype=dtype, device=dev), torch.tensor(1.0, dtype=dtype, device=dev))


def _run(env, inp, twin=1.0, wrapper=False):
    """Phase 0, phase 1 on feature inp.feat and the item statistics on the device; every output buffer starts as
    NaN (7 for the statistics), the H plane has 3 rows more than there are items."""
    torch, _, _, _, be, dev = env
    from collaborative_filtering_amd import _hip
    lib = be.lib
    k, ld, n, f64 = inp.k, inp.ld, inp.n, inp.f64
    dt = torch.float64 if f64 else torch.float32
    up = lambda a: upload(a, dev)       # noqa: E731
    gram = up(inp.gram)
    if twin != 1.0:
        gram = gram * _twin_scale(torch, dev, ld, dt, twin)
    rhs, colsum, V, Z = up(inp.rhs), up(inp.colsum), up(inp.V), up(inp.Z)
    b_new, b_old, X, W, feat_off = up(inp.b_new), up(inp.b_old), up(inp.X), up(inp.W), up(inp.feat_off)
    sumr, sumr2, indptr = up(inp.sumr), up(inp.sumr2), up(inp.indptr)
    nrows_h = n if wrapper else n + 3
    H = torch.full((inp.nfeat, nrows_h, ld), float("nan"), dtype=dt, device=dev)
    d, c0 = inp.dims[inp.feat], int(inp.feat_off[inp.feat])
    if wrapper:
        kw = {"f64": True} if f64 else {}
        be.w_item_vectors(k=k, ld=ld, item_begin=inp.ib, item_end=inp.ie, gram=gram, rhs=rhs, colsum=colsum, V=V,
                          b_new=b_new, b_old=b_old, X=X, feat_off=feat_off, W=W, H=H, **kw)
        A, B = be.w_accumulate(k=k, ld=ld, item_begin=inp.ib, item_end=inp.ie, gram=gram, X=X, H=H,
                               feat_index=inp.feat, feat_col0=c0, feat_d=d, **kw)
    else:
        p = _hip.WParams()
        p.k, p.ld, p.phase, p.nfeat, p.f64 = k, ld, 0, inp.nfeat, int(f64)
        p.item_begin, p.item_end = inp.ib, inp.ie
        p.gram, p.rhs, p.colsum, p.V, p.b_new, p.b_old = ptr(gram), ptr(rhs), ptr(colsum), ptr(V), ptr(b_new), ptr(b_old)
        p.D, p.X, p.feat_off, p.W, p.H, p.nrows_h = inp.D, ptr(X), ptr(feat_off), ptr(W), ptr(H), nrows_h
        st = be._stream()
        assert lib.als_w_normal_equations(C.byref(p), st) == 0
        npairs, kb, nch = d * (d + 1) // 2, ld // 16, inp.nchunks
        nan64 = lambda *s: torch.full(s, float("nan"), dtype=torch.float64, device=dev)      # noqa: E731
        partA, partB = nan64(npairs * nch * (kb * (kb + 1) // 2) * 256), nan64(d * nch * ld)
        A, B = nan64(d * k, d * k), nan64(d * k)
        p.phase, p.feat_index, p.feat_col0, p.feat_d, p.nchunks = 1, inp.feat, c0, d, nch
        p.partA, p.partB, p.A_out, p.B_out = ptr(partA), ptr(partB), ptr(A), ptr(B)
        assert lib.als_w_normal_equations(C.byref(p), st) == 0
    stat = torch.full((n, 2), 7.0, dtype=torch.float32, device=dev)
    be.item_stats(k=k, ld=ld, item_begin=inp.ib, item_end=inp.ie, gram=gram, rhs=rhs, colsum=colsum, sumr=sumr,
                  sumr2=sumr2, indptr=indptr, Z=Z, b_new=b_new, b_old=b_old, stat_out=stat, f64=f64)
    torch.cuda.synchronize()
    return dict(H=H.cpu().numpy(), A=A.cpu(), B=B.cpu().numpy(), stat=stat.cpu().numpy())


def _untouched_outside(inp, out):
    o = np.ones(inp.n, dtype=bool)
    o[inp.ib:inp.ie] = False
    assert np.isnan(out["H"][:, : inp.n][:, o]).all() and np.isnan(out["H"][:, inp.n:]).all()
    assert np.all(out["stat"][o] == 7.0)


def _disjoint_blocks_are_zero(inp, A):
    d, c0, k = inp.dims[inp.feat], int(inp.feat_off[inp.feat]), inp.k
    Xs = inp.X[inp.ib:inp.ie, c0:c0 + d]
    A = A.numpy()
    for a in range(d):
        for a2 in range(a + 1, d):
            if not (Xs[:, a] * Xs[:, a2]).any():
                assert not A[a * k:(a + 1) * k, a2 * k:(a2 + 1) * k].any()
                assert not A[a2 * k:(a2 + 1) * k, a * k:(a + 1) * k].any()


def _check_exact(env, inp, out):
    torch = env[0]
    sl = slice(inp.ib, inp.ie)
    H, _ = ref.expected_h(inp)
    assert np.array_equal(out["H"][:, sl], H[:, sl])
    _untouched_outside(inp, out)
    A, _, B, _ = ref.expected_ab(inp, out["H"][inp.feat])
    assert np.array_equal(out["A"].numpy(), A) and np.array_equal(out["B"], B)
    assert torch.equal(out["A"], out["A"].T)
    _disjoint_blocks_are_zero(inp, out["A"])
    stat, _ = ref.expected_stats(inp)
    assert np.array_equal(out["stat"][sl], stat[sl].astype(np.float32))


def _check_real(env, inp, out, key):
    torch = env[0]
    sl = slice(inp.ib, inp.ie)
    m, KP, D = inp.ie - inp.ib, inp.ld, inp.D
    u = U64 if inp.f64 else U32
    wide = inp.f64                                   # long double reference where the kernel works in fp64
    ratios = {}
    H, S = ref.expected_h(inp, wide=wide)
    ratios["H"] = ratio(out["H"][:, sl], H[:, sl], (KP + D + 4) * u * S[:, sl] + u * np.abs(H[:, sl]), "H")
    d = inp.dims[inp.feat]
    A, SA, B, SB = ref.expected_ab(inp, out["H"][inp.feat], wide=wide and m * d * d * inp.k * inp.k <= 1e8)
    ratios["B"] = ratio(out["B"], B, (m + 2) * U64 * SB, "B")
    ratios["A"] = ratio(out["A"].numpy(), A, ((m + 2) * U64 + (0.0 if inp.f64 else U32)) * SA, "A")
    stat, Ss = ref.expected_stats(inp, wide=wide)
    ratios["stat"] = ratio(out["stat"][sl], stat[sl], (KP + 4) * u * Ss[sl] + U32 * np.abs(stat[sl]), "stat")
    print(key, ratios)
    record_margins(key, ratios)
    # worst-case bounds (module docstring), derived, not tuned; the observed error / bound of every quantity goes to the
    # ALS_RECORD_MARGINS file (profiles/w_step_kernel_test_margins.json once recorded on the device)
    assert all(r <= 1.0 for r in ratios.values()), ratios
    assert torch.equal(out["A"], out["A"].T)
    _disjoint_blocks_are_zero(inp, out["A"])
    _untouched_outside(inp, out)


@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_w_step_exact_inputs(k, f64):
    """Integer inputs: H, A, B equal the exact values, the statistics their float rounding; A bitwise symmetric."""
    env = gpu_env()
    inp = ref.build_inputs(k=k, kind="exact", f64=f64, seed=k, **ref.CASES[k])
    _check_exact(env, inp, _run(env, inp))


@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_w_step_real_inputs(k, f64):
    """Real inputs within the derived bounds, and the lower-twin rule: with the upper triangle of every diagonal
    Gram block scaled by 1.5 every output keeps every bit."""
    env = gpu_env()
    inp = ref.build_inputs(k=k, kind="real", f64=f64, seed=1000 + k, **ref.CASES[k])
    out = _run(env, inp)
    out15 = _run(env, inp, twin=1.5)
    for name in ("H", "A", "B", "stat"):
        assert same_bits(out[name], out15[name]), f"{name} depends on the upper twin of a diagonal block"
    _check_real(env, inp, out, f"w_step k={k} {'f64' if f64 else 'f32'}")


@pytest.mark.parametrize("f64", [0, 1])
@pytest.mark.parametrize("kind", ["exact", "real"])
@pytest.mark.parametrize("case", sorted(ref.EXTRA_CASES))
def test_w_step_extra_cases(case, kind, f64):
    """A shard whose last chunk is empty, and the path through HipBackend.w_item_vectors / w_accumulate with the
    wrapper's own chunking (d = 20, 4900 items: 19 chunks of 258)."""
    env = gpu_env()
    cfg = ref.EXTRA_CASES[case]
    inp = ref.build_inputs(kind=kind, f64=f64, seed=77, **cfg)
    out = _run(env, inp, wrapper=(case == "wrapper"))
    if kind == "exact":
        _check_exact(env, inp, out)
    else:
        _check_real(env, inp, out, f"w_step {case} {'f64' if f64 else 'f32'}")


def test_w_step_bad_arguments_are_rejected():
    """Every argument check of als_w_normal_equations and of both statistics entry points returns before any launch
    (the pointers below are not device memory); an empty item range is a no-op."""
    torch, _, _, _, be, dev = gpu_env()
    from collaborative_filtering_amd import _hip
    lib = be.lib
    BADARG, BADK = -1, -2
    fake = C.c_void_p(64)

    def params(phase, **kw):
        p = _hip.WParams()
        p.k, p.ld, p.phase, p.nfeat, p.D = 50, 64, phase, 2, 5
        p.item_begin, p.item_end, p.nrows_h = 0, 10, 10
        for name in ("gram", "rhs", "colsum", "V", "b_new", "b_old", "X", "feat_off", "W", "H", "partA", "partB",
                     "A_out", "B_out"):
            setattr(p, name, fake)
        p.feat_index, p.feat_col0, p.feat_d, p.nchunks = 1, 2, 3, 2
        for name, v in kw.items():
            setattr(p, name, v)
        return p

    call = lambda p: lib.als_w_normal_equations(C.byref(p), None)       # noqa: E731
    assert lib.als_w_normal_equations(None, None) == BADARG
    assert call(params(2)) == BADARG
    assert call(params(0, nfeat=0)) == BADARG and call(params(0, nfeat=9)) == BADARG
    assert call(params(1, feat_col0=3)) == BADARG                       # 3 + 3 > D = 5
    assert call(params(1, nchunks=0)) == BADARG
    assert call(params(0, ld=48)) == BADARG and call(params(1, ld=80)) == BADARG
    assert call(params(0, item_begin=5, item_end=4)) == BADARG and call(params(1, item_begin=5, item_end=4)) == BADARG
    assert call(params(0, gram=None)) == BADARG and call(params(1, gram=None)) == BADARG
    assert call(params(0, k=161, ld=176)) == BADK and call(params(1, k=0, ld=0)) == BADK
    for fn in (lib.als_item_stats, lib.als_item_stats_f64):
        args = [50, 64, 0, 10] + [fake] * 10 + [None]
        bad_ld = list(args)
        bad_ld[1] = 48
        assert fn(*bad_ld) == BADARG
        for j in range(4, 14):                                          # each of the ten pointers
            nul = list(args)
            nul[j] = None
            assert fn(*nul) == BADARG
        assert fn(161, 176, 0, 10, *([fake] * 10), None) == BADK
        rev = list(args)
        rev[2], rev[3] = 5, 4
        assert fn(*rev) == BADARG
    # empty item range: 0, and nothing is written
    inp = ref.build_inputs(kind="exact", f64=False, seed=1, **ref.EXTRA_CASES["short"])
    inp.ie = inp.ib
    out = _run((torch, None, None, None, be, dev), inp)
    assert np.isnan(out["H"]).all() and np.isnan(out["A"].numpy()).all() and np.isnan(out["B"]).all()
    assert np.all(out["stat"] == 7.0)
    for f64 in (False, True):
        stat = torch.full((4, 2), 7.0, dtype=torch.float32, device=dev)
        fn = lib.als_item_stats_f64 if f64 else lib.als_item_stats
        assert fn(50, 64, 3, 3, *([ptr(stat)] * 10), None) == 0
        torch.cuda.synchronize()
        assert bool((stat == 7.0).all())
