"""K13 (GPU): als_row_inv_norms / als_similar_topk (csrc/similar.hip) and ALS.similar_items / similar_users.

The oracle of the top-N kernel is exact: its dot products are bitwise the fp32 values als_predict_dense writes for
(U = T[q_ids], Z = T, zero biases, mu = 0), so the expected lists are `similar_topn` of tests/similar_ref.py on those
rows and the kernel's own downloaded inverse norms, and all three outputs are compared with ==.  The inverse norms and
the model-level similarities are held to float64 numpy within bounds derived from the number formats (stated where
they are used)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import mmr_ref
from tests import similar_ref as sref
from tests.common import Golden, model_for
from tests.gpu_common import assert_same, env, factors, same_bits, upload


# ------------------------------------------------------------------------------------------------ launches
def _table(layout, n, k, seed, scale=1.0):
    """T fp32 [n, ld], padding columns zero."""
    ld = layout.padded_k(k)
    T = np.zeros((n, ld), np.float32)
    T[:, :k] = np.random.default_rng(seed).normal(scale=scale, size=(n, k))
    return T


def run_inv(torch, be, k, Td):
    """als_row_inv_norms into a buffer that starts from 7 -> device fp32 [rows]."""
    inv = torch.full((Td.shape[0],), 7.0, dtype=torch.float32, device=Td.device)
    be.row_inv_norms(k=k, ld=Td.shape[1], T=Td, inv_norm=inv)
    return inv


def run_similar(torch, be, k, Td, inv, q_ids, self_ids, N, allow=None):
    """als_similar_topk of the rows q_ids of Td against all of Td -> numpy (values, ids, counts).  self_ids: None
    (NULL) or an int array."""
    dev = Td.device
    q = upload(np.asarray(q_ids, np.int32), dev)
    B = q.numel()
    tv = torch.full((B, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((B, N), 7, dtype=torch.int32, device=dev)
    tc = torch.full((B,), 7, dtype=torch.int32, device=dev)
    be.similar_topk(k=k, ld=Td.shape[1], q_ids=q, Q=Td, q_inv=inv,
                    self_ids=None if self_ids is None else upload(np.asarray(self_ids, np.int32), dev),
                    n=Td.shape[0], T=Td, t_inv=inv, allow=allow, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)
    return tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()


def dense_dots(torch, be, k, Td, q_ids):
    """The rows als_predict_dense writes for U = Td[q_ids], Z = Td, zero biases and mu = 0 -> numpy fp32 [B, n]."""
    dev, n = Td.device, Td.shape[0]
    U = Td[upload(np.asarray(q_ids, np.int64), dev)].contiguous()
    out = torch.empty(U.shape[0], n, dtype=torch.float32, device=dev)
    z = lambda r: torch.zeros(r, dtype=torch.float32, device=dev)          # noqa: E731
    be.predict_dense(k=k, ld=Td.shape[1], m=U.shape[0], n=n, U=U, Z=Td, b_u=z(U.shape[0]), b_i=z(n),
                     mu=torch.zeros(1, dtype=torch.float64, device=dev), out=out)
    return out.cpu().numpy()


def oracle(torch, be, k, Td, inv, q_ids, self_ids, N, ok=None):
    q_ids = np.asarray(q_ids)
    inv_h = inv.cpu().numpy()
    return sref.similar_topn(dense_dots(torch, be, k, Td, q_ids), inv_h[q_ids], inv_h, self_ids, ok, N)


def _bitmap(torch, mask, dev):
    """The C ABI's bitmap, packed here with numpy: row j = bit j & 31 of word j >> 5."""
    bits = np.zeros((mask.size + 31) // 32 * 32, np.uint8)
    bits[: mask.size] = mask
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return torch.from_numpy(words.view(np.int32).copy()).to(dev)


# ------------------------------------------------------------------------------------------------ inverse norms
# Bound: the fp64 sum of k exact squares is off by less than k 2^-53 relatively, sqrt and the division add 2^-53 each,
# the single rounding to fp32 2^-24: together below 2^-23.
INV_REL = 2.0 ** -23


@pytest.mark.parametrize("k", [1, 50, 160])
def test_inv_norms_of_many_rows(k):
    torch, layout, be, dev = env().short
    rows = 1000
    T = _table(layout, rows, k, seed=k)
    T[3] = 0.0
    T[5, k - 1] = np.nan
    T[6, 0] = np.inf
    T[7, 0] = -np.inf
    T[10:20] *= np.float32(2.0 ** -60)
    T[20:30] *= np.float32(2.0 ** 60)
    got = run_inv(torch, be, k, upload(T, dev)).cpu().numpy()
    exp = sref.inv_norms(T)
    assert got[3] == 0.0 and not np.signbit(got[3])
    assert np.isnan(got[[5, 6, 7]]).all() and np.isnan(exp[[5, 6, 7]]).all()
    fin = np.isfinite(exp) & (exp != 0)
    assert fin.sum() == rows - 4 and np.isfinite(got[fin]).all()
    rel = np.abs(got[fin].astype(np.float64) - exp[fin]) / exp[fin]
    print(f"k={k}: worst relative error of inv_norm {rel.max():.3e} (bound {INV_REL:.3e})")
    assert rel.max() <= INV_REL
    assert exp[10:20].min() > 2.0 ** 50 and exp[20:30].max() < 2.0 ** -50          # the scaled rows really are extreme


@pytest.mark.parametrize("k", [1, 50, 160])
def test_inv_norm_of_one_row(k):
    torch, layout, be, dev = env().short
    base = _table(layout, 1, k, seed=100 + k)
    for kind in ("normal", "zero", "nan", "tiny", "huge"):
        T = base.copy()
        if kind == "zero":
            T[:] = 0.0
        elif kind == "nan":
            T[0, 0] = np.nan
        elif kind == "tiny":
            T *= np.float32(2.0 ** -60)
        elif kind == "huge":
            T *= np.float32(2.0 ** 60)
        got = float(run_inv(torch, be, k, upload(T, dev)).cpu().numpy()[0])
        exp = float(sref.inv_norms(T)[0])
        if kind == "zero":
            assert got == 0.0
        elif kind == "nan":
            assert np.isnan(got)
        else:
            assert abs(got - exp) / exp <= INV_REL, (kind, got, exp)


# ------------------------------------------------------------------------------------------------ exact oracle
def _special_table(layout, n, k, seed):
    """A normal table with one zero-norm row (3) and one row holding a NaN (7) where n allows."""
    T = _table(layout, n, k, seed)
    if n > 7:
        T[3] = 0.0
        T[7, 0] = np.nan
    return T


@pytest.mark.parametrize("k", [1, 16, 50, 64, 128, 160])
@pytest.mark.parametrize("n", [1, 17, 1000, 4099])
def test_kernel_equals_the_exact_oracle(k, n):
    torch, layout, be, dev = env().short
    Td = upload(_special_table(layout, n, k, seed=10 * k + n), dev)
    inv = run_inv(torch, be, k, Td)
    q = (np.concatenate([np.arange(40), [3, 1, 3, 0]]) % n)[::-1].copy()  # order and duplicates kept
    dots = dense_dots(torch, be, k, Td, q)
    inv_h = inv.cpu().numpy()
    if n > 7:
        assert inv_h[3] == 0 and np.isnan(inv_h[7]) and (q == 3).any() and (q == 7).any()
    for N in (1, 10, 128):
        got = run_similar(torch, be, k, Td, inv, q, q, N)
        exp = sref.similar_topn(dots, inv_h[q], inv_h, q, None, N)
        assert_same(got, exp)
        tv, ti, tc = got
        assert (ti != q[:, None]).all() and not (ti == 7).any() if n > 7 else (tc == 0).all()
        if n > 7:
            b = int(np.nonzero(q == 7)[0][0])
            assert tc[b] == 0 and (ti[b] == -1).all() and np.isneginf(tv[b]).all()   # NaN query: empty list
            b = int(np.nonzero(q == 3)[0][0])
            assert tc[b] == min(N, n - 2) and (tv[b, : tc[b]] == 0).all()            # zero row: 0 to everything
            assert (ti[b, : tc[b]] == np.delete(np.arange(n), [3, 7])[: tc[b]]).all()
        if n <= N:                                                         # padding
            full = tc == min(N, n - 1 - (n > 7))
            assert full[(q != 7) | (n <= 7)].all()
            for b in range(q.size):
                assert (ti[b, tc[b]:] == -1).all() and np.isneginf(tv[b, tc[b]:]).all()


@pytest.mark.parametrize("N", [1, 10, 33, 128])
def test_ties_go_to_the_lowest_row_index(N):
    torch, layout, be, dev = env().short
    m, n, k = 64, 3001, 5
    Td = factors(torch, layout, dev, m, n, k, seed=N, integer=True)["Z"]    # small integers, duplicated rows
    inv = run_inv(torch, be, k, Td)
    q = np.arange(m)
    got = run_similar(torch, be, k, Td, inv, q, q, N)
    inv_h = inv.cpu().numpy()
    dots = dense_dots(torch, be, k, Td, q)
    exp = sref.similar_topn(dots, inv_h[q], inv_h, q, None, N)
    sim = sref.similarities(dots, inv_h[q], inv_h)
    sim[q, q] = np.nan
    # ties across the N-th boundary really occur
    assert sum(int((sim[b] == exp[0][b, N - 1]).sum()) > 1 for b in range(m)) > m // 2
    assert_same(got, exp)
    # row b + 1 is a copy of row b for b = 0, 3, 6, ...: it comes back, the query itself does not
    T = Td.cpu().numpy()
    for b in range(0, m, 3):
        assert (T[b] == T[b + 1]).all() and b not in got[1][b]
        if inv_h[b] != 0 and N >= 10:
            assert b + 1 in got[1][b]


@pytest.mark.parametrize("B,N", [(1, 10), (1, 128), (3000, 10), (3000, 128)])
def test_result_does_not_depend_on_the_slice_count(B, N, monkeypatch):
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    n, k = 5003, 64
    Td = upload(_special_table(layout, n, k, seed=B + N), dev)
    inv = run_inv(torch, be, k, Td)
    q = np.random.default_rng(B).permutation(n)[:B]
    outs = []
    for s in (1, 2, 7, 64):
        assert _hip.load().als_similar_workspace_bytes(B, n, N, s) == (0 if s == 1 else s * B * N * 8)
        monkeypatch.setenv("ALS_RECOMMEND_SLICES", str(s))
        outs.append(run_similar(torch, be, k, Td, inv, q, q, N))
    monkeypatch.delenv("ALS_RECOMMEND_SLICES")
    outs.append(run_similar(torch, be, k, Td, inv, q, q, N))              # automatic
    for o in outs[1:]:
        for g, e in zip(o, outs[0]):
            assert same_bits(g, e)
    if B == 1:
        assert_same(outs[0], oracle(torch, be, k, Td, inv, q, q, N))


def test_allow_bitmap():
    torch, layout, be, dev = env().short
    n, k = 4099, 64                                                        # three slices, the last chunk ragged
    Td = upload(_special_table(layout, n, k, seed=5), dev)
    inv = run_inv(torch, be, k, Td)
    rng = np.random.default_rng(6)
    q = np.concatenate([rng.permutation(n)[:40], [3, 7, n - 1]])
    only = np.zeros(n, bool)
    only[q[0]] = True
    sparse = np.zeros(n, bool)                                             # whole chunks without an allowed row
    sparse[[40, 41, 2000, n - 1]] = True
    masks = {"30 %": rng.random(n) < 0.3, "only the first query": only, "sparse": sparse, "none": np.zeros(n, bool),
             "all": np.ones(n, bool)}
    for name, ok in masks.items():
        for N in (10, 128):
            got = run_similar(torch, be, k, Td, inv, q, q, N, _bitmap(torch, ok, dev))
            assert_same(got, oracle(torch, be, k, Td, inv, q, q, N, ok))
            if name == "none":
                assert (got[2] == 0).all() and (got[1] == -1).all()
            if name == "only the first query":
                assert got[2][0] == 0 and (got[1][0] == -1).all()         # its only allowed row is itself
    assert_same(run_similar(torch, be, k, Td, inv, q, q, 10), oracle(torch, be, k, Td, inv, q, q, 10))    # NULL
    ones = _bitmap(torch, np.ones(n, bool), dev)
    ones[-1] = -1                                                          # bits at positions >= n are ignored
    for g, e in zip(run_similar(torch, be, k, Td, inv, q, q, 10, ones), run_similar(torch, be, k, Td, inv, q, q, 10)):
        assert same_bits(g, e)


def test_scaling_rows_by_powers_of_two_changes_nothing():
    torch, layout, be, dev = env().short
    n, k = 2051, 50
    T = _special_table(layout, n, k, seed=9)
    a = np.random.default_rng(10).integers(-30, 31, size=n)
    T2 = np.ldexp(T, a[:, None]).astype(np.float32)
    assert (np.ldexp(T2.astype(np.float64), -a[:, None]) == T)[~np.isnan(T)].all()     # the scaling is exact
    q = np.random.default_rng(11).permutation(n)[:100]
    res = []
    for tab in (T, T2):
        Td = upload(tab, dev)
        inv = run_inv(torch, be, k, Td)
        res.append([run_similar(torch, be, k, Td, inv, q, q, N) for N in (10, 128)])
    for o1, o2 in zip(*res):
        for g, e in zip(o1, o2):
            assert same_bits(g, e)
    assert (res[0][0][2] > 0).any()


def test_without_self_ids_the_query_comes_first():
    torch, layout, be, dev = env().short
    n, k = 1000, 16
    Td = upload(_table(layout, n, k, seed=12), dev)
    inv = run_inv(torch, be, k, Td)
    q = np.random.default_rng(13).permutation(n)[:50]
    for self_ids in (None, np.full(q.size, -1)):
        got = run_similar(torch, be, k, Td, inv, q, self_ids, 5)
        assert_same(got, oracle(torch, be, k, Td, inv, q, self_ids, 5))
        assert (got[1][:, 0] == q).all()
        assert np.abs(got[0][:, 0] - 1.0).max() <= (k + 8) * 2.0 ** -24
    mixed = np.where(np.arange(q.size) % 2 == 0, q, -1)                    # every other row excludes itself
    got = run_similar(torch, be, k, Td, inv, q, mixed, 5)
    assert_same(got, oracle(torch, be, k, Td, inv, q, mixed, 5))
    assert (got[1][1::2, 0] == q[1::2]).all() and (got[1][0::2] != q[0::2, None]).all()


def test_bad_arguments_return_the_documented_status():
    import ctypes as C
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    n, k, nq, N = 5000, 64, 8, 10
    Td = upload(_table(layout, n, k, seed=1), dev)
    inv = run_inv(torch, be, k, Td)
    q = torch.arange(nq, dtype=torch.int32, device=dev)
    tv = torch.full((nq, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((nq, N), 7, dtype=torch.int32, device=dev)
    tc = torch.full((nq,), 7, dtype=torch.int32, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())          # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def call(k=k, ld=Td.shape[1], nq=nq, topn=N, nslices=0, out=(tv, ti, tc), ws=None, wsb=0, inv=inv):
        return lib.als_similar_topk(k, ld, nq, p(q), p(Td), p(inv), p(q), n, p(Td), p(inv), None, topn, nslices,
                                    p(out[0]), p(out[1]), p(out[2]), p(ws), wsb, stream)
    E_BADARG, E_BADK = -1, -2
    assert call(k=0) == E_BADK and call(k=161) == E_BADK
    assert call(ld=16) == E_BADARG
    assert call(topn=0) == E_BADARG and call(topn=129) == E_BADARG
    assert call(nslices=-1) == E_BADARG and call(nslices=65) == E_BADARG
    assert call(out=(None, ti, tc)) == E_BADARG and call(out=(tv, ti, None)) == E_BADARG and call(inv=None) == E_BADARG
    need = lib.als_similar_workspace_bytes(nq, n, N, 4)
    assert need == 4 * nq * N * 8
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert call(nslices=4) == E_BADARG and call(nslices=4, ws=ws, wsb=need - 1) == E_BADARG
    assert call(nq=0) == 0                                                 # no-op
    assert lib.als_row_inv_norms(k, 16, n, p(Td), p(inv), stream) == E_BADARG
    assert lib.als_row_inv_norms(k, Td.shape[1], 0, None, None, stream) == 0
    torch.cuda.synchronize()
    assert (tv == 7.0).all() and (ti == 7).all() and (tc == 7).all()
    assert call(nslices=4, ws=ws, wsb=need) == 0
    torch.cuda.synchronize()
    assert (tc == N).all()


# ------------------------------------------------------------------------------------------------ model level
def _check_table(torch, be, call, Td, k):
    """`call` = similar_items / similar_users bound to its arguments, Td the table it walks.  Lists == the oracle;
    every similarity within (k + 8) 2^-24 of the float64 cosine of the fp32 rows: the fp32 dot product is within
    k 2^-24 |a||b| of the exact one, the two inverse norms and the two multiplications add one rounding (2^-24) each,
    four more are slack; the top-1 neighbour equals the float64 argmax wherever its float64 lead over the runner-up
    exceeds twice that bound."""
    rows = Td.shape[0]
    inv = run_inv(torch, be, k, Td)
    allq = np.arange(rows)
    for N in (1, 10, 128):
        ids, sims = call(None, N)
        assert ids.shape == sims.shape == (rows, N) and ids.dtype == np.int64 and sims.dtype == np.float64
        tv, ti, _ = oracle(torch, be, k, Td, inv, allq, allq, N)
        assert (ids == ti).all() and (sims == tv.astype(np.float64)).all()
        assert (ids != allq[:, None]).all()
    sub = np.array([rows - 1, 0, rows - 1, rows // 2])                    # order and duplicates kept
    ids, sims = call(sub, 7)
    tv, ti, _ = oracle(torch, be, k, Td, inv, sub, sub, 7)
    assert (ids == ti).all() and (sims == tv.astype(np.float64)).all()
    # against float64
    ids, sims = call(None, min(10, rows - 1))
    S = mmr_ref.similarities(Td.cpu().numpy()[:, :k])
    bound = (k + 8) * 2.0 ** -24
    err = np.abs(sims - S[allq[:, None], ids])
    print(f"rows={rows} k={k}: worst |sim - float64 cosine| {err.max():.3e} (bound {bound:.3e})")
    assert err.max() <= bound
    np.fill_diagonal(S, -np.inf)
    srt = np.sort(S, axis=1)
    clear = srt[:, -1] - srt[:, -2] > 2 * bound
    assert (~clear).mean() <= 0.10
    assert (ids[clear, 0] == np.argmax(S, axis=1)[clear]).all()


@pytest.mark.parametrize("name,use_features,kw", [
    ("g4_feat_uw5", True, {}),
    ("g4_feat_uw5", False, {}),
    ("g5_graph_a5.0", True, {}),
    ("g1_plain", True, {"solve_dtype": "float64"}),
])
def test_model_similar_on_fixtures(name, use_features, kw):
    torch, layout, be, dev = env().short
    g = Golden(name)
    r, c, v = g.train
    model = model_for(g, device="cuda:0", **kw)
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"], verbose=0)
    feats = g.features if use_features else None
    eng, k = model._eng, model.V.shape[1]
    Z = eng._compose_for(feats or {})                                      # what the call composes, bit for bit
    _check_table(torch, be, lambda q, N: model.similar_items(q, N, features=feats), Z, k)
    _check_table(torch, be, model.similar_users, eng.U, k)
    # filters reach the kernel
    ok = np.random.default_rng(1).random(g.n) < 0.5
    ids, sims = model.similar_items(None, 10, features=feats, allow_items=ok)
    inv = run_inv(torch, be, k, Z)
    tv, ti, _ = oracle(torch, be, k, Z, inv, np.arange(g.n), np.arange(g.n), 10, ok)
    assert (ids == ti).all() and (sims == tv.astype(np.float64)).all()
    ids2, sims2 = model.similar_items(None, 10, features=feats, filter_items=~ok)
    assert (ids2 == ids).all() and (sims2 == sims).all()


def test_model_chunks_are_crossed_on_the_device(monkeypatch):
    torch, layout, be, dev = env().short
    g = Golden("g1_plain")
    r, c, v = g.train
    model = model_for(g, device="cuda:0")
    model.fit_coo(r, c, v, (g.m, g.n), features=None, tol=g.cfg["tol"], verbose=0)
    base = model.similar_users(None, 5)
    monkeypatch.setattr(model._eng, "REC_BATCH", 16, raising=False)      # 60 users: four chunks
    got = model.similar_users(None, 5)
    assert (got[0] == base[0]).all() and (got[1] == base[1]).all()
