"""K21 (GPU): als_recommend_topk_priced, als_capacity_settle (csrc/capacity.hip) and ALS.recommend_capacity /
recommend_new_capacity.

The priced walk is held to als_recommend_topk_masked (zero floors) and to `priced_topn` of tests/capacity_ref.py on
als_predict_dense rows; the settle pass to `settle`; the model calls to `greedy` - the sorted scan of the definition -
on `predict()` rows.  Every comparison is ==, and every output buffer starts from a poison value."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import capacity_ref as cref
from tests.gpu_common import assert_same, env, factors, predict_dense, run_topk, seen_csr, upload
from tests.serving_ref import bitmap_numpy
from tests.synth import make_ratings


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)


def run_priced(torch, be, f, users, row_ids, n, seen_ptr, seen_idx, N, dev, allow, floor):
    """als_recommend_topk_priced into poisoned buffers -> numpy (values, items, counts); allow: uint32 words or None,
    floor: uint64 [n]."""
    us = upload(np.asarray(users, np.int32), dev)
    B = us.numel()
    tv = torch.full((B, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((B, N), -7, dtype=torch.int32, device=dev)
    tc = torch.full((B,), -7, dtype=torch.int32, device=dev)
    be.recommend_topk_priced(k=f["k"], ld=f["ld"], users=us, row_ids=upload(np.asarray(row_ids, np.int32), dev), n=n,
                             U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"], mu=f["mu"],
                             seen_ptr=None if seen_ptr is None else upload(seen_ptr, dev),
                             seen_idx=None if seen_idx is None else upload(seen_idx, dev),
                             allow=None if allow is None else upload(allow.view(np.int32), dev),
                             floor_key=upload(_i64(floor), dev), topn=N, top_val=tv, top_idx=ti, top_cnt=tc)
    return tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the priced walk
@pytest.mark.parametrize("slices", ["1", "3"])
@pytest.mark.parametrize("k", [1, 5, 64])
def test_zero_floors_equal_the_masked_call(k, slices, monkeypatch):
    torch, layout, be, dev = env().short
    monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)
    m, n = 60, 333                                                         # n: not a multiple of 32
    f = factors(torch, layout, dev, m, n, k, seed=10 * k)
    ptr, idx, rows = seen_csr(m, n, seed=k)
    rng = np.random.default_rng(k)
    users = np.concatenate([np.arange(m), rng.integers(0, m, 90)])[::-1].copy()    # 150 rows: partial last workgroups
    row_ids = rng.permutation(users.size) + 1000                           # shuffled: they must not matter
    allow = bitmap_numpy(rng.random(n) < 0.6)
    zero = np.zeros(n, np.uint64)
    for N in (1, 10, 32, 33, 128):                                         # 32 / 33: the narrow and the wide workgroup
        for a in (None, allow):
            got = run_priced(torch, be, f, users, row_ids, n, ptr, idx, N, dev, a, zero)
            want = run_topk(torch, be, f, users, n, ptr, idx, N, dev,
                            allow=None if a is None else upload(a.view(np.int32), dev))
            assert_same(got, want)
        got = run_priced(torch, be, f, users, row_ids, n, None, None, N, dev, allow, zero)
        assert_same(got, run_topk(torch, be, f, users, n, None, None, N, dev, allow=upload(allow.view(np.int32), dev)))


@pytest.mark.parametrize("slices", ["1", "3"])
def test_floors_on_massively_tied_scores(slices, monkeypatch):
    """Tables of small integers: a handful of distinct scores, so the row word of the item-side key decides.  Floors
    set exactly to a pair's key (it passes), to the same score with the next lower row (it fails) and with the next
    higher row (it passes)."""
    torch, layout, be, dev = env().short
    monkeypatch.setenv("ALS_RECOMMEND_SLICES", slices)
    m, n, k = 40, 333, 4
    ld = layout.padded_k(k)
    rng = np.random.default_rng(7)
    U = np.zeros((m, ld), np.float32)
    Z = np.zeros((n, ld), np.float32)
    U[:, :k] = rng.integers(-1, 2, size=(m, k))
    Z[:, :k] = rng.integers(-1, 2, size=(n, k))
    f = dict(k=k, ld=ld, U=upload(U, dev), Z=upload(Z, dev), b_u=upload(np.zeros(m, np.float32), dev),
             b_i=upload(np.zeros(n, np.float32), dev), mu=torch.tensor([0.0], dtype=torch.float64, device=dev))
    P = predict_dense(torch, be, f, m, n, dev)
    assert np.unique(P).size <= 9
    ptr, idx, rows = seen_csr(m, n, seed=3)
    users = np.concatenate([np.arange(m), rng.integers(0, m, 110)])        # 150 batch rows
    B = users.size
    row_ids = rng.permutation(B) + 5
    S = P[users]
    seen = [rows[u] for u in users]
    # every item's floor comes from one batch row b(i): kinds 0 exact, 1 next lower row, 2 next higher row, 3 none
    owner = rng.integers(0, B, n)
    kind = rng.integers(0, 4, n)
    shift = np.array([0, -1, 1, 0])[kind]
    floor = cref.make_key(S[owner, np.arange(n)], row_ids[owner] + shift)
    floor[kind == 3] = 0
    mask = np.zeros(n, bool)
    for w in (0, 2, 3, 7, 10):                                             # the other words are empty: skipped chunks
        mask[32 * w: 32 * w + 32] = rng.random(len(mask[32 * w: 32 * w + 32])) < 0.6
    assert mask.sum() <= 128
    for allowed in (None, mask):
        a = None if allowed is None else bitmap_numpy(allowed)
        for N in (10, 128):
            for sp, si, sr in ((ptr, idx, seen), (None, None, [np.zeros(0, np.int64)] * B)):
                got = run_priced(torch, be, f, users, row_ids, n, sp, si, N, dev, a, floor)
                assert_same(got, cref.priced_topn(S, sr, allowed, row_ids, floor, N))
    # under the small bitmap N = 128 lists every passing candidate: the three kinds, pair by pair
    tv, ti, tc = run_priced(torch, be, f, users, row_ids, n, None, None, 128, dev, bitmap_numpy(mask), floor)
    seen_kinds = set()
    for i in np.nonzero(mask)[0]:
        listed = i in ti[owner[i]]
        assert listed == (kind[i] != 1), (i, kind[i])
        seen_kinds.add(int(kind[i]))
    assert seen_kinds == {0, 1, 2, 3}
    zero = np.zeros(n, np.uint64)
    plain = run_priced(torch, be, f, users, row_ids, n, None, None, 128, dev, bitmap_numpy(mask), zero)
    assert (plain[2] > tc).any()                                           # the floors took candidates away


# ------------------------------------------------------------------------------------------------ settle
def run_settle(torch, be, dev, ti, tv, capacity, floor):
    n = capacity.size
    fl = upload(_i64(floor), dev)
    fill = torch.full((n,), -7, dtype=torch.int32, device=dev)
    dirty = torch.full((ti.shape[0],), -7, dtype=torch.int32, device=dev)
    n_over = torch.full((1,), -7, dtype=torch.int32, device=dev)
    be.capacity_settle(n=n, top_idx=upload(ti, dev), top_val=upload(tv, dev), capacity=upload(capacity, dev),
                       floor_key=fl, fill=fill, dirty=dirty, n_over=n_over)
    return fl.cpu().numpy().view(np.uint64), fill.cpu().numpy(), dirty.cpu().numpy(), int(n_over.item())


def _hand_made_lists(rng, B, n):
    """[B, 4] lists: slot 0 names item 0 in every row; slot 1 item 1 (rows 0 .. 9), item 2 (rows 10 .. 14), item 3 (rows
    20 .. 22) or a random item >= 4 or nothing; slot 2 another random item or nothing; slot 3 always empty.  Scores on a
    grid of 7 values: the row word decides among equal scores."""
    ti = np.full((B, 4), -1, np.int32)
    ti[:, 0] = 0
    ti[:10, 1], ti[10:15, 1], ti[20:23, 1] = 1, 2, 3
    for b in range(23, B):
        a, c = rng.choice(np.arange(4, n), 2, replace=False)
        if rng.random() < 0.6:
            ti[b, 1] = a
        if rng.random() < 0.4:
            ti[b, 2] = c
    tv = (rng.integers(0, 7, size=(B, 4)) * 0.25 - 0.5).astype(np.float32)
    tv[ti < 0] = -np.inf
    return ti, tv


@pytest.mark.parametrize("c0", [1, 255, 256, 257, 699])
def test_settle_equals_the_reference(c0):
    torch, layout, be, dev = env().short
    B, n = 700, 40
    rng = np.random.default_rng(c0)
    ti, tv = _hand_made_lists(rng, B, n)
    capacity = rng.integers(1, 30, n).astype(np.int32)
    capacity[:4] = [c0, 10, 2, 0]              # all B rows on item 0; item 1 exactly at capacity; item 3 has none
    floor = np.zeros(n, np.uint64)
    floor[2] = cref.make_key(np.float32(-5.0), 3)                          # already non-zero, below every demander
    floor[5] = cref.make_key(np.float32(0.25), 100)                        # non-zero on a randomly demanded item
    floor[39] = 12345                                                      # an item with a floor and no rise
    capacity[39] = B
    want = cref.settle(ti, tv, capacity, floor)
    assert want[3] >= 3 and want[0][1] == 0 and want[1][1] == 10 and want[0][3] == np.uint64(0xFFFFFFFFFFFFFFFF)
    assert want[0][39] == 12345 and want[2].sum() >= B - c0 and want[1][0] == c0
    got = run_settle(torch, be, dev, ti, tv, capacity, floor)
    again = run_settle(torch, be, dev, ti, tv, capacity, floor)
    for g, a, w in zip(got[:3], again[:3], want[:3]):
        assert g.dtype == w.dtype and (g == w).all(), np.argwhere(g != w)[:5]
        assert (a == g).all()                                              # no dependence on the order of the atomics
    assert got[3] == again[3] == want[3]


def test_settle_without_over_demand_changes_nothing():
    torch, layout, be, dev = env().short
    B, n = 700, 40
    rng = np.random.default_rng(0)
    ti, tv = _hand_made_lists(rng, B, n)
    capacity = np.full(n, B, np.int32)
    floor = rng.integers(0, 1 << 40, n).astype(np.uint64)                  # below every real key
    fl, fill, dirty, n_over = run_settle(torch, be, dev, ti, tv, capacity, floor)
    assert n_over == 0 and not dirty.any() and (fl == floor).all()
    assert (fill == np.bincount(ti[ti >= 0], minlength=n)).all()
    assert_same((fl, fill, dirty), cref.settle(ti, tv, capacity, floor)[:3])


# ------------------------------------------------------------------------------------------------ model level
M, N_ITEMS, K_F = 150, 333, 5


@pytest.fixture(scope="module")
def contested():
    """A small fit whose item bias is then spread by popularity rank, so that the same items top most lists."""
    E = env()
    torch = E.torch
    from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig
    r, c, v = make_ratings(M, N_ITEMS, 4000, seed=11, empty_users=(3,))
    cfg = ALSConfig(core=CoreConfig(n_factors=K_F, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    model = ALS(cfg, device="cuda:0").fit_coo(r, c, v, (M, N_ITEMS), tol=None, verbose=0)
    rng = np.random.default_rng(12)
    skew = (2.0 * (1.0 + rng.permutation(N_ITEMS)) ** -0.5).astype(np.float32)
    model._eng.b_i.add_(torch.from_numpy(skew).to(model._eng.dev))         # predict() and the walks read this table
    seen = [np.sort(c[r == u]) for u in range(M)]
    return model, seen, model.predict()


def _assert_lists(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    assert (got[0] == want[0]).all(), np.argwhere(got[0] != want[0])[:5]
    assert (got[1] == want[1]).all()                                       # bitwise predict's: greedy copies them


def _folded(rng, B=9):
    from collaborative_filtering_amd.serving import FoldedItems
    Z = rng.normal(size=(B, K_F)).astype(np.float32).astype(np.float64)
    raters = [np.sort(rng.permutation(M)[: 2 + b]) for b in range(B)]      # with exclude_seen they lose the item
    ptr = np.zeros(B + 1, np.int64)
    ptr[1:] = np.cumsum([x.size for x in raters])
    idx = np.concatenate(raters).astype(np.int32)
    return FoldedItems(Z.copy(), rng.normal(size=B).astype(np.float32).astype(np.float64) + 2.0, Z, None,
                       (ptr, idx, np.ones(idx.size, np.float32))), raters


def test_model_equals_greedy_end_to_end(contested, monkeypatch):
    model, seen, P = contested
    monkeypatch.setattr(model._eng, "REC_BATCH", 100, raising=False)       # B = 450: chunks of 100 and one of 50
    rng = np.random.default_rng(1)
    users = np.tile(np.arange(M), 3)                   # every user three times: cross-row ties on every score
    B, N = users.size, 7
    cap = rng.choice([0, 1, 3, B + 1], size=N_ITEMS).astype(np.int64)
    none = [np.zeros(0, np.int64)] * B
    for exclude_seen in (True, False):
        got = model.recommend_capacity(users, N, capacity=cap, exclude_seen=exclude_seen, return_info=True)
        want = cref.greedy(P[users], [seen[u] for u in users] if exclude_seen else none, None, cap, N)
        _assert_lists(got, want)
        info = got[2]
        assert info.rounds >= 2 and info.walked_rows < (info.rounds + 1) * B
        assert (info.fill == want[2]).all() and (info.fill <= cap).all()
        assert (info.fill == np.bincount(got[0][got[0] >= 0], minlength=N_ITEMS)).all()
        full = (info.fill == cap) & (cap > 0)
        assert full.any() and np.isnan(info.cutoff[~full]).all()
        i = int(np.nonzero(full)[0][0])
        assert info.cutoff[i] == got[1][got[0] == i].min()
    # both filters
    allow = rng.permutation(N_ITEMS)[:250]
    block = rng.random(N_ITEMS) < 0.2
    ok = np.isin(np.arange(N_ITEMS), allow) & ~block
    got = model.recommend_capacity(users, N, capacity=cap, items=allow, filter_items=block)
    _assert_lists(got, cref.greedy(P[users], [seen[u] for u in users], ok, cap, N))
    # new items: the joint catalogue, the raters of a folded item have seen it
    folded, raters = _folded(rng)
    nt = N_ITEMS + folded.n_items
    PJ = np.concatenate([P[users], model.predict_new_items(folded, users)], axis=1)
    seen_j = [np.concatenate([seen[u], [N_ITEMS + b for b in range(folded.n_items) if u in raters[b]]]).astype(np.int64)
              for u in users]
    capj = np.concatenate([cap, [1, 2, 3, 0, 1, B + 1, 2, 1, 3]])
    got = model.recommend_capacity(users, N, capacity=capj, new_items=folded, return_info=True)
    want = cref.greedy(PJ, seen_j, None, capj, N)
    _assert_lists(got, want)
    assert (got[0] >= N_ITEMS).any() and got[2].fill.shape == (nt,) and (got[2].fill == want[2]).all()


def test_rows_come_up_short_when_the_capacity_runs_out(contested):
    model, seen, P = contested
    users = np.tile(np.arange(M), 2)
    B, N = users.size, 7
    cap = np.zeros(N_ITEMS, np.int64)
    cap[::3] = 5                                                           # 555 units for 2100 slots
    assert cap.sum() < B * N
    got = model.recommend_capacity(users, N, capacity=cap, return_info=True)
    want = cref.greedy(P[users], [seen[u] for u in users], None, cap, N)
    _assert_lists(got, want)
    assert (got[0] == -1).any() and np.isneginf(got[1][got[0] == -1]).all()
    assert (np.sort(got[0] < 0, axis=1) == (got[0] < 0)).all()             # the padding comes last
    assert got[2].fill.sum() == (got[0] >= 0).sum() <= cap.sum()


def test_loose_capacity_is_recommend_with_zero_rounds(contested):
    model, seen, P = contested
    users = np.tile(np.arange(M), 2)
    for cap in (users.size, np.full(N_ITEMS, users.size + 1)):
        for N in (7, 40):
            got = model.recommend_capacity(users, N, capacity=cap, return_info=True)
            want = model.recommend(users, N)
            assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
            assert got[2].rounds == 0 and got[2].walked_rows == users.size


def test_recommend_new_capacity_equals_greedy(contested, monkeypatch):
    model, seen, P = contested
    torch = env().torch
    monkeypatch.setattr(model._eng, "REC_BATCH", 64, raising=False)
    rng = np.random.default_rng(4)
    B, N = 120, 7
    R_new = np.full((B, N_ITEMS), np.nan)
    for b in range(B // 2):
        if b != 4:                                                         # one row without ratings
            R_new[b, rng.permutation(N_ITEMS)[: 3 + b % 9]] = rng.integers(1, 6, 3 + b % 9)
    R_new[B // 2:] = R_new[: B // 2]                                       # every row twice: ties across rows
    # the folded users' score rows: als_predict_dense on their folded factors
    eng = model._eng
    Uf, bf = model.fold_in(R_new)
    Ut = torch.zeros(B, eng.ld, dtype=torch.float32)
    Ut[:, : eng.k] = torch.from_numpy(Uf).float()
    f = dict(k=eng.k, ld=eng.ld, U=Ut.to(eng.dev), Z=eng.V, b_u=torch.from_numpy(bf).float().to(eng.dev), b_i=eng.b_i,
             mu=eng.mu)
    PN = predict_dense(torch, eng.be, f, B, N_ITEMS, eng.dev).astype(np.float64)
    cap = rng.choice([0, 1, 3, B + 1], size=N_ITEMS).astype(np.int64)
    rows_seen = [np.nonzero(~np.isnan(R_new[b]))[0] for b in range(B)]
    got = model.recommend_new_capacity(R_new, N, capacity=cap, return_info=True)
    want = cref.greedy(PN, rows_seen, None, cap, N)
    _assert_lists(got, want)
    assert got[2].rounds >= 1 and (got[2].fill == want[2]).all()
