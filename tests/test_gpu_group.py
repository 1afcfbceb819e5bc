"""K15 (GPU): als_group_topk (csrc/group.hip) and ALS.recommend_group.

Everything in the contract is exact, so every comparison is ==: the expected lists are `group_topn` of
tests/group_ref.py on the member rows als_predict_dense itself writes - the kernel's member scores have to equal those
bitwise - with the seen rows and the allow mask of the call.  The mean is compared with == as well: its fp64 sum is
exact while the member scores of an item lie within a factor 2^17 of each other, and the inputs of those tests
(`banded`) are asserted to lie in [2^-3, 2^4], a factor 2^7.  That band is a condition of the test, not a tolerance.

A list of N entries is the first N of a total order, so the expected list for a smaller N is a prefix of the one for
N = 128: the reference is computed once per batch, at N = 128 (`prefix`)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import group_ref as gref
from tests.common import Golden, model_for
from tests.gpu_common import assert_same, env, factors, predict_dense, run_topk, same_bits, seen_csr, upload

M_USERS = 200
SIZES = (1, 2, 3, 15, 16, 17, 32, 33, 64)
AGGREGATES = gref.AGGREGATES
NONE = np.zeros(0, np.int64)


# ------------------------------------------------------------------------------------------------ inputs, launches
def banded(torch, layout, dev, m, n, k, seed):
    """`factors` with entries of variance 0.25 / sqrt(k) - a dot product of standard deviation 0.25 -, biases of scale
    0.3 and mu = 3.5: scores around 3.5 +- 0.5, far inside [2^-3, 2^4]."""
    ld = layout.padded_k(k)
    rng = np.random.default_rng(seed)
    U = np.zeros((m, ld), np.float32)
    Z = np.zeros((n, ld), np.float32)
    sd = np.sqrt(0.25 / np.sqrt(k))
    U[:, :k] = rng.normal(scale=sd, size=(m, k))
    Z[:, :k] = rng.normal(scale=sd, size=(n, k))
    bu = rng.normal(scale=0.3, size=m).astype(np.float32)
    bi = rng.normal(scale=0.3, size=n).astype(np.float32)
    return dict(k=k, ld=ld, U=upload(U, dev), Z=upload(Z, dev), b_u=upload(bu, dev), b_i=upload(bi, dev),
                mu=torch.tensor([3.5], dtype=torch.float64, device=dev))


def in_band(dense):
    """The condition under which the fp64 sum of up to 64 fp32 scores is exact in any order."""
    assert (dense >= 2.0 ** -3).all() and (dense <= 2.0 ** 4).all(), (dense.min(), dense.max())
    return dense


def make_groups(m, seed, count=20):
    """`count` distinct groups of users < m, their sizes cycling through SIZES."""
    rng = np.random.default_rng(seed)
    return [rng.permutation(m)[: min(SIZES[i % len(SIZES)], m)].astype(np.int64) for i in range(count)]


def _csr(lists):
    ptr = np.zeros(len(lists) + 1, np.int64)
    ptr[1:] = np.cumsum([len(s) for s in lists])
    idx = np.concatenate([np.asarray(s, np.int64) for s in lists]).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    return ptr, idx


def run_group(torch, be, f, groups, n, seen_ptr, seen_idx, N, aggregate, allow=None, max_members=None):
    """als_group_topk of the batch `groups` (arrays of user ids) over the first n items of f, into buffers that start
    from 7 -> numpy (values, items, counts).  seen_ptr / seen_idx: host arrays by batch group, or None (NULL)."""
    dev = f["U"].device
    gp, gu = _csr(groups)
    G = len(groups)
    tv = torch.full((G, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((G, N), 7, dtype=torch.int32, device=dev)
    tc = torch.full((G,), 7, dtype=torch.int32, device=dev)
    if max_members is None:
        max_members = int(np.diff(gp).max())
    be.group_topk(k=f["k"], ld=f["ld"], g_ptr=upload(gp, dev), g_users=upload(gu if gu.size else np.zeros(1, np.int32), dev),
                  max_members=max_members, n=n, U=f["U"], Z=f["Z"], b_u=f["b_u"], b_i=f["b_i"], mu=f["mu"],
                  seen_ptr=None if seen_ptr is None else upload(np.asarray(seen_ptr, np.int64), dev),
                  seen_idx=None if seen_idx is None else upload(np.asarray(seen_idx, np.int32), dev),
                  allow=allow, aggregate=aggregate, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)
    return tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()


def oracle(dense, groups, seen_lists, ok, N, aggregate):
    return gref.group_topn([dense[np.asarray(g, np.int64)] for g in groups], seen_lists, ok, N, aggregate)


def prefix(exp128, nb, N):
    """The expected outputs of the first nb groups at list length N from those at N = 128."""
    tv, ti, tc = exp128
    return tv[:nb, :N], ti[:nb, :N], np.minimum(tc[:nb], N)


def _bitmap(torch, mask, dev):
    """The C ABI's bitmap, packed here with numpy: item i = bit i & 31 of word i >> 5."""
    bits = np.zeros((mask.size + 31) // 32 * 32, np.uint8)
    bits[: mask.size] = mask
    words = np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view("<u4").reshape(-1)
    return torch.from_numpy(words.view(np.int32).copy()).to(dev)


# ------------------------------------------------------------------------------------------------ shape sweep
@pytest.mark.parametrize("k", [1, 16, 17, 64, 65, 128, 160])
@pytest.mark.parametrize("n", [1, 17, 1000, 4099])
def test_kernel_equals_the_aggregate_of_predict_dense_rows(k, n):
    torch, layout, be, dev = env().short
    m = M_USERS
    fb = banded(torch, layout, dev, m, n, k, seed=10 * k + n)
    fr = factors(torch, layout, dev, m, n, k, seed=10 * k + n + 1)
    dense = {"mean": in_band(predict_dense(torch, be, fb, m, n, dev)), "min": predict_dense(torch, be, fr, m, n, dev)}
    dense["max"] = dense["min"]
    base = make_groups(m, seed=k + n)
    batch = [base[(7 * i + 1) % len(base)] for i in range(129)]            # all sizes, repeated groups
    assert {len(g) for g in batch} == set(SIZES)
    ptr, idx, seen = seen_csr(len(batch), n, seed=k + n)                   # by BATCH GROUP: 0 none, 1 all but 3
    for aggregate in AGGREGATES:
        f = fb if aggregate == "mean" else fr
        exp = oracle(dense[aggregate], batch, seen, None, 128, aggregate)
        for nb in (1, 9, 129):
            for N in (1, 10, 32, 33, 128):
                tv, ti, tc = got = run_group(torch, be, f, batch[:nb], n, ptr[: nb + 1], idx, N, aggregate)
                assert_same(got, prefix(exp, nb, N))
                assert (tc == np.minimum(N, [n - seen[b].size for b in range(nb)])).all()
                for b in range(nb):                                        # padding (N > candidates)
                    assert (ti[b, tc[b]:] == -1).all() and np.isneginf(tv[b, tc[b]:]).all()


# ------------------------------------------------------------------------------------------------ member order
@pytest.mark.parametrize("aggregate", AGGREGATES)
def test_permuting_the_members_changes_no_bit(aggregate):
    torch, layout, be, dev = env().short
    m, n, k = M_USERS, 4099, 64
    if aggregate == "mean":
        f = banded(torch, layout, dev, m, n, k, seed=31)
        in_band(predict_dense(torch, be, f, m, n, dev))
    else:
        f = factors(torch, layout, dev, m, n, k, seed=32)
    groups = make_groups(m, seed=33, count=18)
    rng = np.random.default_rng(34)
    ptr, idx, seen = seen_csr(len(groups), n, seed=35)
    for N in (10, 128):
        ref = run_group(torch, be, f, groups, n, ptr, idx, N, aggregate)
        for _ in range(2):
            perm = [g[rng.permutation(g.size)] for g in groups]
            assert any((p != g).any() for p, g in zip(perm, groups))
            for a, e in zip(run_group(torch, be, f, perm, n, ptr, idx, N, aggregate), ref):
                assert same_bits(a, e)


@pytest.mark.parametrize("aggregate", AGGREGATES)
def test_a_group_of_one_is_recommend_topk(aggregate):
    torch, layout, be, dev = env().short
    m, n, k = M_USERS, 4099, 64
    f = factors(torch, layout, dev, m, n, k, seed=41)
    users = np.concatenate([np.arange(40), [3, 1, 3, 0]])[::-1].copy()
    ptr_u, idx_u, rows = seen_csr(m, n, seed=42)                           # by user id
    ptr_g, idx_g = _csr([rows[u] for u in users])                          # the same rows by batch group
    for N in (1, 10, 128):
        exp = run_topk(torch, be, f, users, n, ptr_u, idx_u, N, dev)
        got = run_group(torch, be, f, [np.array([u]) for u in users], n, ptr_g, idx_g, N, aggregate)
        for a, e in zip(got, exp):
            assert same_bits(a, e)


# ------------------------------------------------------------------------------------------------ seen lists
@pytest.mark.parametrize("n", [4090, 4099])             # automatic slices of 2048 (two) and of 1376 (three) items
def test_seen_lists(n):
    torch, layout, be, dev = env().short
    m, k = M_USERS, 16
    f = banded(torch, layout, dev, m, n, k, seed=n)
    dense = in_band(predict_dense(torch, be, f, m, n, dev))
    rng = np.random.default_rng(n)
    edges = [31, 32, 1375, 1376, 2047, 2048, 2751, 2752, n - 1]
    seen = [NONE,                                       # 0 empty
            np.array([100]),                            # 1 one entry
            np.arange(n),                               # 2 everything
            np.array(edges),                            # 3 chunk and slice boundaries, the last item
            np.arange(60, 100),                         # 4 a run of 40: a whole chunk and parts of two others
            np.arange(0, 200),                          # 5 a run across chunks from item 0: more than one 64-entry load
            np.nonzero(rng.random(n) < 0.1)[0],         # 6 scattered
            np.setdiff1d(np.arange(n), edges)]          # 7 everything but the boundary items
    base = make_groups(m, seed=n, count=9)              # one group of every size
    order = [0, 1, 2, 3, 4, 5, 6, 7, 3, 2, 0]
    batch = [base[(2 * j + 1) % 9] for j in range(len(order))]
    lists = [seen[j] for j in order]
    ptr, idx = _csr(lists)
    for aggregate in AGGREGATES:
        for N in (10, 128):
            tv, ti, tc = got = run_group(torch, be, f, batch, n, ptr, idx, N, aggregate)
            assert_same(got, oracle(dense, batch, lists, None, N, aggregate))
            assert tc[2] == 0 and (ti[2] == -1).all() and np.isneginf(tv[2]).all()         # everything seen
            assert tc[7] == len(edges) and sorted(ti[7][: tc[7]].tolist()) == edges        # N >= 9: exactly those
            for b in range(len(batch)):
                assert not np.isin(ti[b], lists[b]).any()
            none = run_group(torch, be, f, batch, n, None, None, N, aggregate)              # both pointers NULL
            assert_same(none, oracle(dense, batch, [NONE] * len(batch), None, N, aggregate))
            assert (none[2] == min(N, n)).all()


# ------------------------------------------------------------------------------------------------ slices
@pytest.mark.parametrize("G,N", [(1, 10), (1, 128), (200, 10), (200, 128)])
def test_result_does_not_depend_on_the_slice_count(G, N, monkeypatch):
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    m, n, k = M_USERS, 4099, 64
    f = banded(torch, layout, dev, m, n, k, seed=G + N)
    dense = in_band(predict_dense(torch, be, f, m, n, dev))
    base = make_groups(m, seed=G, count=27)
    batch = [base[(5 * i + 2) % len(base)] for i in range(G)]
    ptr, idx, seen = seen_csr(G, n, seed=G, density=0.1)                   # seen items in every slice
    for aggregate in AGGREGATES:
        outs = []
        for s in (1, 2, 3, 64):
            assert _hip.load().als_group_workspace_bytes(G, n, N, s) == (0 if s == 1 else s * G * N * 8)
            monkeypatch.setenv("ALS_RECOMMEND_SLICES", str(s))
            outs.append(run_group(torch, be, f, batch, n, ptr, idx, N, aggregate))
        monkeypatch.delenv("ALS_RECOMMEND_SLICES")
        outs.append(run_group(torch, be, f, batch, n, ptr, idx, N, aggregate))              # automatic
        for o in outs[1:]:
            for g, e in zip(o, outs[0]):
                assert same_bits(g, e)
        assert_same(outs[0], oracle(dense, batch, seen, None, N, aggregate))


# ------------------------------------------------------------------------------------------------ allow bitmap
def test_allow_bitmap():
    torch, layout, be, dev = env().short
    m, n, k = M_USERS, 4099, 64                                            # three slices, the last chunk ragged
    f = banded(torch, layout, dev, m, n, k, seed=5)
    dense = in_band(predict_dense(torch, be, f, m, n, dev))
    base = make_groups(m, seed=8, count=9)
    batch = base + [base[2], base[0], base[2]]
    G = len(batch)
    ptr, idx, seen = seen_csr(G, n, seed=6, density=0.1)
    rng = np.random.default_rng(7)
    only = np.zeros(n, bool)
    only[1234] = True
    sparse = np.zeros(n, bool)             # whole zero words between the set ones; seen items inside the skipped chunks
    sparse[[40, 41, 2000, 2001, 2002, 3990, n - 1]] = True
    assert seen[2].size > 3000 and not np.isin(np.nonzero(sparse)[0], seen[2]).all()
    assert ((seen[2] > 41) & (seen[2] < 1984)).sum() > 1000                # > 64 seen items under the skipped words
    masks = {"30 %": rng.random(n) < 0.3, "one bit": only, "sparse": sparse, "none": np.zeros(n, bool),
             "all": np.ones(n, bool)}
    for aggregate in AGGREGATES:
        for name, ok in masks.items():
            for N in (10, 128):
                got = run_group(torch, be, f, batch, n, ptr, idx, N, aggregate, _bitmap(torch, ok, dev))
                assert_same(got, oracle(dense, batch, seen, ok, N, aggregate))
                if name == "none":
                    assert (got[2] == 0).all() and (got[1] == -1).all()
                free = run_group(torch, be, f, batch, n, None, None, N, aggregate, _bitmap(torch, ok, dev))
                assert_same(free, oracle(dense, batch, [NONE] * G, ok, N, aggregate))      # without seen lists
                assert (free[2] == min(N, int(ok.sum()))).all()
        null = run_group(torch, be, f, batch, n, ptr, idx, 10, aggregate)                   # NULL
        assert_same(null, oracle(dense, batch, seen, None, 10, aggregate))
        ones = _bitmap(torch, np.ones(n, bool), dev)
        ones[-1] = -1                                                      # bits at positions >= n are ignored
        for g, e in zip(run_group(torch, be, f, batch, n, ptr, idx, 10, aggregate, ones), null):
            assert same_bits(g, e)


# ------------------------------------------------------------------------------------------------ ties, NaN
@pytest.mark.parametrize("aggregate", ["min", "max"])
@pytest.mark.parametrize("N", [1, 10, 33, 128])
def test_ties_go_to_the_lowest_item_id(aggregate, N, monkeypatch):
    torch, layout, be, dev = env().short
    m, n, k = M_USERS, 3001, 5
    f = factors(torch, layout, dev, m, n, k, seed=N, integer=True)         # small integers, duplicated item rows
    dense = predict_dense(torch, be, f, m, n, dev)
    batch = make_groups(m, seed=N + 1, count=18)
    G = len(batch)
    exp = oracle(dense, batch, [NONE] * G, None, N, aggregate)
    agg = np.stack([gref.group_scores(dense[g], aggregate) for g in batch])
    # equal group scores across the N-th place really occur
    assert sum(int((agg[b] == exp[0][b, N - 1]).sum()) > 1 for b in range(G)) > G // 2
    for s in ("1", "4"):                   # 4 slices of 768 items: equal scores on both sides of every boundary
        monkeypatch.setenv("ALS_RECOMMEND_SLICES", s)
        got = run_group(torch, be, f, batch, n, None, None, N, aggregate)
        assert_same(got, exp)
        for b in range(G):                                                 # among equal scores the lower id is first
            v, i = got[0][b], got[1][b]
            eq = v[1:] == v[:-1]
            assert (i[1:][eq] > i[:-1][eq]).all()
        for b in range(G):                                                 # of the items tied at the N-th place, the
            tied = np.nonzero(agg[b] == got[0][b, N - 1])[0]               # lowest ids are the ones in the list
            taken = np.isin(tied, got[1][b])
            assert taken.any() and taken[: int(taken.sum())].all()
    assert any(((agg[b][:768] == exp[0][b, N - 1]).any() and (agg[b][768:] == exp[0][b, N - 1]).any())
               for b in range(G))


def test_nan_member_empties_the_group_and_a_nan_item_is_never_returned():
    torch, layout, be, dev = env().short
    m, n, k = M_USERS, 1000, 17
    f = factors(torch, layout, dev, m, n, k, seed=3)
    f["U"][5, 0] = float("nan")                                            # user 5: a NaN factor
    f["b_u"][40] = float("nan")                                            # user 40: a NaN bias
    f["Z"][7, 1] = float("nan")                                            # item 7: NaN for everybody
    f["b_i"][900] = float("nan")
    dense = predict_dense(torch, be, f, m, n, dev)
    clean = np.setdiff1d(np.arange(m), [5, 40])
    rng = np.random.default_rng(4)
    pick = lambda g: rng.permutation(clean)[:g]                            # noqa: E731
    batch = [pick(3),                                                      # 0 clean
             np.concatenate([pick(2), [5]]),                               # 1 NaN member last
             np.concatenate([[40], pick(16)]),                             # 2 NaN member first, second tile used
             np.concatenate([pick(20), [5], pick(12)]),                    # 3 NaN member in the second tile
             np.array([5]), np.array([40]),                                # 4, 5 alone
             pick(64),                                                     # 6 clean, four tiles
             np.concatenate([pick(63), [40]])]                             # 7 NaN member is the last of 64
    G = len(batch)
    bad = [1, 2, 3, 4, 5, 7]
    ptr, idx, seen = seen_csr(G, n, seed=4)
    seen[1] = seen[3]                                                      # (row 1 of seen_csr leaves 3 items)
    ptr, idx = _csr(seen)
    for aggregate in AGGREGATES:
        for N in (10, 128):
            tv, ti, tc = got = run_group(torch, be, f, batch, n, ptr, idx, N, aggregate)
            assert_same(got, oracle(dense, batch, seen, None, N, aggregate))
            assert not np.isnan(tv).any() and not np.isin(ti, [7, 900]).any()
            for b in bad:
                assert tc[b] == 0 and (ti[b] == -1).all() and np.isneginf(tv[b]).all()
            assert tc[0] == N and tc[6] == N


@pytest.mark.parametrize("aggregate", ["min", "max"])
def test_a_nan_member_that_is_not_the_extreme_one_still_removes_the_item(aggregate):
    """v_min_f32 / v_max_f32 return the other operand when one is a NaN: without the explicit flag the item below would
    be returned with the score of the remaining members."""
    torch, layout, be, dev = env().short
    m, n, k = M_USERS, 300, 16
    f = factors(torch, layout, dev, m, n, k, seed=9)
    # a NaN in ONE (member, item) score only: inf * 0 in the dot product of user 11 with item 123.  Everywhere else
    # user 11 is never the extreme member: +inf under "min", -inf under "max", so the group score is the others'
    never = float("inf") if aggregate == "min" else float("-inf")
    f["U"][11, 0] = never
    f["Z"][:, 0] = 1.0
    f["Z"][123, 0] = 0.0
    # ... and make item 123 the best of the other members by far, so that it would win every list if it stayed
    f["b_i"][123] = 50.0
    dense = predict_dense(torch, be, f, m, n, dev)
    assert np.isnan(dense[11, 123]) and np.isnan(dense[11]).sum() == 1 and dense[11, 0] == never
    others = np.array([20, 21, 22])
    assert (dense[others].argmax(axis=1) == 123).all()
    for pos in range(4):                                                   # the NaN member in every position
        g = np.insert(others, pos, 11)
        big = np.concatenate([np.arange(100, 117), [11], np.arange(130, 140)])             # second tile, not row 0
        batch = [g, others, big]
        for N in (1, 10, 128):
            tv, ti, tc = got = run_group(torch, be, f, batch, n, None, None, N, aggregate)
            assert_same(got, oracle(dense, batch, [NONE] * 3, None, N, aggregate))
            assert not (ti[0] == 123).any() and not (ti[2] == 123).any() and ti[1, 0] == 123
            assert tc[0] == min(N, n - 1) and not np.isnan(tv).any()


# ------------------------------------------------------------------------------------------------ model level
def _expected(P32, groups, seen, ok, N, aggregate, exclude=True):
    lists = [np.unique(np.concatenate([seen[u] for u in g])) if exclude else NONE for g in groups]
    tv, ti, _ = gref.group_topn([P32[np.asarray(g)] for g in groups], lists, ok, N, aggregate)
    return ti.astype(np.int64), tv.astype(np.float64)


def _exact_mean(P32, groups):
    """The band of the contract itself, on a fitted model's scores: per group and item the nonzero member scores lie
    within a factor 2^17 of each other, so the fp64 sum is exact in any order."""
    for g in groups:
        a = np.abs(P32[np.asarray(g)])
        assert np.isfinite(a).all()
        assert (a.max(axis=0) <= np.where(a > 0, a, np.inf).min(axis=0) * 2.0 ** 17).all()


def _check_model(model, g, features, with_new_items):
    r, c, _ = g.train
    m, n = g.m, g.n
    P = model.predict(features).astype(np.float32)                         # fp32 values widened: exact round trip
    seen = [np.sort(c[r == u]) for u in range(m)]
    rng = np.random.default_rng(11)
    groups = [rng.permutation(m)[:s] for s in (1, 2, 3, 5, 16, 17, min(40, m), 2, 1)]
    groups.append(groups[3].copy())
    _exact_mean(P, groups)
    for aggregate in AGGREGATES:
        for N in (1, 10, 128):
            items, scores = model.recommend_group(groups, N, aggregate=aggregate, features=features)
            assert items.shape == (len(groups), N) and items.dtype == np.int64 and scores.dtype == np.float64
            ti, tv = _expected(P, groups, seen, None, N, aggregate)
            assert (items == ti).all() and (scores == tv).all()
            for b, grp in enumerate(groups):                               # nothing any member has rated
                for u in grp:
                    assert not np.isin(items[b], seen[u]).any()
        items, scores = model.recommend_group(groups, 10, aggregate=aggregate, features=features, exclude_seen=False)
        ti, tv = _expected(P, groups, seen, None, 10, aggregate, exclude=False)
        assert (items == ti).all() and (scores == tv).all()
        allow = np.random.default_rng(1).random(n) < 0.5                   # filters reach the kernel, three ways
        ti, tv = _expected(P, groups, seen, allow, 10, aggregate)
        for kw in (dict(items=allow), dict(items=np.nonzero(allow)[0]), dict(filter_items=~allow)):
            items, scores = model.recommend_group(groups, 10, aggregate=aggregate, features=features, **kw)
            assert (items == ti).all() and (scores == tv).all()
        ones = np.array([[u] for u in (0, m - 1, m // 2)])                 # a group of one is `recommend`
        a, b = model.recommend_group(ones, 10, aggregate=aggregate, features=features)
        ri, rs = model.recommend(ones[:, 0], 10, features=features)
        assert (a == ri).all() and (b == rs).all()
    if not with_new_items:
        return
    B = 5
    C_new = np.full((B, m), np.nan)
    for b in range(B - 1):                                                 # the last one: no ratings
        C_new[b, rng.permutation(m)[:12]] = rng.integers(1, 6, 12)
    fn = {name: X[:B] for name, X in (g.features or {}).items()} or None
    folded = model.fold_in_items(C_new, features_new=fn)
    Pj = np.concatenate([P, model.predict_new_items(folded).astype(np.float32)], axis=1)
    _exact_mean(Pj, groups)
    sj = [np.concatenate([seen[u], n + np.nonzero(~np.isnan(C_new[:, u]))[0]]) for u in range(m)]
    for aggregate in AGGREGATES:
        items, scores = model.recommend_group(groups, 10, aggregate=aggregate, features=features, new_items=folded)
        ti, tv = _expected(Pj, groups, sj, None, 10, aggregate)
        assert (items == ti).all() and (scores == tv).all()
        only_new = np.arange(n + B) >= n
        items, scores = model.recommend_group(groups, B, aggregate=aggregate, features=features, new_items=folded,
                                              items=only_new)
        ti, tv = _expected(Pj, groups, sj, only_new, B, aggregate)
        assert (items == ti).all() and (scores == tv).all() and (items >= n).any()


@pytest.mark.parametrize("name,use_features,kw,with_new_items", [
    ("g3_empty", True, {}, False),
    ("g4_feat_uw5", True, {}, True),
    ("g4_feat_uw5", False, {}, False),
    ("g5_graph_a5.0", True, {}, False),
    ("g1_plain", True, {"solve_dtype": "float64"}, True),
])
def test_model_recommend_group_on_fixtures(name, use_features, kw, with_new_items):
    env()
    g = Golden(name)
    r, c, v = g.train
    model = model_for(g, device="cuda:0", **kw)
    model.fit_coo(r, c, v, (g.m, g.n), features=g.features or None, tol=g.cfg["tol"], verbose=0)
    _check_model(model, g, (g.features or None) if use_features else None, with_new_items)


# ------------------------------------------------------------------------------------------------ C ABI
def test_bad_arguments_return_the_documented_status():
    import ctypes as C
    torch, layout, be, dev = env().short
    from collaborative_filtering_amd import _hip
    lib = _hip.load()
    m, n, k, G, N = M_USERS, 5000, 64, 8, 10
    f = factors(torch, layout, dev, m, n, k, seed=1)
    groups = [np.arange(3 * b, 3 * b + 3) for b in range(G)]
    gp, gu = (upload(a, dev) for a in _csr(groups))
    tv = torch.full((G, N), 7.0, dtype=torch.float32, device=dev)
    ti = torch.full((G, N), 7, dtype=torch.int32, device=dev)
    tc = torch.full((G,), 7, dtype=torch.int32, device=dev)
    sp = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())          # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    MEAN, MIN, MAX = 0, 1, 2

    def call(k=k, ld=f["ld"], G=G, n=n, topn=N, nslices=0, out=(tv, ti, tc), ws=None, wsb=0, bias=f["b_i"],
             seen=(None, None), aggregate=MIN, max_members=3, members=(gp, gu)):
        return lib.als_group_topk(k, ld, G, p(members[0]), p(members[1]), max_members, n, p(f["U"]), p(f["Z"]),
                                  p(f["b_u"]), p(bias), p(f["mu"]), p(seen[0]), p(seen[1]), None, aggregate, topn,
                                  nslices, p(out[0]), p(out[1]), p(out[2]), p(ws), wsb, stream)
    E_BADARG, E_BADK = -1, -2
    assert call(k=0) == E_BADK and call(k=161) == E_BADK
    assert call(ld=16) == E_BADARG
    assert call(topn=0) == E_BADARG and call(topn=129) == E_BADARG
    assert call(nslices=-1) == E_BADARG and call(nslices=65) == E_BADARG
    assert call(n=0) == E_BADARG and call(n=2 ** 31) == E_BADARG
    assert call(out=(None, ti, tc)) == E_BADARG and call(out=(tv, ti, None)) == E_BADARG and call(bias=None) == E_BADARG
    assert call(members=(None, gu)) == E_BADARG and call(members=(gp, None)) == E_BADARG
    assert call(seen=(sp, None)) == E_BADARG                               # one of the two pointers
    assert call(aggregate=3) == E_BADARG and call(aggregate=-1) == E_BADARG            # an unknown aggregate
    assert call(max_members=65) == E_BADARG and call(max_members=-1) == E_BADARG       # a group over the limit
    need = lib.als_group_workspace_bytes(G, n, N, 4)
    assert need == 4 * G * N * 8
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert call(nslices=4) == E_BADARG and call(nslices=4, ws=ws, wsb=need - 1) == E_BADARG
    assert call(G=0) == 0                                                  # no-op
    torch.cuda.synchronize()
    assert (tv == 7.0).all() and (ti == 7).all() and (tc == 7).all()       # nothing was launched
    dense = predict_dense(torch, be, f, m, n, dev)
    none = [NONE] * G
    for agg, name in ((MEAN, "mean"), (MIN, "min"), (MAX, "max")):
        assert call(nslices=4, ws=ws, wsb=need, aggregate=agg, max_members=64) == 0
        torch.cuda.synchronize()
        if name != "mean":                                                 # (`factors` is not banded)
            assert_same((tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()), oracle(dense, groups, none, None, N, name))
        assert (tc == N).all()
    # max_members bounds what the kernel reads of a group: with 2, every group is its first two members
    assert call(aggregate=MIN, max_members=2, nslices=1) == 0
    torch.cuda.synchronize()
    assert_same((tv.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()),
                oracle(dense, [g[:2] for g in groups], none, None, N, "min"))
    # a group without members: an empty list
    gp0 = upload(np.array([0, 3, 3, 6, 6, 6, 6, 6, 6], np.int64), dev)
    assert call(aggregate=MAX, members=(gp0, gu), nslices=1) == 0
    torch.cuda.synchronize()
    assert tc.tolist() == [N, 0, N, 0, 0, 0, 0, 0]
    assert (ti[1] == -1).all() and torch.isinf(tv[1]).all() and (tv[1] < 0).all()
