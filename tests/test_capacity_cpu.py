"""Top-N under per-item exposure caps (ALS.recommend_capacity, recommend_new_capacity, cv.capacity_at_k) without a GPU:
the numpy reference against itself (threshold rounds == the sorted greedy scan), validation, and the host loop of
serving.py over the stand-in backend of tests/capacity_ref.py - every list compared with == against `greedy` on
`predict()` rows."""
import os

import numpy as np
import pytest
import torch

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CapacityInfo, CoreConfig, _hip, cv, serving
from collaborative_filtering_amd.serving import FoldedItems
from tests import capacity_ref as cref
from tests.synth import make_ratings

M, N_ITEMS, K_F = 24, 310, 5          # n not a multiple of 32, ten bitmap words


@pytest.fixture(scope="module")
def fitted():
    r, c, v = make_ratings(M, N_ITEMS, 900, seed=5, empty_users=(3,))
    cfg = ALSConfig(core=CoreConfig(n_factors=K_F, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    model = ALS(cfg, device="cpu", backend=cref.CapacityNumpyBackend()).fit_coo(r, c, v, (M, N_ITEMS), tol=None,
                                                                                verbose=0)
    seen = [np.sort(c[r == u]) for u in range(M)]
    return model, seen


def _folded(rng, B=9):
    Z = rng.normal(size=(B, K_F)).astype(np.float32).astype(np.float64)
    return FoldedItems(Z.copy(), rng.normal(size=B).astype(np.float32).astype(np.float64) + 1.0, Z, None,
                       (np.zeros(B + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)))


def _mixed_capacity(rng, n, B):
    return rng.choice([0, 1, 3, B + 1], size=n).astype(np.int64)


def _assert_lists(got, want):
    assert got[0].dtype == np.int64 and got[1].dtype == np.float64
    assert (got[0] == want[0]).all(), np.argwhere(got[0] != want[0])[:5]
    assert (got[1] == want[1]).all()


# ------------------------------------------------------------------------------------------ the reference itself
def test_keys_order_pairs_by_score_then_row():
    s = np.array([1.0, 1.0, -0.0, 0.0, -2.5, np.inf, -np.inf], np.float32)
    k = cref.make_key(s, np.array([3, 2, 0, 1, 0, 9, 9]))
    assert k.dtype == np.uint64 and (k > 0).all()
    assert k[5] > k[1] > k[0] > k[2] > k[3] > k[4] > k[6]                  # equal scores: the lower row is larger
    assert cref.make_key(np.float32(-0.0), 7) == cref.make_key(np.float32(0.0), 7)


@pytest.mark.parametrize("seed", range(60))
def test_rounds_model_equals_greedy_on_tie_heavy_instances(seed):
    rng = np.random.default_rng(seed)
    B, n, N = int(rng.integers(1, 41)), int(rng.integers(1, 61)), int(rng.integers(1, 8))
    scores = (rng.integers(-3, 4, size=(B, n)) * 0.5).astype(np.float32)   # quantised: ties everywhere
    scores[rng.random((B, n)) < 0.02] = np.nan
    seen = [np.nonzero(rng.random(n) < rng.choice([0.0, 0.3, 0.9]))[0] for _ in range(B)]
    allowed = None if seed % 3 == 0 else rng.random(n) < 0.7
    capacity = rng.choice([0, 1, 2, 5, B + 3], size=n)
    want = cref.greedy(scores, seen, allowed, capacity, N)
    for dirty_only in (True, False):
        ti, tv, fill, rounds, walked = cref.rounds_model(scores, seen, allowed, capacity, N, dirty_only)
        assert (ti == want[0]).all() and (tv == want[1]).all() and (fill == want[2]).all()
        assert walked <= (rounds + 1) * B
    assert (want[2] <= capacity).all() and (want[2] == np.bincount(want[0][want[0] >= 0], minlength=n)).all()


def test_settle_reference_on_a_hand_made_batch():
    # three rows want item 0 (capacity 2): rows 0 and 1 tie on the score, the lower row has priority; row 2 scores less
    ti = np.array([[0, 1], [0, 2], [0, -1]], np.int32)
    tv = np.array([[2.0, 1.0], [2.0, 1.0], [1.5, -np.inf]], np.float32)
    floor, fill, dirty, n_over = cref.settle(ti, tv, np.array([2, 1, 1]), np.zeros(3, np.uint64))
    assert n_over == 1 and fill.tolist() == [2, 1, 1] and dirty.tolist() == [0, 0, 1]
    assert floor[0] == cref.make_key(np.float32(2.0), 1) and floor[1] == 0 and floor[2] == 0
    floor, fill, dirty, n_over = cref.settle(ti, tv, np.array([1, 1, 1]), np.zeros(3, np.uint64))
    assert floor[0] == cref.make_key(np.float32(2.0), 0) and dirty.tolist() == [0, 1, 1]
    floor, fill, dirty, n_over = cref.settle(ti, tv, np.array([0, 1, 1]), np.zeros(3, np.uint64))
    assert floor[0] == np.uint64(0xFFFFFFFFFFFFFFFF) and fill[0] == 0 and dirty.tolist() == [1, 1, 1]


# ------------------------------------------------------------------------------------------ exports, validation
def test_exports_and_header_name_the_new_entry_points():
    for name in ("als_recommend_topk_priced", "als_capacity_settle", "als_capacity_settle_workspace_bytes"):
        assert name in _hip.EXPORTS
    assert "als_capacity_settle_workspace_bytes" in _hip.SIZE_QUERIES
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "als_hip.h")).read()
    assert "int als_recommend_topk_priced(" in text and "int als_capacity_settle(" in text
    assert "size_t als_capacity_settle_workspace_bytes(" in text
    assert "capacity.hip" in open(os.path.join(root, "collaborative-filtering_amd", "csrc", "Makefile")).read()


def test_arguments_are_validated(fitted, monkeypatch):
    model = fitted[0]
    with pytest.raises(TypeError):
        model.recommend_capacity([0, 1], 5)                                # capacity is required
    with pytest.raises(ValueError, match="None is not accepted"):
        model.recommend_capacity([0, 1], 5, capacity=None)
    with pytest.raises(ValueError, match="Expected number of items"):
        model.recommend_capacity([0, 1], 5, capacity=np.ones(N_ITEMS - 1, np.int64))
    with pytest.raises(ValueError, match="Expected number of items"):
        model.recommend_capacity([0, 1], 5, capacity=np.ones((N_ITEMS, 1), np.int64))
    with pytest.raises(ValueError, match="integers"):
        model.recommend_capacity([0, 1], 5, capacity=np.ones(N_ITEMS))     # float dtype
    with pytest.raises(ValueError, match="integers"):
        model.recommend_capacity([0, 1], 5, capacity=np.ones(N_ITEMS, bool))
    with pytest.raises(ValueError, match="integers"):
        model.recommend_capacity([0, 1], 5, capacity=2.0)
    with pytest.raises(ValueError, match="negative"):
        model.recommend_capacity([0, 1], 5, capacity=-1)
    neg = np.ones(N_ITEMS, np.int64)
    neg[7] = -2
    with pytest.raises(ValueError, match="negative"):
        model.recommend_capacity([0, 1], 5, capacity=neg)
    with pytest.raises(ValueError):
        model.recommend_capacity([0, 1], 129, capacity=1)
    with pytest.raises(IndexError):
        model.recommend_capacity([0, M], 5, capacity=1)
    for bad in (-1, 1.5, True, "2"):
        with pytest.raises(ValueError, match="max_rounds"):
            model.recommend_capacity([0, 1], 5, capacity=1, max_rounds=bad)
    folded = _folded(np.random.default_rng(0))
    with pytest.raises(ValueError, match="Expected number of items"):      # the capacities span n + B ids
        model.recommend_capacity([0], 5, capacity=np.ones(N_ITEMS, np.int64), new_items=folded)
    with pytest.raises(ValueError, match="None is not accepted"):
        model.recommend_new_capacity(np.full((2, N_ITEMS), np.nan), 5, capacity=None)
    # the named limit on B N, looked up at call time
    assert serving.CAPACITY_MAX_PAIRS == 1 << 26
    monkeypatch.setattr(serving, "CAPACITY_MAX_PAIRS", 9)
    with pytest.raises(ValueError, match="CAPACITY_MAX_PAIRS"):
        model.recommend_capacity([0, 1], 5, capacity=1)
    model.recommend_capacity([0, 1, 2], 3, capacity=1)
    empty = model.recommend_capacity([], 4, capacity=1, return_info=True)
    assert empty[0].shape == (0, 4) and empty[1].shape == (0, 4) and empty[2].rounds == 0
    assert empty[2].fill.shape == (N_ITEMS,) and np.isnan(empty[2].cutoff).all()


# ------------------------------------------------------------------------------------------ the host loop
@pytest.mark.parametrize("exclude_seen", [True, False])
def test_host_loop_equals_greedy_on_predict_rows(fitted, monkeypatch, exclude_seen):
    model, seen = fitted
    be = model._eng.be
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)         # REC_BATCH below B, and below the work lists
    rng = np.random.default_rng(3)
    P = model.predict()
    users = np.concatenate([np.arange(M)[::-1], np.arange(M), [5, 5, 5]])  # duplicates: separate rows
    B = users.size
    rows_seen = [seen[u] if exclude_seen else np.zeros(0, np.int64) for u in users]
    none = [np.zeros(0, np.int64)] * B
    cap = _mixed_capacity(rng, N_ITEMS, B)
    for N in (1, 7):
        del be.calls[:]
        got = model.recommend_capacity(users, N, capacity=cap, exclude_seen=exclude_seen, return_info=True)
        want = cref.greedy(P[users], rows_seen, None, cap, N)
        _assert_lists(got, want)
        info = got[2]
        assert isinstance(info, CapacityInfo) and info.rounds >= 2 and info.walked_rows < (info.rounds + 1) * B
        assert info.fill.dtype == np.int64 and (info.fill == want[2]).all() and (info.fill <= cap).all()
        assert (info.fill == np.bincount(got[0][got[0] >= 0], minlength=N_ITEMS)).all()
        full = (info.fill == cap) & (cap > 0)
        assert np.isnan(info.cutoff[~full]).all() and full.any()
        for i in np.nonzero(full)[0]:
            assert info.cutoff[i] == got[1][got[0] == i].min()
        # round 0 walks all rows in chunks of 7; every settle sees the whole batch
        walks = [c[1] for c in be.calls if c[0] == "recommend_topk_priced"]
        assert walks[: (B + 6) // 7] == [7] * (B // 7) + ([B % 7] if B % 7 else []) and max(walks) <= 7
        assert sum(walks) == info.walked_rows
        assert [c for c in be.calls if c[0] == "capacity_settle"] == [("capacity_settle", B)] * (info.rounds + 1)
    # both filters, an id list and a mask
    allow = rng.permutation(N_ITEMS)[:220]
    block = rng.random(N_ITEMS) < 0.2
    ok = np.isin(np.arange(N_ITEMS), allow) & ~block
    got = model.recommend_capacity(users, 7, capacity=cap, exclude_seen=exclude_seen, items=allow, filter_items=block)
    _assert_lists(got, cref.greedy(P[users], rows_seen, ok, cap, 7))
    assert ok[got[0][got[0] >= 0]].all()
    # a scalar capacity; users=None: all m users in id order
    got = model.recommend_capacity(None, 7, capacity=2, exclude_seen=exclude_seen)
    _assert_lists(got, cref.greedy(P, rows_seen[M: 2 * M] if exclude_seen else none[:M], None,
                                   np.full(N_ITEMS, 2), 7))


def test_new_items_span_the_joint_catalogue(fitted, monkeypatch):
    model, seen = fitted
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)
    rng = np.random.default_rng(6)
    folded = _folded(rng)
    nt = N_ITEMS + folded.n_items
    users = np.concatenate([rng.integers(0, M, 30), np.arange(M)])
    B = users.size
    P = np.concatenate([model.predict()[users], model.predict_new_items(folded, users)], axis=1)
    cap = _mixed_capacity(rng, nt, B)
    cap[N_ITEMS:] = [1, 1, 2, 0, 3, B + 1, 1, 1, 2]
    block = rng.random(nt) < 0.1
    got = model.recommend_capacity(users, 7, capacity=cap, new_items=folded, filter_items=block, return_info=True)
    want = cref.greedy(P, [seen[u] for u in users], ~block, cap, 7)
    _assert_lists(got, want)
    assert (got[0] >= N_ITEMS).any() and got[2].fill.shape == (nt,) and (got[2].fill == want[2]).all()


def _new_user_scores(model, R_new):
    """The score rows of folded-in users: the predict epilogue on their folded factors, through the model's backend."""
    eng = model._eng
    U, b = model.fold_in(R_new)
    Ut = torch.zeros(U.shape[0], eng.ld, dtype=torch.float32)
    Ut[:, : eng.k] = torch.from_numpy(U).float()
    out = torch.empty(U.shape[0], eng.n, dtype=torch.float32, device=eng.dev)
    eng.be.predict_dense(k=eng.k, ld=eng.ld, m=U.shape[0], n=eng.n, U=Ut.to(eng.dev), Z=eng.V,
                         b_u=torch.from_numpy(b).float().to(eng.dev), b_i=eng.b_i, mu=eng.mu, out=out)
    return out.cpu().numpy().astype(np.float64)


def test_recommend_new_capacity_equals_greedy(fitted, monkeypatch):
    model = fitted[0]
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)
    rng = np.random.default_rng(4)
    B = 40
    R_new = np.full((B, N_ITEMS), np.nan)
    for b in range(B):
        if b != 4:                                                         # one row without ratings
            R_new[b, rng.permutation(N_ITEMS)[: 3 + b % 9]] = rng.integers(1, 6, 3 + b % 9)
    R_new[20:] = R_new[:20]                                                # every row twice: ties across rows
    P = _new_user_scores(model, R_new)
    cap = _mixed_capacity(rng, N_ITEMS, B)
    for exclude_seen in (True, False):
        rows_seen = [np.nonzero(~np.isnan(R_new[b]))[0] if exclude_seen else np.zeros(0, np.int64) for b in range(B)]
        got = model.recommend_new_capacity(R_new, 6, capacity=cap, exclude_seen=exclude_seen, return_info=True)
        want = cref.greedy(P, rows_seen, None, cap, 6)
        _assert_lists(got, want)
        assert got[2].rounds >= 1 and (got[2].fill == want[2]).all()


def test_loose_capacity_is_recommend_with_zero_rounds(fitted):
    model = fitted[0]
    users = np.concatenate([np.arange(M), np.arange(M)])
    for cap in (users.size, np.full(N_ITEMS, users.size + 5)):
        got = model.recommend_capacity(users, 9, capacity=cap, return_info=True)
        want = model.recommend(users, 9)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
        assert got[2].rounds == 0 and got[2].walked_rows == users.size and np.isnan(got[2].cutoff).all()
    assert len(model.recommend_capacity(users, 9, capacity=users.size)) == 2


def test_short_rows_when_the_capacity_runs_out(fitted):
    model, seen = fitted
    users = np.arange(M)
    cap = np.zeros(N_ITEMS, np.int64)
    cap[::9] = 1                                                           # 35 units for 24 x 7 slots
    got = model.recommend_capacity(users, 7, capacity=cap, return_info=True)
    want = cref.greedy(model.predict(), seen, None, cap, 7)
    _assert_lists(got, want)
    assert (got[0] == -1).any() and np.isneginf(got[1][got[0] == -1]).all() and got[2].fill.sum() <= cap.sum()


def test_max_rounds_raises_on_a_contested_instance(fitted):
    model = fitted[0]
    users = np.concatenate([np.arange(M), np.arange(M)])
    info = model.recommend_capacity(users, 7, capacity=1, return_info=True)[2]
    assert info.rounds >= 2
    with pytest.raises(RuntimeError, match="max_rounds"):
        model.recommend_capacity(users, 7, capacity=1, max_rounds=1)
    model.recommend_capacity(users, 7, capacity=1, max_rounds=info.rounds)  # enough: no error


# ------------------------------------------------------------------------------------------ cv
def test_capacity_at_k_hand_checked(fitted):
    model = fitted[0]
    users = np.array([0, 1])
    top = model.recommend(users, 3)[0]
    # held out: each user's best item; under capacity 1 everywhere the lists stay disjoint
    rows, cols = users, top[:, 0]
    loose = cv.capacity_at_k(model, rows, cols, K=3, capacity=M)
    assert loose["users"] == 2 and loose["rounds"] == 0
    assert loose["recall@K"] == loose["recall@K_uncapped"] == 1.0
    assert loose["ndcg@K"] == pytest.approx(loose["ndcg@K_uncapped"], abs=1e-15) and loose["ndcg@K"] == 1.0
    tight = cv.capacity_at_k(model, rows, cols, K=3, capacity=1)
    capped = model.recommend_capacity(users, 3, capacity=1)[0]
    assert np.unique(capped).size == 6
    assert tight["max_exposure"] == 1 and tight["coverage@K"] == pytest.approx(6 / N_ITEMS, abs=1e-15)
    assert tight["gini_exposure"] == pytest.approx(1.0 - 6 / N_ITEMS, abs=1e-12)
    assert tight["max_exposure_uncapped"] == int(np.bincount(top.ravel()).max())
    hit = [(cols[j] in capped[j]) for j in range(2)]
    assert tight["recall@K"] == pytest.approx(np.mean(hit), abs=1e-15)
    assert tight["recall@K_uncapped"] == 1.0
    with pytest.raises(ValueError):
        cv.capacity_at_k(model, rows, cols, K=3, capacity=None)
