"""Per-user item eligibility (ALS.eligibility, recommend_eligible, recommend_new_eligible, rank_of_eligible,
cv.eligible_ranking_at_k) without a GPU: validation, packing of tags and rules against the numpy definition, and the
host orchestration over the stand-in backend of tests/eligible_ref.py - every result compared with == against the loop
over segments of the existing filtered calls."""
import os

import numpy as np
import pytest
import torch

from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, ItemEligibility, _hip, cv, serving
from collaborative_filtering_amd.serving import FoldedItems
from tests import eligible_ref as eref
from tests.synth import make_ratings

M, N_ITEMS, K_F = 24, 310, 5          # n not a multiple of 32, ten bitmap words
S = 4


@pytest.fixture(scope="module")
def fitted():
    r, c, v = make_ratings(M, N_ITEMS, 900, seed=5, empty_users=(3,))
    cfg = ALSConfig(core=CoreConfig(n_factors=K_F, n_iters=3, lambda_u=2.0, lambda_v=2.0),
                    biases=BiasesConfig(lambda_bu=1.0, lambda_bi=1.0))
    model = ALS(cfg, device="cpu", backend=eref.EligibleNumpyBackend()).fit_coo(r, c, v, (M, N_ITEMS), tol=None,
                                                                                verbose=0)
    return model, r, c


def _masks(rng, n=N_ITEMS):
    """S segment masks: random half, everything, nothing, one item."""
    masks = np.zeros((S, n), dtype=bool)
    masks[0] = rng.random(n) < 0.5
    masks[1] = True
    masks[3, n - 1] = True
    return masks


def _table(e):
    return e.table.numpy().view(np.uint32)


def _folded(model, rng, B=9):
    Z = rng.normal(size=(B, K_F)).astype(np.float32).astype(np.float64)
    return FoldedItems(Z.copy(), rng.normal(size=B).astype(np.float32).astype(np.float64) + 1.0, Z, None,
                       (np.zeros(B + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float32)))


# ------------------------------------------------------------------------------------------ validation
def test_exports_name_the_new_entry_points():
    for name in ("als_recommend_topk_segmented", "als_rank_count_segmented", "als_eligibility_bitmaps"):
        assert name in _hip.EXPORTS
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                             "als_hip.h")).read()
    assert "int als_recommend_topk_segmented(" in text and "int als_eligibility_bitmaps(" in text


def test_table_inputs_are_validated(fitted, monkeypatch):
    model = fitted[0]
    masks = _masks(np.random.default_rng(0))
    tags = np.zeros((N_ITEMS, 3), dtype=bool)
    rules = {"forbid": np.zeros((S, 3), dtype=bool)}
    with pytest.raises(ValueError, match="exactly one"):
        model.eligibility()
    with pytest.raises(ValueError, match="exactly one"):
        model.eligibility(masks, item_tags=tags, rules=rules)
    with pytest.raises(ValueError):
        model.eligibility(masks[:, :-1])                                   # not n_total columns
    with pytest.raises(ValueError):
        model.eligibility([[0, 1], [N_ITEMS]])                             # an id outside the catalogue
    with pytest.raises(ValueError):
        model.eligibility(item_tags=tags)                                  # tags without rules
    with pytest.raises(ValueError):
        model.eligibility(item_tags=tags, rules={"forbid": np.zeros((S, 4), dtype=bool)})     # another width
    with pytest.raises(ValueError):
        model.eligibility(item_tags=np.zeros((N_ITEMS, 257), dtype=bool),
                          rules={"forbid": np.zeros((S, 257), dtype=bool)})
    with pytest.raises(ValueError):
        model.eligibility(item_tags=tags, rules={"forbidden": np.zeros((S, 3), dtype=bool)})
    # the byte limit, named and looked up at call time: S = 4 segments x 10 words x 4 bytes = 160 bytes
    assert serving.ELIGIBILITY_MAX_BYTES == 1 << 30
    monkeypatch.setattr(serving, "ELIGIBILITY_MAX_BYTES", 159)
    with pytest.raises(ValueError, match="ELIGIBILITY_MAX_BYTES"):
        model.eligibility(masks)
    with pytest.raises(ValueError, match="ELIGIBILITY_MAX_BYTES"):
        model.eligibility(item_tags=tags, rules=rules)
    monkeypatch.setattr(serving, "ELIGIBILITY_MAX_BYTES", 160)
    e = model.eligibility(masks)
    assert isinstance(e, ItemEligibility) and e.n_segments == S and e.n_items == N_ITEMS


def test_call_arguments_are_validated(fitted):
    model = fitted[0]
    rng = np.random.default_rng(1)
    e = model.eligibility(_masks(rng))
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        model.recommend_eligible([0, 1], 5, eligibility=e, segments=[0, S])
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        model.recommend_eligible([0, 1], 5, eligibility=e, segments=[-1, 0])
    with pytest.raises(ValueError, match="one per"):
        model.recommend_eligible([0, 1], 5, eligibility=e, segments=[0])
    with pytest.raises(ValueError, match="one per"):
        model.recommend_eligible(None, 5, eligibility=e, segments=np.zeros(M - 1, np.int64))    # users=None: m rows
    with pytest.raises(ValueError):
        model.recommend_eligible([0], 5, eligibility=e, segments=[0.0])
    with pytest.raises(ValueError):
        model.recommend_eligible([0], 5, eligibility=e, segments=None)
    with pytest.raises(ValueError):
        model.recommend_eligible([0], 5, eligibility=e.table, segments=[0])                   # not an ItemEligibility
    with pytest.raises(ValueError):
        model.recommend_eligible([0], 129, eligibility=e, segments=[0])
    folded = _folded(model, rng)
    with pytest.raises(ValueError, match="Expected number of items"):
        model.recommend_eligible([0], 5, eligibility=e, segments=[0], new_items=folded)       # table over n, not n + B
    ej = model.eligibility(np.ones((2, N_ITEMS + folded.n_items), dtype=bool), new_items=folded)
    assert ej.n_items == N_ITEMS + 9
    with pytest.raises(ValueError, match="Expected number of items"):
        model.recommend_eligible([0], 5, eligibility=ej, segments=[0])
    with pytest.raises(ValueError, match="Expected number of items"):
        model.rank_of_eligible([0], [1], eligibility=ej, segments=[0])
    R_new = np.full((2, N_ITEMS), np.nan)
    with pytest.raises(ValueError, match="one per"):
        model.recommend_new_eligible(R_new, 5, eligibility=e, segments=[0])
    with pytest.raises(ValueError, match="same segment"):
        model.rank_of_eligible([2, 5, 2], [1, 1, 7], eligibility=e, segments=[0, 1, 1])
    with pytest.raises(ValueError, match="one per"):
        model.rank_of_eligible([2, 5], [1, 1], eligibility=e, segments=[0])
    model.rank_of_eligible([2, 5, 2], [1, 1, 7], eligibility=e, segments=[1, 0, 1])             # consistent: accepted


# ------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("A", [1, 32, 33, 256])
def test_bool_tags_and_rules_pack_to_the_numpy_definition(fitted, A):
    model = fitted[0]
    rng = np.random.default_rng(10 + A)
    tags = rng.random((N_ITEMS, A)) < 0.5
    need_all = rng.random((S, A)) < 1.5 / A
    need_any = rng.random((S, A)) < 3.0 / A
    forbid = rng.random((S, A)) < 1.0 / A
    need_any[1] = False                                                    # an empty need_any asks for nothing
    forbid[2] = True                                                       # everything with a tag is out
    want_bool = eref.eligible_bool(tags, need_all, need_any, forbid)
    e = model.eligibility(item_tags=tags, rules=dict(need_all=need_all, need_any=need_any, forbid=forbid))
    assert e.n_segments == S and tuple(e.table.shape) == (S, (N_ITEMS + 31) // 32)
    assert (_table(e) == eref.table_numpy(want_bool)).all()
    # the packed words, given directly, and a rule left out
    tw = (A + 31) // 32
    words = lambda b: np.stack([[sum(int(v) << j for j, v in enumerate(row[32 * w: 32 * w + 32])) for w in range(tw)]
                                for row in b]).astype(np.uint32)           # noqa: E731
    e2 = model.eligibility(item_tags=words(tags), rules=dict(need_all=words(need_all), need_any=words(need_any),
                                                             forbid=words(forbid)))
    assert (_table(e2) == _table(e)).all()
    e3 = model.eligibility(item_tags=tags, rules=dict(forbid=forbid))
    assert (_table(e3) == eref.table_numpy(eref.eligible_bool(tags, None, None, forbid))).all()
    # items / filter_items go into every segment
    allow = rng.permutation(N_ITEMS)[:200]
    block = rng.random(N_ITEMS) < 0.2
    base = np.isin(np.arange(N_ITEMS), allow) & ~block
    e4 = model.eligibility(item_tags=tags, rules=dict(need_all=need_all, forbid=forbid), items=allow,
                           filter_items=block)
    assert (_table(e4) == eref.table_numpy(eref.eligible_bool(tags, need_all, None, forbid, base))).all()


def test_segment_items_forms_and_global_filters(fitted):
    model = fitted[0]
    rng = np.random.default_rng(2)
    masks = _masks(rng)
    e = model.eligibility(masks)
    assert e.table.dtype == torch.int32 and (_table(e) == eref.table_numpy(masks)).all()
    lists = [np.nonzero(mk)[0][::-1] for mk in masks]                       # id lists, any order
    lists[0] = np.concatenate([lists[0], lists[0][:5]])                     # duplicates
    assert (_table(model.eligibility(lists)) == _table(e)).all()
    block = rng.random(N_ITEMS) < 0.3
    ef = model.eligibility(masks, filter_items=block, items=np.arange(5, N_ITEMS))
    keep = ~block
    keep[:5] = False
    assert (_table(ef) == eref.table_numpy(masks & keep)).all()
    seg, it = rng.integers(0, S, 500), rng.integers(0, N_ITEMS, 500)
    assert (ef.allowed(seg, it) == (masks & keep)[seg, it]).all()


# ------------------------------------------------------------------------------------------ orchestration
def _loop_recommend(model, users, seg, masks, N, **kw):
    """The parent's way: one filtered `recommend` per segment over the rows of that segment."""
    items = np.full((users.size, N), -7, np.int64)
    scores = np.full((users.size, N), np.nan)
    for s in np.unique(seg):
        rows = np.nonzero(seg == s)[0]
        items[rows], scores[rows] = model.recommend(users[rows], N, items=masks[s], **kw)
    return items, scores


@pytest.mark.parametrize("exclude_seen", [True, False])
def test_recommend_eligible_is_the_loop_over_segments(fitted, monkeypatch, exclude_seen):
    model = fitted[0]
    be = model._eng.be
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)         # the chunks cut through the segments
    rng = np.random.default_rng(3)
    masks = _masks(rng)
    e = model.eligibility(masks)
    users = np.concatenate([np.arange(M)[::-1], [5, 5, 5, 5]])             # one user under every segment at the end
    seg = np.concatenate([rng.integers(0, S, M), np.arange(4)])
    for N in (1, 10, 128):
        del be.calls[:]
        got = model.recommend_eligible(users, N, eligibility=e, segments=seg, exclude_seen=exclude_seen)
        assert [c[0] for c in be.calls] == ["recommend_topk_segmented"] * 4 and [c[1] for c in be.calls] == [7, 7, 7, 7]
        want = _loop_recommend(model, users, seg, masks, N, exclude_seen=exclude_seen)
        assert got[0].dtype == np.int64 and got[1].dtype == np.float64
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
        assert (got[0][seg == 2] == -1).all() and np.isneginf(got[1][seg == 2]).all()         # the empty segment
    # users=None: m rows in id order; segments as a tensor
    seg_all = rng.integers(0, S, M)
    got = model.recommend_eligible(None, 6, eligibility=e, segments=torch.from_numpy(seg_all))
    want = _loop_recommend(model, np.arange(M), seg_all, masks, 6)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    empty = model.recommend_eligible([], 6, eligibility=e, segments=[])
    assert empty[0].shape == (0, 6) and empty[1].shape == (0, 6)


def test_all_ones_segment_is_recommend(fitted):
    model = fitted[0]
    e = model.eligibility(np.ones((1, N_ITEMS), dtype=bool))
    got = model.recommend_eligible(None, 9, eligibility=e, segments=np.zeros(M, np.int64))
    want = model.recommend(None, 9)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()


def test_recommend_new_eligible_is_the_loop_over_segments(fitted, monkeypatch):
    model, r, c = fitted
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)
    rng = np.random.default_rng(4)
    masks = _masks(rng)
    e = model.eligibility(masks)
    B = 17
    R_new = np.full((B, N_ITEMS), np.nan)
    for b in range(B):
        if b != 4:                                                         # one row without ratings
            R_new[b, rng.permutation(N_ITEMS)[: 3 + b]] = rng.integers(1, 6, 3 + b)
    seg = rng.integers(0, S, B)
    got = model.recommend_new_eligible(R_new, 12, eligibility=e, segments=seg)
    for s in np.unique(seg):
        rows = np.nonzero(seg == s)[0]
        want = model.recommend_new(R_new[rows], 12, items=masks[s])
        assert (got[0][rows] == want[0]).all() and (got[1][rows] == want[1]).all()
    got0 = model.recommend_new_eligible(R_new, 12, eligibility=e, segments=seg, exclude_seen=False, n_sweeps=2)
    for s in np.unique(seg):
        rows = np.nonzero(seg == s)[0]
        want = model.recommend_new(R_new[rows], 12, items=masks[s], exclude_seen=False, n_sweeps=2)
        assert (got0[0][rows] == want[0]).all() and (got0[1][rows] == want[1]).all()


def test_rank_of_eligible_is_the_loop_over_segments(fitted, monkeypatch):
    model = fitted[0]
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)
    rng = np.random.default_rng(5)
    masks = _masks(rng)
    e = model.eligibility(masks)
    seg_of = rng.integers(0, S, M)
    P = 150
    u = rng.integers(0, M, P)
    u[:20] = 11                                                            # more than 16 targets on one row
    it = rng.integers(0, N_ITEMS, P)
    got = model.rank_of_eligible(u, it, eligibility=e, segments=seg_of[u])
    for s in np.unique(seg_of[u]):
        p = np.nonzero(seg_of[u] == s)[0]
        want = model.rank_of(u[p], it[p], allow_items=masks[s])
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and (g[p] == w).all()
    # the position recommend_eligible gives an item is its rank
    top, _ = model.recommend_eligible(np.arange(M), 10, eligibility=e, segments=seg_of)
    uu, jj = np.nonzero(top >= 0)
    rank, _, _ = model.rank_of_eligible(uu, top[uu, jj], eligibility=e, segments=seg_of[uu])
    assert (rank == jj).all()


def test_new_items_path_spans_the_joint_catalogue(fitted, monkeypatch):
    model = fitted[0]
    monkeypatch.setattr(model._eng, "REC_BATCH", 7, raising=False)
    rng = np.random.default_rng(6)
    folded = _folded(model, rng)
    nt = N_ITEMS + folded.n_items
    masks = _masks(rng, nt)
    masks[0, N_ITEMS: N_ITEMS + 4] = True                                  # folded ids inside ...
    masks[0, N_ITEMS + 4:] = False                                         # ... and outside segment 0
    e = model.eligibility(masks, new_items=folded)
    users = rng.integers(0, M, 20)
    seg = rng.permutation(np.arange(M) % S)[users]                         # one segment per user id: rank_of_eligible below
    got = model.recommend_eligible(users, 128, eligibility=e, segments=seg, new_items=folded)
    want = _loop_recommend(model, users, seg, masks, 128, new_items=folded)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    assert (got[0][seg == 1] >= N_ITEMS).any() and not (got[0][seg == 0] >= N_ITEMS + 4).any()
    uu, jj = np.nonzero(got[0][:, :10] >= 0)
    rank, ncand, _ = model.rank_of_eligible(users[uu], got[0][uu, jj], eligibility=e, segments=seg[uu],
                                            new_items=folded)
    assert (rank == jj).all()


def test_rank_of_eligible_with_new_items_row_by_row(fitted):
    model = fitted[0]
    rng = np.random.default_rng(7)
    folded = _folded(model, rng)
    nt = N_ITEMS + folded.n_items
    masks = _masks(rng, nt)
    e = model.eligibility(masks, new_items=folded)
    for u, s in ((0, 0), (0, 1), (9, 3), (9, 2)):
        top, _ = model.recommend_eligible([u], 20, eligibility=e, segments=[s], new_items=folded)
        j = np.nonzero(top[0] >= 0)[0]
        rank, ncand, _ = model.rank_of_eligible(np.full(j.size + 1, u), np.append(top[0, j], nt - 1), eligibility=e,
                                                segments=np.full(j.size + 1, s), new_items=folded)
        assert (rank[:-1] == j).all()
        seen = model._seen_pairs(np.full(N_ITEMS, u), np.arange(N_ITEMS))
        assert (ncand == (masks[s, :N_ITEMS] & ~seen).sum() + masks[s, N_ITEMS:].sum()).all()


# ------------------------------------------------------------------------------------------ cv
def test_eligible_ranking_at_k_hand_checked(fitted):
    model = fitted[0]
    seg_of = np.zeros(M, np.int64)
    seg_of[1] = 1
    top0 = model.recommend([0], 3)[0][0]                                   # user 0, everything eligible
    masks = np.ones((2, N_ITEMS), dtype=bool)
    masks[1, top0[0]] = True
    block1 = model.recommend([1], 1)[0][0]                                 # user 1's best item is not eligible for them
    masks[1, block1[0]] = False
    top1 = model.recommend([1], 3, items=masks[1])[0][0]
    e = model.eligibility(masks)
    # held out: user 0 - their 2nd item and one far down the list; user 1 - their 1st eligible item, and the blocked one
    far = model.recommend([0], 128)[0][0][100]
    rows = np.array([0, 0, 1, 1])
    cols = np.array([top0[1], far, top1[0], block1[0]])
    out = cv.eligible_ranking_at_k(model, rows, cols, K=3, eligibility=e, segments_of_user=seg_of)
    d = lambda r: 1.0 / np.log2(r + 1)                                      # noqa: E731
    assert out["users"] == 2 and out["ineligible"] == 1
    assert out["recall@K"] == pytest.approx((0.5 + 1.0) / 2, abs=1e-15)
    assert out["ndcg@K"] == pytest.approx((d(2) / (d(1) + d(2)) + 1.0) / 2, abs=1e-15)
    # nothing left: NaN means, every pair counted
    none = cv.eligible_ranking_at_k(model, [1], [block1[0]], K=3, eligibility=e, segments_of_user=seg_of)
    assert none["users"] == 0 and none["ineligible"] == 1 and np.isnan(none["recall@K"])
    with pytest.raises(ValueError):
        cv.eligible_ranking_at_k(model, rows, cols, K=3, eligibility=e, segments_of_user=seg_of[:-1])
