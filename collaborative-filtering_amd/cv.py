"""Sparse-native cross-validation / ablation harness around `ALS` (SURVEY.md section 8(f), row n1 + n3).

The reference drives `fit` / `predict` from two dense loops
(`scripts/evaluate_models.py:194-276`, `scripts/tune_params.py:341-421`): every fold materialises
dense NaN train / valid matrices (`scripts/create_folds.py:177-208`) and a dense m x n prediction
that is then read at the validation flat indices only (`scripts/tune_params.py:147-167`).  This
module restates that caller on COO triplets and flat indices - `fit_coo` + `predict_at`, nothing
m x n - with the same fold files, the same metrics, the same statistics and the same artifact
schema, so that results can be compared file by file:

  folds        make_entrywise_folds / save_folds_npz / load_folds_npz   create_folds.py:50-149
  split        train_valid_split                                        create_folds.py:152-208
  metrics      rmse_at, popularity_bins, split_by_popularity            tune_params.py:147-167,
                                                                        evaluate_models.py:131-191
               ranking_at_k (recall@K / NDCG@K of ALS.recommend)        new: the reference has RMSE only
               rank_metrics (recall / NDCG at any K, MRR, AUC, MPR from ALS.rank_of)    new
  statistics   aggregate_convergence, aggregate_bins_mean,              evaluate_models.py:279-379
               sign_test_paired, fdr_bh
  variants     variant_grid                                             evaluate_models.py:382-455
  drivers      eval_variant_cv, run_ablation                            evaluate_models.py:194-276, 708-862

Plots (matplotlib) and the Optuna search are not part of it.
"""
from __future__ import annotations

import csv
import json
import math
import os
import time
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import validate
from .als import ALS
from .helpers import DEFAULT_RANDOM_STATE, ES_MIN_ITERS, ES_TOL, make_config, normalize_params

N_POP_BINS = 5                     # evaluate_models.py:108
POP_BIN_STRATEGY = "quantile"      # evaluate_models.py:109


# ------------------------------------------------------------------------------- ratings container
@dataclass
class CooRatings:
    """Observed ratings, row-major sorted; `flat = rows * n + cols` is the reference's index space
    (create_folds.py:76, tune_params.py:165-166)."""
    rows: np.ndarray
    cols: np.ndarray
    vals: np.ndarray
    shape: Tuple[int, int]

    def __post_init__(self):
        m, n = self.shape
        flat = self.rows.astype(np.int64) * n + self.cols.astype(np.int64)
        order = np.argsort(flat, kind="stable")
        self.rows = np.asarray(self.rows)[order].astype(np.int64)
        self.cols = np.asarray(self.cols)[order].astype(np.int64)
        self.vals = np.asarray(self.vals, dtype=np.float64)[order]
        self.flat = flat[order]

    @classmethod
    def from_dense(cls, R: np.ndarray) -> "CooRatings":
        r, c = np.nonzero(~np.isnan(R))
        return cls(r, c, R[r, c], R.shape)

    def positions_of(self, flat_idx: np.ndarray) -> np.ndarray:
        pos = np.searchsorted(self.flat, flat_idx)
        if pos.size and (pos.max() >= self.flat.size or np.any(self.flat[pos] != flat_idx)):
            raise ValueError("flat index that is not an observed entry")
        return pos


# ------------------------------------------------------------------------------------------ folds
def make_entrywise_folds(ratings: CooRatings, n_splits: int = 5, seed: int = 42,
                         shuffle: bool = True) -> List[np.ndarray]:
    """K disjoint validation sets of flat indices over the observed entries.  Same generator, same
    shuffle of the same ascending flat-index array as the reference, hence identical folds."""
    obs = ratings.flat.copy()
    if shuffle:
        np.random.default_rng(seed).shuffle(obs)
    return [np.asarray(part, dtype=np.int64) for part in np.array_split(obs, n_splits)]


def save_folds_npz(path: str, folds: Sequence[np.ndarray], shape: Tuple[int, int], seed: int) -> None:
    """Reference fold-file format: `shape`, `seed`, `fold0..foldK-1` (int64 flat indices)."""
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    payload = {f"fold{i}": np.asarray(f, dtype=np.int64) for i, f in enumerate(folds)}
    np.savez_compressed(path, shape=np.asarray(shape, dtype=np.int64),
                        seed=np.asarray([seed], dtype=np.int64), **payload)


def load_folds_npz(path: str) -> Tuple[List[np.ndarray], Tuple[int, int], int]:
    with np.load(path, allow_pickle=False) as z:
        keys = sorted((k for k in z.files if k.startswith("fold")), key=lambda s: int(s[4:]))
        folds = [z[k].astype(np.int64) for k in keys]
        shape = tuple(int(v) for v in z["shape"])
        seed = int(z["seed"][0])
    return folds, shape, seed


def train_valid_split(ratings: CooRatings, folds: Sequence[np.ndarray], k: int):
    """Fold k as validation: ((rows, cols, vals) train, (rows, cols, vals) valid, val_idx)."""
    val_idx = np.asarray(folds[k], dtype=np.int64)
    vpos = ratings.positions_of(val_idx)
    keep = np.ones(ratings.flat.size, dtype=bool)
    keep[vpos] = False
    train = (ratings.rows[keep], ratings.cols[keep], ratings.vals[keep])
    valid = (ratings.rows[vpos], ratings.cols[vpos], ratings.vals[vpos])
    return train, valid, val_idx


# ---------------------------------------------------------------------------------------- metrics
def rmse_at(y_true: np.ndarray, y_pred: np.ndarray) -> float:
    """RMSE over already-gathered values; NaN on an empty set (tune_params.py:163-164)."""
    if np.size(y_true) == 0:
        return float("nan")
    return float(np.sqrt(np.mean((np.asarray(y_true) - np.asarray(y_pred)) ** 2)))


def _item_filter(model, cols: np.ndarray, items, filter_items, allow_name: str = "items"):
    """The pass-through of `items=` / `filter_items=` (ALS.recommend) in the ranking measures: (keep, kw) - keep[p]
    False when the held-out item cols[p] is not allowed (such a pair cannot be ranked within the restricted
    catalogue and is left out), kw the keywords for the model's call ({} when neither is given: the call is then
    today's), the allow-list under `allow_name` (the rank calls take it as allow_items)."""
    if items is None and filter_items is None:
        return np.ones(cols.size, dtype=bool), {}
    validate.fitted(model)
    n = model.V.shape[0]
    mask = validate.allowed_mask(validate.item_filters(items, filter_items, n), n)
    inside = (cols >= 0) & (cols < n)
    keep = np.zeros(cols.size, dtype=bool)
    keep[inside] = mask[cols[inside]]
    kw = {"filter_items": filter_items} if items is None else {allow_name: items, "filter_items": filter_items}
    return keep, kw


def ranking_at_k(model: ALS, rows, cols, vals=None, *, K: int = 10, min_rating: Optional[float] = None,
                 features: Optional[Dict[str, np.ndarray]] = None, items=None, filter_items=None) -> Dict[str, Any]:
    """recall@K and NDCG@K of `model.recommend` on held-out (user, item) pairs (new: the reference evaluates RMSE
    only).  For every user u of the held-out set:

      rel(u)       = {i : (u, i) held out, and vals >= min_rating unless min_rating is None}
      top(u)       = model.recommend([u], K, features=features) - the training items of the fit excluded
      recall@K(u)  = |top(u) & rel(u)| / |rel(u)|
      DCG@K(u)     = sum over ranks r = 1 .. K of [top_r(u) in rel(u)] / log2(r + 1)     (binary gains)
      NDCG@K(u)    = DCG@K(u) / IDCG@K(u),  IDCG@K(u) = sum over r = 1 .. min(K, |rel(u)|) of 1 / log2(r + 1)

    Users with an empty rel(u) are left out; the result holds the means over the others:
    {"users": their number, "recall@K": mean recall, "ndcg@K": mean NDCG} (NaN means when no user is left).

    `items` / `filter_items` (as `ALS.recommend`): the measures within the restricted catalogue - top(u) is taken
    among the allowed items, held-out pairs whose item is not allowed are left out of rel(u), and the result gains
    "filtered_out", their number (after `min_rating`)."""
    users, ub, cols, kw, extra = _users_at_k(model, rows, cols, vals, min_rating, items, filter_items)
    if users.size == 0:
        return {"users": 0, "recall@K": float("nan"), "ndcg@K": float("nan"), **extra}
    top, _ = model.recommend(users, K, features=features, **kw)
    return {**_ranking_metrics(top, ub, cols, model.V.shape[0], K), **extra}


def eligible_ranking_at_k(model: ALS, rows, cols, vals=None, *, K: int = 10, eligibility, segments_of_user,
                          min_rating: Optional[float] = None,
                          features: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, Any]:
    """`ranking_at_k` over `model.recommend_eligible`: recall@K and NDCG@K when every user is served from the
    catalogue of their segment.  `eligibility` is an `ALS.eligibility` table over the n fitted items and
    `segments_of_user` an integer array [m], the segment of every user id.

    top(u) = model.recommend_eligible([u], K, eligibility=eligibility, segments=[segments_of_user[u]]).  A held-out
    pair whose item is not eligible for its user cannot be ranked within that user's catalogue: it is left out of
    rel(u), and "ineligible" in the result is the number of such pairs (after `min_rating`).  Otherwise the result is
    `ranking_at_k`'s: {"users", "recall@K", "ndcg@K", "ineligible"}."""
    validate.fitted(model)
    m, n = model.U.shape[0], model.V.shape[0]
    elig = validate.eligibility_table(eligibility, n)
    seg_of = validate.segment_ids(segments_of_user, m, elig.n_segments, "user")
    rows, cols = _held_out_pairs(rows, cols, vals, min_rating)
    validate._in_range(rows, m, "user")
    validate._in_range(cols, n, "item")
    ok = elig.allowed(seg_of[rows], cols)
    extra = {"ineligible": int((~ok).sum())}
    rows, cols = rows[ok], cols[ok]
    users, ub = np.unique(rows, return_inverse=True)
    if users.size == 0:
        return {"users": 0, "recall@K": float("nan"), "ndcg@K": float("nan"), **extra}
    top, _ = model.recommend_eligible(users, K, eligibility=elig, segments=seg_of[users], features=features)
    return {**_ranking_metrics(top, ub, cols, n, K), **extra}


def diversity_at_k(model: ALS, rows, cols, vals=None, *, K: int = 10, diversity: float = 0.0,
                   pool: Optional[int] = None, min_rating: Optional[float] = None,
                   features: Optional[Dict[str, np.ndarray]] = None, items=None, filter_items=None) -> Dict[str, Any]:
    """Accuracy and beyond-accuracy measures of `model.recommend_diverse(users, K, diversity=diversity, pool=pool)`
    on held-out (user, item) pairs: {"users", "recall@K", "ndcg@K", "ild@K", "coverage@K"}.

    users, rel(u), recall@K and NDCG@K are `ranking_at_k`'s (same arguments, same held-out pairs left out); with
    `diversity=0.0` the lists are `recommend`'s and the two values equal `ranking_at_k`'s exactly.
      ild@K       mean, over the users whose list holds at least two items, of the list's intra-list diversity
                  (`ALS.list_diversity`; NaN when there is no such user)
      coverage@K  distinct items over all the lists / size of the allowed catalogue (n, or what `items` /
                  `filter_items` leave of it; NaN when nothing is allowed)
    With `items` / `filter_items` the result also holds "filtered_out" as in `ranking_at_k`."""
    users, ub, cols, kw, extra = _users_at_k(model, rows, cols, vals, min_rating, items, filter_items)
    if users.size == 0:
        nan = float("nan")
        return {"users": 0, "recall@K": nan, "ndcg@K": nan, "ild@K": nan, "coverage@K": nan, **extra}
    top, _, ild = model._recommend_diverse(users, K, diversity, pool, features, True, None, kw.get("items"),
                                           kw.get("filter_items"), True)
    n = model.V.shape[0]
    n_allowed = int(validate.allowed_mask(validate.item_filters(items, filter_items, n), n).sum()) if kw else n
    two = (top >= 0).sum(axis=1) >= 2
    return {**_ranking_metrics(top, ub, cols, n, K),
            "ild@K": float(np.mean(ild[two])) if two.any() else float("nan"),
            "coverage@K": np.unique(top[top >= 0]).size / n_allowed if n_allowed else float("nan"), **extra}


def explore_at_k(model: ALS, rows, cols, vals=None, *, K: int = 10, betas: Sequence[float] = (0.0, 1.0),
                 min_rating: Optional[float] = None, features: Optional[Dict[str, np.ndarray]] = None, items=None,
                 filter_items=None) -> Dict[str, Any]:
    """What exploration costs and buys: `model.recommend_explore(users, K, beta=beta)` on held-out (user, item)
    pairs for every beta of `betas` - {"users", "betas": [{"beta", "recall@K", "ndcg@K", "leverage@K",
    "coverage@K"}, ...]} (plus "filtered_out" with `items` / `filter_items`).

    users, rel(u), recall@K, NDCG@K and coverage@K are `diversity_at_k`'s (same arguments, same pairs left out), so
    the entry of beta = 0 equals `ranking_at_k`; leverage@K is the mean leverage over all filled slots of all lists
    (NaN when every list is empty) - it rises with beta as the lists move to what the histories do not cover."""
    betas = [float(b) for b in betas]
    users, ub, cols, kw, extra = _users_at_k(model, rows, cols, vals, min_rating, items, filter_items)
    nan = float("nan")
    if users.size == 0:
        return {"users": 0, "betas": [{"beta": b, "recall@K": nan, "ndcg@K": nan, "leverage@K": nan,
                                       "coverage@K": nan} for b in betas], **extra}
    n = model.V.shape[0]
    n_allowed = int(validate.allowed_mask(validate.item_filters(items, filter_items, n), n).sum()) if kw else n
    out = []
    for b in betas:
        top, _, lev = model.recommend_explore(users, K, beta=b, features=features, return_leverage=True, **kw)
        m = _ranking_metrics(top, ub, cols, n, K)
        filled = top >= 0
        out.append({"beta": b, "recall@K": m["recall@K"], "ndcg@K": m["ndcg@K"],
                    "leverage@K": float(lev[filled].mean()) if filled.any() else nan,
                    "coverage@K": np.unique(top[filled]).size / n_allowed if n_allowed else nan})
    return {"users": int(users.size), "betas": out, **extra}


def calibration_at_k(model: ALS, rows, cols, vals=None, *, K: int = 10, categories,
                     calibrations: Sequence[float] = (0.0, 0.5), pool: Optional[int] = None, smoothing: float = 0.01,
                     min_rating: Optional[float] = None, features: Optional[Dict[str, np.ndarray]] = None, items=None,
                     filter_items=None) -> Dict[str, Any]:
    """What calibration costs and buys: `model.recommend_calibrated(users, K, categories=categories, calibration=c)`
    on held-out (user, item) pairs for every c of `calibrations` - {"users", "profiled_users", "calibrations":
    [{"calibration", "recall@K", "ndcg@K", "miscalibration@K"}, ...]} (plus "filtered_out" with `items` /
    `filter_items`).

    users, rel(u), recall@K and NDCG@K are `ranking_at_k`'s (same arguments, same pairs left out), so the entry of
    calibration 0 equals `ranking_at_k`.  miscalibration@K is the mean, over the "profiled_users" - those whose
    category profile (`ALS.category_profile`) is not all zero -, of the KL divergence of the user's list from the
    profile as the re-ranking kernel itself reports it (NaN when there is no such user); it falls as the calibration
    rises."""
    calibrations = [float(c) for c in calibrations]
    users, ub, cols, kw, extra = _users_at_k(model, rows, cols, vals, min_rating, items, filter_items)
    nan = float("nan")
    if users.size == 0:
        return {"users": 0, "profiled_users": 0,
                "calibrations": [{"calibration": c, "recall@K": nan, "ndcg@K": nan, "miscalibration@K": nan}
                                 for c in calibrations], **extra}
    known = (model.category_profile(users, categories=categories) > 0).any(axis=1)
    out = []
    for c in calibrations:
        top, _, kl = model.recommend_calibrated(users, K, categories=categories, calibration=c, pool=pool,
                                                smoothing=smoothing, features=features, return_miscalibration=True,
                                                **kw)
        m = _ranking_metrics(top, ub, cols, model.V.shape[0], K)
        out.append({"calibration": c, "recall@K": m["recall@K"], "ndcg@K": m["ndcg@K"],
                    "miscalibration@K": float(np.mean(kl[known])) if known.any() else nan})
    return {"users": int(users.size), "profiled_users": int(known.sum()), "calibrations": out, **extra}


def capacity_at_k(model: ALS, rows, cols, vals=None, *, K: int = 10, capacity, min_rating: Optional[float] = None,
                  features: Optional[Dict[str, np.ndarray]] = None, items=None, filter_items=None) -> Dict[str, Any]:
    """What exposure caps cost and buy: `model.recommend_capacity(users, K, capacity=capacity)` over the users of the
    held-out (user, item) pairs - one batch, every user one row - next to the uncapped `model.recommend`:
    {"users", "recall@K", "ndcg@K", "recall@K_uncapped", "ndcg@K_uncapped", "coverage@K", "coverage@K_uncapped",
    "max_exposure", "gini_exposure", "max_exposure_uncapped", "gini_exposure_uncapped", "rounds", "walked_rows"} (plus
    "filtered_out" with `items` / `filter_items`).

    users, rel(u), recall@K and NDCG@K are `ranking_at_k`'s (same arguments, same pairs left out); the uncapped values
    equal `ranking_at_k`'s.  The exposure of an item is the number of lists that hold it: coverage@K is the share of
    the allowed catalogue with exposure > 0, max_exposure the largest exposure (<= the item's cap under caps), and
    gini_exposure the Gini coefficient of the exposures over the allowed catalogue (0: every item shown equally
    often; towards 1: a few items take all the slots; NaN when nothing is shown).  `rounds` and `walked_rows` are the
    call's `CapacityInfo` values."""
    users, ub, cols, kw, extra = _users_at_k(model, rows, cols, vals, min_rating, items, filter_items)
    validate.fitted(model)
    n = model.V.shape[0]
    cap = validate.item_capacity(capacity, n)
    nan = float("nan")
    names = ("recall@K", "ndcg@K", "coverage@K", "max_exposure", "gini_exposure")
    if users.size == 0:
        return {"users": 0, **{f"{k}{s}": nan for k in names for s in ("", "_uncapped")}, "rounds": 0,
                "walked_rows": 0, **extra}
    allowed = validate.allowed_mask(validate.item_filters(items, filter_items, n), n) if kw else np.ones(n, dtype=bool)

    def measures(top):
        exposure = np.sort(np.bincount(top[top >= 0], minlength=n)[allowed].astype(np.float64))
        na, total = exposure.size, exposure.sum()
        gini = (2.0 * (np.arange(1, na + 1) * exposure).sum() / (na * total) - (na + 1) / na) if total > 0 else nan
        m = _ranking_metrics(top, ub, cols, n, K)
        return {"recall@K": m["recall@K"], "ndcg@K": m["ndcg@K"],
                "coverage@K": float((exposure > 0).sum() / na) if na else nan,
                "max_exposure": int(exposure[-1]) if na else 0, "gini_exposure": float(gini)}
    top, _, info = model.recommend_capacity(users, K, capacity=cap, features=features, return_info=True, **kw)
    capped = measures(top)
    plain = measures(model.recommend(users, K, features=features, **kw)[0])
    return {"users": int(users.size), **capped, **{f"{k}_uncapped": v for k, v in plain.items()},
            "rounds": info.rounds, "walked_rows": info.walked_rows, **extra}


def quota_at_k(model: ALS, rows, cols, vals=None, *, K: int = 10, groups, max_per_group,
               min_rating: Optional[float] = None, features: Optional[Dict[str, np.ndarray]] = None, items=None,
               filter_items=None) -> Dict[str, Any]:
    """What per-group caps cost and buy: `model.recommend_quota(users, K, groups=groups, max_per_group=max_per_group)`
    over the users of the held-out (user, item) pairs next to the uncapped `model.recommend`: {"users", "recall@K",
    "ndcg@K", "recall@K_uncapped", "ndcg@K_uncapped", "groups_per_list", "groups_per_list_uncapped",
    "max_group_share", "max_group_share_uncapped"} (plus "filtered_out" with `items` / `filter_items`).

    users, rel(u), recall@K and NDCG@K are `ranking_at_k`'s (same arguments, same pairs left out); the uncapped values
    equal `ranking_at_k`'s.  groups_per_list: the mean over the non-empty lists of the number of distinct groups in a
    list, an item without a group (label -1) counting as a group of its own.  max_group_share: the mean over the
    non-empty lists of (the most entries one group has in the list) / (the entries of the list), 1 / entries for a list
    without a grouped item.  Both are NaN when every list is empty."""
    users, ub, cols, kw, extra = _users_at_k(model, rows, cols, vals, min_rating, items, filter_items)
    validate.fitted(model)
    n = model.V.shape[0]
    labels, caps = validate.item_groups(groups, max_per_group, n)
    nan = float("nan")
    names = ("recall@K", "ndcg@K", "groups_per_list", "max_group_share")
    if users.size == 0:
        return {"users": 0, **{f"{k}{s}": nan for k in names for s in ("", "_uncapped")}, **extra}

    def measures(top):
        distinct, share = [], []
        for row in top:
            row = row[row >= 0]
            if row.size == 0:
                continue
            g = labels[row]
            counts = np.bincount(g[g >= 0]) if (g >= 0).any() else np.ones(1, np.int64)
            distinct.append(int((counts > 0).sum() if (g >= 0).any() else 0) + int((g < 0).sum()))
            share.append(counts.max() / row.size)
        m = _ranking_metrics(top, ub, cols, n, K)
        return {"recall@K": m["recall@K"], "ndcg@K": m["ndcg@K"],
                "groups_per_list": float(np.mean(distinct)) if distinct else nan,
                "max_group_share": float(np.mean(share)) if share else nan}
    capped = measures(model.recommend_quota(users, K, groups=labels, max_per_group=caps, features=features, **kw)[0])
    plain = measures(model.recommend(users, K, features=features, **kw)[0])
    return {"users": int(users.size), **capped, **{f"{k}_uncapped": v for k, v in plain.items()}, **extra}


def audience_at_k(model: ALS, rows, cols, vals=None, *, K: int = 10, min_rating: Optional[float] = None,
                  features: Optional[Dict[str, np.ndarray]] = None, users=None, filter_users=None) -> Dict[str, Any]:
    """recall@K and NDCG@K of `model.recommend_users` on held-out (user, item) pairs: `ranking_at_k` per ITEM - is
    the held-out rater among the item's top-K users who did not rate it in the fit?  For every item i of the
    held-out set, rel(i) = {u : (u, i) held out, and vals >= min_rating unless min_rating is None}, top(i) =
    model.recommend_users([i], K, features=features), and recall / DCG / NDCG as in `ranking_at_k` with users and
    items swapped.  Items with an empty rel(i) are left out: {"items": their number, "recall@K", "ndcg@K"} (NaN
    means when no item is left).

    `users` / `filter_users` (as `ALS.recommend_users`): the measures within the restricted audience - held-out
    pairs whose user is not allowed are left out, and the result gains "filtered_out", their number."""
    rows, cols = _held_out_pairs(rows, cols, vals, min_rating)
    extra, kw = {}, {}
    if users is not None or filter_users is not None:
        validate.fitted(model)
        m = model.U.shape[0]
        mask = validate.allowed_mask(validate.user_filters(users, filter_users, m), m)
        keep = np.zeros(rows.size, dtype=bool)
        inside = (rows >= 0) & (rows < m)
        keep[inside] = mask[rows[inside]]
        extra, kw = {"filtered_out": int((~keep).sum())}, {"users": users, "filter_users": filter_users}
        rows, cols = rows[keep], cols[keep]
    items, ib = np.unique(cols, return_inverse=True)
    if items.size == 0:
        return {"items": 0, "recall@K": float("nan"), "ndcg@K": float("nan"), **extra}
    top, _ = model.recommend_users(items, K, features=features, **kw)
    out = _ranking_metrics(top, ib, rows, model.U.shape[0], K)
    return {"items": out.pop("users"), **out, **extra}


def _users_at_k(model, rows, cols, vals, min_rating, items, filter_items):
    """The users scored by ranking_at_k / diversity_at_k: (users, ub, cols, kw, extra) - the distinct users of the
    held-out pairs that survive `min_rating` and the item filter, the position `ub` of every surviving pair's user,
    its item, the filter keywords of the model's call and the "filtered_out" entry of the result."""
    rows, cols = _held_out_pairs(rows, cols, vals, min_rating)
    allowed, kw = _item_filter(model, cols, items, filter_items)
    extra = {"filtered_out": int((~allowed).sum())} if kw else {}
    rows, cols = rows[allowed], cols[allowed]
    users, ub = np.unique(rows, return_inverse=True)
    return users, ub, cols, kw, extra


def _ranking_rows(items: np.ndarray, ub: np.ndarray, cols: np.ndarray, n_items: int, K: int):
    """(recall@K [U], NDCG@K [U]) of ranked lists `items` [U, K] (-1 = empty slot) against the relevant (position ub,
    item cols) pairs; every position 0 .. U-1 has at least one (see ranking_at_k)."""
    nu = items.shape[0]
    n = int(max(n_items, cols.max() + 1))
    rel = np.unique(ub * n + cols)                                      # (user position, item), duplicates merged
    nrel = np.bincount(rel // n, minlength=nu)
    hit = (items >= 0) & np.isin(np.arange(nu)[:, None] * n + items, rel)
    disc = 1.0 / np.log2(np.arange(2, K + 2, dtype=np.float64))         # rank r = 1 .. K
    dcg = (hit * disc).sum(axis=1)
    idcg = np.cumsum(disc)[np.minimum(nrel, K) - 1]
    return hit.sum(axis=1) / nrel, dcg / idcg


def _ranking_metrics(items: np.ndarray, ub: np.ndarray, cols: np.ndarray, n_items: int, K: int) -> Dict[str, Any]:
    """The means of `_ranking_rows` over the U lists, as ranking_at_k reports them."""
    recall, ndcg = _ranking_rows(items, ub, cols, n_items, K)
    return {"users": int(items.shape[0]), "recall@K": float(np.mean(recall)), "ndcg@K": float(np.mean(ndcg))}


def group_ranking_at_k(model: ALS, groups, rows, cols, vals=None, *, K: int = 10, aggregate: str = "mean",
                       min_rating: Optional[float] = None,
                       features: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, Any]:
    """recall@K and NDCG@K of `model.recommend_group(groups, K, aggregate=aggregate)` on held-out (user, item) pairs:
    how well does ONE list serve every member?  For member u of group g:

      rel(g, u) = {i : (u, i) held out, and vals >= min_rating unless min_rating is None}, without the items that a
                  member of g has among the training ratings of the fit - the group's list leaves those out, so they
                  cannot be candidates;
      recall@K(g, u), NDCG@K(g, u): `ranking_at_k`'s definitions for the list of g against rel(g, u).

    Members with an empty rel(g, u) are left out, and groups without a member left as well.  The result is
    {"groups": groups evaluated, "members": (group, member) pairs evaluated,
     "recall@K": {"mean_member": ..., "min_member": ...}, "ndcg@K": {"mean_member": ..., "min_member": ...}}:
    mean_member is the mean over the evaluated members of a group, averaged over the groups; min_member is the value
    of the worst-off evaluated member of a group, averaged over the groups - what least misery ("min") is meant to
    raise.  NaN when no group is left.  `groups` as in `ALS.recommend_group`; a group listed twice counts twice."""
    validate.fitted(model)
    aggregate = validate.group_aggregate(aggregate)
    m, n = model.U.shape[0], model.V.shape[0]
    g_ptr, g_users = validate.user_groups(groups, m)
    rows, cols = _held_out_pairs(rows, cols, vals, min_rating)
    nan = float("nan")
    empty = {"groups": 0, "members": 0, "recall@K": {"mean_member": nan, "min_member": nan},
             "ndcg@K": {"mean_member": nan, "min_member": nan}}
    # every (member slot, held-out item of that member): slot s = position in g_users, group gs[s]
    sizes = np.diff(g_ptr)
    gs = np.repeat(np.arange(sizes.size, dtype=np.int64), sizes)
    order = np.argsort(rows, kind="stable")
    rows, cols = rows[order], cols[order]
    first = np.searchsorted(rows, g_users, side="left")
    count = np.searchsorted(rows, g_users, side="right") - first
    slot = np.repeat(np.arange(g_users.size, dtype=np.int64), count)
    item = cols[np.repeat(first, count) + (np.arange(slot.size) - np.repeat(np.cumsum(count) - count, count))]
    if slot.size == 0:
        return empty
    # drop the entries whose item a member of the group has in training: one (fellow, item) pair per fellow
    gsz = sizes[gs[slot]]
    entry = np.repeat(np.arange(slot.size, dtype=np.int64), gsz)
    fellow = g_users[np.repeat(g_ptr[gs[slot]], gsz) + (np.arange(entry.size) - np.repeat(np.cumsum(gsz) - gsz, gsz))]
    inside = (np.repeat(item, gsz) >= 0) & (np.repeat(item, gsz) < n)
    seen = np.zeros(entry.size, dtype=bool)
    seen[inside] = model._seen_pairs(fellow[inside].astype(np.int64), np.repeat(item, gsz)[inside])
    keep = np.bincount(entry, weights=seen, minlength=slot.size) == 0
    slot, item = slot[keep], item[keep]
    if slot.size == 0:
        return empty
    # the evaluated members (slots with a relevant item left) and their groups
    mslots, mb = np.unique(slot, return_inverse=True)
    gids, gpos = np.unique(gs[mslots], return_inverse=True)
    top, _ = model.recommend_group([g_users[g_ptr[g]: g_ptr[g + 1]] for g in gids], K, aggregate=aggregate,
                                   features=features)
    recall, ndcg = _ranking_rows(top[gpos], mb, item, n, K)
    out = {"groups": int(gids.size), "members": int(mslots.size)}
    starts = np.searchsorted(gpos, np.arange(gids.size))               # gpos ascends with the slots
    for name, v in (("recall@K", recall), ("ndcg@K", ndcg)):
        out[name] = {"mean_member": float(np.mean(np.add.reduceat(v, starts) / np.bincount(gpos))),
                     "min_member": float(np.mean(np.minimum.reduceat(v, starts)))}
    return out


def fold_in_ranking_at_k(model: ALS, known, held_out, *, K: int = 10, min_rating: Optional[float] = None,
                         features: Optional[Dict[str, np.ndarray]] = None,
                         n_sweeps: Optional[int] = None, items=None, filter_items=None) -> Dict[str, Any]:
    """recall@K and NDCG@K for users outside the fit (strong generalisation): every user of `held_out` is folded
    in from its `known` ratings (`model.recommend_new`, the known items excluded) and scored on its held-out items
    with the definitions of `ranking_at_k`.

    known: (rows, cols, vals) - the new users' ratings that the model may see; held_out: (rows, cols) or
    (rows, cols, vals).  Row ids are labels of the new users shared by the two sets (any integers; they are not
    user ids of the fit).  A held-out user without known ratings is scored with zero factors (mu + b_i).
    min_rating, features, n_sweeps, items, filter_items: as in ranking_at_k / ALS.fold_in."""
    if len(known) != 3:
        raise ValueError("known must be (rows, cols, vals)")
    if len(held_out) not in (2, 3):
        raise ValueError("held_out must be (rows, cols) or (rows, cols, vals)")
    rows = np.asarray(held_out[0], dtype=np.int64).ravel()
    cols = np.asarray(held_out[1], dtype=np.int64).ravel()
    if rows.shape != cols.shape:
        raise ValueError("held-out rows and cols must have the same length")
    if min_rating is not None:
        if len(held_out) != 3:
            raise ValueError("min_rating needs the held-out ratings (vals)")
        keep = np.asarray(held_out[2], dtype=np.float64).ravel() >= min_rating
        rows, cols = rows[keep], cols[keep]
    allowed, kw = _item_filter(model, cols, items, filter_items)
    extra = {"filtered_out": int((~allowed).sum())} if kw else {}
    rows, cols = rows[allowed], cols[allowed]
    users, ub = np.unique(rows, return_inverse=True)
    if users.size == 0:
        return {"users": 0, "recall@K": float("nan"), "ndcg@K": float("nan"), **extra}
    kr = np.asarray(known[0], dtype=np.int64).ravel()
    kc = np.asarray(known[1], dtype=np.int64).ravel()
    kv = np.asarray(known[2], dtype=np.float64).ravel()
    if not kr.shape == kc.shape == kv.shape:
        raise ValueError("known rows, cols and vals must have the same length")
    pos = np.searchsorted(users, kr)
    mine = (pos < users.size) & (users[np.minimum(pos, users.size - 1)] == kr)     # known ratings of scored users
    pos, kc, kv = pos[mine], kc[mine], kv[mine]
    order = np.argsort(pos, kind="stable")
    indptr = np.zeros(users.size + 1, dtype=np.int64)
    np.cumsum(np.bincount(pos, minlength=users.size), out=indptr[1:])
    top, _ = model.recommend_new((indptr, kc[order], kv[order]), K, features=features, n_sweeps=n_sweeps, **kw)
    return {**_ranking_metrics(top, ub, cols, model.V.shape[0], K), **extra}


def _check_Ks(Ks) -> Tuple[int, ...]:
    Ks = tuple(Ks)
    for K in Ks:
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
            raise ValueError(f"every K must be an integer >= 1, got {K!r}")
    return tuple(int(K) for K in Ks)


def _empty_rank_metrics(Ks, pairs: int, dropped: int) -> Dict[str, Any]:
    out: Dict[str, Any] = {"users": 0, "pairs": pairs, "dropped": dropped}
    for name in [f"{a}@{K}" for K in Ks for a in ("recall", "ndcg")] + ["mrr", "auc", "mpr"]:
        out[name] = float("nan")
    return out


def _rank_metrics(ub: np.ndarray, rank: np.ndarray, cand: np.ndarray, dropped: int, Ks) -> Dict[str, Any]:
    """Means over users of the rank measures (see rank_metrics) from the kept pairs: user position ub, 0-based
    rank, candidate count of the pair's user.  The ranks of one user are distinct (a total order over distinct
    candidate items)."""
    if ub.size == 0:
        return _empty_rank_metrics(Ks, 0, dropped)
    order = np.lexsort((rank, ub))                                      # by user, ranks ascending within a user
    ub, rho, cand = ub[order], rank[order].astype(np.float64), cand[order].astype(np.float64)
    users, first, nrel = np.unique(ub, return_index=True, return_counts=True)
    pos = np.arange(ub.size) - np.repeat(first, nrel)                   # relevant items ranked above, same user
    c = cand[first]
    out: Dict[str, Any] = {"users": int(users.size), "pairs": int(ub.size), "dropped": int(dropped)}
    disc_t = 1.0 / np.log2(rho + 2.0)                                   # rank r = rho + 1
    ideal = np.cumsum(1.0 / np.log2(np.arange(2, int(nrel.max()) + 2, dtype=np.float64)))
    for K in Ks:
        hit = rho < K
        out[f"recall@{K}"] = float(np.mean(np.add.reduceat(hit.astype(np.float64), first) / nrel))
        dcg = np.add.reduceat(np.where(hit, disc_t, 0.0), first)
        out[f"ndcg@{K}"] = float(np.mean(dcg / ideal[np.minimum(nrel, K) - 1]))
    out["mrr"] = float(np.mean(1.0 / (1.0 + rho[first])))
    neg = c - nrel                                                      # candidates that are not relevant
    ok = neg > 0
    inv = np.add.reduceat(rho - pos, first)                             # (irrelevant, relevant) pairs in the wrong order
    out["auc"] = float(np.mean(1.0 - inv[ok] / (nrel[ok] * neg[ok]))) if ok.any() else float("nan")
    out["mpr"] = float(np.mean(np.add.reduceat(rho / np.maximum(np.repeat(c, nrel) - 1.0, 1.0), first) / nrel))
    return out


def _held_out_pairs(rows, cols, vals, min_rating, what: str = ""):
    rows = np.asarray(rows, dtype=np.int64).ravel()
    cols = np.asarray(cols, dtype=np.int64).ravel()
    if rows.shape != cols.shape:
        raise ValueError(f"{what}rows and cols must have the same length")
    if min_rating is not None:
        if vals is None:
            raise ValueError("min_rating needs the held-out ratings (vals)")
        keep = np.asarray(vals, dtype=np.float64).ravel() >= min_rating
        rows, cols = rows[keep], cols[keep]
    return rows, cols


def rank_metrics(model: ALS, rows, cols, vals=None, *, Ks: Sequence[int] = (10, 100),
                 min_rating: Optional[float] = None,
                 features: Optional[Dict[str, np.ndarray]] = None, items=None, filter_items=None) -> Dict[str, Any]:
    """Full-catalogue ranking measures of held-out (user, item) pairs from exact ranks (`model.rank_of`; no
    sampled negatives, no list limit).  Arguments as `ranking_at_k`.  For every user u of the held-out set, with
    rel(u) as in `ranking_at_k` (duplicates merged), c(u) the number of candidates (items that are neither
    training items of the fit nor NaN-scored) and rho_t the 0-based rank of t among them:

      a pair whose item is a training item of u, or whose score is NaN, is DROPPED (it cannot be ranked among the
      candidates) and counted in "dropped"; R(u) is what is left, users with an empty R(u) are left out;
      recall@K(u) = |{t in R(u): rho_t < K}| / |R(u)|, NDCG@K(u) as `ranking_at_k` with "t in top-K" = rho_t < K,
          for every K of `Ks` (any K >= 1);
      mrr(u)      = 1 / (1 + min_t rho_t);
      auc(u)      = 1 - sum_t (rho_t - #{t' in R(u): rho_t' < rho_t}) / (|R(u)| (c(u) - |R(u)|)): the fraction of
                    (relevant, other candidate) pairs the model orders correctly; users with c(u) = |R(u)| are
                    left out of this mean only;
      mpr(u)      = mean over t of rho_t / max(c(u) - 1, 1)   (mean percentile rank, 0 = best).

    Returns the means over users under "recall@K", "ndcg@K" (per K), "mrr", "auc", "mpr", with "users", "pairs"
    (kept, after merging) and "dropped" (NaN means when no user is left).

    `items` / `filter_items` (as `ALS.recommend`): the measures within the restricted catalogue - the candidates
    are intersected with the allowed items (`ALS.rank_of`), and a pair whose item is not allowed is dropped and
    counted in "dropped" like a training pair."""
    Ks = _check_Ks(Ks)
    rows, cols = _held_out_pairs(rows, cols, vals, min_rating)
    if rows.size:
        w = max(model.V.shape[0] if model.V is not None else 1, int(cols.max()) + 1)
        rows, cols = np.divmod(np.unique(rows * w + cols), w)           # duplicates merged
    allowed, kw = _item_filter(model, cols, items, filter_items, "allow_items")
    rank, cand, _ = model.rank_of(rows, cols, features=features, **kw)
    if rows.size == 0:
        return _empty_rank_metrics(Ks, 0, 0)
    keep = ~model._seen_pairs(rows, cols) & (rank >= 0) & allowed
    _, ub = np.unique(rows[keep], return_inverse=True)
    return _rank_metrics(ub, rank[keep], cand[keep], int((~keep).sum()), Ks)


def fold_in_rank_metrics(model: ALS, known, held_out, *, Ks: Sequence[int] = (10, 100),
                         min_rating: Optional[float] = None, features: Optional[Dict[str, np.ndarray]] = None,
                         n_sweeps: Optional[int] = None, items=None, filter_items=None) -> Dict[str, Any]:
    """`rank_metrics` for users outside the fit (strong generalisation), with the conventions of
    `fold_in_ranking_at_k`: every user of `held_out` is folded in from its `known` ratings (`model.rank_of_new`,
    the known items are no candidates) and its held-out items are ranked.  A held-out pair whose item is among the
    user's known items is dropped and counted, as is one with a NaN score - and, with `items` / `filter_items`
    (as in `rank_metrics`), one whose item is not allowed."""
    Ks = _check_Ks(Ks)
    if len(known) != 3:
        raise ValueError("known must be (rows, cols, vals)")
    if len(held_out) not in (2, 3):
        raise ValueError("held_out must be (rows, cols) or (rows, cols, vals)")
    if min_rating is not None and len(held_out) != 3:
        raise ValueError("min_rating needs the held-out ratings (vals)")
    rows, cols = _held_out_pairs(held_out[0], held_out[1], held_out[2] if len(held_out) == 3 else None, min_rating,
                                 "held-out ")
    if rows.size == 0:
        model._check_predict(features)
        return _empty_rank_metrics(Ks, 0, 0)
    users, ub = np.unique(rows, return_inverse=True)
    w = max(model.V.shape[0] if model.V is not None else 1, int(cols.max()) + 1)
    ub, cols = np.divmod(np.unique(ub * w + cols), w)                   # by user position, duplicates merged
    kr = np.asarray(known[0], dtype=np.int64).ravel()
    kc = np.asarray(known[1], dtype=np.int64).ravel()
    kv = np.asarray(known[2], dtype=np.float64).ravel()
    if not kr.shape == kc.shape == kv.shape:
        raise ValueError("known rows, cols and vals must have the same length")
    pos = np.searchsorted(users, kr)
    mine = (pos < users.size) & (users[np.minimum(pos, users.size - 1)] == kr)     # known ratings of scored users
    pos, kc, kv = pos[mine], kc[mine], kv[mine]
    order = np.argsort(pos, kind="stable")
    indptr = np.zeros(users.size + 1, dtype=np.int64)
    np.cumsum(np.bincount(pos, minlength=users.size), out=indptr[1:])
    tptr = np.zeros(users.size + 1, dtype=np.int64)
    np.cumsum(np.bincount(ub, minlength=users.size), out=tptr[1:])
    allowed, kw = _item_filter(model, cols, items, filter_items, "allow_items")
    rank, cand, _ = model.rank_of_new((indptr, kc[order], kv[order]), (tptr, cols), features=features,
                                      n_sweeps=n_sweeps, **kw)
    keep = ~np.isin(ub * w + cols, pos * w + kc) & (rank >= 0) & allowed
    _, ubk = np.unique(ub[keep], return_inverse=True)
    return _rank_metrics(ubk, rank[keep], cand[keep], int((~keep).sum()), Ks)


def leverage_calibration(model: ALS, rows, cols, vals, *, features: Optional[Dict[str, np.ndarray]] = None,
                         n_bins: int = 10) -> Dict[str, Any]:
    """Does the leverage of `model.explain` order the prediction error?  For held-out ratings (rows, cols, vals) of
    users of the fit: leverage[p] = z_i^T A^-1 z_i of the pair (`model.explain`), the pairs sorted by leverage
    (stable: ties keep the order given) and cut into `n_bins` consecutive groups of equal size (the first
    P mod n_bins groups hold one pair more, as numpy.array_split); per group the mean leverage, the number of pairs
    and the RMSE of `model.predict_at` on its pairs.  Returns {"leverage": [n_bins], "count": [n_bins],
    "rmse": [n_bins]} as lists, low leverage first; a group without pairs has count 0 and NaN elsewhere.  A
    calibrated leverage shows an RMSE that rises along the bins."""
    if isinstance(n_bins, bool) or not isinstance(n_bins, (int, np.integer)) or n_bins < 1:
        raise ValueError(f"n_bins must be an integer >= 1, got {n_bins!r}")
    rows, cols = _held_out_pairs(rows, cols, None, None)
    vals = np.asarray(vals, dtype=np.float64).ravel()
    if vals.shape != rows.shape:
        raise ValueError("rows, cols and vals must have the same length")
    lev = model.explain(rows, cols, 1, features=features).leverage
    pred = model.predict_at(rows * model.V.shape[0] + cols, features=features) if rows.size else np.empty(0)
    err2 = (np.asarray(pred, dtype=np.float64) - vals) ** 2
    out: Dict[str, Any] = {"leverage": [], "count": [], "rmse": []}
    for grp in np.array_split(np.argsort(lev, kind="stable"), int(n_bins)):
        out["count"].append(int(grp.size))
        out["leverage"].append(float(lev[grp].mean()) if grp.size else float("nan"))
        out["rmse"].append(float(np.sqrt(err2[grp].mean())) if grp.size else float("nan"))
    return out


def cold_item_rmse(model: ALS, held_out, *, known=None, features_new: Optional[Dict[str, np.ndarray]] = None,
                   features: Optional[Dict[str, np.ndarray]] = None,
                   n_sweeps: Optional[int] = None) -> Dict[str, Any]:
    """RMSE on items outside the fit (strong generalisation for items): the B new items are folded in from their
    `known` ratings (`model.fold_in_items`; None = no ratings, the cold-start case), scored with
    `model.predict_new_items` on the `held_out` pairs, and compared with the bias-only baseline mu + b_u on the
    same pairs.

    held_out / known: (user ids, new item positions b in [0, B), ratings).  B is the row count of `features_new`
    (every feature of the fit, as in fold_in_items), or 1 + the largest position when the model has no features.
    features (the fitted items', for the graph rows) and n_sweeps: as in fold_in_items.
    Returns {"pairs": held-out pairs, "rmse": folded-in RMSE, "baseline_rmse": mu + b_u RMSE} (NaN when empty)."""
    if len(held_out) != 3:
        raise ValueError("held_out must be (user ids, new item positions, ratings)")
    hu, hb, hv = (np.asarray(a).ravel() for a in held_out)
    if not hu.shape == hb.shape == hv.shape:
        raise ValueError("held-out users, items and ratings must have the same length")
    if known is not None:
        if len(known) != 3:
            raise ValueError("known must be (user ids, new item positions, ratings)")
        ku, kb, kv = (np.asarray(a).ravel() for a in known)
        if not ku.shape == kb.shape == kv.shape:
            raise ValueError("known users, items and ratings must have the same length")
    else:
        ku = kb = np.zeros(0, np.int64)
        kv = np.zeros(0)
    if features_new:
        B = int(np.shape(next(iter(features_new.values())))[0])
    else:
        B = int(max(hb.max(initial=-1), kb.max(initial=-1))) + 1
    for what, b in (("held_out", hb), ("known", kb)):
        if b.size and (b.min() < 0 or b.max() >= B):
            raise IndexError(f"{what}: new item positions must lie in [0, {B})")
    kb = kb.astype(np.int64)
    order = np.lexsort((ku, kb))
    indptr = np.zeros(B + 1, dtype=np.int64)
    np.cumsum(np.bincount(kb, minlength=B), out=indptr[1:])
    folded = model.fold_in_items((indptr, ku[order], kv[order]), features_new=features_new, features=features,
                                 n_sweeps=n_sweeps)
    if hu.size == 0:
        return {"pairs": 0, "rmse": float("nan"), "baseline_rmse": float("nan")}
    users, inv = np.unique(hu.astype(np.int64), return_inverse=True)
    pred = model.predict_new_items(folded, users)[inv, hb.astype(np.int64)]
    y = hv.astype(np.float64)
    base = model.mu + model.b_u[users][inv]
    return {"pairs": int(hu.size), "rmse": rmse_at(y, pred), "baseline_rmse": rmse_at(y, base)}


def popularity_bins(item_counts: np.ndarray, n_bins: int = N_POP_BINS,
                    strategy: str = POP_BIN_STRATEGY) -> Tuple[np.ndarray, np.ndarray]:
    """Item popularity bins from per-item rating counts: (bin per item, bin edges)."""
    counts = np.asarray(item_counts, dtype=float)
    if strategy == "quantile":
        edges = np.quantile(counts, np.linspace(0, 1, n_bins + 1))
    elif strategy == "uniform":
        edges = np.linspace(float(counts.min()), float(counts.max()), n_bins + 1)
    else:
        raise ValueError(f"Unknown popularity binning strategy '{strategy}'")
    edges = np.array(edges, dtype=float)
    for i in range(1, edges.size):                  # strictly increasing edges
        if edges[i] <= edges[i - 1]:
            edges[i] = edges[i - 1] + 1e-9
    which = np.searchsorted(edges, counts, side="right") - 1
    return np.clip(which, 0, n_bins - 1).astype(int), edges


def split_by_popularity(val_idx: np.ndarray, shape: Tuple[int, int], item_bin: np.ndarray,
                        n_bins: int) -> List[np.ndarray]:
    b = item_bin[np.asarray(val_idx) % shape[1]]
    return [np.asarray(val_idx)[b == j] for j in range(n_bins)]


# ------------------------------------------------------------------------------------- statistics
def aggregate_convergence(curves: Sequence[Sequence[float]]) -> Dict[str, Any]:
    """Mean / std of the train-RMSE curves of the folds, iteration by iteration (NaN padded)."""
    if not curves:
        return {"iters": [], "rmse_mean": [], "rmse_std": [], "n_folds": 0}
    width = max(len(c) for c in curves)
    table = np.full((len(curves), width), np.nan)
    for j, c in enumerate(curves):
        table[j, :len(c)] = c
    return {"iters": list(range(1, width + 1)), "rmse_mean": np.nanmean(table, axis=0).tolist(),
            "rmse_std": np.nanstd(table, axis=0).tolist(), "n_folds": len(curves)}


def aggregate_bins_mean(fold_bin_rmse: Sequence[Dict[str, float]]) -> Dict[str, float]:
    if not fold_bin_rmse:
        return {}
    return {k: float(np.nanmean([d[k] for d in fold_bin_rmse])) for k in sorted(fold_bin_rmse[0])}


def sign_test_paired(x: Sequence[float], y: Sequence[float]) -> float:
    """Exact two-sided sign test on the paired differences (ties dropped)."""
    d = [a - b for a, b in zip(x, y) if not np.isclose(a - b, 0.0)]
    n = len(d)
    if n == 0:
        return 1.0
    pos = sum(1 for v in d if v > 0)
    total = 2 ** n
    lower = sum(math.comb(n, i) for i in range(pos + 1)) / total             # P(X <= pos)
    upper = 1.0 - (sum(math.comb(n, i) for i in range(pos)) / total) if pos > 0 else 1.0   # P(X >= pos)
    return float(min(1.0, 2.0 * min(lower, upper)))


def fdr_bh(pvals: Sequence[float]) -> List[float]:
    """Benjamini-Hochberg adjusted p-values, in the input order."""
    m = len(pvals)
    if m == 0:
        return []
    p = np.asarray(pvals, dtype=float)
    order = np.argsort(p)
    scaled = p[order] * m / np.arange(1, m + 1)
    scaled = np.minimum.accumulate(scaled[::-1])[::-1]
    out = np.empty(m)
    out[order] = np.clip(scaled, 0.0, 1.0)
    return out.tolist()


# --------------------------------------------------------------------------------------- variants
def variant_grid(best_params: Dict[str, Any], feature_names: List[str]) -> List[Tuple[str, Dict[str, Any]]]:
    """Baseline plus controlled removals: no_features / only_<f> / no_graph / graph_feature=<f> /
    no_pop_reg, de-duplicated by parameter signature (last name wins, as in the reference)."""
    base = dict(best_params)
    out: List[Tuple[str, Dict[str, Any]]] = [("full", base)]
    alpha = float(base.get("alpha", 0.0))
    graph_on = alpha > 0.0 and base.get("graph_feature", "__none__") in feature_names
    used = {f: float(base.get(f"lambda_w_{f}", 0.0)) > 0.0 for f in feature_names}
    if any(used.values()):
        p = dict(base)
        p.update({f"lambda_w_{f}": 0.0 for f in feature_names})
        out.append(("no_features", p))
        for f in feature_names:
            if used[f]:
                q = dict(base)
                q.update({f"lambda_w_{g}": 0.0 for g in feature_names})
                q[f"lambda_w_{f}"] = float(base.get(f"lambda_w_{f}", 0.0))
                out.append((f"only_{f}", q))
    if graph_on:
        p = dict(base)
        p["alpha"], p["graph_feature"] = 0.0, "__none__"
        out.append(("no_graph", p))
        for f in feature_names:
            if f != base.get("graph_feature"):
                q = dict(base)
                q["alpha"], q["graph_feature"] = alpha, f
                out.append((f"graph_feature={f}", q))
    if base.get("pop_reg_mode", None) is not None:
        p = dict(base)
        p["pop_reg_mode"] = None
        out.append(("no_pop_reg", p))
    seen: Dict[Tuple, Tuple[str, Dict[str, Any]]] = {}
    for name, p in out:
        seen[tuple(sorted(p.items(), key=lambda kv: kv[0]))] = (name, p)
    return list(seen.values())


# ---------------------------------------------------------------------------------------- drivers
@dataclass
class AblationResultRow:
    variant: str
    rmse_mean: float
    rmse_std: float
    time_mean: float
    time_std: float
    mean_iters: float
    early_stopped_folds: int
    target_n_iters: int
    es_tol: float
    es_min_iters: int
    rmse_bins: Dict[str, float]
    params: Dict[str, Any]
    p_raw: Optional[float] = None
    p_fdr: Optional[float] = None
    delta_mean: Optional[float] = None
    fold_rmse: List[float] = field(default_factory=list)


def eval_variant_cv(variant_name: str, ratings: CooRatings, features: Dict[str, np.ndarray],
                    folds: Sequence[np.ndarray], params: Dict[str, Any], item_bin: np.ndarray,
                    n_pop_bins: int, es_tol: Optional[float], es_min_iters: int,
                    convergence_curves: Dict[str, List[List[float]]], verbose_fit: int = 0,
                    als_kwargs: Optional[Dict[str, Any]] = None):
    """One fixed-parameter model across the folds (evaluate_models.py:194-276 on sparse data):
    returns (fold_rmse, fold_time, fold_bin_rmse, fold_iters).  The timed region is fit + the
    predictions the caller reads, as in the reference (there: fit + dense predict)."""
    params = normalize_params(dict(params), ratings.shape, list(features))
    cfg = make_config(params)
    lambda_w = {name: float(params.get(f"lambda_w_{name}", 0.0)) for name in features}
    fold_rmse, fold_time, fold_bins, fold_iters = [], [], [], []
    for k in range(len(folds)):
        (tr, tc, tv), (_, _, vv), val_idx = train_valid_split(ratings, folds, k)
        t0 = time.perf_counter()
        model = ALS(config=cfg, lambda_w=lambda_w, **(als_kwargs or {}))
        model.fit_coo(tr, tc, tv, ratings.shape, features=features, tol=es_tol, min_iters=es_min_iters,
                      verbose=verbose_fit)
        pred = model.predict_at(val_idx, features=features)
        t1 = time.perf_counter()
        curve = list(model.history.get("train_rmse", []))
        convergence_curves.setdefault(variant_name, []).append(curve)
        fold_rmse.append(rmse_at(vv, pred))
        fold_time.append(t1 - t0)
        fold_iters.append(len(curve))
        bins = item_bin[val_idx % ratings.shape[1]]
        fold_bins.append({f"rmse_pop_{b + 1}": rmse_at(vv[bins == b], pred[bins == b]) for b in range(n_pop_bins)})
    return fold_rmse, fold_time, fold_bins, fold_iters


def row_to_dict(r: AblationResultRow, feature_names: List[str]) -> Dict[str, Any]:
    d: Dict[str, Any] = {"variant": r.variant, "rmse_mean": r.rmse_mean, "rmse_std": r.rmse_std,
                         "time_mean": r.time_mean, "time_std": r.time_std, "mean_iters": r.mean_iters,
                         "early_stopped_folds": r.early_stopped_folds, "target_n_iters": r.target_n_iters,
                         "es_tol": r.es_tol, "es_min_iters": r.es_min_iters, "p_raw": r.p_raw,
                         "p_fdr": r.p_fdr, "delta_mean": r.delta_mean}
    d.update(sorted(r.rmse_bins.items()))
    for key in ("alpha", "graph_feature", "pop_reg_mode", "n_factors", "n_iters", "lambda_u", "lambda_v",
                "lambda_bu", "lambda_bi", "update_w_every"):
        if key in r.params:
            d[f"param_{key}"] = r.params[key]
    for f in feature_names:
        d[f"param_lambda_w_{f}"] = r.params.get(f"lambda_w_{f}")
    return d


def run_ablation(ratings, folds, best_params: Dict[str, Any], features: Dict[str, np.ndarray],
                 out_dir: Optional[str] = None, n_pop_bins: int = N_POP_BINS,
                 es_tol: Optional[float] = None, es_min_iters: Optional[int] = None,
                 verbose_fit: int = 0, folds_seed: int = DEFAULT_RANDOM_STATE,
                 als_kwargs: Optional[Dict[str, Any]] = None) -> Tuple[List[AblationResultRow], Dict[str, Any]]:
    """Ablation study on frozen folds (evaluate_models.py:708-862 without the plots).

    `ratings`: CooRatings, a dense NaN array, or a path to the reference's ratings `.npy`;
    `folds`: list of flat-index arrays or a path to a fold file; `best_params`: dict (either the
    raw dict or {"params": {...}}) or a path to the JSON.  Writes `<out_dir>/ablations/ablations.csv`,
    `ablations.json` and `convergence/<variant>.json` when `out_dir` is given.
    """
    if isinstance(ratings, str):
        ratings = np.load(ratings)
    if isinstance(ratings, np.ndarray):
        ratings = CooRatings.from_dense(ratings)
    if isinstance(folds, str):
        folds, fshape, folds_seed = load_folds_npz(folds)
        if tuple(fshape) != tuple(ratings.shape):
            raise AssertionError("Folds were built for a different matrix shape.")
    if isinstance(best_params, str):
        with open(best_params) as fh:
            best_params = json.load(fh)
    best_params = dict(best_params["params"]) if "params" in best_params else dict(best_params)
    es_tol = float(ES_TOL if es_tol is None else es_tol)
    es_min_iters = int(ES_MIN_ITERS if es_min_iters is None else es_min_iters)
    counts = np.bincount(ratings.cols, minlength=ratings.shape[1])
    item_bin, edges = popularity_bins(counts, n_pop_bins, POP_BIN_STRATEGY)
    feature_names = list(features)
    rows: List[AblationResultRow] = []
    curves: Dict[str, List[List[float]]] = {}
    for name, params in variant_grid(best_params, feature_names):
        f_rmse, f_time, f_bins, f_iters = eval_variant_cv(
            name, ratings, features, folds, params, item_bin, n_pop_bins, es_tol, es_min_iters, curves,
            verbose_fit=verbose_fit, als_kwargs=als_kwargs)
        target = int(params.get("n_iters", 0))
        rows.append(AblationResultRow(
            variant=name, rmse_mean=float(np.mean(f_rmse)),
            rmse_std=float(np.std(f_rmse, ddof=1)) if len(f_rmse) > 1 else 0.0,
            time_mean=float(np.mean(f_time)),
            time_std=float(np.std(f_time, ddof=1)) if len(f_time) > 1 else 0.0,
            mean_iters=float(np.mean(f_iters)), early_stopped_folds=int(sum(i < target for i in f_iters)),
            target_n_iters=target, es_tol=es_tol, es_min_iters=es_min_iters,
            rmse_bins=aggregate_bins_mean(f_bins), params=params, fold_rmse=list(f_rmse)))
    base = next((r for r in rows if r.variant == "full"), None)
    if base is not None:
        others = [r for r in rows if r.variant != "full"]
        for r in others:
            r.p_raw = sign_test_paired(r.fold_rmse, base.fold_rmse)
            r.delta_mean = float(np.mean(np.asarray(r.fold_rmse) - np.asarray(base.fold_rmse)))
        for r, adj in zip(others, fdr_bh([r.p_raw for r in others])):
            r.p_fdr = float(adj)
    payload = {"seed": DEFAULT_RANDOM_STATE, "matrix_shape": [int(ratings.shape[0]), int(ratings.shape[1])],
               "folds_seed": int(folds_seed), "feature_names": feature_names, "n_pop_bins": int(n_pop_bins),
               "pop_bin_edges": [float(e) for e in edges], "es_tol": es_tol, "es_min_iters": es_min_iters,
               "variants_evaluated": [r.variant for r in rows], "best_params_used": best_params,
               "results": [row_to_dict(r, feature_names) for r in rows]}
    if out_dir is not None:
        base_dir = os.path.join(out_dir, "ablations")
        os.makedirs(os.path.join(base_dir, "convergence"), exist_ok=True)
        dict_rows = payload["results"]
        cols: List[str] = []
        for d in dict_rows:
            cols.extend(c for c in d if c not in cols)
        with open(os.path.join(base_dir, "ablations.csv"), "w", newline="") as fh:
            w = csv.DictWriter(fh, fieldnames=cols)
            w.writeheader()
            w.writerows(dict_rows)
        with open(os.path.join(base_dir, "ablations.json"), "w") as fh:
            json.dump(payload, fh, indent=2)
        for variant, cs in curves.items():
            with open(os.path.join(base_dir, "convergence", f"{variant}.json"), "w") as fh:
                json.dump(aggregate_convergence(cs), fh, indent=2)
    return rows, payload
