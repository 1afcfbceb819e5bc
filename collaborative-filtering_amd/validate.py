"""Input checks of the `ALS` facade (als.py), as plain functions: everything a public method verifies about its
arguments before any device work - fitted-ness, features, list lengths, id arrays, `targets`, `n_sweeps`, the item
allow / block lists, the host CSR forms of new users' / new items' ratings and graph rows, and the structure of
caller-supplied ratings CSR and similarity graphs (`_check_csr`, `_as_side`, `_validate_graph`).  Exception types and
messages are part of the public behaviour (the reference's where it has one: scripts/als.py:554-565)."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import layout
from .containers import _SideDev
from .serving import RECOMMEND_DEEP_MAX_N, RECOMMEND_MAX_N, FoldedItems, ItemEligibility, pack_words


def host_features(features):
    """The features dict with device tensors (e.g. the output of features.normalize_feature_device) brought to the
    host: the fit keeps float32 / float64 copies of its own in HBM and validates on the host, as the reference."""
    if not features:
        return {}
    return {name: (X.detach().cpu().numpy() if torch.is_tensor(X) else X) for name, X in features.items()}


def fitted(model) -> None:
    if model.U is None or model.V is None:                   # scripts/als.py:554-555
        raise RuntimeError("Model must be fitted before prediction.")


def predict_features(model, features):
    features = host_features(features)
    fitted(model)
    n = model.V.shape[0]
    for name, X in features.items():                         # scripts/als.py:560-565
        if X.shape[0] != n:
            raise ValueError(f"Feature '{name}' has {X.shape[0]} rows. "
                             f"Expected number of rows: {n}.")
        if not np.isfinite(X).all():
            raise ValueError(f"Feature '{name}' contains infinite values.")
    return features


def top_count(x, name: str) -> int:
    """The length N of a top-N list / M of an explanation: what the selection kernels hold per row."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= x <= RECOMMEND_MAX_N:
        raise ValueError(f"{name} must be an integer in [1, {RECOMMEND_MAX_N}], got {x!r}")
    return int(x)


def deep_topn(x) -> int:
    """The length N of `recommend_deep`: an integer in [1, RECOMMEND_DEEP_MAX_N]."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not 1 <= x <= RECOMMEND_DEEP_MAX_N:
        raise ValueError(f"N must be an integer in [1, {RECOMMEND_DEEP_MAX_N}], got {x!r}")
    return int(x)


def deep_cursor(after, B: int, n_total: int):
    """`after=` of `recommend_deep`: None, or (after_items [B], after_scores [B]) - the last entry of the page each
    row already has -> (int64 [B], float64 [B]).  Items are integer ids in [-1, n_total) (-1: the padding of an
    exhausted list), scores real and not NaN (+-inf are values a list can hold)."""
    if after is None:
        return None
    if not isinstance(after, (tuple, list)) or len(after) != 2:
        raise ValueError("after must be (after_items, after_scores)")
    it, sc = (np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a) for a in after)
    if it.shape != (B,) or sc.shape != (B,):
        raise ValueError(f"after_items and after_scores must have shape ({B},), one entry per row of the batch")
    if it.dtype == np.bool_ or not (np.issubdtype(it.dtype, np.integer) or it.size == 0):
        raise ValueError(f"after_items must hold integer item ids, got dtype {it.dtype}")
    if sc.dtype == np.bool_ or not (np.issubdtype(sc.dtype, np.integer) or np.issubdtype(sc.dtype, np.floating)):
        raise ValueError(f"after_scores must hold real numbers, got dtype {sc.dtype}")
    if it.size and (it.min() < -1 or it.max() >= n_total):
        raise ValueError(f"after_items: item ids must lie in [-1, {n_total})")
    sc = sc.astype(np.float64)
    if np.isnan(sc).any():
        raise ValueError("after_scores must not contain NaN")
    return it.astype(np.int64), sc


def diversity_args(diversity, N: int, pool):
    """(lambda, pool) of `recommend_diverse`: `diversity` a real number in [0, 1]; `pool` None = min(128, 4 N), else
    an integer with N <= pool <= 128."""
    if (isinstance(diversity, (bool, np.bool_)) or not isinstance(diversity, (int, float, np.integer, np.floating))
            or not 0.0 <= float(diversity) <= 1.0):                       # NaN fails the comparison
        raise ValueError(f"diversity must be a real number in [0, 1], got {diversity!r}")
    if pool is None:
        pool = min(RECOMMEND_MAX_N, 4 * N)
    elif isinstance(pool, bool) or not isinstance(pool, (int, np.integer)) or not N <= pool <= RECOMMEND_MAX_N:
        raise ValueError(f"pool must be an integer in [N, {RECOMMEND_MAX_N}] = [{N}, {RECOMMEND_MAX_N}], got {pool!r}")
    return float(diversity), int(pool)


CALIBRATE_MAX_CATEGORIES = 64      # one lane per category in als_calibrated_rerank
TARGET_MIN = 2.0 ** -100           # a target entry below this counts as 0 (the hardware log2 takes no subnormals)


def _distribution_rows(a: np.ndarray, min_entry: float = 0.0) -> np.ndarray:
    """Non-negative rows [rows, ncat] -> fp32 [rows, ldc]: every row divided by its sum in float64 (an all-zero row
    stays zero) and rounded once, ldc = ncat rounded up to a multiple of 16, padding columns zero; entries that end
    up below `min_entry` are set to 0."""
    a = a.astype(np.float64)
    s = a.sum(axis=1, keepdims=True)
    out = np.zeros((a.shape[0], 16 * ((a.shape[1] + 15) // 16)), dtype=np.float32)
    with np.errstate(over="ignore"):
        out[:, : a.shape[1]] = np.divide(a, s, out=np.zeros_like(a), where=s > 0)
    if min_entry:
        out[out < min_entry] = 0.0
    return out


def _real_2d(x, name: str) -> np.ndarray:
    a = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    if a.ndim != 2 or a.dtype == np.bool_ or not (np.issubdtype(a.dtype, np.integer) or np.issubdtype(a.dtype, np.floating)):
        raise ValueError(f"{name} must be a real 2-D array")
    return a


def category_table(categories, n_total: int) -> np.ndarray:
    """The category table of `recommend_calibrated`: `categories` a real array [n_total, 1 .. 64], finite and >= 0
    (multi-hot or weighted; an all-zero row is an item without a category) -> the rows as distributions p(c | i),
    fp32 [n_total, ldc] (`_distribution_rows`)."""
    a = _real_2d(categories, "categories")
    if a.shape[0] != n_total:
        raise ValueError(f"categories has {a.shape[0]} rows. Expected number of rows: {n_total}.")
    if not 1 <= a.shape[1] <= CALIBRATE_MAX_CATEGORIES:
        raise ValueError(f"categories must have 1 to {CALIBRATE_MAX_CATEGORIES} columns, got {a.shape[1]}")
    if not np.isfinite(a).all() or (a < 0).any():
        raise ValueError("categories must be finite and non-negative")
    return _distribution_rows(a)


def calibration_args(calibration, N: int, pool, smoothing):
    """(lambda, pool, alpha) of `recommend_calibrated`: `calibration` a real number in [0, 1]; `pool` as
    `diversity_args` (None = min(128, 4 N), else an integer with N <= pool <= 128); `smoothing` a real number in
    (0, 1)."""
    if (isinstance(calibration, (bool, np.bool_)) or not isinstance(calibration, (int, float, np.integer, np.floating))
            or not 0.0 <= float(calibration) <= 1.0):                     # NaN fails the comparison
        raise ValueError(f"calibration must be a real number in [0, 1], got {calibration!r}")
    _, pool = diversity_args(0.0, N, pool)
    return float(calibration), pool, smoothing_arg(smoothing)


def smoothing_arg(smoothing) -> float:
    if (isinstance(smoothing, (bool, np.bool_)) or not isinstance(smoothing, (int, float, np.integer, np.floating))
            or not 0.0 < float(np.float32(smoothing)) < 1.0):             # as the kernel sees it
        raise ValueError(f"smoothing must be a real number in (0, 1), got {smoothing!r}")
    return float(smoothing)


def target_rows(target, B: int, ncat: int) -> np.ndarray:
    """Explicit targets of `recommend_calibrated` / `list_miscalibration`: a real array [B, ncat], finite and >= 0
    -> the rows as distributions, fp32 [B, ldc], normalised like the category table; entries below TARGET_MIN
    count as 0."""
    a = _real_2d(target, "target")
    if a.shape != (B, ncat):
        raise ValueError(f"target has shape {a.shape}; expected ({B}, {ncat}) (one row per user, one column per "
                         "category)")
    if not np.isfinite(a).all() or (a < 0).any():
        raise ValueError("target must be finite and non-negative")
    return _distribution_rows(a, TARGET_MIN)


def item_lists(lists, n_total: int) -> np.ndarray:
    """Id lists of `list_diversity`: an integer array [B, L], 1 <= L <= 128, entries -1 (padding) or item ids in
    [0, n_total) -> int32 [B, L]."""
    a = np.asarray(lists.detach().cpu().numpy() if torch.is_tensor(lists) else lists)
    if a.ndim != 2 or not np.issubdtype(a.dtype, np.integer) or not 1 <= a.shape[1] <= RECOMMEND_MAX_N:
        raise ValueError(f"item_lists must be an integer array [B, L] with 1 <= L <= {RECOMMEND_MAX_N}")
    if a.size and (a.min() < -1 or a.max() >= n_total):
        raise ValueError(f"item_lists: entries must be -1 (padding) or item ids in [0, {n_total})")
    return np.ascontiguousarray(a, dtype=np.int32)


def sweeps(n_sweeps) -> int:
    if n_sweeps is None:
        return 0
    if isinstance(n_sweeps, bool) or not isinstance(n_sweeps, (int, np.integer)) or not 1 <= n_sweeps < 2 ** 31:
        raise ValueError(f"n_sweeps must be None (fixed point) or an integer >= 1, got {n_sweeps!r}")
    return int(n_sweeps)


def _ids(a, kind: str) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"{kind}s must be a 1-D array-like of integer {kind} ids")
    return a


def _in_range(a: np.ndarray, bound: int, kind: str) -> None:
    if a.size and (a.min() < 0 or a.max() >= bound):
        raise IndexError(f"{kind} ids must lie in [0, {bound})")


def user_ids(users, m: int) -> np.ndarray:
    """User ids in [0, m), order and duplicates kept; None = all m users in id order."""
    if users is None:
        return np.arange(m, dtype=np.int64)
    u = _ids(users, "user")
    _in_range(u, m, "user")
    return u


def item_ids(items, n: int) -> np.ndarray:
    """Query item ids in [0, n) of `similar_items`, order and duplicates kept; None = all n items in id order."""
    if items is None:
        return np.arange(n, dtype=np.int64)
    i = _ids(items, "item")
    _in_range(i, n, "item")
    return i


GROUP_MAX_MEMBERS = 64      # ALS_GROUP_MAX_MEMBERS: the members one wave of als_group_topk holds
GROUP_AGGREGATES = ("mean", "min", "max")


def user_groups(groups, m: int):
    """The groups of `recommend_group`: a ragged sequence of 1-D arrays of user ids, or a 2-D integer array [G, g] of
    equal-size groups -> (ptr int64 [G + 1], users int32): group b is users[ptr[b]:ptr[b + 1]], order and repeated
    groups kept.  Raises ValueError for an empty group, an id outside [0, m), a user twice in one group, or a group of
    more than GROUP_MAX_MEMBERS members."""
    if torch.is_tensor(groups):
        groups = groups.detach().cpu().numpy()
    if isinstance(groups, np.ndarray) and groups.ndim == 2:
        if groups.size and not np.issubdtype(groups.dtype, np.integer):
            raise ValueError("groups must hold integer user ids")
        rows = list(groups)
    elif isinstance(groups, np.ndarray) and groups.ndim != 1:
        raise ValueError("groups must be a sequence of 1-D arrays of user ids or a 2-D integer array [G, g]")
    else:
        try:
            rows = [np.asarray(g.detach().cpu().numpy() if torch.is_tensor(g) else g) for g in groups]
        except TypeError:
            raise ValueError("groups must be a sequence of 1-D arrays of user ids or a 2-D integer array [G, g]")
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    for b, g in enumerate(rows):
        if g.ndim != 1 or (g.size and not np.issubdtype(g.dtype, np.integer)):
            raise ValueError(f"group {b} must be a 1-D array of integer user ids")
        if g.size == 0:
            raise ValueError(f"group {b} is empty: a group needs at least one member")
        if g.size > GROUP_MAX_MEMBERS:
            raise ValueError(f"group {b} has {g.size} members; a group holds at most {GROUP_MAX_MEMBERS}")
        if g.min() < 0 or g.max() >= m:
            raise ValueError(f"group {b}: user ids must lie in [0, {m})")
        if np.unique(g).size != g.size:
            raise ValueError(f"group {b} names a user more than once")
        ptr[b + 1] = ptr[b] + g.size
    users = np.concatenate(rows).astype(np.int32) if rows else np.empty(0, dtype=np.int32)
    return ptr, users


def group_aggregate(aggregate) -> str:
    if not isinstance(aggregate, str) or aggregate not in GROUP_AGGREGATES:
        raise ValueError(f"aggregate must be one of {GROUP_AGGREGATES}, got {aggregate!r}")
    return aggregate


EXPLORE_MODES = ("ucb", "thompson")


def explore_args(beta, mode, seed, new_items=None):
    """(beta float, seed int or None) of `ALS.recommend_explore`: beta a finite real of either sign, mode one of
    EXPLORE_MODES, seed a non-negative integer - required for "thompson" (the draw is the caller's to reproduce),
    not accepted for "ucb" (nothing is drawn).  The returned seed is None exactly for "ucb"."""
    if new_items is not None:
        raise ValueError("new_items is not supported by recommend_explore")
    if isinstance(beta, bool) or not isinstance(beta, (int, float, np.integer, np.floating)) or not np.isfinite(beta):
        raise ValueError(f"beta must be a finite number, got {beta!r}")
    if not isinstance(mode, str) or mode not in EXPLORE_MODES:
        raise ValueError(f"mode must be one of {EXPLORE_MODES}, got {mode!r}")
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or seed < 0):
        raise ValueError(f"seed must be a non-negative integer, got {seed!r}")
    if mode == "thompson" and seed is None:
        raise ValueError('mode="thompson" needs a seed')
    if mode == "ucb" and seed is not None:
        raise ValueError('seed is only used with mode="thompson"')
    return float(beta), (None if seed is None else int(seed))


def id_pairs(users, items, m: int, n: int):
    u, i = _ids(users, "user"), _ids(items, "item")
    if u.shape != i.shape:
        raise ValueError("users and items must have the same length")
    _in_range(u, m, "user")
    _in_range(i, n, "item")
    return u.astype(np.int64), i.astype(np.int64)


def target_lists(targets, B: int, n: int):
    """`targets` = (indptr [B + 1], items in [0, n)) of `rank_of_new` / `explain_new` -> (int64, int64)."""
    if not isinstance(targets, (tuple, list)) or len(targets) != 2:
        raise ValueError("targets must be (indptr, items)")
    tptr = np.asarray(targets[0])
    if tptr.ndim != 1 or tptr.size != B + 1 or not np.issubdtype(tptr.dtype, np.integer):
        raise ValueError(f"targets indptr must hold {B + 1} integers (one row per row of R_new)")
    tptr = tptr.astype(np.int64)
    ti = _ids(targets[1], "item")
    _in_range(ti, n, "item")
    if tptr[0] != 0 or tptr[-1] != ti.size or (np.diff(tptr) < 0).any():
        raise ValueError("targets indptr must start at 0, be non-decreasing and end at len(items)")
    return tptr, ti.astype(np.int64)


def item_filter(x, n_total: int, name: str, kind: str = "item") -> Optional[np.ndarray]:
    """One of `items=` / `filter_items=` (`name`) over a catalogue of n_total items -> None (not given), a bool mask
    [n_total], or int64 item ids in [0, n_total) (any order, duplicates kept).  Raises ValueError otherwise.
    `kind`: what the ids name in the messages ("user" for `user_filters`)."""
    if x is None:
        return None
    a = np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)
    if a.ndim != 1:
        raise ValueError(f"{name} must be a 1-D array of integer {kind} ids or a boolean mask of length {n_total}")
    if a.dtype == np.bool_:
        if a.size != n_total:
            raise ValueError(f"{name} as a boolean mask has {a.size} entries. Expected number of {kind}s: {n_total}.")
        return a
    if a.size == 0:                                          # an empty list, whatever dtype numpy gave it
        return np.empty(0, dtype=np.int64)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name} must hold integer {kind} ids or booleans, got dtype {a.dtype}")
    if a.min() < 0 or a.max() >= n_total:
        raise ValueError(f"{name}: {kind} ids must lie in [0, {n_total})")
    return a.astype(np.int64)


def item_filters(items, filter_items, n_total: int):
    """The allow-list `items=` and the block-list `filter_items=` of a serving call: None when neither is given
    (the call then takes the unfiltered path), else the pair of `item_filter` results."""
    if items is None and filter_items is None:
        return None
    return item_filter(items, n_total, "items"), item_filter(filter_items, n_total, "filter_items")


def user_filters(users, filter_users, m: int):
    """The allow-list `users=` and the block-list `filter_users=` of `recommend_users`, over the m users: as
    `item_filters` (None when neither is given), the messages naming these two parameters and user ids."""
    if users is None and filter_users is None:
        return None
    return item_filter(users, m, "users", "user"), item_filter(filter_users, m, "filter_users", "user")


def allowed_mask(filters, n_total: int) -> np.ndarray:
    """bool [n_total] of an `item_filters` pair: `items` (every item when None) minus `filter_items`.  The host
    definition of what serving._Serving.allow_bitmap packs on the device."""
    allow, block = filters
    mask = np.ones(n_total, dtype=bool)
    if allow is not None:
        if allow.dtype == np.bool_:
            mask = allow.copy()
        else:
            mask[:] = False
            mask[allow] = True
    if block is not None:
        if block.dtype == np.bool_:
            mask &= ~block
        else:
            mask[block] = False
    return mask


def item_capacity(capacity, n_total: int) -> np.ndarray:
    """`capacity=` of `recommend_capacity` over n_total items -> int32 [n_total]: an integer scalar (the same cap for
    every item) or a 1-D integer array with one entry per item, every entry >= 0 (values above 2^31 - 1 mean the same:
    no batch is that long).  None is refused: a call without caps is `recommend`."""
    if capacity is None:
        raise ValueError("capacity is required: an integer array with one entry per item, or an integer scalar "
                         "(None is not accepted; a call without caps is recommend)")
    a = np.asarray(capacity.detach().cpu().numpy() if torch.is_tensor(capacity) else capacity)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"capacity must hold integers, got dtype {a.dtype}")
    if a.ndim == 0:
        a = np.full(n_total, a.item(), dtype=np.int64)
    if a.shape != (n_total,):
        raise ValueError(f"capacity has shape {a.shape}. Expected number of items: {n_total}.")
    if a.size and a.min() < 0:
        raise ValueError("capacity must not be negative")
    return np.minimum(a, np.iinfo(np.int32).max).astype(np.int32)


def capacity_filters(filters, capacity: np.ndarray):
    """The `item_filters` pair of a capped call with the items of capacity 0 blocked as well: they go into the allow
    bitmap together with the filters.  None when there is nothing to block."""
    stocked = capacity > 0
    if filters is None:
        return None if stocked.all() else (stocked, None)
    return allowed_mask(filters, capacity.size) & stocked, None


def max_rounds_arg(max_rounds) -> Optional[int]:
    """`max_rounds=` of `recommend_capacity`: None (run to the fixed point) or an integer >= 0."""
    if max_rounds is None:
        return None
    if isinstance(max_rounds, bool) or not isinstance(max_rounds, (int, np.integer)) or max_rounds < 0:
        raise ValueError(f"max_rounds must be None or an integer >= 0, got {max_rounds!r}")
    return int(max_rounds)


def _int_array(a, what: str) -> np.ndarray:
    a = np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a)
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} must hold integers, got dtype {a.dtype}")
    return a


def item_groups(groups, max_per_group, n_total: int):
    """`groups=` / `max_per_group=` of `recommend_quota` over n_total items -> (labels int32 [n_total], caps int32 [G]).
    `groups`: a 1-D integer array with one label >= -1 per item (-1: the item belongs to no group and is never
    capped).  `max_per_group`: a non-negative integer scalar - the same cap for every group - or a 1-D integer array
    of non-negative caps that covers every label used (cap[g] for label g).  Caps above 2^31 - 1 mean the same: no
    list is that long."""
    if groups is None or max_per_group is None:
        raise ValueError("groups and max_per_group are required (None is not accepted; a call without caps is "
                         "recommend)")
    g = _int_array(groups, "groups")
    if g.shape != (n_total,):
        raise ValueError(f"groups has shape {g.shape}. Expected number of items: {n_total}.")
    if g.size and g.min() < -1:
        raise ValueError("groups must hold labels >= 0, or -1 for an item without a group")
    top = int(g.max()) if g.size else -1
    if top >= np.iinfo(np.int32).max:
        raise ValueError("group labels must be below 2^31 - 1")
    c = _int_array(max_per_group, "max_per_group")
    if c.ndim == 0:
        c = np.full(top + 1, c.item(), dtype=np.int64)
    if c.ndim != 1:
        raise ValueError(f"max_per_group must be an integer scalar or a 1-D array, got shape {c.shape}")
    if c.size and c.min() < 0:
        raise ValueError("max_per_group must not be negative")
    if c.size <= top:
        raise ValueError(f"max_per_group has {c.size} entries: label {top} has no cap")
    return g.astype(np.int32), np.minimum(c, np.iinfo(np.int32).max).astype(np.int32)


def quota_allowed(filters, n_total: int) -> Optional[np.ndarray]:
    """The `item_filters` pair of a `recommend_quota` call as one boolean mask over the catalogue (None: every item):
    what serving.quota_plan counts the groups over."""
    return None if filters is None else allowed_mask(filters, n_total)


ELIGIBILITY_MAX_ATTRS = 256     # 32 ALS_ELIGIBILITY_MAX_TAG_WORDS
ELIGIBILITY_RULES = ("need_all", "need_any", "forbid")


def _host(x):
    return np.asarray(x.detach().cpu().numpy() if torch.is_tensor(x) else x)


def _tag_words(x, rows: int, tw: Optional[int], name: str, row_kind: str, attrs: Optional[int] = None) -> np.ndarray:
    """One of item_tags / a rule of `ALS.eligibility` -> int32 words [rows, tw]: bool [rows, A <= 256] is packed
    (`pack_words`), uint32 / int32 [rows, tw <= 8] taken as the words.  `tw`: the width the tags fixed, None for the
    tags themselves; `attrs`: the attribute count of boolean tags, which a boolean rule has to match."""
    a = _host(x)
    if a.ndim != 2 or a.shape[0] != rows:
        raise ValueError(f"{name} must be a 2-D array with one row per {row_kind} ({rows}), got shape {a.shape}")
    if a.dtype == np.bool_:
        if not 1 <= a.shape[1] <= ELIGIBILITY_MAX_ATTRS:
            raise ValueError(f"{name}: between 1 and {ELIGIBILITY_MAX_ATTRS} attributes, got {a.shape[1]}")
        if attrs is not None and a.shape[1] != attrs:
            raise ValueError(f"{name} has {a.shape[1]} attributes; item_tags has {attrs}")
        w = pack_words(a)
    elif a.dtype in (np.uint32, np.int32):
        if not 1 <= a.shape[1] <= ELIGIBILITY_MAX_ATTRS // 32:
            raise ValueError(f"{name}: between 1 and {ELIGIBILITY_MAX_ATTRS // 32} words per row, got {a.shape[1]}")
        w = np.ascontiguousarray(a).view(np.int32)
    else:
        raise ValueError(f"{name} must be boolean [rows, attributes] or uint32 [rows, words], got dtype {a.dtype}")
    if tw is not None and w.shape[1] != tw:
        raise ValueError(f"{name} has {w.shape[1]} words of attribute bits per row; item_tags has {tw}")
    return w


def eligibility_inputs(segment_items, item_tags, rules, n_total: int, max_bytes: int):
    """The table input of `ALS.eligibility` over a catalogue of n_total items: ("masks", bool [S, n_total]) from
    `segment_items` (a bool array or S id lists), or ("tags", (tags, need_all, need_any, forbid)) - int32 words
    [n_total, tw] and [S, tw], an absent rule None - from `item_tags` and `rules`.  Exactly one of the two; a table of
    more than `max_bytes` (serving.ELIGIBILITY_MAX_BYTES) is refused before anything is built."""
    if (segment_items is None) == (item_tags is None):
        raise ValueError("give exactly one of segment_items and item_tags")

    def check_size(S: int):
        if S < 1:
            raise ValueError("an eligibility table needs at least one segment")
        need = S * ((n_total + 31) // 32) * 4
        if need > max_bytes:
            raise ValueError(f"the eligibility table of {S} segments over {n_total} items takes {need} bytes; "
                             f"ELIGIBILITY_MAX_BYTES is {max_bytes}")

    if segment_items is not None:
        if rules is not None:
            raise ValueError("rules go with item_tags, not with segment_items")
        a = segment_items if isinstance(segment_items, (list, tuple)) else _host(segment_items)
        if isinstance(a, np.ndarray) and a.dtype == np.bool_:
            if a.ndim != 2 or a.shape[1] != n_total:
                raise ValueError(f"segment_items as a boolean array must be [segments, {n_total}], got {a.shape}")
            check_size(a.shape[0])
            return "masks", a
        check_size(len(a))
        masks = np.zeros((len(a), n_total), dtype=bool)
        for s, ids in enumerate(a):
            ids = item_filter(ids, n_total, f"segment_items[{s}]")
            masks[s] = ids if ids.dtype == np.bool_ else np.isin(np.arange(n_total), ids)
        return "masks", masks
    if not isinstance(rules, dict) or not rules or set(rules) - set(ELIGIBILITY_RULES):
        raise ValueError(f"rules must be a dict with some of the keys {ELIGIBILITY_RULES}")
    given = [r for r in ELIGIBILITY_RULES if rules.get(r) is not None]
    if not given:
        raise ValueError("rules holds no rule")
    first, raw_tags = _host(rules[given[0]]), _host(item_tags)
    S = first.shape[0] if first.ndim == 2 else 0
    check_size(S)
    tags = _tag_words(raw_tags, n_total, None, "item_tags", "item")
    attrs = raw_tags.shape[1] if raw_tags.dtype == np.bool_ else None
    words = [None if rules.get(r) is None else
             _tag_words(rules[r], S, tags.shape[1], f"rules[{r!r}]", "segment", attrs) for r in ELIGIBILITY_RULES]
    return "tags", (tags, *words)


def eligibility_table(elig, n_total: int):
    """The `eligibility=` argument of the *_eligible calls: an ItemEligibility over exactly the catalogue scored."""
    if not isinstance(elig, ItemEligibility):
        raise ValueError("eligibility must be an ItemEligibility (ALS.eligibility)")
    if elig.n_items != n_total:
        raise ValueError(f"the eligibility table spans {elig.n_items} items. Expected number of items: {n_total}.")
    return elig


def segment_ids(segments, rows: int, n_segments: int, what: str = "batch row") -> np.ndarray:
    """`segments=` -> int32 [rows]: one id in [0, n_segments) per `what`."""
    if segments is None:
        raise ValueError("segments is required: one segment id per " + what)
    s = _host(segments)
    if s.ndim != 1 or (s.size and not np.issubdtype(s.dtype, np.integer)):
        raise ValueError("segments must be a 1-D array of integer segment ids")
    if s.size != rows:
        raise ValueError(f"segments has {s.size} entries. Expected one per {what}: {rows}.")
    if s.size and (s.min() < 0 or s.max() >= n_segments):
        raise ValueError(f"segment ids must lie in [0, {n_segments})")
    return s.astype(np.int32)


def folded_items(model, folded) -> None:
    fitted(model)
    if not isinstance(folded, FoldedItems):
        raise ValueError("new items must be a FoldedItems record (ALS.fold_in_items)")
    k, B = model.V.shape[1], folded.n_items
    if folded.Z.shape != (B, k) or folded.b_i.shape != (B,):
        raise ValueError(f"FoldedItems holds Z {folded.Z.shape} and b_i {folded.b_i.shape}; this model needs "
                         f"({B}, {k}) and ({B},)")
    if len(folded.ratings[0]) != B + 1:
        raise ValueError("FoldedItems: ratings CSR does not have one row per item")


# ------------------------------------------------------------------ host CSR
def _host_csr(triple, ncols: int, nrows=None):
    """Structure of a host CSR triple: (fault, ptr int64, idx, val) with fault None or the first of "shape" (not
    1-D, non-integer ptr / idx; without `nrows` also an empty ptr), "rows" (ptr.size != nrows + 1), "ptr" (does not
    start at 0, decreases, or does not end at len(idx) == len(val)), "range" (idx outside [0, ncols)).  The callers
    word the errors - and choose their types - themselves."""
    ptr, idx, val = (np.asarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a) for a in triple)
    if (ptr.ndim != 1 or idx.ndim != 1 or val.ndim != 1 or (nrows is None and ptr.size < 1)
            or (ptr.size and not np.issubdtype(ptr.dtype, np.integer))
            or (idx.size and not np.issubdtype(idx.dtype, np.integer))):
        return "shape", ptr, idx, val
    if nrows is not None and ptr.size != nrows + 1:
        return "rows", ptr, idx, val
    ptr = ptr.astype(np.int64)
    if ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != idx.size or idx.size != val.size:
        return "ptr", ptr, idx, val
    if idx.size and (idx.min() < 0 or idx.max() >= ncols):
        return "range", ptr, idx, val
    return None, ptr, idx, val


def _finite_f32(vals: np.ndarray, message: str) -> np.ndarray:
    with np.errstate(over="ignore"):
        vals32 = vals.astype(np.float32)
    if not np.isfinite(vals32).all():
        raise ValueError(message)
    return vals32


def fold_in_csr(R_new, n: int):
    """Ratings of users outside the fit -> host CSR (indptr int64 [B+1], indices int32, vals float32), every row's
    columns ascending (values carried along).  `R_new`: a dense (B, n) array with NaN for missing ratings, or a CSR
    triple (indptr, indices, vals) in any column order.  Raises ValueError for a wrong dense width, a malformed
    triple, a duplicate column in a row or a non-finite rating, IndexError for a column outside [0, n)."""
    if isinstance(R_new, (tuple, list)) and len(R_new) == 3 and not np.isscalar(R_new[0]) and np.ndim(R_new[0]) == 1:
        fault, indptr, indices, vals = _host_csr(R_new, n)
        if fault == "shape":
            raise ValueError("R_new as CSR must be 1-D (indptr, indices, vals) with integer indptr / indices")
        if fault == "ptr":
            raise ValueError("R_new: indptr must start at 0, not decrease, and end at len(indices) == len(vals)")
        if fault == "range":
            raise IndexError(f"R_new: column indices must lie in [0, {n})")
        indices = indices.astype(np.int64)
        vals = vals.astype(np.float64)
    else:
        R = np.asarray(R_new, dtype=np.float64)
        if R.ndim != 2 or R.shape[1] != n:
            raise ValueError(f"R_new must be a dense (B, {n}) array (NaN = missing) or a CSR triple, "
                             f"got shape {R.shape}")
        mask = ~np.isnan(R)
        indptr = np.zeros(R.shape[0] + 1, dtype=np.int64)
        np.cumsum(mask.sum(axis=1), out=indptr[1:])
        indices = np.nonzero(mask)[1].astype(np.int64)
        vals = R[mask]
    vals32 = _finite_f32(vals, "R_new contains non-finite ratings (or ones beyond the float32 range)")
    B = indptr.size - 1
    row = np.repeat(np.arange(B, dtype=np.int64), np.diff(indptr))
    order = np.lexsort((indices, row))
    indices, vals32 = indices[order], vals32[order]
    if indices.size > 1 and ((np.diff(indices) == 0) & (np.diff(row) == 0)).any():
        raise ValueError("R_new has a duplicate column within a row")
    return indptr, indices.astype(np.int32), vals32


def new_item_features(features_new, W_dims: Dict[str, int], B: int) -> Dict[str, np.ndarray]:
    """Validated features of new items: every feature of the fit (`W_dims`: name -> columns) and nothing else, each
    a finite (B, d) array.  Raises ValueError otherwise."""
    fn = host_features(features_new)
    missing = [f for f in W_dims if f not in fn]
    if missing:
        raise ValueError(f"features_new must name every feature of the fit; missing: {missing}")
    unknown = [f for f in fn if f not in W_dims]
    if unknown:
        raise ValueError(f"features_new names features the model was not fitted with: {unknown}")
    out = {}
    for f, d in W_dims.items():
        X = np.asarray(fn[f])
        if X.ndim != 2 or X.shape != (B, d):
            raise ValueError(f"Feature '{f}' of the new items has shape {X.shape}; expected ({B}, {d})")
        if not np.isfinite(X).all():
            raise ValueError(f"Feature '{f}' of the new items contains non-finite values.")
        out[f] = X
    return out


def new_item_graph_csr(S_new, B: int, n: int):
    """Caller-supplied graph rows of new items -> host CSR (ptr int64 [B+1], idx int32 in [0, n), val float32).
    Raises ValueError for a malformed triple, a wrong row count, an index outside [0, n) or a non-finite weight."""
    if not (isinstance(S_new, (tuple, list)) and len(S_new) == 3):
        raise ValueError("S_new must be a CSR triple (ptr, idx, val)")
    fault, ptr, idx, val = _host_csr(S_new, n, nrows=B)
    if fault == "shape":
        raise ValueError("S_new must be 1-D (ptr, idx, val) with integer ptr / idx")
    if fault == "rows":
        raise ValueError(f"S_new has {ptr.size - 1} rows; expected {B} (one per new item)")
    if fault == "ptr":
        raise ValueError("S_new: ptr must start at 0, not decrease, and end at len(idx) == len(val)")
    if fault == "range":
        raise ValueError(f"S_new: item indices must lie in [0, {n}) (fitted items)")
    return ptr, idx.astype(np.int32), _finite_f32(val, "S_new contains non-finite weights")


def _check_csr(indptr: torch.Tensor, indices: torch.Tensor, nrows: int, ncols: int, what: str):
    """Structural validation of a caller-supplied CSR (one device reduction each): an index outside
    [0, ncols) would be an out-of-bounds gather inside the kernels."""
    if indptr.numel() != nrows + 1:
        raise ValueError(f"{what}: indptr has {indptr.numel()} entries, expected {nrows + 1}")
    nnz = indices.numel()
    if int(indptr[0]) != 0 or int(indptr[-1]) != nnz or (nrows and bool((indptr[1:] < indptr[:-1]).any())):
        raise ValueError(f"{what}: indptr must rise monotonically from 0 to nnz = {nnz}")
    if nnz and (int(indices.min()) < 0 or int(indices.max()) >= ncols):
        raise ValueError(f"{what}: index outside [0, {ncols})")


def _as_side(triple, nrows: int, ncols: int):
    indptr, indices, vals = triple
    if isinstance(indptr, torch.Tensor):
        if indptr.dtype != torch.int64 or indices.dtype != torch.int32 or vals.dtype != torch.float32:
            raise ValueError("device CSR needs int64 indptr, int32 indices, float32 vals")
        if indptr.numel() != nrows + 1 or indices.numel() != vals.numel():
            raise ValueError("inconsistent CSR sizes")
        _check_csr(indptr, indices, nrows, ncols, "ratings CSR")
        return _SideDev(nrows, ncols, indptr.contiguous(), indices.contiguous(), vals.contiguous())
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    indices = np.ascontiguousarray(indices, dtype=np.int32)
    _check_csr(torch.from_numpy(indptr), torch.from_numpy(indices), nrows, ncols, "ratings CSR")
    return layout.SparseSide(nrows, ncols, indptr, indices, np.ascontiguousarray(vals, dtype=np.float32))


def _validate_graph(ptr: torch.Tensor, idx: torch.Tensor, val: torch.Tensor, n: int):
    """A caller-supplied similarity graph must be what the reference would have built (scripts/als.py:224-240):
    indices inside [0, n), ascending inside every row, no diagonal, and SYMMETRIC in pattern and value
    (S = max(S, S^T)).  The level schedule of the Gauss-Seidel sweep relies on the symmetry: a neighbour
    j > i must sit on a later level so that it still holds its previous value when i is solved."""
    _check_csr(ptr, idx, n, n, "similarity graph S")
    if val.numel() != idx.numel():
        raise ValueError("similarity graph S: values and indices differ in length")
    if idx.numel() == 0:
        return
    rows = torch.repeat_interleave(torch.arange(n, device=ptr.device), ptr[1:] - ptr[:-1])
    cols = idx.to(torch.int64)
    key = rows * n + cols
    if bool((key[1:] <= key[:-1]).any()):
        raise ValueError("similarity graph S: column indices must be strictly ascending inside every row")
    if bool((rows == cols).any()):
        raise ValueError("similarity graph S: diagonal entries are not allowed (the reference zeroes them)")
    tkey, order = torch.sort(cols * n + rows)
    if not torch.equal(tkey, key) or not torch.equal(val[order], val):
        raise ValueError("similarity graph S must be symmetric in pattern and value (S == S^T); "
                         "symmetrise with max(S, S^T) as the reference does")
