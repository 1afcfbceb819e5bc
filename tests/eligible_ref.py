"""The contracts of als_recommend_topk_segmented, als_rank_count_segmented and als_eligibility_bitmaps
(include/als_hip.h), in numpy, read by both suites.

The two segmented kernels have a one-sentence definition - row b is row b of the masked call with allow =
E[row_seg[b]] - so `EligibleNumpyBackend` IS that sentence: it loops the masked stand-ins of tests/cpu_backend.py
(the contracts of tests/serving_ref.py) over the batch rows.  The table builder is defined item by item, on bool arrays
(`eligible_bool`: what the rule means) and on the packed words the kernel reads (`eligibility_words`)."""
import numpy as np
import torch

from tests.cpu_backend import NumpyBackend
from tests.serving_ref import bitmap_numpy


def eligible_bool(tags, need_all, need_any, forbid, base=None):
    """bool [S, n]: the rule of `ALS.eligibility` on bool tags [n, A] and bool rules [S, A] (None = no such rule),
    `base` bool [n] ANDed into every segment."""
    n, A = tags.shape
    S = next(r for r in (need_all, need_any, forbid) if r is not None).shape[0]
    zero = np.zeros((S, A), dtype=bool)
    need_all, need_any, forbid = (zero if r is None else r for r in (need_all, need_any, forbid))
    out = np.zeros((S, n), dtype=bool)
    for s in range(S):
        for i in range(n):
            ok = not (tags[i] & forbid[s]).any() and (tags[i] | ~need_all[s]).all()
            ok = ok and (not need_any[s].any() or (tags[i] & need_any[s]).any())
            out[s, i] = ok and (base is None or base[i])
    return out


def eligibility_words(tags, need_all, need_any, forbid, base_words=None):
    """uint32 [S, ceil(n / 32)]: als_eligibility_bitmaps on uint32 tag words [n, tw], rule words [S, tw] (None = all
    zero) and the base bitmap (uint32 words or None), item by item; the bits >= n of the last word are 0."""
    tags = np.ascontiguousarray(tags).view(np.uint32)
    n, tw = tags.shape
    S = next(r for r in (need_all, need_any, forbid) if r is not None).shape[0]
    zero = np.zeros((S, tw), dtype=np.uint32)
    need_all, need_any, forbid = (zero if r is None else np.ascontiguousarray(r).view(np.uint32)
                                  for r in (need_all, need_any, forbid))
    out = np.zeros((S, (n + 31) // 32), dtype=np.uint32)
    for s in range(S):
        mask = np.zeros(n, dtype=bool)
        for i in range(n):
            ok = all((tags[i, w] & forbid[s, w]) == 0 and (tags[i, w] & need_all[s, w]) == need_all[s, w]
                     for w in range(tw))
            ok = ok and (not need_any[s].any() or any((tags[i, w] & need_any[s, w]) != 0 for w in range(tw)))
            if base_words is not None:
                ok = ok and bool((int(base_words[i >> 5]) >> (i & 31)) & 1)
            mask[i] = ok
        out[s] = bitmap_numpy(mask)
    return out


def table_numpy(masks):
    """uint32 [S, ceil(n / 32)] from bool [S, n]: `bitmap_numpy` row by row."""
    return np.stack([bitmap_numpy(m) for m in masks])


class EligibleNumpyBackend(NumpyBackend):
    """NumpyBackend with the three eligibility entry points; `calls` records one tuple per segmented call."""

    def recommend_topk_segmented(self, *, seg_allow, row_seg, users, top_val, top_idx, top_cnt, **kw):
        assert row_seg.dtype == torch.int32 and row_seg.numel() == users.numel() and seg_allow.dtype == torch.int32
        W = (kw["n"] + 31) // 32
        mark = len(self.calls)
        for b in range(users.numel()):
            self.recommend_topk(users=users[b: b + 1], allow=seg_allow[int(row_seg[b]), :W].contiguous(),
                                top_val=top_val[b: b + 1], top_idx=top_idx[b: b + 1], top_cnt=top_cnt[b: b + 1], **kw)
        self.calls[mark:] = [("recommend_topk_segmented", users.numel(), seg_allow.data_ptr())]

    def rank_count_segmented(self, *, seg_allow, row_seg, q_users, q_ptr, q_items, t_score, above, n_cand, **kw):
        assert row_seg.dtype == torch.int32 and row_seg.numel() == q_users.numel() and seg_allow.dtype == torch.int32
        W = (kw["n"] + 31) // 32
        mark = len(self.calls)
        for b in range(q_users.numel()):
            t0, t1 = int(q_ptr[b]), int(q_ptr[b + 1])
            self.rank_count(q_users=q_users[b: b + 1], q_ptr=q_ptr[b: b + 2] - t0, q_items=q_items[t0:t1],
                            allow=seg_allow[int(row_seg[b]), :W].contiguous(), t_score=t_score[t0:t1],
                            above=above[t0:t1], n_cand=n_cand[b: b + 1], **kw)
        self.calls[mark:] = [("rank_count_segmented", q_users.numel(), seg_allow.data_ptr())]

    def eligibility_bitmaps(self, *, n, item_tags, need_all, need_any, forbid, base_allow, out):
        assert item_tags.dtype == torch.int32 and tuple(out.shape) == (out.shape[0], (n + 31) // 32)
        self.calls.append(("eligibility_bitmaps", n, out.shape[0], item_tags.shape[1]))
        w = lambda t: None if t is None else t.numpy().view(np.uint32)      # noqa: E731
        words = eligibility_words(w(item_tags), w(need_all), w(need_any), w(forbid), w(base_allow))
        out.copy_(torch.from_numpy(words.view(np.int32)))
