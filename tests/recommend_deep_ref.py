"""The contract of als_recommend_deep (include/als_hip.h) in numpy, and the stand-in backend that serves it to the
engine on the CPU.

`deep_topn_batch` is serving_ref's selection - `candidates`, then the first N in (score descending, item ascending) -
on the candidates that lie strictly below the row's cursor.  The cursor is applied in the two ways the contract states
it, and the tests use both: as an entry (`below_entry`: a lower score, or the same score and a higher item id) and as
the 64-bit key of the C ABI (`keys`, `below_key`).  Scores are taken as given - on the GPU the rows als_predict_dense
writes.  `DeepNumpyBackend` forms them with the stand-in's own epilogue."""
import numpy as np
import torch

from tests import serving_ref as ref
from tests.audience_ref import AudienceNumpyBackend

NO_CURSOR = np.uint64(0xFFFFFFFFFFFFFFFF)


def keys(scores_f32, items):
    """uint64 keys of (score, item) pairs as the header defines them: (enc(score) << 32) | (0xFFFFFFFF - item)."""
    s = np.asarray(scores_f32, dtype=np.float32) + np.float32(0.0)           # -0.0 -> +0.0
    bits = s.view(np.uint32).astype(np.uint64)
    neg = (bits >> np.uint64(31)) == 1
    enc = np.where(neg, ~bits & np.uint64(0xFFFFFFFF), bits | np.uint64(0x80000000))
    return (enc << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(items).astype(np.uint64))


def below_key(scores_row, key):
    """bool [n]: item i's key is strictly below `key` (uint64)."""
    return keys(scores_row, np.arange(scores_row.size)) < np.uint64(key)


def below_entry(scores_row, after_item, after_score):
    """bool [n]: item i comes strictly after the entry (after_item, after_score) in (score descending, item
    ascending); nothing does for after_item == -1."""
    if after_item < 0:
        return np.zeros(scores_row.size, bool)
    a = np.float32(after_score)
    with np.errstate(invalid="ignore"):
        return (scores_row < a) | ((scores_row == a) & (np.arange(scores_row.size) > after_item))


def deep_topn_batch(scores, seen_rows, allowed, N, after=None, after_keys=None):
    """What als_recommend_deep writes for a batch: (values [B, N] padded with -inf, items int32 [B, N] padded with -1,
    counts int32 [B]).  after: None or (after_items [B], after_scores [B]); after_keys: None or uint64 [B]."""
    B, n = scores.shape
    tv = np.full((B, N), -np.inf, scores.dtype)
    ti = np.full((B, N), -1, np.int32)
    tc = np.zeros(B, np.int32)
    for b in range(B):
        ok = np.ones(n, bool) if allowed is None else allowed.copy()
        if after is not None:
            ok &= below_entry(scores[b], int(after[0][b]), after[1][b])
        if after_keys is not None:
            ok &= below_key(scores[b], after_keys[b])
        v, i, c = ref.topn(scores[b], seen_rows[b], ok, N)
        tv[b, :c], ti[b, :c], tc[b] = v, i, c
    return tv, ti, tc


def full_order(scores_row, seen, allowed):
    """Every candidate of the row, in order: what paging to exhaustion must enumerate."""
    return ref.topn(scores_row, seen, allowed, scores_row.size)[1]


class DeepNumpyBackend(AudienceNumpyBackend):
    """The stand-in backend (tests/cpu_backend.NumpyBackend; AudienceNumpyBackend adds the item fold-in) with
    `recommend_deep`: the cursor arrives as the C ABI's keys (int64 bit patterns)."""

    def recommend_deep_workspace_bytes(self, nusers, n, topn):
        """The documented size with the most slices and the longest list: 74 240 bytes per row."""
        self.calls.append(("recommend_deep_workspace_bytes", nusers, n, topn))
        return 8 * nusers * (128 * 64 + 1024 + 64) + 64

    def recommend_deep(self, *, k, ld, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow, after_key, topn,
                       top_val, top_idx, top_cnt, rounds=None):
        self.calls.append(("recommend_deep", users.numel(), topn, None if allow is None else allow.data_ptr(),
                           after_key is not None))
        assert 1 <= topn <= 1024
        S, seen = self._serving_rows(users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx)
        ok = None if allow is None else ref.unpack_bitmap(allow.numpy(), n)
        ak = None
        if after_key is not None:
            assert after_key.dtype == torch.int64 and after_key.numel() == users.numel()
            ak = after_key.numpy().view(np.uint64)
        for out, a in zip((top_val, top_idx, top_cnt), deep_topn_batch(S, seen, ok, topn, after_keys=ak)):
            out[: a.shape[0]] = torch.from_numpy(a)
        if rounds is not None:
            rounds.fill_(1)
