#!/usr/bin/env python3
"""Top-N recommendation over a restricted catalogue (csrc/recommend.hip, als_recommend_topk_masked) at the set-up of
profiles/recommend_time.py: 1M users x 100K items, k = 64, ~100 seen items per user, seeded random factors, N = 10.
Times the unfiltered call, an all-ones bitmap, a scattered 1 % allow-list and a contiguous 1 % allow-list, each for
all users and for a batch of 4096, and als_rank_count(_masked) for 4096 users with 10 targets each.  Every masked
list is checked against the unfiltered N = 128 list where that decides it (all-ones: equal).  Writes one JSON object
to argv[1] (default: stdout only).

    python profiles/recommend_filter_time.py profiles/recommend_filter_time.json

The unfiltered path is compared with the previous commit by another route, because two versions of the package
cannot live in one process: `git worktree add ../parent HEAD~1`, build its library, then run
`python ../parent/profiles/recommend_time.py a_i.json` and `python profiles/recommend_time.py b_i.json` alternately,
three times each, in one session.  The committed JSON carries those runs under "unfiltered_vs_parent_commit"."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import layout  # noqa: E402
from collaborative_filtering_amd.backend import HipBackend  # noqa: E402
from collaborative_filtering_amd.serving import pack_bitmap  # noqa: E402

M, NI, K, N = 1_000_000, 100_000, 64, 10
quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]

dev = torch.device("cuda", 0)
be = HipBackend(dev)
gen = torch.Generator(device=dev).manual_seed(3)
ld = layout.padded_k(K)
U = torch.zeros(M, ld, device=dev)
U[:, :K] = torch.randn(M, K, device=dev, generator=gen) * 0.3
Z = torch.zeros(NI, ld, device=dev)
Z[:, :K] = torch.randn(NI, K, device=dev, generator=gen) * 0.3
b_u = torch.randn(M, device=dev, generator=gen) * 0.1
b_i = torch.randn(NI, device=dev, generator=gen) * 0.1
mu = torch.tensor([3.6], dtype=torch.float64, device=dev)
raw = torch.randint(0, NI, (M, 100), device=dev, generator=gen).sort(dim=1).values
keep = torch.ones_like(raw, dtype=torch.bool)
keep[:, 1:] = raw[:, 1:] != raw[:, :-1]
seen_ptr = torch.zeros(M + 1, dtype=torch.int64, device=dev)
seen_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
seen_idx = raw[keep].to(torch.int32)
del raw, keep

rng = np.random.default_rng(0)
scattered = rng.random(NI) < 0.01
run = np.zeros(NI, bool)
run[40_000: 41_000] = True
masks = {"unfiltered": None, "all_ones": np.ones(NI, bool), "scattered_1pct": scattered, "contiguous_1pct": run}


def timed(fn, reps):
    fn()                                              # warm-up (and first-call costs)
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts)), [float(t) for t in ts]


def recommend(users, allow, topn=N):
    B = users.numel()
    tv = torch.empty(B, topn, dtype=torch.float32, device=dev)
    ti = torch.empty(B, topn, dtype=torch.int32, device=dev)
    tc = torch.empty(B, dtype=torch.int32, device=dev)
    kw = dict(k=K, ld=ld, users=users, n=NI, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, seen_ptr=seen_ptr, seen_idx=seen_idx,
              topn=topn, top_val=tv, top_idx=ti, top_cnt=tc)
    if allow is None:
        return (lambda: be.recommend_topk(**kw)), (tv, ti, tc)
    return (lambda: be.recommend_topk_masked(allow=allow, **kw)), (tv, ti, tc)


def rank(users, targets, allow):
    B, T = targets.shape
    q_ptr = torch.arange(0, B * T + 1, T, dtype=torch.int64, device=dev)
    out = (torch.empty(B * T, dtype=torch.float32, device=dev), torch.empty(B * T, dtype=torch.int32, device=dev),
           torch.empty(B, dtype=torch.int32, device=dev))
    kw = dict(k=K, ld=ld, n=NI, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, seen_ptr=seen_ptr, seen_idx=seen_idx,
              q_users=users, q_ptr=q_ptr, q_items=targets.reshape(-1).contiguous(), t_score=out[0], above=out[1],
              n_cand=out[2])
    if allow is None:
        return (lambda: be.rank_count(**kw)), out
    return (lambda: be.rank_count_masked(allow=allow, **kw)), out


all_users = torch.arange(M, dtype=torch.int32, device=dev)
batch = torch.from_numpy(rng.choice(M, 4096, replace=False).astype(np.int32)).to(dev)
res = {"shape": {"users": M, "items": NI, "k": K, "N": N, "seen_per_user": float(seen_idx.numel() / M)},
       "masks": {}, "runs": {}}
bitmaps = {}
for name, mask in masks.items():
    if mask is None:
        bitmaps[name] = None
        continue
    bitmaps[name] = pack_bitmap(torch.from_numpy(mask).to(dev))
    res["masks"][name] = {"allowed": int(mask.sum()),
                          "nonempty_chunks": float((bitmaps[name] != 0).float().mean().item())}

# the unfiltered N = 128 lists of the batch decide what every masked N = 10 list must be, as long as 10 survive
fn, (_, full_i, _) = recommend(batch, None, 128)
fn()
full_i = full_i.cpu().numpy()
for scope, users, reps in (("all", all_users, 7), ("batch4096", batch, 30)):
    for name in masks:
        fn, (tv, ti, tc) = recommend(users, bitmaps[name])
        med, best, worst, ts = timed(fn, 1 if quick else reps)
        row = {"users": users.numel(), "ms": med, "ms_min": best, "ms_max": worst, "spread": (worst - best) / med,
               "ms_each": ts}
        if scope == "batch4096" and masks[name] is not None:
            got = ti.cpu().numpy()
            ok = masks[name]
            checked = 0
            for b in range(got.shape[0]):
                want = full_i[b][ok[full_i[b]]][:N]
                if want.size == N:
                    assert (got[b] == want).all(), (name, b)
                    checked += 1
            row["rows_checked_against_unfiltered_top128"] = checked
        res["runs"][f"{scope}_{name}"] = row
        print(f"{scope}_{name}", row, flush=True)
    base = res["runs"][f"{scope}_unfiltered"]["ms"]
    for name in masks:
        res["runs"][f"{scope}_{name}"]["vs_unfiltered"] = res["runs"][f"{scope}_{name}"]["ms"] / base

targets = torch.randint(0, NI, (4096, 10), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
for name in masks:
    fn, _ = rank(batch, targets, bitmaps[name])
    med, best, worst, _ = timed(fn, 1 if quick else 20)
    res["runs"][f"rank_batch4096_{name}"] = {"users": 4096, "targets": 10, "ms": med, "ms_min": best, "ms_max": worst}
    print(f"rank_batch4096_{name}", res["runs"][f"rank_batch4096_{name}"], flush=True)
print(json.dumps(res))
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
