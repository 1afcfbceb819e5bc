#!/usr/bin/env python3
"""Exact full-catalogue ranks (csrc/rank_eval.hip, als_rank_count) at the configs[3] shape: 1M users x 100K items,
k = 64, ~100 seen items per user, seeded random factors (no fit needed).  Times all users / 4096 / 64 / 1 users
with 1, 8 and 64 targets per user, in the same process als_recommend_topk (N = 10) on the same users, and for the
4096-user case a composed baseline (blocked torch matmul, -inf at the seen items, one masked compare per target).
Writes one JSON object to argv[1] (default: stdout only).

    python profiles/rank_eval_time.py profiles/rank_eval_time.json
    rocprofv3 --kernel-trace --stats -d DIR -o rank -- python profiles/rank_eval_time.py --quick   # kernel table"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import layout  # noqa: E402
from collaborative_filtering_amd.backend import HipBackend  # noqa: E402

M, NI, K = 1_000_000, 100_000, 64
MFMA_F32_FLOPS = 155e12          # fp32 matrix-core peak of the MI355X
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
seen_rows = torch.repeat_interleave(torch.arange(M, device=dev), seen_ptr[1:] - seen_ptr[:-1])
del raw, keep


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
    return float(np.median(ts)), float(np.min(ts))


def recommend(users, N):
    B = users.numel()
    tv = torch.empty(B, N, dtype=torch.float32, device=dev)
    ti = torch.empty(B, N, dtype=torch.int32, device=dev)
    tc = torch.empty(B, dtype=torch.int32, device=dev)
    return lambda: be.recommend_topk(k=K, ld=ld, users=users, n=NI, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu,
                                     seen_ptr=seen_ptr, seen_idx=seen_idx, topn=N, top_val=tv, top_idx=ti,
                                     top_cnt=tc)


def targets(B, T, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return (torch.arange(B + 1, dtype=torch.int64, device=dev) * T,
            torch.randint(0, NI, (B * T,), device=dev, generator=g, dtype=torch.int32))


def rank(users, T):
    B = users.numel()
    q_ptr, q_items = targets(B, T, T)
    sc = torch.empty(B * T, dtype=torch.float32, device=dev)
    ab = torch.empty(B * T, dtype=torch.int32, device=dev)
    nc = torch.empty(B, dtype=torch.int32, device=dev)
    return lambda: be.rank_count(k=K, ld=ld, n=NI, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, seen_ptr=seen_ptr,
                                 seen_idx=seen_idx, q_users=users, q_ptr=q_ptr, q_items=q_items, t_score=sc, above=ab,
                                 n_cand=nc)


def baseline(users, T, chunk=1024):
    """What a caller composes without the kernel: scores of a block of users by a matmul, -inf at their seen items,
    then per target one compare over the block's score matrix (ties are not broken by item here)."""
    q_ptr, q_items = targets(users.numel(), T, T)
    tgt = q_items.view(-1, T).long()

    def run():
        for c0 in range(0, users.numel(), chunk):
            us = users[c0: c0 + chunk].long()
            S = U[us] @ Z.T + (mu.float() + b_u[us])[:, None] + b_i[None, :]
            ts = torch.gather(S, 1, tgt[c0: c0 + chunk])
            cnt = seen_ptr[us + 1] - seen_ptr[us]
            rows = torch.repeat_interleave(torch.arange(us.numel(), device=dev), cnt)
            off = torch.arange(int(cnt.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
            S[rows, seen_idx[seen_ptr[us][rows] + off].long()] = -float("inf")
            for t in range(T):
                (S > ts[:, t: t + 1]).sum(dim=1)
    return run


res = {"shape": {"users": M, "items": NI, "k": K, "seen_per_user": float(seen_idx.numel() / M)},
       "bound_note": "fp32 matrix-core bound 2 m n k / 155e12 s", "runs": {}}
rng = np.random.default_rng(0)
groups = [("all", torch.arange(M, dtype=torch.int32, device=dev))]
for B in (4096, 64, 1):
    groups.append((f"batch{B}", torch.from_numpy(rng.choice(M, B, replace=False).astype(np.int32)).to(dev)))
for gname, users in groups:
    reps = 1 if quick else (3 if users.numel() == M else 20)
    pairs = users.numel() * NI
    bound_ms = 2.0 * pairs * K / MFMA_F32_FLOPS * 1e3
    runs = [(f"{gname}_recommend_N10", recommend(users, 10), None)]
    runs += [(f"{gname}_rank_T{T}", rank(users, T), T) for T in (1, 8, 64)]
    for name, fn, T in runs:
        med, best = timed(fn, reps)
        res["runs"][name] = {"users": users.numel(), "targets_per_user": T, "ms": med, "ms_min": best,
                             "pairs_per_s": pairs / med * 1e3, "matrix_core_bound_ms": bound_ms,
                             "share_of_bound": bound_ms / med}
        print(name, res["runs"][name], flush=True)
    r = res["runs"]
    res[f"{gname}_rank_T8_over_recommend_N10"] = r[f"{gname}_rank_T8"]["ms"] / r[f"{gname}_recommend_N10"]["ms"]
    res[f"{gname}_rank_T64_over_T8"] = r[f"{gname}_rank_T64"]["ms"] / r[f"{gname}_rank_T8"]["ms"]
users = groups[1][1]
med, best = timed(baseline(users, 8), 1 if quick else 5)
res["runs"]["baseline_batch4096_T8"] = {"users": users.numel(), "targets_per_user": 8, "ms": med, "ms_min": best,
                                        "pairs_per_s": users.numel() * NI / med * 1e3}
print("baseline_batch4096_T8", res["runs"]["baseline_batch4096_T8"], flush=True)
res["speedup_batch4096_T8_vs_baseline"] = med / res["runs"]["batch4096_rank_T8"]["ms"]
print(json.dumps(res))
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
