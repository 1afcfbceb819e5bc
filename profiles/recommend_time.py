#!/usr/bin/env python3
"""Top-N recommendation (csrc/recommend.hip, als_recommend_topk) at the configs[3] shape: 1M users x 100K items,
k = 64, ~100 seen items per user, seeded random factors (no fit needed).  Times all users at N = 10 and N = 100,
batches of 1 / 64 / 4096 users, and the composed baseline on the same inputs (chunked predict_dense + -inf scatter of
the seen items + torch.topk).  Writes one JSON object to argv[1] (default: stdout only).

    python profiles/recommend_time.py profiles/recommend_time.json
    rocprofv3 --kernel-trace --stats -d DIR -o rec -- python profiles/recommend_time.py --quick   # kernel table"""
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


def baseline(users, N, chunk=8192):
    """What a caller composes today: predict_dense on a chunk of users, -inf at their seen items, torch.topk."""
    out = torch.empty(chunk, NI, dtype=torch.float32, device=dev)

    def run():
        for c0 in range(0, users.numel(), chunk):
            us = users[c0: c0 + chunk].long()
            nb = us.numel()
            be.predict_dense(k=K, ld=ld, m=nb, n=NI, U=U[us], Z=Z, b_u=b_u[us], b_i=b_i, mu=mu, out=out)
            lo, hi = int(us[0]), int(us[-1]) + 1           # contiguous user ids
            s0, s1 = int(seen_ptr[lo]), int(seen_ptr[hi])
            out.view(-1)[(seen_rows[s0:s1] - lo) * NI + seen_idx[s0:s1].long()] = -float("inf")
            torch.topk(out[:nb], N, dim=1)
    return run


res = {"shape": {"users": M, "items": NI, "k": K, "seen_per_user": float(seen_idx.numel() / M)},
       "bound_note": "fp32 matrix-core bound 2 m n k / 155e12 s", "runs": {}}
all_users = torch.arange(M, dtype=torch.int32, device=dev)
cases = [("all_N10", all_users, 10), ("all_N100", all_users, 100)]
rng = np.random.default_rng(0)
for B in (1, 64, 4096):
    cases.append((f"batch{B}_N10", torch.from_numpy(rng.choice(M, B, replace=False).astype(np.int32)).to(dev), 10))
for name, users, N in cases:
    reps = 3 if users.numel() == M else 20
    if quick:
        reps = 1
    med, best = timed(recommend(users, N), reps)
    pairs = users.numel() * NI
    bound_ms = 2.0 * pairs * K / MFMA_F32_FLOPS * 1e3
    res["runs"][name] = {"users": users.numel(), "N": N, "ms": med, "ms_min": best, "pairs_per_s": pairs / med * 1e3,
                         "matrix_core_bound_ms": bound_ms, "share_of_bound": bound_ms / med}
    print(name, res["runs"][name], flush=True)
for name, users, N in [("baseline_all_N10", all_users, 10), ("baseline_batch4096_N10",
                                                              torch.arange(4096, dtype=torch.int32, device=dev), 10)]:
    med, best = timed(baseline(users, N), 1 if quick or users.numel() == M else 5)
    res["runs"][name] = {"users": users.numel(), "N": N, "ms": med, "ms_min": best,
                         "pairs_per_s": users.numel() * NI / med * 1e3}
    print(name, res["runs"][name], flush=True)
res["speedup_all_N10_vs_baseline"] = res["runs"]["baseline_all_N10"]["ms"] / res["runs"]["all_N10"]["ms"]
print(json.dumps(res))
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
