#!/usr/bin/env python3
"""Diversified top-N (csrc/diversify.hip, als_mmr_rerank) at the configs[3] shape: 1M users x 100K items, k = 64,
~100 seen items per user, seeded random factors (no fit needed).  For 1 / 64 / 4096 / all users and pool = 40 / 128
(N = 10) it times, device side (events, warm-up first, median and minimum of the repetitions):
  pool     als_recommend_topk with N = pool - the unchanged code of ALS.recommend, the baseline
  rerank   als_mmr_rerank alone on that pool
  diverse  the two back to back on one stream, what ALS.recommend_diverse launches per chunk
and the ratio rerank / pool.  All users run in chunks of 65536 rows (serving.REC_BATCH), so the pool of a chunk is
what the re-rank reads.  Writes one JSON object to argv[1] (default: stdout only).

    python profiles/diversify_time.py profiles/diversify_time.json"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import layout  # noqa: E402
from collaborative_filtering_amd.backend import HipBackend  # noqa: E402

M, NI, K, N, CHUNK = 1_000_000, 100_000, 64, 10, 1 << 16
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


def stages(users, pool):
    """(pool call, re-rank, both) over `users` in CHUNK-row chunks; the buffers of one chunk are reused."""
    nb = min(users.numel(), CHUNK)
    pv = torch.empty(nb, pool, dtype=torch.float32, device=dev)
    pi = torch.empty(nb, pool, dtype=torch.int32, device=dev)
    pc = torch.empty(nb, dtype=torch.int32, device=dev)
    tv = torch.empty(nb, N, dtype=torch.float32, device=dev)
    ti = torch.empty(nb, N, dtype=torch.int32, device=dev)
    tc = torch.empty(nb, dtype=torch.int32, device=dev)

    def pool_call(us):
        be.recommend_topk(k=K, ld=ld, users=us, n=NI, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, seen_ptr=seen_ptr,
                          seen_idx=seen_idx, topn=pool, top_val=pv[: us.numel()], top_idx=pi[: us.numel()],
                          top_cnt=pc[: us.numel()])

    def rerank(us):
        be.mmr_rerank(k=K, ld=ld, n=NI, Z=Z, cand_val=pv[: us.numel()], cand_idx=pi[: us.numel()], lam=0.3, topn=N,
                      top_val=tv[: us.numel()], top_idx=ti[: us.numel()], top_cnt=tc[: us.numel()])

    def over(*fns):
        def run():
            for c0 in range(0, users.numel(), CHUNK):
                for fn in fns:
                    fn(users[c0: c0 + CHUNK])
        return run
    return over(pool_call), over(rerank), over(pool_call, rerank)


res = {"shape": {"users": M, "items": NI, "k": K, "N": N, "seen_per_user": float(seen_idx.numel() / M), "lambda": 0.3},
       "note": "ms: median of the repetitions, ms_min: their minimum; rerank times the last chunk's pool again for "
               "every chunk (same work per row)", "runs": {}}
rng = np.random.default_rng(0)
batches = [(B, torch.from_numpy(rng.choice(M, B, replace=False).astype(np.int32)).to(dev)) for B in (1, 64, 4096)]
batches.append((M, torch.arange(M, dtype=torch.int32, device=dev)))
for B, users in batches:
    for pool in (40, 128):
        reps = 1 if quick else (3 if B == M else 20)
        fns = stages(users, pool)
        fns[0]()                                                     # the pool the re-rank reads
        run = {"users": B, "pool": pool}
        for name, fn in zip(("pool", "rerank", "diverse"), fns):
            run[f"{name}_ms"], run[f"{name}_ms_min"] = timed(fn, reps)
        run["rerank_over_pool"] = run["rerank_ms"] / run["pool_ms"]
        run["rerank_us_per_user"] = run["rerank_ms"] * 1e3 / B
        res["runs"][f"users{B}_pool{pool}"] = run
        print(f"users{B}_pool{pool}", run, flush=True)
print(json.dumps(res))
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
