#!/usr/bin/env python3
"""Calibrated top-N (csrc/calibrate.hip) at the configs[3] shape: 1M users x 100K items, k = 64, ~100 seen items per
user, seeded random factors (no fit needed), 19 categories (every item 1 .. 3 of them drawn from a 1 / rank
distribution, 5 % of the items none).  For 64 / 4096 users and pool = 40 / 128 (N = 10, calibration 0.5, smoothing
0.01) it times, device side (events, one warm-up call first, median and minimum of 20 repetitions):
  pool      als_recommend_topk with N = pool - the unchanged code of ALS.recommend, the baseline
  profile   als_category_profile over the users' seen rows
  rerank    als_calibrated_rerank alone on that pool and those profiles
and the ratio rerank / pool.  Writes one JSON object to argv[1] (default: stdout only).

    python profiles/calibrate_time.py profiles/calibrate_time.json"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import layout, validate  # noqa: E402
from collaborative_filtering_amd.backend import HipBackend  # noqa: E402

M, NI, K, N, NCAT, REPS = 1_000_000, 100_000, 64, 10, 19, 20
LAM, ALPHA = 0.5, 0.01
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
w = 1.0 / np.arange(1, NCAT + 1)
G = np.zeros((NI, NCAT))
draws = rng.choice(NCAT, size=(NI, 3), p=w / w.sum())
take = np.arange(3)[None, :] < rng.integers(1, 4, size=NI)[:, None]
G[np.repeat(np.arange(NI), 3)[take.ravel()], draws.ravel()[take.ravel()]] = 1.0
G[rng.random(NI) < 0.05] = 0.0
Cd = torch.from_numpy(validate.category_table(G, NI)).to(dev)


def timed(fn):
    fn()                                              # warm-up (and first-call costs)
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


res = {"shape": {"users": M, "items": NI, "k": K, "N": N, "ncat": NCAT, "seen_per_user": float(seen_idx.numel() / M),
                 "calibration": LAM, "smoothing": ALPHA},
       "note": "ms: median of 20 repetitions after one warm-up call, ms_min: their minimum", "runs": {}}
for B in (64, 4096):
    users = torch.from_numpy(rng.choice(M, B, replace=False).astype(np.int32)).to(dev)
    for pool in (40, 128):
        pv = torch.empty(B, pool, dtype=torch.float32, device=dev)
        pi = torch.empty(B, pool, dtype=torch.int32, device=dev)
        pc = torch.empty(B, dtype=torch.int32, device=dev)
        P = torch.empty(B, Cd.shape[1], dtype=torch.float32, device=dev)
        tv = torch.empty(B, N, dtype=torch.float32, device=dev)
        ti = torch.empty(B, N, dtype=torch.int32, device=dev)
        tc = torch.empty(B, dtype=torch.int32, device=dev)
        kl = torch.empty(B, dtype=torch.float32, device=dev)

        def pool_call():
            be.recommend_topk(k=K, ld=ld, users=users, n=NI, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, seen_ptr=seen_ptr,
                              seen_idx=seen_idx, topn=pool, top_val=pv, top_idx=pi, top_cnt=pc)

        def profile():
            be.category_profile(ncat=NCAT, indptr=seen_ptr, indices=seen_idx, rows=users, n=NI, C=Cd, P_out=P)

        def rerank():
            be.calibrated_rerank(ncat=NCAT, n=NI, C=Cd, P=P, cand_val=pv, cand_idx=pi, lam=LAM, alpha=ALPHA, topn=N,
                                 top_val=tv, top_idx=ti, top_cnt=tc, top_kl=kl)
        run = {"users": B, "pool": pool}
        for name, fn in (("pool", pool_call), ("profile", profile), ("rerank", rerank)):      # in dependency order
            run[f"{name}_ms"], run[f"{name}_ms_min"] = timed(fn)
        run["rerank_over_pool"] = run["rerank_ms"] / run["pool_ms"]
        run["rerank_us_per_user"] = run["rerank_ms"] * 1e3 / B
        run["mean_kl"] = float(kl.mean())
        res["runs"][f"users{B}_pool{pool}"] = run
        print(f"users{B}_pool{pool}", run, flush=True)
print(json.dumps(res))
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
