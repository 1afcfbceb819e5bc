#!/usr/bin/env python3
"""Deep top-N (csrc/recommend_deep.hip, als_recommend_deep) at the configs[3] shape of profiles/recommend_time.py: 1M
users x 100K items, k = 64, ~100 seen items per user, seeded random factors.  For N = 129 / 256 / 500 / 1000 and batches
of 1 / 64 / 4096 / 65 536 users it times the deep call (in the chunks serving._Serving issues it in: the batch halved
until the workspace is within DEEP_WS_BYTES) against the same run's als_recommend_topk at N = 128 - the same walk, so
the floor - and against the composed baseline (chunked predict_dense + -inf scatter + torch.topk).  It records the scoring rounds of every chunk and the
automatic slice count, on two catalogues - i.i.d. biases, and a popularity-sorted one (b_i descending in the item id) -
and repeats the deep call with the slice count that a slice factor of 2 instead of ALS_DEEP_SLICE_FACTOR = 4 would
choose.  Writes one JSON object to argv[1] (default: stdout only).

    python profiles/bench_recommend_deep.py profiles/recommend_deep_time.json"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import _hip, layout  # noqa: E402
from collaborative_filtering_amd.backend import HipBackend  # noqa: E402

M, NI, K = 1_000_000, 100_000, 64
WS_BYTES = 512 << 20            # serving._Serving.DEEP_WS_BYTES
quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]

dev = torch.device("cuda", 0)
be = HipBackend(dev)
lib = _hip.load()
gen = torch.Generator(device=dev).manual_seed(3)
ld = layout.padded_k(K)
U = torch.zeros(M, ld, device=dev)
U[:, :K] = torch.randn(M, K, device=dev, generator=gen) * 0.3
Z = torch.zeros(NI, ld, device=dev)
Z[:, :K] = torch.randn(NI, K, device=dev, generator=gen) * 0.3
b_u = torch.randn(M, device=dev, generator=gen) * 0.1
b_iid = torch.randn(NI, device=dev, generator=gen) * 0.1
# popularity-sorted: the biases descending in the id, with a spread (sd 1) above that of the dot products (sd 0.72)
b_pop = (torch.randn(NI, device=dev, generator=gen)).sort(descending=True).values.contiguous()
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


def outputs(B, N):
    return (torch.empty(B, N, dtype=torch.float32, device=dev), torch.empty(B, N, dtype=torch.int32, device=dev),
            torch.empty(B, dtype=torch.int32, device=dev))


def recommend(users, N, b_i):
    tv, ti, tc = outputs(users.numel(), N)
    return lambda: be.recommend_topk(k=K, ld=ld, users=users, n=NI, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu,
                                     seen_ptr=seen_ptr, seen_idx=seen_idx, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)


def deep(users, N, b_i, rounds, CHUNK):
    """The deep call in chunks of CHUNK users; rounds: int32 [chunks] device tensor, one word per chunk."""
    B = users.numel()
    tv, ti, tc = outputs(B, N)

    def run():
        for j, c0 in enumerate(range(0, B, CHUNK)):
            be.recommend_deep(k=K, ld=ld, users=users[c0: c0 + CHUNK], n=NI, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu,
                              seen_ptr=seen_ptr, seen_idx=seen_idx, allow=None, after_key=None, topn=N,
                              top_val=tv[c0:], top_idx=ti[c0:], top_cnt=tc[c0:], rounds=rounds[j: j + 1])
    return run


def chunk_rows(B, N):
    """serving._Serving._deep_chunks' rule under the slice count in force."""
    step = B
    while step > 1 and be.recommend_deep_workspace_bytes(step, NI, N) > WS_BYTES:
        step = (step + 1) // 2
    return step


def baseline(users, N, b_i, chunk=8192):
    """What a caller composes today: predict_dense on a chunk of users, -inf at their seen items, torch.topk."""
    out = torch.empty(min(chunk, users.numel()), NI, dtype=torch.float32, device=dev)

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


def slices_of(B, N, forced=0):
    """The slice count of a deep call from its documented workspace size 8 B (128 S + NL + S) + 64."""
    nl = 128
    while nl < N:
        nl *= 2
    return ((lib.als_recommend_deep_workspace_bytes(B, NI, N, forced) - 64) // (8 * B) - nl) // 129


def factor2_slices(B, N):
    """What the automatic plan would choose with a slice factor of 2: als_recommend_topk's count, at least 2 per round."""
    auto = (lib.als_recommend_workspace_bytes(B, NI, 128, 0) // (8 * B * 128)) or 1
    return int(min(max(auto, 2 * ((N + 127) // 128)), 64))


res = {"shape": {"users": M, "items": NI, "k": K, "seen_per_user": float(seen_idx.numel() / M)},
       "workspace_bound_bytes": WS_BYTES,
       "runs": {}}
for cat, b_i in (("iid", b_iid), ("popularity_sorted", b_pop)):
    for B in (1, 64, 4096, 65536):
        users = torch.arange(B, dtype=torch.int32, device=dev) + 1000         # contiguous ids (the baseline wants them)
        reps = 1 if quick else (3 if B == 65536 else 10)
        floor, _ = timed(recommend(users, 128, b_i), reps)
        entry = {"recommend_N128_ms": floor, "deep": {}}
        for N in (129, 256, 500, 1000):
            os.environ.pop("ALS_RECOMMEND_SLICES", None)
            nb = chunk_rows(B, N)
            rounds = torch.zeros((B + nb - 1) // nb, dtype=torch.int32, device=dev)
            med, best = timed(deep(users, N, b_i, rounds, nb), reps)
            r4 = rounds.cpu().tolist()
            s2 = factor2_slices(nb, N)          # at the same chunk, so that only the slice count differs
            os.environ["ALS_RECOMMEND_SLICES"] = str(s2)
            med2, _ = timed(deep(users, N, b_i, rounds, nb), reps)
            r2 = rounds.cpu().tolist()
            os.environ.pop("ALS_RECOMMEND_SLICES", None)
            entry["deep"][str(N)] = {"ms": med, "ms_min": best, "ratio_to_recommend_N128": med / floor,
                                     "chunk_rows": nb, "slices": int(slices_of(nb, N)),
                                     "rounds_per_chunk": sorted(set(r4)),
                                     "rounds_max": max(r4), "factor2": {"slices": s2, "ms": med2,
                                                                        "rounds_max": max(r2)}}
        if cat == "iid" and B in (4096, 65536):
            for N in (500, 1000):
                entry[f"baseline_N{N}_ms"] = timed(baseline(users, N, b_i), 1 if quick else 2)[0]
        res["runs"][f"{cat}_batch{B}"] = entry
        print(cat, B, json.dumps(entry), flush=True)
print(json.dumps(res))
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
