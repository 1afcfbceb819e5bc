"""Timing of ALS.recommend_users' device path - als_audience_topk - against the route available without it:
als_recommend_topk called with the two sides swapped (U := item table, Z := user table, b_u := b_i, b_i := b_u, the
seen CSR := the rater CSR by item).  That call does the same walk and the same exclusion; it only adds the two biases
in the other order, so its scores are not bitwise predict()'s.

m = 1 000 000 users, k = 64, N = 10; 8192 items with synthetic rater lists of 100 users on average and one hub item
(item 0) with 100 000 raters.  Series: one ordinary item, the hub item alone, 64 and 4096 items with the hub item among
them.  One process; the two routes alternate call by call, every call between two device events, after a warm-up of
both; median, minimum, maximum and quartiles of the repeated calls are reported.

Checked after the timed calls: wherever the two lists hold the same user at a position the two scores are within four
fp32 roundings of each other (the associations share fl(d + mu) and round twice each: 2^-22 (|score| + max |bias|)),
and wherever they hold different users - the two bias associations can swap two users whose scores are that close, at
the list's end also against the first user outside - the scores at that position are within twice that.  Usage: timeout 900 python profiles/bench_audience.py [--out profiles/audience_topk_ab.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import layout                      # noqa: E402
from collaborative_filtering_amd.backend import HipBackend         # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "audience_topk_ab.json"))
ap.add_argument("--m", type=int, default=1_000_000)
ap.add_argument("--items", type=int, default=8192)
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--topn", type=int, default=10)
ap.add_argument("--hub", type=int, default=100_000)
ap.add_argument("--repeats", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_audience.py measures on the GPU: no device is visible"
dev = torch.device("cuda", 0)
be = HipBackend(dev)
m, n, k, N = args.m, args.items, args.k, args.topn
ld = layout.padded_k(k)
gen = torch.Generator(device=dev).manual_seed(1)
U = torch.zeros(m, ld, dtype=torch.float32, device=dev)
U[:, :k] = torch.randn(m, k, device=dev, generator=gen) * 0.3
Q = torch.zeros(n, ld, dtype=torch.float32, device=dev)
Q[:, :k] = torch.randn(n, k, device=dev, generator=gen) * 0.3
b_u = torch.randn(m, device=dev, generator=gen) * 0.3
b_i = torch.randn(n, device=dev, generator=gen) * 0.3
mu = torch.tensor([3.5], dtype=torch.float64, device=dev)
bias_max = float(max(b_u.abs().max(), b_i.abs().max()))

rng = np.random.default_rng(2)
lists = [np.unique(rng.integers(0, m, size=c)) for c in rng.poisson(100, size=n)]
lists[0] = np.sort(rng.choice(m, size=min(args.hub, m), replace=False))               # the hub item
ptr_h = np.zeros(n + 1, np.int64)
ptr_h[1:] = np.cumsum([s.size for s in lists])
seen_ptr = torch.from_numpy(ptr_h).to(dev)
seen_idx = torch.from_numpy(np.concatenate(lists).astype(np.int32)).to(dev)
del lists

result = dict(m=m, items=n, k=k, topn=N, hub_raters=int(ptr_h[1]), mean_raters=float(ptr_h[-1] - ptr_h[1]) / (n - 1),
              repeats=args.repeats, warmup=args.warmup, device=torch.cuda.get_device_name(0), unit="ms per call",
              series=[])


def queries(nq, hub):
    q = 1 + np.random.default_rng(nq).permutation(n - 1)[:nq]           # ordinary items
    if hub:
        q[0] = 0
    return q.astype(np.int32)


for label, nq, hub in (("one ordinary item", 1, False), ("the hub item", 1, True), ("64 items, hub among them", 64, True),
                       ("4096 items, hub among them", 4096, True)):
    q = torch.from_numpy(queries(nq, hub)).to(dev)
    out = {r: (torch.empty(nq, N, dtype=torch.float32, device=dev), torch.empty(nq, N, dtype=torch.int32, device=dev),
               torch.empty(nq, dtype=torch.int32, device=dev)) for r in ("audience", "swapped")}

    def audience():
        tv, ti, tc = out["audience"]
        be.audience_topk(k=k, ld=ld, q_ids=q, Q=Q, q_bias=b_i, m=m, U=U, b_u=b_u, mu=mu, seen_ptr=seen_ptr,
                         seen_idx=seen_idx, allow=None, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)

    def swapped():
        tv, ti, tc = out["swapped"]
        be.recommend_topk(k=k, ld=ld, users=q, n=m, U=Q, Z=U, b_u=b_i, b_i=b_u, mu=mu, seen_ptr=seen_ptr,
                          seen_idx=seen_idx, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)

    routes = (("audience", audience), ("swapped", swapped))
    for _ in range(args.warmup):
        for _, fn in routes:
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in routes}
    for _ in range(args.repeats):
        for name, fn in routes:                          # alternating: both routes meet the same machine state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    (va, ia, ca), (vs, is_, cs) = out["audience"], out["swapped"]
    assert bool((ca == N).all()) and bool((cs == N).all())
    same = ia == is_
    # the two associations share fl(d + mu) and then round twice each, every rounding at most 2^-24 (|score| + bias)
    err = ((va - vs).abs() / (va.abs() + bias_max)).double()
    assert float(err[same].max()) <= 2.0 ** -22, "same user, scores further apart than four roundings"
    if not bool(same.all()):
        assert float(err[~same].max()) <= 2.0 ** -21, "different users at a position whose scores are not a near-tie"
    hub_rows = (q == 0).nonzero().flatten()
    for b in hub_rows.tolist():                          # no rater of the hub item comes back
        assert not bool(torch.isin(ia[b], seen_idx[: int(ptr_h[1])]).any())
    row = dict(series=label, nq=nq, hub=hub, same_ids=float(same.float().mean()),
               bitwise_equal_scores=float((va == vs).float().mean()))
    for name, _ in routes:
        t = np.sort(np.asarray(times[name]))
        row[name] = dict(median=float(np.median(t)), min=float(t[0]), max=float(t[-1]),
                         q25=float(np.percentile(t, 25)), q75=float(np.percentile(t, 75)))
    result["series"].append(row)
    a, s = row["audience"], row["swapped"]
    print(f"{label:28s} audience_topk {a['median']:8.3f} ms [{a['min']:.3f} .. {a['max']:.3f}]   "
          f"swapped recommend_topk {s['median']:8.3f} ms [{s['min']:.3f} .. {s['max']:.3f}]   "
          f"ids equal {row['same_ids']:.4f}  scores bitwise equal {row['bitwise_equal_scores']:.4f}", flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
