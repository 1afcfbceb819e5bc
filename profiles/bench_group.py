"""Timing of ALS.recommend_group's device path - als_group_topk - against als_recommend_topk on the same member rows:
G groups of g members against G * g user rows.  The second call does the same scoring work (the same matrix
instructions on the same rows of U and Z) and keeps a list per MEMBER; it is what a caller without the group kernel
would start from before aggregating on the host, and it is unchanged by the group kernel.  No seen lists, no bitmap:
the two calls then differ in the aggregation and the selection state only.

n = 100 000 items, k = 64, N = 10; G in {1, 64, 4096}, g in {4, 16, 64}, aggregate in {mean, min, max}; the members of
a group are distinct users drawn from m = G * g (at least 4096) users.  One process; per (G, g) the four routes
(three aggregates and recommend) alternate call by call, every call between two device events, after a warm-up of
all four; median, minimum, maximum and quartiles of the repeated calls are reported, and the ratio of the medians
group / recommend.

Checked after the timed calls, on the first groups of the batch: the scores of the list equal, with ==, the N largest
aggregates of the member rows als_predict_dense writes (fp64 mean rounded to fp32, min, max).
Usage: timeout 1100 python profiles/bench_group.py [--out profiles/group_topk_ab.json]"""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "group_topk_ab.json"))
ap.add_argument("--n", type=int, default=100_000)
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--topn", type=int, default=10)
ap.add_argument("--groups", type=int, nargs="+", default=[1, 64, 4096])
ap.add_argument("--sizes", type=int, nargs="+", default=[4, 16, 64])
ap.add_argument("--repeats", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--check-groups", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_group.py measures on the GPU: no device is visible"
dev = torch.device("cuda", 0)
be = HipBackend(dev)
n, k, N = args.n, args.k, args.topn
ld = layout.padded_k(k)
AGGREGATES = ("mean", "min", "max")
gen = torch.Generator(device=dev).manual_seed(1)
Z = torch.zeros(n, ld, dtype=torch.float32, device=dev)
Z[:, :k] = torch.randn(n, k, device=dev, generator=gen) * 0.25
b_i = torch.randn(n, device=dev, generator=gen) * 0.3
mu = torch.tensor([3.5], dtype=torch.float64, device=dev)

result = dict(n=n, k=k, topn=N, repeats=args.repeats, warmup=args.warmup, device=torch.cuda.get_device_name(0),
              unit="ms per call", series=[])

for G in args.groups:
    for g in args.sizes:
        m = max(G * g, 4096)
        U = torch.zeros(m, ld, dtype=torch.float32, device=dev)
        U[:, :k] = torch.randn(m, k, device=dev, generator=gen) * 0.25
        b_u = torch.randn(m, device=dev, generator=gen) * 0.3
        rng = np.random.default_rng(G * 100 + g)
        members = np.stack([rng.choice(m, size=g, replace=False) for _ in range(G)]).astype(np.int32)
        g_ptr = torch.arange(0, (G + 1) * g, g, dtype=torch.int64, device=dev)
        g_users = torch.from_numpy(members.reshape(-1)).to(dev)
        rows = G * g
        out = {a: (torch.empty(G, N, dtype=torch.float32, device=dev), torch.empty(G, N, dtype=torch.int32, device=dev),
                   torch.empty(G, dtype=torch.int32, device=dev)) for a in AGGREGATES}
        out["recommend"] = (torch.empty(rows, N, dtype=torch.float32, device=dev),
                            torch.empty(rows, N, dtype=torch.int32, device=dev),
                            torch.empty(rows, dtype=torch.int32, device=dev))

        def group(aggregate):
            tv, ti, tc = out[aggregate]
            be.group_topk(k=k, ld=ld, g_ptr=g_ptr, g_users=g_users, max_members=g, n=n, U=U, Z=Z, b_u=b_u, b_i=b_i,
                          mu=mu, seen_ptr=None, seen_idx=None, allow=None, aggregate=aggregate, topn=N, top_val=tv,
                          top_idx=ti, top_cnt=tc)

        def recommend():
            tv, ti, tc = out["recommend"]
            be.recommend_topk(k=k, ld=ld, users=g_users, n=n, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, seen_ptr=None,
                              seen_idx=None, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)

        routes = [(a, (lambda a=a: group(a))) for a in AGGREGATES] + [("recommend", recommend)]
        for _ in range(args.warmup):
            for _, fn in routes:
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in routes}
        for _ in range(args.repeats):
            for name, fn in routes:                      # alternating: every route meets the same machine state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        # the lists against the member rows als_predict_dense writes
        for b in range(min(G, args.check_groups)):
            us = g_users[b * g: (b + 1) * g].long()
            dense = torch.empty(g, n, dtype=torch.float32, device=dev)
            be.predict_dense(k=k, ld=ld, m=g, n=n, U=U.index_select(0, us).contiguous(), Z=Z,
                             b_u=b_u.index_select(0, us).contiguous(), b_i=b_i, mu=mu, out=dense)
            agg = {"min": dense.min(dim=0).values, "max": dense.max(dim=0).values,
                   "mean": (dense.double().sum(dim=0) / g).float()}
            for a in AGGREGATES:
                tv, ti, tc = out[a]
                assert int(tc[b]) == N
                assert bool((tv[b] == torch.topk(agg[a], N).values).all()), (G, g, a, b)
                assert bool((tv[b] == agg[a][ti[b].long()]).all()), (G, g, a, b)
        assert bool((out["recommend"][2] == N).all())
        row = dict(groups=G, members=g, user_rows=rows)
        for name, _ in routes:
            t = np.sort(np.asarray(times[name]))
            row[name] = dict(median=float(np.median(t)), min=float(t[0]), max=float(t[-1]),
                             q25=float(np.percentile(t, 25)), q75=float(np.percentile(t, 75)))
        for a in AGGREGATES:
            row[a]["ratio_to_recommend"] = row[a]["median"] / row["recommend"]["median"]
        result["series"].append(row)
        print(f"G {G:5d} g {g:3d}  " + "  ".join(f"{a} {row[a]['median']:9.3f} ms [{row[a]['min']:.3f} .. "
                                                  f"{row[a]['max']:.3f}] x{row[a]['ratio_to_recommend']:.2f}"
                                                  for a in AGGREGATES)
              + f"  recommend on {rows} rows {row['recommend']['median']:9.3f} ms "
                f"[{row['recommend']['min']:.3f} .. {row['recommend']['max']:.3f}]", flush=True)
        del U, b_u, out

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
