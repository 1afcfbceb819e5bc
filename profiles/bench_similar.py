"""Timing of ALS.similar_items' device path - als_row_inv_norms + als_similar_topk - against the route available
without them: a normalising pass into a unit copy of the table, then als_recommend_topk on that copy with an identity
"seen" CSR (each row sees itself), zero biases and mu = 0.  n = 100 000 rows, k = 64, N = 10, nq in {1, 64, 4096}.

One process; the two routes alternate call by call, every call between two device events, after a warm-up of both;
median, minimum, maximum and quartiles of the repeated calls are reported.  The identity CSR of the yardstick is built
once outside the timed calls (it could be kept), its normalising pass is inside, as the inverse norms are for the new
route.  Usage: timeout 600 python profiles/bench_similar.py [--out profiles/similar_topk_ab.json]"""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "similar_topk_ab.json"))
ap.add_argument("--n", type=int, default=100_000)
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--topn", type=int, default=10)
ap.add_argument("--repeats", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_similar.py measures on the GPU: no device is visible"
dev = torch.device("cuda", 0)
be = HipBackend(dev)
n, k, N = args.n, args.k, args.topn
ld = layout.padded_k(k)
gen = torch.Generator(device=dev).manual_seed(1)
Z = torch.zeros(n, ld, dtype=torch.float32, device=dev)
Z[:, :k] = torch.randn(n, k, device=dev, generator=gen) * 0.3
zeros_n = torch.zeros(n, dtype=torch.float32, device=dev)
mu0 = torch.zeros(1, dtype=torch.float64, device=dev)
ident_ptr = torch.arange(n + 1, dtype=torch.int64, device=dev)
ident_idx = torch.arange(n, dtype=torch.int32, device=dev)
inv = torch.empty(n, dtype=torch.float32, device=dev)
result = dict(n=n, k=k, topn=N, repeats=args.repeats, warmup=args.warmup, device=torch.cuda.get_device_name(0),
              unit="ms per call", series=[])

for nq in (1, 64, 4096):
    q = torch.from_numpy(np.random.default_rng(nq).permutation(n)[:nq].astype(np.int32)).to(dev)
    out = {r: (torch.empty(nq, N, dtype=torch.float32, device=dev), torch.empty(nq, N, dtype=torch.int32, device=dev),
               torch.empty(nq, dtype=torch.int32, device=dev)) for r in ("similar", "unit_copy")}

    def similar():
        tv, ti, tc = out["similar"]
        be.row_inv_norms(k=k, ld=ld, T=Z, inv_norm=inv)
        be.similar_topk(k=k, ld=ld, q_ids=q, Q=Z, q_inv=inv, self_ids=q, n=n, T=Z, t_inv=inv, allow=None, topn=N,
                        top_val=tv, top_idx=ti, top_cnt=tc)

    def unit_copy():
        tv, ti, tc = out["unit_copy"]
        Zn = Z / torch.linalg.vector_norm(Z, dim=1, keepdim=True).clamp_min(1e-30)
        be.recommend_topk(k=k, ld=ld, users=q, n=n, U=Zn, Z=Zn, b_u=zeros_n, b_i=zeros_n, mu=mu0, seen_ptr=ident_ptr,
                          seen_idx=ident_idx, topn=N, top_val=tv, top_idx=ti, top_cnt=tc)

    routes = (("similar", similar), ("unit_copy", unit_copy))
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
    same_ids = float((out["similar"][1] == out["unit_copy"][1]).float().mean())
    dsim = float((out["similar"][0] - out["unit_copy"][0]).abs().max())
    row = dict(nq=nq, same_ids=same_ids, max_abs_sim_diff=dsim)
    for name, _ in routes:
        t = np.sort(np.asarray(times[name]))
        row[name] = dict(median=float(np.median(t)), min=float(t[0]), max=float(t[-1]),
                         q25=float(np.percentile(t, 25)), q75=float(np.percentile(t, 75)))
    result["series"].append(row)
    s, u = row["similar"], row["unit_copy"]
    print(f"nq={nq:5d}  inv_norms + similar_topk {s['median']:8.3f} ms [{s['min']:.3f} .. {s['max']:.3f}]   "
          f"unit copy + recommend_topk {u['median']:8.3f} ms [{u['min']:.3f} .. {u['max']:.3f}]   "
          f"ids equal {same_ids:.4f}  max |d sim| {dsim:.2e}", flush=True)

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
