"""Timing of ALS.recommend_explore's device path - als_row_whitener + als_explore_topk - against what a caller could
compose at the parent commit: batched torch.linalg.cholesky of the rows' ridge systems, solve_triangular for L^-1, the
batched GEMM L^-1 Z^T (a B x k x n matrix), its column norms, the score GEMM, key = score + beta * sigma and
torch.topk.

n = 100 000 items, k in {64, 128}, 100 ratings per row, N = 10, beta = 1; 1, 64, 4096 and 65 536 users.  One process;
per (k, users) the routes alternate call by call, every call between two device events, after a warm-up of all of
them (measuring-on-mi355x: interleaved, medians and spread, not a single number):

  explore    als_explore_topk on whiteners already formed (the seen rows excluded)
  whitener   als_row_whitener alone
  recommend  als_recommend_topk on the same users - the catalogue walk without the uncertainty term
  baseline   the torch composition, on min(users, what a 4 GiB B x k x n intermediate allows) users

Reported per (k, users): median / min / max / quartiles in ms, the fp32 matrix-core bound
2 B n k^2 (KB + 1) / (2 KB) / 157e12 s of the leverage work (KB = k / 16: only the lower blocks of W are multiplied;
the base-score chain is not counted), the share of it the explore call reaches, and the ratio of the per-user times
(whitener + explore) / baseline.

Checked after the timed calls, on the first users: top_val == base + beta * sqrt(top_lev) in float32 with base the row
als_predict_dense writes, and the keys agree with the baseline's to 1e-3.
Usage: timeout 1100 python profiles/bench_explore.py [--ks 64 128] [--out profiles/explore_topk_ab.json]"""
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
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "explore_topk_ab.json"))
ap.add_argument("--n", type=int, default=100_000)
ap.add_argument("--ks", type=int, nargs="+", default=[64, 128])
ap.add_argument("--topn", type=int, default=10)
ap.add_argument("--beta", type=float, default=1.0)
ap.add_argument("--ratings", type=int, default=100)
ap.add_argument("--users", type=int, nargs="+", default=[1, 64, 4096, 65536])
ap.add_argument("--repeats", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--baseline-bytes", type=int, default=4 << 30)
ap.add_argument("--check-users", type=int, default=3)
args = ap.parse_args()

assert torch.cuda.is_available(), "bench_explore.py measures on the GPU: no device is visible"
dev = torch.device("cuda", 0)
be = HipBackend(dev)
n, N, beta, R = args.n, args.topn, args.beta, args.ratings
LAM = 5.0
PEAK_F32 = 157e12
gen = torch.Generator(device=dev).manual_seed(1)
mu = torch.tensor([3.5], dtype=torch.float64, device=dev)

result = dict(n=n, topn=N, beta=beta, ratings_per_row=R, lambda_u=LAM, warmup=args.warmup,
              device=torch.cuda.get_device_name(0), unit="ms per call", series=[])


def stats(ts):
    t = np.sort(np.asarray(ts))
    return dict(median=float(np.median(t)), min=float(t[0]), max=float(t[-1]), q25=float(np.percentile(t, 25)),
                q75=float(np.percentile(t, 75)), calls=int(t.size))


for k in args.ks:
    ld = layout.padded_k(k)
    KB = ld // 16
    Z = torch.zeros(n, ld, dtype=torch.float32, device=dev)
    Z[:, :k] = torch.randn(n, k, device=dev, generator=gen) * 0.25
    b_i = torch.randn(n, device=dev, generator=gen) * 0.3
    for B in args.users:
        U = torch.zeros(B, ld, dtype=torch.float32, device=dev)
        U[:, :k] = torch.randn(B, k, device=dev, generator=gen) * 0.25
        b_u = torch.randn(B, device=dev, generator=gen) * 0.3
        rng = np.random.default_rng(1000 * k + B)
        idx_h = np.cumsum(rng.integers(1, n // R, size=(B, R)), axis=1).astype(np.int32)    # ascending, distinct, < n
        indptr = torch.arange(0, (B + 1) * R, R, dtype=torch.int64, device=dev)
        indices = torch.from_numpy(idx_h.reshape(-1)).to(dev)
        users = torch.arange(B, dtype=torch.int32, device=dev)
        W = torch.empty(B, ld, ld, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        tv, tl = (torch.empty(B, N, dtype=torch.float32, device=dev) for _ in range(2))
        ti = torch.empty(B, N, dtype=torch.int32, device=dev)
        tc = torch.empty(B, dtype=torch.int32, device=dev)
        rv = torch.empty(B, N, dtype=torch.float32, device=dev)
        ri = torch.empty(B, N, dtype=torch.int32, device=dev)
        rc = torch.empty(B, dtype=torch.int32, device=dev)
        Bb = max(1, min(B, args.baseline_bytes // (4 * k * n)))
        base_out = {}

        def whitener():
            be.row_whitener(k=k, ld=ld, indptr=indptr, indices=indices, rows=None, n=n, Z=Z, lam_u=LAM, W_out=W,
                            status=status)

        def explore():
            be.explore_topk(k=k, ld=ld, users=users, n=n, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, W=W, beta=beta,
                            seen_ptr=indptr, seen_idx=indices, allow=None, topn=N, top_val=tv, top_idx=ti, top_cnt=tc,
                            top_lev=tl)

        def recommend():
            be.recommend_topk(k=k, ld=ld, users=users, n=n, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, seen_ptr=indptr,
                              seen_idx=indices, topn=N, top_val=rv, top_idx=ri, top_cnt=rc)

        def baseline():
            S = indices[: Bb * R].view(Bb, R).long()
            Zs = Z[:, :k][S]                                                        # [Bb, R, k]
            A = torch.bmm(Zs.transpose(1, 2), Zs) + (LAM + 1e-10) * torch.eye(k, device=dev)
            L = torch.linalg.cholesky(A)
            # L^-1 by solve_triangular on the identity, then one batched GEMM against Z^T: the triangular solve
            # against Z^T itself (k x n right-hand sides per user) fails in hipBLAS' batched TRSM with
            # HIPBLAS_STATUS_ALLOC_FAILED from 64 users on, and the GEMM is the faster composition anyway
            Linv = torch.linalg.solve_triangular(L, torch.eye(k, device=dev).expand(Bb, k, k), upper=False)
            Y = torch.matmul(Linv, Z[:, :k].T)
            sig = (Y * Y).sum(dim=1).sqrt_()
            key = U[:Bb, :k] @ Z[:, :k].T + (float(mu) + b_u[:Bb, None] + b_i[None, :]) + beta * sig
            key.scatter_(1, S, float("-inf"))
            base_out["topk"] = torch.topk(key, N, dim=1)

        routes = [("explore", explore), ("whitener", whitener), ("recommend", recommend), ("baseline", baseline)]
        repeats = args.repeats if B <= 4096 else max(3, args.repeats // 5)
        whitener()
        for _ in range(args.warmup if B <= 4096 else 1):
            for _, fn in routes:
                fn()
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        times = {name: [] for name, _ in routes}
        for _ in range(repeats):
            for name, fn in routes:                      # alternating: every route meets the same machine state
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                times[name].append(e0.elapsed_time(e1))
        # the lists against als_predict_dense and against the composition
        nc = min(B, Bb, args.check_users)
        dense = torch.empty(nc, n, dtype=torch.float32, device=dev)
        be.predict_dense(k=k, ld=ld, m=nc, n=n, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, out=dense)
        for b in range(nc):
            assert int(tc[b]) == N
            base = dense[b][ti[b].long()].cpu().numpy()
            lev = tl[b].cpu().numpy()
            key = (base + (np.float32(beta) * np.sqrt(lev)).astype(np.float32)).astype(np.float32)
            assert (tv[b].cpu().numpy() == key).all(), (k, B, b)
            assert bool((tv[b] - base_out["topk"].values[b]).abs().max() < 1e-3), (k, B, b)
        bound_ms = 2.0 * B * n * ld * ld * (KB + 1) / (2 * KB) / PEAK_F32 * 1e3
        row = dict(k=k, users=B, baseline_users=Bb, bound_ms=bound_ms)
        for name, _ in routes:
            row[name] = stats(times[name])
        row["share_of_bound"] = bound_ms / row["explore"]["median"]
        row["explore_over_recommend"] = row["explore"]["median"] / row["recommend"]["median"]
        per_user = (row["explore"]["median"] + row["whitener"]["median"]) / B
        row["baseline"]["ms_per_user"] = row["baseline"]["median"] / Bb
        row["per_user_ratio_to_baseline"] = per_user / row["baseline"]["ms_per_user"]
        result["series"].append(row)
        print(f"k {k:3d} users {B:6d}  explore {row['explore']['median']:10.3f} ms [{row['explore']['min']:.3f} .. "
              f"{row['explore']['max']:.3f}]  whitener {row['whitener']['median']:9.3f}  recommend "
              f"{row['recommend']['median']:9.3f}  baseline({Bb}) {row['baseline']['median']:9.3f}  bound "
              f"{bound_ms:9.3f} ms = {100 * row['share_of_bound']:.1f} %  per-user vs baseline x"
              f"{row['per_user_ratio_to_baseline']:.3f}", flush=True)
        del U, b_u, W, tv, tl, ti, tc, rv, ri, rc, indices, base_out
        torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print("wrote", args.out)
