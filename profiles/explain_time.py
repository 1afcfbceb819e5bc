#!/usr/bin/env python3
"""Explanations (csrc/explain.hip, als_explain) at the inputs of profiles/fold_in_time.py: Z for 100K items at
k = 64 plus biases, seeded random (no fit needed), B in {1, 64, 4096, 65536} rows of ~100 ratings from the synth
distribution, 1 and 10 targets per row, M = 10.  Compared within the same process, alternating, event-timed:
  (a) als_fold_in on the same rows - the factorisation the two kernels share;
  (b) (B <= 4096) what a caller could write without the kernel: the same quantities in torch fp64 on the device -
      padded gather of Z_S, batched Gram, torch.linalg.cholesky, cholesky_solve for p, q and the targets' w, the
      weights / contributions and torch.topk.  The padded index and mask are built outside the timed region.
Every round times each candidate once per repetition, alternating; the JSON holds per candidate the median over
all repetitions and the smallest / largest per-round median (the spread).

    python profiles/explain_time.py profiles/explain_time.json
    rocprofv3 --kernel-trace --stats -d DIR -o explain -- python profiles/explain_time.py --quick   # kernel table"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import layout  # noqa: E402
from collaborative_filtering_amd.backend import HipBackend  # noqa: E402
from tests.synth import make_ratings  # noqa: E402

NI, K, LAM_U, LAM_BU, TOPM = 100_000, 64, 5.0, 3.0, 10
quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]

dev = torch.device("cuda", 0)
be = HipBackend(dev)
gen = torch.Generator(device=dev).manual_seed(3)
ld = layout.padded_k(K)
Z = torch.zeros(NI + 1, ld, device=dev)
Z[:NI, :K] = torch.randn(NI, K, device=dev, generator=gen) * 0.3
b_i = torch.randn(NI, device=dev, generator=gen) * 0.1
mu = torch.tensor([3.6], dtype=torch.float64, device=dev)


def rows(B, seed):
    """B users x ~100 ratings: synth power-law items, duplicates merged, CSR sorted by column."""
    r, c, v = make_ratings(B, NI, 100 * B, seed=seed, user_exp=0.0)
    ptr = np.zeros(B + 1, np.int64)
    np.add.at(ptr, r + 1, 1)
    return np.cumsum(ptr), c.astype(np.int32), v.astype(np.float32)


def alternate(cands, rounds, reps):
    """cands: {name: fn}.  Per round `reps` passes over the candidates in turn; returns per name the median over
    all timings and the (min, max) of the per-round medians, in ms."""
    for fn in cands.values():
        fn()
    torch.cuda.synchronize()
    per_round = {name: [] for name in cands}
    every = {name: [] for name in cands}
    for _ in range(rounds):
        ts = {name: [] for name in cands}
        for _ in range(reps):
            for name, fn in cands.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                b.synchronize()
                ts[name].append(a.elapsed_time(b))
        for name in cands:
            per_round[name].append(float(np.median(ts[name])))
            every[name] += ts[name]
    return {name: {"median_ms": float(np.median(every[name])), "round_median_min_ms": min(per_round[name]),
                   "round_median_max_ms": max(per_round[name])} for name in cands}


res = {"shape": {"items": NI, "k": K, "lambda_u": LAM_U, "lambda_bu": LAM_BU, "M": TOPM}, "runs": {}}
for B in (1, 64, 4096, 65536):
    ptr, idx, val = rows(B, seed=B)
    d = lambda a: torch.from_numpy(a).to(dev)
    ptr_d, idx_d, val_d = d(ptr), d(idx), d(val)
    U = torch.empty(B, ld, device=dev)
    bu32 = torch.zeros(B, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def fold():
        be.fold_in(k=K, ld=ld, indptr=ptr_d, indices=idx_d, vals=val_d, n=NI, Z=Z, b_i=b_i, mu=mu, lam_u=LAM_U,
                   lam_bu=LAM_BU, n_sweeps=0, U_out=U, b_u_out=bu32, status=status)

    for NT in (1, 10):
        P = B * NT
        tptr = torch.arange(B + 1, dtype=torch.int64, device=dev) * NT
        titems = torch.randint(0, NI, (P,), device=dev, generator=gen).to(torch.int32)
        f64 = dict(dtype=torch.float64, device=dev)
        out = dict(score=torch.empty(P, **f64), latent=torch.empty(P, **f64), leverage=torch.empty(P, **f64),
                   top_item=torch.empty(P, TOPM, dtype=torch.int32, device=dev), top_contrib=torch.empty(P, TOPM, **f64),
                   top_weight=torch.empty(P, TOPM, **f64), top_cnt=torch.empty(P, dtype=torch.int32, device=dev),
                   b_u_out=torch.empty(B, **f64))

        def explain():
            be.explain(k=K, ld=ld, indptr=ptr_d, indices=idx_d, vals=val_d, rows=None, n=NI, Z=Z, b_i=b_i, mu=mu,
                       lam_u=LAM_U, lam_bu=LAM_BU, n_sweeps=0, t_ptr=tptr, t_items=titems, topm=TOPM, largest=True,
                       status=status, **out)

        cands = {"a_fold_in": fold, "explain": explain}
        if B <= 4096:
            lens = torch.from_numpy(np.diff(ptr)).to(dev)
            Lmax = int(lens.max())
            col = torch.arange(Lmax, device=dev)[None, :]
            mask = col < lens[:, None]                                            # [B, Lmax]
            pos = (ptr_d[:-1, None] + col).clamp(max=idx.size - 1)
            ipad = torch.where(mask, idx_d[pos].long(), torch.zeros_like(pos))
            rpad = torch.where(mask, val_d[pos].double(), torch.zeros_like(pos, dtype=torch.float64))
            tl = titems.long().view(B, NT)
            eye = torch.eye(K, **f64)

            def torch_f64():
                m = mask.double()
                Zs = Z[ipad, :K].double() * m[:, :, None]                         # [B, Lmax, K]
                res_ = (rpad - mu - b_i[ipad].double()) * m
                A = Zs.transpose(1, 2) @ Zs + (LAM_U + 1e-10) * eye
                L = torch.linalg.cholesky(A)
                g = (Zs * res_[:, :, None]).sum(1)
                h = Zs.sum(1)
                Zt = Z[tl, :K].double()                                            # [B, NT, K]
                X = torch.cholesky_solve(torch.cat([g[:, :, None], h[:, :, None], Zt.transpose(1, 2)], 2), L)
                p, q, Wt = X[:, :, 0], X[:, :, 1], X[:, :, 2:]                      # Wt [B, K, NT]
                dd = lens.double() + LAM_BU + 1e-10
                b = (res_.sum(1) - (h * p).sum(1)) / (dd - (h * q).sum(1))
                wgt = Zs @ Wt                                                      # [B, Lmax, NT]
                ctr = wgt * ((res_ - b[:, None]) * m)[:, :, None]
                latent = ctr.sum(1)
                lev = (Wt * Zt.transpose(1, 2)).sum(1)
                score = mu + b[:, None] + b_i[tl].double() + latent
                top = torch.topk(torch.where(mask[:, :, None], ctr, torch.full_like(ctr, -float("inf"))),
                                 min(TOPM, Lmax), dim=1)
                return score, lev, top
            cands["b_torch_f64"] = torch_f64
        rounds, reps = (1, 3) if quick else ((5, 10) if B < 65536 else (3, 5))
        t = alternate(cands, rounds, reps)
        assert int(status.item()) == 0
        if B <= 4096:                                      # the baseline computes what the kernel computes
            sc, lv, _ = torch_f64()
            assert torch.allclose(sc.reshape(-1), out["score"], rtol=1e-9, atol=1e-9)
            assert torch.allclose(lv.reshape(-1), out["leverage"], rtol=1e-9, atol=1e-12)
        run = {"rows": B, "ratings": int(ptr[-1]), "targets_per_row": NT, **t,
               "explain_over_a": t["explain"]["median_ms"] / t["a_fold_in"]["median_ms"]}
        if B <= 4096:
            run["b_over_explain"] = t["b_torch_f64"]["median_ms"] / t["explain"]["median_ms"]
        res["runs"][f"B{B}_T{NT}"] = run
        print(f"B{B}_T{NT}", json.dumps(run), flush=True)

print(json.dumps(res))
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
