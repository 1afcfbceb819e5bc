#!/usr/bin/env python3
"""Item fold-in (csrc/fold_in_items.hip, als_fold_in_items) at k = 64: U for 100K users and V for 100K fitted items,
seeded random (no fit needed), B in {1, 64, 4096} new items with ~100 raters each and 50 graph neighbours.
Compared within the same process:
  (a) als_fold_in (the user fold-in kernel) on the same row shapes - same CSR, U as its item table, no graph;
  (b) als_fold_in_items without the graph rows (the neighbour term's share).
Then, on a model fitted at 2000 users x 100K items with the genres / year features and the graph (top-50 on genres,
d = 19): the graph rows of 1024 new items against the 100K fitted ones, and one new item end to end through
ALS.fold_in_items (graph rows, kernel, compose_z, copies back).  Writes one JSON object to argv[1] (default: stdout
only).

    python profiles/fold_in_items_time.py profiles/fold_in_items_time.json
    rocprofv3 --kernel-trace --stats -d DIR -o fold -- python profiles/fold_in_items_time.py --quick"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import layout  # noqa: E402
from collaborative_filtering_amd.backend import HipBackend  # noqa: E402
from tests.synth import make_features, make_ratings  # noqa: E402

NU, NI, K, LAM_V, LAM_BI, ALPHA, NB = 100_000, 100_000, 64, 5.0, 3.0, 0.5, 50
quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]

dev = torch.device("cuda", 0)
be = HipBackend(dev)
gen = torch.Generator(device=dev).manual_seed(3)
ld = layout.padded_k(K)
U = torch.zeros(NU, ld, device=dev)
U[:, :K] = torch.randn(NU, K, device=dev, generator=gen) * 0.3
V = torch.zeros(NI, ld, device=dev)
V[:, :K] = torch.randn(NI, K, device=dev, generator=gen) * 0.3
b_u = torch.randn(NU, device=dev, generator=gen) * 0.1
mu = torch.tensor([3.6], dtype=torch.float64, device=dev)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts))


def wall(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def rows(B, seed):
    """B items x ~100 raters: synth power-law users, duplicates merged, CSR sorted by column."""
    r, c, v = make_ratings(B, NU, 100 * B, seed=seed, user_exp=0.0)
    ptr = np.zeros(B + 1, np.int64)
    np.add.at(ptr, r + 1, 1)
    return np.cumsum(ptr), c.astype(np.int32), v.astype(np.float32)


res = {"shape": {"users": NU, "items": NI, "k": K, "lambda_v": LAM_V, "lambda_bi": LAM_BI, "alpha": ALPHA,
                 "neighbours": NB}, "runs": {}}
rng = np.random.default_rng(1)
for B in (1, 64, 4096):
    ptr, idx, val = rows(B, seed=B)
    d = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    ptr_d, idx_d, val_d = d(ptr), d(idx), d(val)
    S = (d(np.arange(0, NB * (B + 1), NB, dtype=np.int64)),
         d(np.concatenate([np.sort(rng.permutation(NI)[:NB]) for _ in range(B)]).astype(np.int32)),
         d(rng.uniform(0.1, 1.0, NB * B).astype(np.float32)))
    Vout = torch.empty(B, ld, device=dev)
    bo = torch.empty(B, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    reps = 3 if quick else 20

    def items(graph):
        def run():
            be.fold_in_items(k=K, ld=ld, indptr=ptr_d, indices=idx_d, vals=val_d, m=NU, U=U, b_u=b_u, mu=mu,
                             S=S if graph else None, n=NI, V=V, lam_v=LAM_V, pop_reg=True, lam_bi=LAM_BI,
                             alpha=ALPHA, n_sweeps=0, V_out=Vout, b_i_out=bo, status=status)
        return run

    def users():
        be.fold_in(k=K, ld=ld, indptr=ptr_d, indices=idx_d, vals=val_d, n=NU, Z=U, b_i=b_u, mu=mu, lam_u=LAM_V,
                   lam_bu=LAM_BI, n_sweeps=0, U_out=Vout, b_u_out=bo, status=status)
    t_it, t_it_min = timed(items(True), reps)
    t_nog, _ = timed(items(False), reps)
    t_us, t_us_min = timed(users, reps)
    assert int(status.item()) == 0
    res["runs"][f"B{B}"] = {"items": B, "ratings": int(ptr[-1]), "fold_in_items_ms": t_it,
                            "fold_in_items_ms_min": t_it_min, "fold_in_items_no_graph_ms": t_nog,
                            "a_fold_in_users_same_rows_ms": t_us, "a_fold_in_users_same_rows_ms_min": t_us_min,
                            "items_over_a": t_it / t_us, "graph_term_ms": t_it - t_nog}
    print(f"B{B}", res["runs"][f"B{B}"], flush=True)

# graph rows and one item end to end, on a fitted model with features and the graph
from collaborative_filtering_amd import (ALS, ALSConfig, BiasesConfig, CoreConfig, GraphConfig,  # noqa: E402
                                         GraphSimConfig)
r, c, v = make_ratings(2000, NI, 200_000, seed=5)
G, y = make_features(NI + 1024, seed=6)
feats = {"genres": G[:NI], "year": y[:NI]}
model = ALS(ALSConfig(core=CoreConfig(n_factors=K, n_iters=1, lambda_u=LAM_V, lambda_v=LAM_V),
                      biases=BiasesConfig(lambda_bu=LAM_BI, lambda_bi=LAM_BI),
                      graph=GraphConfig(alpha=ALPHA, sim=GraphSimConfig(topk=NB))),
            {"genres": 1.0, "year": 1.0}, device="cuda:0", graph_build="device")
model.fit_coo(r, c, v, (2000, NI), features=feats, tol=None, verbose=0)
eng = model._eng
new_feats = {"genres": G[NI:], "year": y[NI:]}
X_fit = eng.X64["genres"]
reps = 3 if quick else 20
t_rows, t_rows_min = timed(lambda: eng.graph_rows_new(new_feats["genres"], X_fit), reps)
S_new = eng.graph_rows_new(new_feats["genres"], X_fit)
res["runs"]["graph_rows_1024_items_ms"] = t_rows
res["runs"]["graph_rows_1024_items_ms_min"] = t_rows_min
res["runs"]["graph_rows_1024_items_edges"] = int(S_new[0][-1])
one = np.full((1, 2000), np.nan)
one[0, rng.permutation(2000)[:100]] = rng.integers(1, 11, 100) * 0.5
f1 = {f: X[:1] for f, X in new_feats.items()}
reps = 5 if quick else 50
res["runs"]["fold_in_items_1item_wall_ms"] = wall(lambda: model.fold_in_items(one, features_new=f1), reps)
row0 = (S_new[0][:2], S_new[1][: int(S_new[0][1])], S_new[2][: int(S_new[0][1])])     # one item's graph row
res["runs"]["fold_in_items_1item_S_new_wall_ms"] = wall(lambda: model.fold_in_items(one, features_new=f1, S_new=row0),
                                                        reps)
u_items = np.sort(rng.permutation(NI)[:100]).astype(np.int32)
one_user = (np.array([0, 100]), u_items, (rng.integers(1, 11, 100) * 0.5).astype(np.float32))
res["runs"]["fold_in_1user_wall_ms"] = wall(lambda: model.fold_in(one_user, features=feats), reps)
print(json.dumps(res))
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
