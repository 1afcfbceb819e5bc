#!/usr/bin/env python3
"""Fold-in (csrc/fold_in.hip, als_fold_in) at the configs[3] item side: Z for 100K items at k = 64 plus biases,
seeded random (no fit needed), B in {1, 64, 4096, 65536} new users with ~100 ratings each from the synth
distribution.  Compared within the same process:
  (a) als_row_solve in fp64 mode (ALS_GRAM_F64) over the same rows, once - one user half-step;
  (b) the same 15 times - what a Python-only fold-in with T = 15 would cost;
and recommend (1 known user) against recommend_new (1 new user) at N = 10 on a small fitted model's tables grown to
the same shape.  Writes one JSON object to argv[1] (default: stdout only).

    python profiles/fold_in_time.py profiles/fold_in_time.json
    rocprofv3 --kernel-trace --stats -d DIR -o fold -- python profiles/fold_in_time.py --quick   # kernel table"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import layout  # noqa: E402
from collaborative_filtering_amd.als import _SideDev, _tasks_to_dev  # noqa: E402
from collaborative_filtering_amd.backend import HipBackend  # noqa: E402
from tests.synth import make_ratings  # noqa: E402

NI, K, LAM_U, LAM_BU = 100_000, 64, 5.0, 3.0
quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]

dev = torch.device("cuda", 0)
be = HipBackend(dev, solve_dtype="float64")
gen = torch.Generator(device=dev).manual_seed(3)
ld = layout.padded_k(K)
Z = torch.zeros(NI + 1, ld, device=dev)              # + a zero row: the gather target of als_row_solve's tail lanes
Z[:NI, :K] = torch.randn(NI, K, device=dev, generator=gen) * 0.3
b_i = torch.randn(NI, device=dev, generator=gen) * 0.1
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


def rows(B, seed):
    """B users x ~100 ratings: synth power-law items, duplicates merged, CSR sorted by column."""
    r, c, v = make_ratings(B, NI, 100 * B, seed=seed, user_exp=0.0)
    ptr = np.zeros(B + 1, np.int64)
    np.add.at(ptr, r + 1, 1)
    return np.cumsum(ptr), c.astype(np.int32), v.astype(np.float32)


res = {"shape": {"items": NI, "k": K, "lambda_u": LAM_U, "lambda_bu": LAM_BU}, "runs": {}}
for B in (1, 64, 4096, 65536):
    ptr, idx, val = rows(B, seed=B)
    d = lambda a: torch.from_numpy(a).to(dev)
    ptr_d, idx_d, val_d = d(ptr), d(idx), d(val)
    U = torch.empty(B, ld, device=dev)
    bu = torch.zeros(B, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    reps = 3 if quick else (20 if B < 65536 else 10)

    def fold():
        be.fold_in(k=K, ld=ld, indptr=ptr_d, indices=idx_d, vals=val_d, n=NI, Z=Z, b_i=b_i, mu=mu, lam_u=LAM_U,
                   lam_bu=LAM_BU, n_sweeps=0, U_out=U, b_u_out=bu, status=status)
    t_fold, t_fold_min = timed(fold, reps)
    side = _SideDev(B, NI, ptr_d, idx_d, val_d)
    tasks = _tasks_to_dev(layout.build_row_tasks(ptr, 0, B, dual_len=0, mid_len=0), dev)
    kw = dict(k=K, ld=ld, side=side, F=Z, zero_row=NI, bias_self=bu, bias_other=b_i, mu=mu, lam=LAM_U, lam_row=None,
              lam_b=LAM_BU, lam_b_row=None, rhs_extra=None, diag_extra=None, X_out=U, bias_out=bu, gram_out=None,
              factor_out=None, rhs_out=None, colsum_out=None, sumr_out=None, status=status, tasks=tasks,
              workspace=None)

    def half_steps(T):
        def run():
            bu.zero_()
            for _ in range(T):
                be.row_solve(**kw)
        return run
    t_a, _ = timed(half_steps(1), reps)
    t_b, _ = timed(half_steps(15), max(3, reps // 4))
    assert int(status.item()) == 0
    res["runs"][f"B{B}"] = {"users": B, "ratings": int(ptr[-1]), "fold_in_fixed_point_ms": t_fold,
                            "fold_in_fixed_point_ms_min": t_fold_min, "a_row_solve_f64_once_ms": t_a,
                            "b_row_solve_f64_x15_ms": t_b, "fold_in_over_a": t_fold / t_a,
                            "b_over_fold_in": t_b / t_fold}
    print(f"B{B}", res["runs"][f"B{B}"], flush=True)

# recommend (known user) vs recommend_new (new user), one user, N = 10, through the model API
from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig  # noqa: E402
r, c, v = make_ratings(2000, NI, 200_000, seed=5)
model = ALS(ALSConfig(core=CoreConfig(n_factors=K, n_iters=1, lambda_u=LAM_U, lambda_v=LAM_U),
                      biases=BiasesConfig(lambda_bu=LAM_BU, lambda_bi=LAM_BU)), device="cuda:0")
model.fit_coo(r, c, v, (2000, NI), tol=None, verbose=0)
ptr, idx, val = rows(1, seed=9)
new = (ptr, idx, val)


def wall(fn, reps):
    import time
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


reps = 5 if quick else 50
res["runs"]["recommend_1user_N10_wall_ms"] = wall(lambda: model.recommend([7], 10), reps)
res["runs"]["recommend_new_1user_N10_wall_ms"] = wall(lambda: model.recommend_new(new, 10), reps)
res["runs"]["fold_in_1user_wall_ms"] = wall(lambda: model.fold_in(new), reps)
print(json.dumps(res))
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
