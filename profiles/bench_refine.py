"""U-step time over a long fit under solve_dtype="auto" and "refine": the workload of
profiles/r03_auto_redo_over_a_long_fit.txt (BASELINE configs[4] shape / 50: k = 128, bias + W_f + Laplacian,
popularity-scaled lambda_v, synthetic data), 60 iterations, where "auto" ends up redoing 92 % of the user rows in fp64.

Per iteration: the U-step's als_row_solve / als_row_solve_refine call between two device events, the rows flagged, the
rows that fell back to the fp64 kernel and the histogram of refinement steps.  One process per mode and library; the
fit is repeated `--reps` times in it (a fresh model each time, the same seed: the repetitions differ by the machine
only) and the iterations 5 and 60 of every repetition are summarised.  `--tree` runs the package and library of another
checkout (the parent commit's, for "auto" as it was before the mode existed).

Usage: timeout 900 python profiles/bench_refine.py --mode refine [--reps 3] [--iters 60] [--tree DIR] >> profiles/refine_long_fit.txt"""
import argparse
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--mode", default="refine", choices=["auto", "refine", "float32"])
ap.add_argument("--size", default="cfg5-small")
ap.add_argument("--iters", type=int, default=60)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

import numpy as np                                                                            # noqa: E402
import torch                                                                                  # noqa: E402
import bench                                                                                  # noqa: E402
from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, GraphConfig, GraphSimConfig   # noqa: E402

assert torch.cuda.is_available(), "bench_refine.py measures on the GPU: no device is visible"
dev = torch.device("cuda", 0)
size, iters = args.size, args.iters
m, n, _, k = bench.SIZES[size]
inputs = bench.make_inputs(size, dev, 0, False, "sampled", False)
csr, csc, S, features = inputs[:4]
print(f"# bench_refine.py mode={args.mode} size={size} (m={m}, n={n}, k={k}) iterations={iters} repetitions={args.reps} "
      f"device={torch.cuda.get_device_name(0)} tree={'this checkout' if args.tree == ap.get_default('tree') else 'other checkout'}",
      flush=True)

summary = []
for rep in range(args.reps):
    cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=iters, lambda_u=5.0, lambda_v=6.0, random_state=42,
                                    pop_reg_mode="inverse_sqrt" if size in ("cfg5-small", "cfg5") else None),
                    biases=BiasesConfig(lambda_bu=3.0, lambda_bi=2.0),
                    graph=(GraphConfig(alpha=0.5, sim=GraphSimConfig(source="precomputed", topk=50)) if S is not None else GraphConfig()))
    model = ALS(cfg, lambda_w={"genres": 5.0, "years": 10.0} if features else None, device=dev, solve_dtype=args.mode)
    eng = model.prepare_csr(csr, csc, (m, n), features=features, S=S)
    if features:
        eng.be.compose_z(eng.V, eng.Xcat, eng.Wcat, eng.Z)
    be = eng.be
    timed = []                      # (event, event) of the row_solve calls of the step in flight
    inner = be.row_solve

    def row_solve(**kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        inner(**kw)
        e1.record()
        timed.append((e0, e1))

    be.row_solve = row_solve
    per_iter = []
    for it in range(iters):
        timed.clear()
        eng.user_step()
        torch.cuda.synchronize()
        ms = sum(a.elapsed_time(b) for a, b in timed)
        flagged = int(be._redo_count.item())
        fallback = int(be._fallback_count.item()) if args.mode == "refine" else flagged
        hist = be._refine_steps.tolist() if args.mode == "refine" else []
        do_w = bool(eng.feat_names) and ((it % model.update_w_every == 0) or (it == iters - 1))
        b_i_old = eng.b_i.clone() if (do_w or eng.fused_feat_stats) else None
        eng.b_i_prev = b_i_old
        eng.item_step(want_gram=do_w or eng.fused_feat_stats)
        if do_w:
            eng.w_step(b_i_old)
        eng.stats_step(it)
        eng.iters_run = it + 1
        torch.cuda.synchronize()
        per_iter.append(ms)
        if rep == 0 and (it < 6 or it % 5 == 4):
            print(f"iteration {it + 1:3d}: U-step {ms:7.2f} ms, rows flagged {flagged:7d} of {m}, to the fp64 kernel {fallback:7d}"
                  + (f", accepted after s steps {hist}" if hist else "") + f";  max|Z| {float(eng.Z.abs().max()):.3g}", flush=True)
    i5 = per_iter[min(4, iters - 1)]
    summary.append((i5, per_iter[-1]))
    print(f"repetition {rep + 1}: U-step at iteration 5 {i5:.2f} ms, at iteration {iters} {per_iter[-1]:.2f} ms "
          f"(ratio {per_iter[-1] / i5:.2f}), flagged {flagged}, to the fp64 kernel {fallback}", flush=True)
last = np.asarray([s[1] for s in summary])
print(f"summary mode={args.mode}: U-step at iteration {iters} over {args.reps} repetitions: min {last.min():.2f} "
      f"median {float(np.median(last)):.2f} max {last.max():.2f} ms", flush=True)
