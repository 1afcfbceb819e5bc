#!/usr/bin/env python3
"""The implicit fit (csrc/implicit.hip) at the cfg4 shape of bench.py - 1M x 100K, 100M entries, k = 64 - next to the
explicit fit on the same sides under solve_dtype="float64" (the same fp64 machinery without G and without weights)
and under the default path.  The three engines take turns, iteration by iteration, in one process; every phase is
timed with device events.  Per phase: median and minimum over the timed iterations after two warm-ups.  The longest
single row (one task list with that row alone) is timed on its own.  Writes one JSON object to argv[1].

    python profiles/implicit_time.py profiles/implicit_time.json [--size cfg4-small] [--iters 12]"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import SIZES, gen_ratings  # noqa: E402
from collaborative_filtering_amd import ALS, ALSConfig, BiasesConfig, CoreConfig, ImplicitALS, ImplicitConfig  # noqa: E402
from collaborative_filtering_amd import layout  # noqa: E402
from collaborative_filtering_amd.containers import _tasks_to_dev  # noqa: E402

argv = sys.argv[1:]
size = argv[argv.index("--size") + 1] if "--size" in argv else "cfg4"
iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 12
out_path = argv[0] if argv and not argv[0].startswith("--") else None
WARMUP = 2
m, n, nnz, k = SIZES[size]
dev = torch.device("cuda", 0)
csr, csc = gen_ratings(dev, m, n, nnz, seed=1004)
torch.cuda.synchronize()
n_total = WARMUP + iters
cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=n_total, lambda_u=5.0, lambda_v=6.0, random_state=42),
                biases=BiasesConfig(lambda_bu=3.0, lambda_bi=2.0))
models = {       # (kept alive: an engine holds its model weakly)
    "implicit": ImplicitALS(cfg, ImplicitConfig(alpha=2.0), device=dev),
    "explicit_float64": ALS(cfg, device=dev, solve_dtype="float64"),
    "explicit_default": ALS(cfg, device=dev),
}
engines = {name: md.prepare_csr(csr, csc, (m, n)) for name, md in models.items()}
torch.cuda.synchronize()

phases = {name: {} for name in engines}
for it in range(n_total):
    for name, eng in engines.items():                  # alternating: the engines see the same machine state
        eng.timers = [] if it >= WARMUP else None
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.iteration(it, n_total)
        b.record()
        b.synchronize()
        if it >= WARMUP:
            per = {}
            for ph, e0, e1 in eng.timers:
                per[ph] = per.get(ph, 0.0) + e0.elapsed_time(e1)       # (the two Gram launches add up)
            per["iteration"] = a.elapsed_time(b)
            for ph, t in per.items():
                phases[name].setdefault(ph, []).append(t)
        eng.timers = None
for eng in engines.values():
    eng._check_status()


def stat(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "n": len(ts)}


res = {"shape": {"size": size, "users": m, "items": n, "entries": nnz, "k": k, "warmup": WARMUP, "iters": iters},
       "phases": {name: {ph: stat(ts) for ph, ts in d.items()} for name, d in phases.items()}}

# the longest single row of each side, alone in its task list
eng = engines["implicit"]
for side_name, side, F_store, nF, X, lam in (("user", eng.csr, eng.V_store, eng.n, eng.U, 5.0),
                                             ("item", eng.csc, eng.U_store, eng.m, eng.V, 6.0)):
    ptr = side.indptr.cpu().numpy()
    r = int(np.argmax(np.diff(ptr)))
    tasks = _tasks_to_dev(layout.build_row_tasks(ptr, r, r + 1, dual_len=0, mid_len=0), dev)
    eng.be.table_gram(eng.k, eng.ld, F_store[:nF], eng.G)
    ts = []
    for rep in range(WARMUP + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.be.implicit_row_solve(k=eng.k, ld=eng.ld, side=side, F=F_store, zero_row=nF, G=eng.G, g_scale=eng.a0,
                                  lam=lam, lam_row=None, X_out=X, xb_out=None, status=eng.status, tasks=tasks)
        b.record()
        b.synchronize()
        if rep >= WARMUP:
            ts.append(a.elapsed_time(b))
    res[f"longest_{side_name}_row"] = {"row": r, "entries": int(ptr[r + 1] - ptr[r]), "segments": int(tasks.ntasks),
                                       **stat(ts)}
eng._check_status()

p = res["phases"]
res["ratio_to_explicit_float64"] = {
    ph: p["implicit"][ph]["median_ms"] / p["explicit_float64"][ph]["median_ms"]
    for ph in ("row_solve_user", "row_solve_item", "iteration")}
res["ratio_to_explicit_default"] = {
    ph: p["implicit"][ph]["median_ms"] / p["explicit_default"][ph]["median_ms"]
    for ph in ("row_solve_user", "row_solve_item", "iteration")}
res["loss"] = [float(x) for x in eng.hist[:n_total].cpu().numpy()]
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
