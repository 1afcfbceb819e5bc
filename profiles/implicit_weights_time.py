#!/usr/bin/env python3
"""The implicit fit with weights on the unobserved entries next to the unweighted one at the cfg4
shape of bench.py - 1M x 100K, 100M entries, k = 64.  The weighted engine (item_weight="popularity", eta = 0.5, and a
user_weight drawn uniformly from [0.5, 2]) and the unweighted engine take turns, iteration by iteration, in one
process; every phase is timed with device events.  Per phase: median and minimum over the timed iterations after two
warm-ups.  Writes one JSON object to argv[1].

    python profiles/implicit_weights_time.py profiles/implicit_weights_time.json [--size cfg4-small] [--iters 12]

For the no-regression figure the same script times the unweighted engine of another checkout (the parent commit, built)
in a process of its own, and the main run takes that file in:

    python profiles/implicit_weights_time.py parent.json --root <parent checkout> --unweighted-only
    python profiles/implicit_weights_time.py profiles/implicit_weights_time.json --parent-json parent.json

The unweighted iteration of this tree must not be slower than the parent's by more than the parent's own
median-to-minimum spread ("no_regression" in the output)."""
import json
import os
import sys

import numpy as np
import torch

argv = sys.argv[1:]


def _opt(name, default=None):
    return argv[argv.index(name) + 1] if name in argv else default


ROOT = os.path.abspath(_opt("--root", os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
from bench import SIZES, gen_ratings  # noqa: E402
from collaborative_filtering_amd import ALSConfig, CoreConfig, ImplicitALS, ImplicitConfig  # noqa: E402

size = _opt("--size", "cfg4")
iters = int(_opt("--iters", 12))
parent_json = _opt("--parent-json")
unweighted_only = "--unweighted-only" in argv
out_path = argv[0] if argv and not argv[0].startswith("--") else None
WARMUP = 2
m, n, nnz, k = SIZES[size]
dev = torch.device("cuda", 0)
csr, csc = gen_ratings(dev, m, n, nnz, seed=1004)
torch.cuda.synchronize()
n_total = WARMUP + iters
cfg = ALSConfig(core=CoreConfig(n_factors=k, n_iters=n_total, lambda_u=5.0, lambda_v=6.0, random_state=42))
models = {"unweighted": ImplicitALS(cfg, ImplicitConfig(alpha=2.0), device=dev)}      # (kept alive: engines hold them weakly)
if not unweighted_only:
    p = np.random.default_rng(7).uniform(0.5, 2.0, size=m).astype(np.float32)
    models["weighted"] = ImplicitALS(cfg, ImplicitConfig(alpha=2.0, item_weight="popularity", popularity_exponent=0.5,
                                                         user_weight=p), device=dev)
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
       "tree": "other checkout (--root)" if "--root" in argv else "this tree",
       "phases": {name: {ph: stat(ts) for ph, ts in d.items()} for name, d in phases.items()},
       "loss": {name: [float(x) for x in eng.hist[:n_total].cpu().numpy()] for name, eng in engines.items()}}
ph = res["phases"]
if "weighted" in ph:
    res["weighted_to_unweighted"] = {
        name: ph["weighted"][name]["median_ms"] / ph["unweighted"][name]["median_ms"]
        for name in ("table_gram", "row_solve_user", "row_solve_item", "iteration")}
if parent_json:
    parent = json.load(open(parent_json))
    assert parent["shape"] == res["shape"], "the parent's run is of another shape"
    pit, it_ = parent["phases"]["unweighted"]["iteration"], ph["unweighted"]["iteration"]
    spread = pit["median_ms"] - pit["min_ms"]
    res["parent_unweighted"] = parent["phases"]["unweighted"]
    res["no_regression"] = {"unweighted_iteration_median_ms": it_["median_ms"],
                            "parent_iteration_median_ms": pit["median_ms"], "parent_median_to_min_ms": spread,
                            "holds": bool(it_["median_ms"] <= pit["median_ms"] + spread)}
    # the unweighted fit computes what the parent computed: the same loss history, bit for bit
    res["unweighted_loss_equals_parent"] = res["loss"]["unweighted"] == parent["loss"]["unweighted"]
print(json.dumps(res))
if out_path:
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
