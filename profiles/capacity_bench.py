#!/usr/bin/env python3
"""ALS.recommend_capacity's round loop (serving._Serving._capacity_rounds: als_recommend_topk_priced +
als_capacity_settle) against one plain `recommend` of the same batch in the same run: n = 100 000 items, k = 64, N = 10,
users with ~100 seen items each, seeded random factors, at 4 096 and 65 536 users.

Three capacity regimes per batch size (c = the same cap for every item, at least 1):
  loose         c = ceil(4 B N / n);
  tight         c = ceil(1.2 B N / n);
  tight_skewed  the tight cap on a catalogue whose item bias is spread by popularity rank (+ 2 (1 + rank)^-1/2, as in
                tests/test_gpu_capacity.py), so the same items top most lists.
For each it reports the total time of the call (host clock around the loop, which ends in the copy of the lists to the
host - the same for the yardstick), the rounds, the walked rows, and from a second, instrumented pass (device events
around every backend call) the walk and the settle time of every round.  The yardstick is `_topk_chunks` - the parent
commit's `recommend` - on the same rows, catalogue and seen lists.  Every timed step runs under its own alarm: a step
that exceeds it ends the process, and what was measured until then is already in the file.

    python profiles/capacity_bench.py profiles/capacity_bench.json [--quick] [--only=B65536_tight_skewed]

--quick times every step once; --only keeps the named runs (a kernel trace of one run: rocprofv3 --kernel-trace --stats
-- python profiles/capacity_bench.py --quick --only=...)."""
import json
import math
import os
import signal
import subprocess
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import layout  # noqa: E402
from collaborative_filtering_amd.backend import HipBackend  # noqa: E402
from collaborative_filtering_amd.serving import _Serving  # noqa: E402

NI, K, N = 100_000, 64, 10
quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
only = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--only=")]     # e.g. --only=B65536_tight_skewed
BATCHES = (4096, 65536)
STEP_LIMIT_S = 120

dev = torch.device("cuda", 0)
ld = layout.padded_k(K)


class Loop(_Serving):
    """The serving mixin over tables made here: what `_capacity_rounds` and `_topk_chunks` read of the engine."""

    def __init__(self):
        self.dev, self.be = dev, HipBackend(dev)


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in out.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln)]
    except Exception as exc:                                               # the tool is optional
        return [f"rocm-smi unavailable: {exc!r}"]


def step(fn, limit=STEP_LIMIT_S):
    """fn() under an alarm of its own (default action: the process ends); -> (result, seconds), synchronised."""
    signal.alarm(limit)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    signal.alarm(0)
    return out, dt


def timed(fn, reps):
    step(fn)                                                               # warm-up
    ts, out = [], None
    for _ in range(1 if quick else reps):
        out, dt = step(fn)
        ts.append(dt * 1e3)
    return out, {"ms": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": len(ts)}


class Events:
    """Device events around every call of the backend methods `names`; `ms()` after a synchronise."""

    def __init__(self, be, names):
        self.log, self.be, self.orig = [], be, {n: getattr(be, n) for n in names}
        for n in names:
            setattr(be, n, self._wrap(n, self.orig[n]))

    def _wrap(self, name, fn):
        def call(**kw):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(**kw)
            b.record()
            self.log.append((name, kw["users"].numel() if "users" in kw else 0, a, b))
        return call

    def restore(self):
        for n, fn in self.orig.items():
            setattr(self.be, n, fn)

    def ms(self):
        torch.cuda.synchronize()
        return [(name, rows, a.elapsed_time(b)) for name, rows, a, b in self.log]


def main():
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    loop = Loop()
    gen = torch.Generator(device=dev).manual_seed(3)
    Z = torch.zeros(NI, ld, device=dev)
    Z[:, :K] = torch.randn(NI, K, device=dev, generator=gen) * 0.3
    b_flat = torch.randn(NI, device=dev, generator=gen) * 0.1
    rank = torch.randperm(NI, device=dev, generator=gen).to(torch.float32)
    b_skew = b_flat + 2.0 * (1.0 + rank) ** -0.5
    mu = torch.tensor([3.6], dtype=torch.float64, device=dev)
    res = {"shape": {"items": NI, "k": K, "N": N}, "clocks_before": clocks(), "runs": {}}

    def save():
        if args:
            with open(args[0], "w") as f:
                json.dump(res, f, indent=1)

    for B in BATCHES:
        U = torch.zeros(B, ld, device=dev)
        U[:, :K] = torch.randn(B, K, device=dev, generator=gen) * 0.3
        b_u = torch.randn(B, device=dev, generator=gen) * 0.1
        raw = torch.randint(0, NI, (B, 100), device=dev, generator=gen).sort(dim=1).values
        keep = torch.ones_like(raw, dtype=torch.bool)
        keep[:, 1:] = raw[:, 1:] != raw[:, :-1]
        seen_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        seen_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
        seen_idx = raw[keep].to(torch.int32)
        del raw, keep
        users = torch.arange(B, dtype=torch.int32, device=dev)

        def pick(ix):
            return users[ix], U, b_u, seen_ptr, seen_idx

        def rows(b0, nb):
            return users[b0: b0 + nb], U, b_u, seen_ptr, seen_idx

        for regime, factor, b_i in (("loose", 4.0, b_flat), ("tight", 1.2, b_flat), ("tight_skewed", 1.2, b_skew)):
            items = dict(k=K, ld=ld, n=NI, Z=Z, b_i=b_i, mu=mu)
            c = max(1, math.ceil(factor * B * N / NI))
            cap = np.full(NI, c, dtype=np.int32)
            if only and f"B{B}_{regime}" not in only:
                continue
            row = {"users": B, "regime": regime}
            # the yardstick: the parent's recommend on the same batch, lists copied to the host as well
            _, row["recommend"] = timed(lambda: loop._topk_chunks(B, N, rows, items), 5)
            out, row["capacity"] = timed(lambda: loop._capacity_rounds(B, N, pick, items, None, cap, None), 3)
            info = out[2]
            row["capacity_per_item"] = c
            row["rounds"], row["walked_rows"] = info.rounds, info.walked_rows
            row["walked_over_B"] = info.walked_rows / B
            row["filled_slots"] = int((out[0] >= 0).sum())
            row["full_items"] = int((info.fill == c).sum())
            assert (info.fill <= c).all() and (np.bincount(out[0][out[0] >= 0], minlength=NI) == info.fill).all()
            # the instrumented pass: device time of every walk and settle
            ev = Events(loop.be, ("recommend_topk_priced", "capacity_settle"))
            step(lambda: loop._capacity_rounds(B, N, pick, items, None, cap, None))
            ev.restore()
            log = ev.ms()
            settles = [ms for name, _, ms in log if name == "capacity_settle"]
            walks = [(r, ms) for name, r, ms in log if name == "recommend_topk_priced"]
            row["settle_ms_per_round"] = settles
            row["settle_ms_total"] = float(sum(settles))
            row["walk_ms_total"] = float(sum(ms for _, ms in walks))
            row["walk_calls"] = [[r, ms] for r, ms in walks][:64]
            row["capacity_over_recommend"] = row["capacity"]["ms"] / row["recommend"]["ms"]
            row["model_ms"] = row["walked_over_B"] * row["recommend"]["ms"] + row["settle_ms_total"]
            res["runs"][f"B{B}_{regime}"] = row
            print(f"B{B}_{regime}", json.dumps(row), flush=True)
            save()
    res["clocks_after"] = clocks()
    save()
    print(json.dumps({k: {"capacity_ms": v["capacity"]["ms"], "recommend_ms": v["recommend"]["ms"],
                          "rounds": v["rounds"], "walked_over_B": v["walked_over_B"],
                          "settle_ms_total": v["settle_ms_total"]} for k, v in res["runs"].items()}))


if __name__ == "__main__":
    main()
