#!/usr/bin/env python3
"""ALS.recommend_quota's fused call (serving._Serving._quota_chunks: als_recommend_topk_quota) against the two things a
caller had before it, in the same run: n = 100 000 items, k = 64, N = 10, users with ~100 seen items each, seeded
random factors, at 4 096 and 65 536 users.

  recommend   (a) the parent's plain `recommend` at the same N - `_topk_chunks`, no caps: the floor of any such call;
  overfetch   (b) the alternative to the fused call: `_topk_chunks` at N = 128, the lists copied to the host, a
              vectorised numpy greedy filter over them (`host_filter`), and the share of rows that come up short of
              their exact list - those a caller has to page for with recommend_deep;
  quota       the fused call, lists copied to the host as well.

Label scenarios (labels drawn once, seeded):
  artists   n / 5 groups of Zipf sizes, cap 2;
  genres    20 groups of Zipf sizes, cap 3;
  dominant  90 % of the items in one group, the rest in 1000 small groups, cap 1;
  loose     the genres labels, cap N: the caps never bind, the result is `recommend`'s.
Where the over-fetched list is long enough, it must equal the fused call's, element for element; the script asserts it.
Every timed step runs under its own alarm: a step that exceeds it ends the process, and what was measured until then is
already in the file.

    python profiles/quota_bench.py profiles/quota_bench.json [--quick]"""
import json
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
from collaborative_filtering_amd.serving import _Serving, quota_plan  # noqa: E402

NI, K, N, DEEP = 100_000, 64, 10, 128
quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]
BATCHES = (4096, 65536)
STEP_LIMIT_S = 120

dev = torch.device("cuda", 0)
ld = layout.padded_k(K)


class Loop(_Serving):
    """The serving mixin over tables made here: what `_quota_chunks` and `_topk_chunks` read of the engine."""

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


def zipf_labels(rng, n, G):
    p = 1.0 / np.arange(1, G + 1)
    return rng.choice(G, size=n, p=p / p.sum()).astype(np.int32)


def host_filter(items, labels, caps, N):
    """The greedy cap filter over lists already in recommend's order, all rows at once: entry (b, t) is kept iff fewer
    than cap earlier entries of row b share its group; -> (lists int64 [B, N] padded -1, kept entries per row)."""
    B, D = items.shape
    g = np.where(items >= 0, labels[np.maximum(items, 0)], -1)
    order = np.argsort(g, axis=1, kind="stable")                           # by group, list order within a group
    gs = np.take_along_axis(g, order, axis=1)
    pos = np.broadcast_to(np.arange(D), (B, D))
    start = np.where(np.concatenate([np.ones((B, 1), bool), gs[:, 1:] != gs[:, :-1]], axis=1), pos, 0)
    rank_sorted = pos - np.maximum.accumulate(start, axis=1)
    rank = np.empty_like(rank_sorted)
    np.put_along_axis(rank, order, rank_sorted, axis=1)
    keep = (items >= 0) & ((g < 0) | (rank < caps[np.maximum(g, 0)]))
    slot = np.cumsum(keep, axis=1) - 1
    out = np.full((B, N), -1, np.int64)
    take = keep & (slot < N)
    b, t = np.nonzero(take)
    out[b, slot[b, t]] = items[b, t]
    return out, keep.sum(axis=1)


def main():
    signal.signal(signal.SIGALRM, signal.SIG_DFL)
    loop = Loop()
    gen = torch.Generator(device=dev).manual_seed(3)
    Z = torch.zeros(NI, ld, device=dev)
    Z[:, :K] = torch.randn(NI, K, device=dev, generator=gen) * 0.3
    b_i = torch.randn(NI, device=dev, generator=gen) * 0.1
    mu = torch.tensor([3.6], dtype=torch.float64, device=dev)
    items = dict(k=K, ld=ld, n=NI, Z=Z, b_i=b_i, mu=mu)
    rng = np.random.default_rng(5)
    genres = zipf_labels(rng, NI, 20)
    dominant = np.where(rng.random(NI) < 0.9, 0, 1 + rng.integers(0, 1000, NI)).astype(np.int32)
    scenarios = (("artists", zipf_labels(rng, NI, NI // 5), 2), ("genres", genres, 3), ("dominant", dominant, 1),
                 ("loose", genres, N))
    res = {"shape": {"items": NI, "k": K, "N": N, "overfetch_N": DEEP}, "clocks_before": clocks(), "runs": {}}

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

        def rows(b0, nb):
            return users[b0: b0 + nb], U, b_u, seen_ptr, seen_idx

        _, plain = timed(lambda: loop._topk_chunks(B, N, rows, items), 5)
        deep, fetch = timed(lambda: loop._topk_chunks(B, DEEP, rows, items), 3)
        for name, labels, c in scenarios:
            caps = np.full(int(labels.max()) + 1, c, dtype=np.int32)
            row = {"users": B, "scenario": name, "groups": int(caps.size), "cap": c,
                   "n_eff": quota_plan(None, labels, caps, N)[1], "recommend": plain, "overfetch_walk": fetch}
            got, row["quota"] = timed(lambda: loop._quota_chunks(B, N, rows, items, None, labels, caps), 5)
            (lists, kept), row["overfetch_filter"] = timed(lambda: host_filter(deep[0], labels, caps, N), 3)
            short = kept < N                                               # the pool ran out before the list was full
            row["overfetch_short_rows"] = int(short.sum())
            row["overfetch_short_share"] = float(short.mean())
            assert (lists[~short] == got[0][~short]).all()                 # where the pool sufficed, the same lists
            row["overfetch_ms"] = fetch["ms"] + row["overfetch_filter"]["ms"]
            row["quota_over_recommend"] = row["quota"]["ms"] / plain["ms"]
            row["overfetch_over_quota"] = row["overfetch_ms"] / row["quota"]["ms"]
            g = np.where(got[0] >= 0, labels[np.maximum(got[0], 0)], -1)
            row["max_in_one_group"] = int(max(np.bincount(r[r >= 0]).max(initial=0) for r in g[:: max(1, B // 512)]))
            res["runs"][f"B{B}_{name}"] = row
            print(f"B{B}_{name}", json.dumps(row), flush=True)
            save()
    res["clocks_after"] = clocks()
    save()
    print(json.dumps({k: {"quota_ms": v["quota"]["ms"], "recommend_ms": v["recommend"]["ms"],
                          "overfetch_ms": v["overfetch_ms"], "short_share": v["overfetch_short_share"]}
                      for k, v in res["runs"].items()}))


if __name__ == "__main__":
    main()
