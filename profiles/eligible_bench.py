#!/usr/bin/env python3
"""Per-row eligibility (als_recommend_topk_segmented, als_eligibility_bitmaps) against what the library offered before:
n = 100 000 items, k = 64, 4096 users with ~100 seen items each, N = 10, seeded random factors.

For S in {1, 16, 256, 4096} segments and an allowed share of 1.0, 0.5, 0.05 (independent bits) and 0.05 as one
contiguous run per segment, every user in a random segment (S = 4096: one each), it times
  fused         one als_recommend_topk_segmented call, rows in the caller's order;
  fused_sorted  the same call on the batch stable-sorted by segment (the permutation's own cost is timed apart);
  loop          the parent commit's way: users grouped by segment, one als_recommend_topk_masked per segment, the whole
                loop between two events (its launches and their host cost are what that way costs);
  floor         als_recommend_topk, unfiltered, on the same rows;
and checks fused == fused_sorted (un-permuted) == loop, element for element.  It also counts, from the table and the
row order, the share of (16-row wave, chunk) pairs the kernel skips and the share of (workgroup, chunk) pairs in which
every wave skips - the most a workgroup-level skip of fetch / stage could remove.  The builder is timed at n = 10^6,
S = 1000, tw = 4.  Times are medians of repeated launches after a warm-up, device events; the clocks rocm-smi reports
go into the file.  Writes one JSON object to argv[1] (default: stdout only).

    python profiles/eligible_bench.py profiles/eligible_vs_segment_loop.json"""
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from collaborative_filtering_amd import layout  # noqa: E402
from collaborative_filtering_amd.backend import HipBackend  # noqa: E402

B, NI, K, N = 4096, 100_000, 64, 10
quick = "--quick" in sys.argv
args = [a for a in sys.argv[1:] if not a.startswith("--")]

dev = torch.device("cuda", 0)
be = HipBackend(dev)
gen = torch.Generator(device=dev).manual_seed(3)
ld = layout.padded_k(K)
W = (NI + 31) // 32
U = torch.zeros(B, ld, device=dev)
U[:, :K] = torch.randn(B, K, device=dev, generator=gen) * 0.3
Z = torch.zeros(NI, ld, device=dev)
Z[:, :K] = torch.randn(NI, K, device=dev, generator=gen) * 0.3
b_u = torch.randn(B, device=dev, generator=gen) * 0.1
b_i = torch.randn(NI, device=dev, generator=gen) * 0.1
mu = torch.tensor([3.6], dtype=torch.float64, device=dev)
raw = torch.randint(0, NI, (B, 100), device=dev, generator=gen).sort(dim=1).values
keep = torch.ones_like(raw, dtype=torch.bool)
keep[:, 1:] = raw[:, 1:] != raw[:, :-1]
seen_ptr = torch.zeros(B + 1, dtype=torch.int64, device=dev)
seen_ptr[1:] = torch.cumsum(keep.sum(dim=1), 0)
seen_idx = raw[keep].to(torch.int32)
del raw, keep


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        return [ln.strip() for ln in out.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln)]
    except Exception as exc:                                               # the tool is optional
        return [f"rocm-smi unavailable: {exc!r}"]


def timed(fn, reps):
    fn()                                              # warm-up (and first-call costs)
    ts = []
    for _ in range(1 if quick else reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"ms": float(np.median(ts)), "ms_min": float(np.min(ts)), "ms_max": float(np.max(ts)), "reps": len(ts)}


def pack_rows(bits):
    """bool [R, NI] (device) -> int32 [R, W] bitmap rows."""
    R = bits.shape[0]
    full = torch.zeros(R, W * 32, dtype=torch.int64, device=dev)
    full[:, :NI] = bits
    words = (full.view(R, W, 32) << torch.arange(32, dtype=torch.int64, device=dev)).sum(dim=2)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)


def make_table(S, kind):
    table = torch.empty(S, W, dtype=torch.int32, device=dev)
    for s0 in range(0, S, 64):
        R = min(64, S - s0)
        if kind == "1.0":
            bits = torch.ones(R, NI, dtype=torch.bool, device=dev)
        elif kind == "0.05_contiguous":
            start = torch.randint(0, NI - NI // 20, (R, 1), device=dev, generator=gen)
            col = torch.arange(NI, device=dev)[None, :]
            bits = (col >= start) & (col < start + NI // 20)
        else:
            bits = torch.rand(R, NI, device=dev, generator=gen) < float(kind)
        table[s0: s0 + R] = pack_rows(bits)
    return table


def outputs(rows):
    return (torch.empty(rows, N, dtype=torch.float32, device=dev), torch.empty(rows, N, dtype=torch.int32, device=dev),
            torch.empty(rows, dtype=torch.int32, device=dev))


def common(users, out):
    return dict(k=K, ld=ld, users=users, n=NI, U=U, Z=Z, b_u=b_u, b_i=b_i, mu=mu, seen_ptr=seen_ptr, seen_idx=seen_idx,
                topn=N, top_val=out[0], top_idx=out[1], top_cnt=out[2])


def skip_shares(table, row_seg, rows_per_wg):
    """(share of (wave, chunk) pairs with no set bit in any of the wave's 16 rows, share of (workgroup, chunk) pairs
    with none in any of its rows) for the batch in the order `row_seg`."""
    wave_any = torch.zeros(B // 16, W, dtype=torch.bool, device=dev)
    for w0 in range(0, B // 16, 16):                                       # 256 rows of words at a time
        words = table[row_seg[w0 * 16: (w0 + 16) * 16].long()]
        wave_any[w0: w0 + 16] = (words.view(16, 16, W) != 0).any(dim=1)
    wg_any = wave_any.view(B // rows_per_wg, rows_per_wg // 16, W).any(dim=1)
    return float(1.0 - wave_any.float().mean().item()), float(1.0 - wg_any.float().mean().item())


rng = np.random.default_rng(0)
users = torch.arange(B, dtype=torch.int32, device=dev)
res = {"shape": {"users": B, "items": NI, "k": K, "N": N, "seen_per_user": float(seen_idx.numel() / B)},
       "clocks_before": clocks(), "runs": {}, "builder": {}}

out_floor = outputs(B)
floor = timed(lambda: be.recommend_topk(**common(users, out_floor)), 20)
res["floor_unfiltered"] = floor
print("floor", floor, flush=True)

for S in (1, 16, 256, 4096):
    seg_h = rng.permutation(B) if S == B else rng.integers(0, S, B)
    row_seg = torch.from_numpy(seg_h.astype(np.int32)).to(dev)
    for kind in ("1.0", "0.5", "0.05", "0.05_contiguous"):
        table = make_table(S, kind)
        row = {"segments": S, "allowed": kind}

        out_f = outputs(B)
        row["fused"] = timed(lambda: be.recommend_topk_segmented(seg_allow=table, row_seg=row_seg,
                                                                 **common(users, out_f)), 20)
        # the batch sorted by segment: the permutation and the un-permutation are the driver's to pay
        perm_t = timed(lambda: torch.sort(row_seg.long(), stable=True), 20)
        order = torch.sort(row_seg.long(), stable=True).indices
        users_s, seg_s = users[order].contiguous(), row_seg[order].contiguous()
        out_s = outputs(B)
        row["fused_sorted"] = timed(lambda: be.recommend_topk_segmented(seg_allow=table, row_seg=seg_s,
                                                                        **common(users_s, out_s)), 20)
        unperm = [torch.empty_like(o) for o in out_s]

        def unpermute():
            for dst, src in zip(unperm, out_s):
                dst[order] = src
        row["sort_and_unpermute_ms"] = perm_t["ms"] + timed(unpermute, 20)["ms"]

        # the parent's way: one masked call per segment over that segment's users
        uniq, cnts = np.unique(seg_h, return_counts=True)
        ends = np.cumsum(cnts)
        groups = [(int(s), users_s[a:b].contiguous(), outputs(int(b - a)))
                  for s, a, b in zip(uniq, (ends - cnts).tolist(), ends.tolist())]

        def loop():
            for s, us, o in groups:
                be.recommend_topk_masked(allow=table[s], **common(us, o))
        row["loop"] = timed(loop, 3 if S >= 256 else 10)
        row["loop"]["launches"] = len(groups)

        loop_out = [torch.cat([g[2][j] for g in groups]) for j in range(3)]       # rows in sorted order
        for j in range(3):
            assert torch.equal(out_s[j], loop_out[j]), (S, kind, "fused_sorted != loop", j)
            assert torch.equal(unperm[j], out_f[j]), (S, kind, "fused != fused_sorted", j)
        row["checked_equal"] = True
        row["mean_list_length"] = float(out_f[2].float().mean().item())
        for name, seg_order in (("caller_order", row_seg), ("sorted", seg_s)):
            wave, wg = skip_shares(table, seg_order, 128)                 # N = 10: 128 rows per workgroup
            row[f"skipped_wave_chunks_{name}"] = wave
            row[f"empty_workgroup_chunks_{name}"] = wg
        row["loop_over_fused"] = row["loop"]["ms"] / row["fused"]["ms"]
        row["fused_over_floor"] = row["fused"]["ms"] / floor["ms"]
        row["sorted_over_fused"] = row["fused_sorted"]["ms"] / row["fused"]["ms"]
        res["runs"][f"S{S}_{kind}"] = row
        print(f"S{S}_{kind}", json.dumps(row), flush=True)
        del table, groups, loop_out

# ---- the builder at a production shape
NB, SB, TW = 1_000_000, 1000, 4
tags = torch.randint(-2 ** 31, 2 ** 31, (NB, TW), device=dev, generator=gen, dtype=torch.int64).to(torch.int32)
rules = [(torch.randint(-2 ** 31, 2 ** 31, (SB, TW), device=dev, generator=gen, dtype=torch.int64)
          & torch.randint(-2 ** 31, 2 ** 31, (SB, TW), device=dev, generator=gen, dtype=torch.int64)
          & torch.randint(-2 ** 31, 2 ** 31, (SB, TW), device=dev, generator=gen, dtype=torch.int64)
          & torch.randint(-2 ** 31, 2 ** 31, (SB, TW), device=dev, generator=gen, dtype=torch.int64)).to(torch.int32)
         for _ in range(3)]                                                 # about 8 of 128 attribute bits per rule
out = torch.empty(SB, (NB + 31) // 32, dtype=torch.int32, device=dev)
row = timed(lambda: be.eligibility_bitmaps(n=NB, item_tags=tags, need_all=rules[0] & rules[1], need_any=rules[1],
                                           forbid=rules[2], base_allow=None, out=out), 10)
row.update(items=NB, segments=SB, tag_words=TW, table_bytes=out.numel() * 4,
           write_GBps=out.numel() * 4 / row["ms"] / 1e6,
           allowed_share=float(sum(bin(int(w) & 0xFFFFFFFF).count("1") for w in out[:4].flatten().tolist())
                               / (4 * NB)))
res["builder"] = row
print("builder", row, flush=True)
res["clocks_after"] = clocks()
print(json.dumps(res))
if args:
    with open(args[0], "w") as f:
        json.dump(res, f, indent=1)
