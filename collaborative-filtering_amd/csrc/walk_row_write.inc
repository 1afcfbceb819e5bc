// Catalogue walk, end of the walk for the lambda-form row state (walk_row_lists.inc): the last compaction of every row
// of the wave and its final list - the raw keys of (slice, batch row) for the merge when the call is sliced, the
// outputs otherwise.  Included behind the chunk loop, as the kernel's last statements; plain statements, no parameters
// (DESIGN section 31).
//   expects  lane, b0 (first launched row of the wave), nusers, topn, kw, cnt[4], nlist[4], compact(r), readlane_i,
//            part, top_val, top_idx, top_cnt, key_score, key_index
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (int r = 0; r < 16; ++r) {
        int rc = 0, rn = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) rc = ((r & 3) == e) ? cnt[e] : rc;
        rc = readlane_i(rc, 16 * (r >> 2));
        if (rc > 0) compact(r);
#pragma unroll
        for (int e = 0; e < 4; ++e) rn = ((r & 3) == e) ? nlist[e] : rn;
        rn = readlane_i(rn, 16 * (r >> 2));
        const int64_t rb = b0 + r;
        if (rb >= nusers) continue;
        if (part) {                                      // sliced: raw keys of (slice, user), 0 = empty
            unsigned long long* dst = part + ((int64_t)blockIdx.y * nusers + rb) * topn;
            for (int t = lane; t < topn; t += 64) dst[t] = t < rn ? kw[r][t] : 0ull;
        } else {
            for (int t = lane; t < topn; t += 64) {
                const bool ok = t < rn;
                const unsigned long long key = ok ? kw[r][t] : 0ull;
                top_val[rb * topn + t] = ok ? key_score(key) : -INFINITY;
                top_idx[rb * topn + t] = ok ? key_index(key) : -1;
            }
            if (lane == 0) top_cnt[rb] = rn;
        }
    }
