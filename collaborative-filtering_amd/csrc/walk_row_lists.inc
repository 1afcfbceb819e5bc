// Catalogue walk, the per-row selection state of k_recommend and k_priced in its lambda form (topk_rows.hpp holds the
// same as functions, for the kernels whose streams that form does not move): lane (c, q) holds the state of the rows
// 4q + r; row R of the wave owns kw[R][0 .. CAP), the sorted list [0, L) and the survivor buffer [L, CAP).  Included in
// the kernel body behind the cursor set-up; plain statements, no parameters (DESIGN section 31).
//   expects  lane, q, topn, kw, readlane_i, and the constants CAP, L
//   defines  thr[4], cnt[4], nlist[4], compact(r)
    unsigned long long thr[4] = {0ull, 0ull, 0ull, 0ull};    // key of the current topn-th entry (0: list not full)
    int cnt[4] = {0, 0, 0, 0};                                // buffered survivors (same in the 16 lanes of a q group)
    int nlist[4] = {0, 0, 0, 0};                              // valid entries of the sorted list

    auto compact = [&](int r) {        // wave-uniform r: list + buffer of row r -> sorted list, new threshold
        const int rq = r >> 2, re = r & 3;
        int rc = 0, rn = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) { rc = (re == e) ? cnt[e] : rc; rn = (re == e) ? nlist[e] : rn; }
        rc = readlane_i(rc, 16 * rq);
        rn = readlane_i(rn, 16 * rq);
        unsigned long long k[CAP / 64];
#pragma unroll
        for (int v = 0; v < CAP / 64; ++v) {
            const int i = lane + 64 * v;
            const bool live = (i < rn) || (i >= L && i < L + rc);
            k[v] = live ? kw[r][i] : 0ull;
        }
        topk::sort_desc<CAP / 64>(k, lane);
#pragma unroll
        for (int v = 0; v < CAP / 64; ++v)
            if (lane + 64 * v < L) kw[r][lane + 64 * v] = k[v];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const int nn = min(topn, rn + rc);
        const unsigned long long t = (nn == topn) ? kw[r][topn - 1] : 0ull;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (q == rq && e == re) { thr[e] = t; cnt[e] = 0; nlist[e] = nn; }
    };
