// Per-row selection state of a wave that serves 16 batch rows of a catalogue walk, and the merge of per-slice lists:
// what k_recommend (recommend.hip) keeps in lambdas, in function form.  k_similar, k_audience and k_quota use the
// per-row state; k_group and k_explore keep one list per wave and use the merge alone, as do recommend.hip and
// capacity.hip, whose kernels keep the lambda form of the state - one text as well, the fragments walk_row_lists.inc,
// walk_row_overflow.inc and walk_row_write.inc (catalogue_walk.hpp says why: the function form moved their register
// allocation).  The merge is launched by topk::merge_slices below, with the slice plan of topk_launch.hpp.
//
// Layout: lane (c, q) = (lane & 15, lane >> 4) holds the state of the rows 4q + r, r = 0 ... 3, the same value in the 16
// lanes of a q group; row R of the wave owns kw[R][0 .. CAP): the sorted list [0, L) and the survivor buffer
// [L, CAP) of 64-bit keys (topk_common.hpp).  A candidate above its row's threshold (the key of the current topn-th
// entry, 0 while the list is not full) is appended to the buffer - ballot + prefix popcount -, and a row whose buffer
// could overflow in the next chunk of 32 candidates is compacted by a bitonic sort of (list + buffer).
#pragma once
#include "als_device.hpp"
#include "topk_common.hpp"
#include "topk_launch.hpp"

namespace topk {

template <int CAP>
struct Rows {
    static constexpr int L = CAP == 256 ? 128 : 32, BUF = CAP - L;
    static_assert(L >= 32 && BUF >= 64, "a chunk appends up to 32 keys per row");
    unsigned long long thr[4] = {0ull, 0ull, 0ull, 0ull};    // key of the current topn-th entry (0: list not full)
    int cnt[4] = {0, 0, 0, 0};                                // buffered survivors
    int nlist[4] = {0, 0, 0, 0};                              // valid entries of the sorted list
};

// st.cnt / st.nlist of the wave-uniform row R, read from the q group that holds it
template <int CAP>
__device__ __forceinline__ int row_cnt(const Rows<CAP>& st, int R) {
    int v = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) v = ((R & 3) == e) ? st.cnt[e] : v;
    return __builtin_amdgcn_readlane(v, 16 * (R >> 2));
}
template <int CAP>
__device__ __forceinline__ int row_nlist(const Rows<CAP>& st, int R) {
    int v = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) v = ((R & 3) == e) ? st.nlist[e] : v;
    return __builtin_amdgcn_readlane(v, 16 * (R >> 2));
}

// the 16 candidates of row 4q + r of one 16-column block (lane c holds column c's): those that pass go to the buffer
template <int CAP>
__device__ __forceinline__ void append(unsigned long long (*kw)[CAP], Rows<CAP>& st, int r, bool pass,
                                       unsigned long long key, int c, int q) {
    const unsigned long long m = __ballot(pass);
    const unsigned sub = (unsigned)(m >> (16 * q)) & 0xFFFFu;
    if (pass) kw[4 * q + r][Rows<CAP>::L + st.cnt[r] + __popc(sub & ((1u << c) - 1u))] = key;
    st.cnt[r] += __popc(sub);
}

// wave-uniform R: list + buffer of row R -> sorted list, new threshold
template <int CAP>
__device__ __forceinline__ void compact(unsigned long long (*kw)[CAP], Rows<CAP>& st, int R, int topn, int lane) {
    constexpr int L = Rows<CAP>::L;
    const int q = lane >> 4, rq = R >> 2, re = R & 3;
    const int rc = row_cnt(st, R), rn = row_nlist(st, R);
    unsigned long long k[CAP / 64];
#pragma unroll
    for (int v = 0; v < CAP / 64; ++v) {
        const int i = lane + 64 * v;
        const bool live = (i < rn) || (i >= L && i < L + rc);
        k[v] = live ? kw[R][i] : 0ull;
    }
    sort_desc<CAP / 64>(k, lane);
#pragma unroll
    for (int v = 0; v < CAP / 64; ++v)
        if (lane + 64 * v < L) kw[R][lane + 64 * v] = k[v];
    wave_lds_sync();
    const int nn = min(topn, rn + rc);
    const unsigned long long t = (nn == topn) ? kw[R][topn - 1] : 0ull;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (q == rq && e == re) { st.thr[e] = t; st.cnt[e] = 0; st.nlist[e] = nn; }
}

// after a chunk: compact every row whose buffer could overflow in the next one
template <int CAP>
__device__ __forceinline__ void compact_full_rows(unsigned long long (*kw)[CAP], Rows<CAP>& st, int topn, int lane) {
    constexpr int LIMIT = Rows<CAP>::BUF - 32;
    bool full = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) full = full || st.cnt[r] > LIMIT;
    if (__ballot(full)) {
        wave_lds_sync();
        for (int R = 0; R < 16; ++R)
            if (row_cnt(st, R) > LIMIT) compact(kw, st, R, topn, lane);
    }
}

// end of the walk: the final list of the wave-uniform row R.  part != NULL: the raw keys of (slice, batch row), 0 =
// empty, for merge_slices; otherwise the outputs of batch row rb.
template <int CAP>
__device__ __forceinline__ void finish_row(unsigned long long (*kw)[CAP], Rows<CAP>& st, int R, int topn, int lane,
                                           int64_t rb, int64_t nrows, int64_t slice_index,
                                           unsigned long long* __restrict__ part, float* __restrict__ top_val,
                                           int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt) {
    if (row_cnt(st, R) > 0) compact(kw, st, R, topn, lane);
    const int rn = row_nlist(st, R);
    if (rb >= nrows) return;
    if (part) {
        unsigned long long* dst = part + (slice_index * nrows + rb) * topn;
        for (int t = lane; t < topn; t += 64) dst[t] = t < rn ? kw[R][t] : 0ull;
    } else {
        for (int t = lane; t < topn; t += 64) {
            const bool ok = t < rn;
            const unsigned long long key = ok ? kw[R][t] : 0ull;
            top_val[rb * topn + t] = ok ? key_score(key) : -INFINITY;
            top_idx[rb * topn + t] = ok ? key_index(key) : -1;
        }
        if (lane == 0) top_cnt[rb] = rn;
    }
}

// one wave per batch row: the nslices lists of (at most topn <= 128) keys folded into one by 256-key sorts
static __global__ __launch_bounds__(256)
void k_merge_slices(int64_t nrows, int nslices, int topn, const unsigned long long* __restrict__ part,
                    float* __restrict__ top_val, int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= nrows) return;                              // wave-uniform
    unsigned long long k[4];
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int i = lane + 64 * v;
        k[v] = i < topn ? part[b * topn + i] : 0ull;
    }
    for (int s = 1; s < nslices; ++s) {
        const unsigned long long* src = part + ((int64_t)s * nrows + b) * topn;
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int i = lane + 64 * v;
            k[2 + v] = i < topn ? src[i] : 0ull;
        }
        sort256_desc(k, lane);                           // elements 0 ... 127 (k[0], k[1]) hold the best 128
    }
    int cnt = 0;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const int i = lane + 64 * v;
        const bool ok = i < topn && k[v] != 0ull;
        cnt += __popcll(__ballot(ok));
        if (i < topn) {
            top_val[b * topn + i] = ok ? key_score(k[v]) : -INFINITY;
            top_idx[b * topn + i] = ok ? key_index(k[v]) : -1;
        }
    }
    if (lane == 0) top_cnt[b] = cnt;
}

// host: the lists of nsl slices (raw keys in `part`) folded into the outputs; nothing to do with one slice.  Here and
// not in topk_launch.hpp: a file that sees this launch emits the kernel, and rank_eval.hip has no use for it
inline int merge_slices(int nsl, const unsigned long long* part, int64_t nrows, int topn, float* top_val,
                        int32_t* top_idx, int32_t* top_cnt, hipStream_t st) {
    if (nsl == 1) return 0;
    hipLaunchKernelGGL(k_merge_slices, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, nrows, nsl, topn, part,
                       top_val, top_idx, top_cnt);
    return launch_status();
}

}  // namespace topk
