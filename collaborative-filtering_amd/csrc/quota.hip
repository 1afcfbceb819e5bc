// K22: top-N with per-group caps inside each list (ALS.recommend_quota).
//
// Every item carries a group label (item_group[i] in [0, ngroups), anything else: no group, never capped) and every
// group a cap.  Row b's list is one scan of recommend's candidates in recommend's order (score descending, item
// ascending): a candidate is taken iff fewer than group_cap[g] taken items share its group, and the scan stops after
// topn taken items.  That scan is the greedy basis of a truncated partition matroid, so it survives streaming:
//   compaction  sort a row's (list + buffer), keep a key iff fewer than cap better keys of its group are in the sorted
//               set, cut after topn kept keys - a dropped key is in no later answer;
//   merge       the capped top-N of a union is the capped top-N of the union of the parts' capped lists.
// The threshold keeps its meaning - the key of the topn-th KEPT entry, 0 while fewer are kept - and the candidate test
// of the walk is k_recommend's, unchanged.
//
// k_quota<KB, NW, CAP, MASKED>: the walk of k_recommend (recommend.hip) - staging, prefetch, score tiles, seen cursors,
// bitmap skip: the walk_*.inc fragments that kernel includes, and its candidate test - with the
// per-row state of topk_rows.hpp and the capped compaction below in place of topk::compact.  A kernel of its own, as
// k_priced (capacity.hip) is, so that no existing kernel's stream changes; the text they have in common is one.
// k_quota_merge: topk::k_merge_slices with the capped filter after every fold, the last one included.
//
// The capped filter (capped_keep): the sorted keys are in registers, element i = lane + 64 v.  Each lane fetches the
// labels of its keys' items and those labels' caps, the labels go to a per-wave LDS strip of CAP ints, and the rank of
// a key within its group is counted by one pass over the live part of the strip (broadcast reads, four labels each):
// CAP^2 / 64 compares per lane, about what the bitonic sort in front of it costs.  No per-row group array exists.
// In front of the sort the unsorted keys' caps are looked up once (caps_can_bind): a set in which no cap is below topn
// is compacted as topk::compact does, without the filter.
#include "als_device.hpp"
#include "als_hip.h"
#include "catalogue_walk.hpp"
#include "topk_common.hpp"
#include "topk_launch.hpp"
#include "topk_rows.hpp"

namespace {

using topk::key_index;
using topk::key_score;
using topk::make_key;

constexpr int QC_WIDE = topk::ROWS_WIDE;
constexpr int QC_NARROW = topk::ROWS_NARROW;

typedef int i32x4 __attribute__((ext_vector_type(4)));

// k: 64 V keys sorted descending, element i = lane + 64 v, 0 = empty (behind every real key).  Returns bit v set =
// key v of this lane survives the caps: it is real and its item has no group, or fewer than the group's cap better
// keys of the same group are among the 64 V.  gw: this wave's strip of 64 V ints (16-byte aligned); wave-uniform call.
template <int V>
__device__ __forceinline__ unsigned capped_keep(const unsigned long long (&k)[V], int lane, int* __restrict__ gw,
                                                const int32_t* __restrict__ item_group,
                                                const int32_t* __restrict__ group_cap, int ngroups) {
    int g[V], cap[V], rank[V];
    int live = 0;
    bool grouped = false;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const bool real = k[v] != 0ull;
        live += __popcll(__ballot(real));
        int gi = real ? item_group[key_index(k[v])] : -1;
        gi = (gi >= 0 && gi < ngroups) ? gi : -1;
        g[v] = gi;
        grouped = grouped || gi >= 0;
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        cap[v] = g[v] >= 0 ? group_cap[g[v]] : 0;
        rank[v] = 0;
        gw[lane + 64 * v] = g[v];
    }
    if (__ballot(grouped)) {                             // wave-uniform: some key has a group
        wave_lds_sync();
        for (int j = 0; j < live; j += 4) {              // positions j ... j + 3: the same address in every lane
            const i32x4 gj = *reinterpret_cast<const i32x4*>(gw + j);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int i = lane + 64 * v;
                rank[v] += (gj.x == g[v] && j < i) + (gj.y == g[v] && j + 1 < i) + (gj.z == g[v] && j + 2 < i) +
                           (gj.w == g[v] && j + 3 < i);
            }
        }
        wave_lds_sync();                                 // the strip is free for the next call
    }
    unsigned keep = 0u;
#pragma unroll
    for (int v = 0; v < V; ++v)
        if (k[v] != 0ull && (g[v] < 0 || rank[v] < cap[v])) keep |= 1u << v;
    return keep;
}

// k: keys in any order, 0 = empty.  True in every lane iff some key's group has a cap below topn - the only caps that
// can change a list: a key with cap >= topn better keys of its group has topn kept keys in front of it and falls to
// the cut anyway.  Called in front of the sort, its two dependent loads run under the sort, and a compaction no cap can
// touch (loose caps, items without groups) skips capped_keep and its loads altogether.
template <int V>
__device__ __forceinline__ bool caps_can_bind(const unsigned long long (&k)[V], const int32_t* __restrict__ item_group,
                                              const int32_t* __restrict__ group_cap, int ngroups, int topn) {
    bool bind = false;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int gi = k[v] != 0ull ? item_group[key_index(k[v])] : -1;
        const bool in = gi >= 0 && gi < ngroups;
        bind = bind || (in && group_cap[in ? gi : 0] < topn);
    }
    return __ballot(bind) != 0ull;
}

// every real key kept: what capped_keep returns when no cap can bind
template <int V>
__device__ __forceinline__ unsigned keep_real(const unsigned long long (&k)[V]) {
    unsigned keep = 0u;
#pragma unroll
    for (int v = 0; v < V; ++v)
        if (k[v] != 0ull) keep |= 1u << v;
    return keep;
}

// position of every kept key among the kept ones, in key order; returns their number (wave-uniform)
template <int V>
__device__ __forceinline__ int kept_positions(unsigned keep, int lane, int (&pos)[V]) {
    int base = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const unsigned long long m = __ballot((keep >> v) & 1u);
        pos[v] = base + __popcll(m & ((1ull << lane) - 1ull));
        base += __popcll(m);
    }
    return base;
}

// topk::compact under the caps - wave-uniform R: list + buffer of row R -> the capped sorted list, new threshold
template <int CAP>
__device__ __forceinline__ void compact_capped(unsigned long long (*kw)[CAP], topk::Rows<CAP>& st, int R, int topn,
                                               int lane, int* __restrict__ gw,
                                               const int32_t* __restrict__ item_group,
                                               const int32_t* __restrict__ group_cap, int ngroups) {
    constexpr int L = topk::Rows<CAP>::L, V = CAP / 64;
    const int q = lane >> 4, rq = R >> 2, re = R & 3;
    const int rc = topk::row_cnt(st, R), rn = topk::row_nlist(st, R);
    unsigned long long k[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int i = lane + 64 * v;
        const bool live = (i < rn) || (i >= L && i < L + rc);
        k[v] = live ? kw[R][i] : 0ull;
    }
    const bool bind = caps_can_bind<V>(k, item_group, group_cap, ngroups, topn);
    topk::sort_desc<V>(k, lane);
    const unsigned keep = bind ? capped_keep<V>(k, lane, gw, item_group, group_cap, ngroups) : keep_real<V>(k);
    int pos[V];
    const int nn = min(topn, kept_positions<V>(keep, lane, pos));
#pragma unroll
    for (int v = 0; v < V; ++v)
        if (((keep >> v) & 1u) && pos[v] < topn) kw[R][pos[v]] = k[v];       // topn <= L
    wave_lds_sync();
    const unsigned long long t = (nn == topn) ? kw[R][topn - 1] : 0ull;
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (q == rq && e == re) { st.thr[e] = t; st.cnt[e] = 0; st.nlist[e] = nn; }
}

// CAP keys per user: list [0, L) + survivor buffer [L, CAP)
template <int KB, int NW, int CAP, bool MASKED>
__global__ __launch_bounds__(NW * 64)
void k_quota(int ld, int64_t nusers, const int32_t* __restrict__ users, int64_t n, int64_t slice,
             const float* __restrict__ U, const float* __restrict__ Z, const float* __restrict__ b_u,
             const float* __restrict__ b_i, const double* __restrict__ mu_p, const int64_t* __restrict__ seen_ptr,
             const int32_t* __restrict__ seen_idx, int topn, float* __restrict__ top_val,
             int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt, unsigned long long* __restrict__ part,
             const uint32_t* __restrict__ allow, const int32_t* __restrict__ item_group,
             const int32_t* __restrict__ group_cap, int ngroups) {
    constexpr int E = 4 * KB, LD = 16 * KB, ZS = walk::lds_row_stride(KB);
    constexpr int BUF = topk::Rows<CAP>::BUF;
    constexpr int NT = NW * 64, NV = walk::CHUNK * LD / 4, PF = (NV + NT - 1) / NT;
    __shared__ unsigned long long keys[NW * 16][CAP];
    __shared__ __attribute__((aligned(16))) float zs[walk::CHUNK][ZS];
    __shared__ __attribute__((aligned(16))) int groups[NW][CAP];       // the labels of the keys a wave is compacting

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const float mu = (float)(*mu_p);
    const int64_t b0 = ((int64_t)blockIdx.x * NW + wave) * 16;            // first batch row of this wave
    const int64_t lo = (int64_t)blockIdx.y * slice, hi = min(n, lo + slice);
    unsigned long long (*kw)[CAP] = keys + wave * 16;
    int* gw = groups[wave];

    float ua[E];
    load_frow<E>(U + (size_t)users[min(b0 + c, nusers - 1)] * ld + E * q, ua);
    float bu[4];
    bool valid[4];
    int64_t cur[4], end[4];
    int nxt[4];                                                          // next seen item of rows 4q + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t rb = b0 + 4 * q + r;
        valid[r] = rb < nusers;
        const int u = users[min(rb, nusers - 1)];
        bu[r] = b_u[u];
#include "walk_seen_cursor.inc"
    }
    topk::Rows<CAP> st;

    unsigned deny = 0u;     // MASKED: bit c set = item cb + c of the block `select` is called for is not allowed
    // one 16-item block [cb, cb + 16): scores from the accumulator, seen mask, threshold test, append
    auto select = [&](const f32x4& acc, int64_t cb) {
#include "walk_seen_masks.inc"
        if constexpr (MASKED) {
#pragma unroll
            for (int r = 0; r < 4; ++r) msk[r] |= deny;
        }
        const int64_t col = cb + c;
        const float bi = b_i[min(col, n - 1)];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float score = walk::score(acc[r], mu, bu[r], bi);
            const unsigned long long key = make_key(score, (unsigned)col);
            const bool pass = col < hi && valid[r] && !((msk[r] >> c) & 1u) && score == score && key > st.thr[r];
            topk::append<CAP>(kw, st, r, pass, key, c, q);
        }
    };

    f32x4 pf[PF];
    auto fetch = [&](int64_t it0) {
#include "walk_z_fetch.inc"
    };
    auto stage = [&]() {
#include "walk_z_stage.inc"
    };

#include "walk_allow_scan.inc"
    int64_t nx = 0;                                      // MASKED: the chunk after ch that is scored
    if constexpr (MASKED) {
        nx = next_chunk(0);
        if (nx < nch) { fetch(lo + nx * walk::CHUNK); window(nx + 1); }
    } else if (nch > 0) {
        fetch(lo);
    }
    for (int64_t ch = nx; ch < nch; ch = MASKED ? nx : ch + 1) {
        const int64_t it0 = lo + ch * walk::CHUNK;
        unsigned word = 0u;
        if constexpr (MASKED) word = __builtin_amdgcn_readfirstlane(aw[ch]);
        __syncthreads();                                 // every wave is done with the previous chunk
        stage();
        __syncthreads();
        if constexpr (MASKED) {
            nx = after(ch);
            if (nx < nch) { fetch(lo + nx * walk::CHUNK); window(nx + 1); }      // however far ahead
        } else if (ch + 1 < nch) {
            fetch(it0 + walk::CHUNK);
        }
#include "walk_score_tiles.inc"
        if constexpr (MASKED) deny = ~word & 0xFFFFu;
        select(acc0, it0);
        if constexpr (MASKED) deny = ~word >> 16;
        select(acc1, it0 + 16);
        bool full = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) full = full || st.cnt[r] > BUF - walk::CHUNK;
        if (__ballot(full)) {                            // some row's buffer could overflow in the next chunk
            wave_lds_sync();
            for (int R = 0; R < 16; ++R)
                if (topk::row_cnt(st, R) > BUF - walk::CHUNK)
                    compact_capped<CAP>(kw, st, R, topn, lane, gw, item_group, group_cap, ngroups);
        }
    }
    wave_lds_sync();
    for (int R = 0; R < 16; ++R) {
        if (topk::row_cnt(st, R) > 0) compact_capped<CAP>(kw, st, R, topn, lane, gw, item_group, group_cap, ngroups);
        const int rn = topk::row_nlist(st, R);
        const int64_t rb = b0 + R;
        if (rb >= nusers) continue;
        if (part) {                                      // sliced: raw keys of (slice, user), 0 = empty
            unsigned long long* dst = part + ((int64_t)blockIdx.y * nusers + rb) * topn;
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
}

// one wave per batch row: the nslices capped lists of (at most topn <= 128) keys folded left by 256-key sorts, the
// capped filter after every fold
__global__ __launch_bounds__(256)
void k_quota_merge(int64_t nrows, int nslices, int topn, const unsigned long long* __restrict__ part,
                   const int32_t* __restrict__ item_group, const int32_t* __restrict__ group_cap, int ngroups,
                   float* __restrict__ top_val, int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt) {
    __shared__ __attribute__((aligned(16))) int groups[4][256];
    __shared__ unsigned long long kept[4][ALS_TOPK_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t b = (int64_t)blockIdx.x * 4 + wave;
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
        const bool bind = caps_can_bind<4>(k, item_group, group_cap, ngroups, topn);
        topk::sort256_desc(k, lane);
        const unsigned keep = bind ? capped_keep<4>(k, lane, groups[wave], item_group, group_cap, ngroups)
                                   : keep_real<4>(k);
        int pos[4];
        const int nk = min(topn, kept_positions<4>(keep, lane, pos));
#pragma unroll
        for (int v = 0; v < 4; ++v)
            if (((keep >> v) & 1u) && pos[v] < topn) kept[wave][pos[v]] = k[v];
        wave_lds_sync();
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const int i = lane + 64 * v;
            k[v] = i < nk ? kept[wave][i] : 0ull;
        }
        wave_lds_sync();                                 // read before the next fold writes
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

template <int KB>
int launch_quota(int ld, int64_t nusers, const int32_t* users, int64_t n, int nsl, const float* U, const float* Z,
                 const float* b_u, const float* b_i, const double* mu, const int64_t* seen_ptr,
                 const int32_t* seen_idx, const uint32_t* allow, const int32_t* item_group, const int32_t* group_cap,
                 int ngroups, int topn, float* tv, int32_t* ti, int32_t* tc, unsigned long long* part,
                 hipStream_t st) {
    constexpr int NN = QC_NARROW / 16, NWD = QC_WIDE / 16;
    const auto narrow = allow ? k_quota<KB, NN, 128, true> : k_quota<KB, NN, 128, false>;
    const auto wide = allow ? k_quota<KB, NWD, 256, true> : k_quota<KB, NWD, 256, false>;
    return topk::launch_by_width(narrow, wide, topn, nusers, nsl, st, ld, nusers, users, n, walk::slice_items(n, nsl),
                                 U, Z, b_u, b_i, mu, seen_ptr, seen_idx, topn, tv, ti, tc, part, allow, item_group,
                                 group_cap, ngroups);
}

}  // namespace

extern "C" int als_recommend_topk_quota(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                                        const float* Z, const float* b_u, const float* b_i, const double* mu,
                                        const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow,
                                        const int32_t* item_group, const int32_t* group_cap, int64_t ngroups, int topn,
                                        int nslices, float* top_val, int32_t* top_idx, int32_t* top_cnt,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    const int bad = topk::check_shape(k, ld, nusers, n, topn, ALS_TOPK_MAX, nslices);
    if (bad || ngroups < 0 || ngroups >= ((int64_t)1 << 31)) return bad ? bad : ALS_E_BADARG;
    if (nusers == 0) return 0;
    if (!users || !U || !Z || !b_u || !b_i || !mu || !item_group || (ngroups > 0 && !group_cap) || !top_val ||
        !top_idx || !top_cnt || (!seen_ptr != !seen_idx))
        return ALS_E_BADARG;
    const topk::SlicePlan p = topk::plan(nusers, topk::rows_per_wg(topn), n, nslices, nusers * topn,
                                         sizeof(unsigned long long), workspace, workspace_bytes);
    if (!p.nsl) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const int ng = (int)ngroups;
    int rc;
    ALS_DISPATCH_KB(ld / 16, rc = launch_quota<KB>(ld, nusers, users, n, p.nsl, U, Z, b_u, b_i, mu, seen_ptr, seen_idx,
                                                   allow, item_group, group_cap, ng, topn, top_val, top_idx, top_cnt,
                                                   p.keys(), st));
    if (rc != 0 || p.nsl == 1) return rc;
    hipLaunchKernelGGL(k_quota_merge, dim3((unsigned)((nusers + 3) / 4)), dim3(256), 0, st, nusers, p.nsl, topn,
                       p.keys(), item_group, group_cap, ng, top_val, top_idx, top_cnt);
    return topk::launch_status();
}
