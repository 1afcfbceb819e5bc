// K21: batch top-N under per-item exposure caps (ALS.recommend_capacity) - the two device pieces of
// the threshold rounds: the priced walk and the settle pass.
//
// Item-side keys.  The pair (batch row b, item i) with score s has the ITEM-SIDE key make_key(s, b): the encoding of the
// item keys (topk_common.hpp) with the batch row in the index word, so one item's demanders are ordered by (score
// descending, row ascending) and their keys are distinct.  Every item has a 64-bit floor (0: none); a pair is a
// candidate only while its item-side key is >= the floor of its item.
//
// k_priced (als_recommend_topk_priced): k_recommend (recommend.hip) with that one more term in the candidate test.  It
// is a kernel of its own, because a further template parameter of k_recommend has to leave the instruction streams of
// its 60 existing instances as they are, and two more kernel arguments do not promise that - but not a copy: the walk
// and the row state are the walk_*.inc fragments k_recommend includes, and only what differs is
// written here, around the includes.  What differs from k_recommend<KB, NW, CAP, MASKED>: row_ids (the batch row of
// every launched row: a compacted work list keeps its rows' priorities) and floor_key; the floors of a chunk's 32 items
// are per-column data like b_i and travel with the chunk - lane (c, q) fetches the floors of items c and 16 + c of the
// next chunk behind the Z prefetch and takes them over when the chunk is staged.  Slices, raw-key workspace and merge
// are the family's (topk_launch.hpp, topk::merge_slices).  With all floors 0 the kernel is k_recommend:
// make_key(...) >= 0 always holds.
//
// Settle (als_capacity_settle): from the batch's lists to per-item demand, new floors, dirty rows - six launches on
// the caller's stream, no host synchronisation, nothing allocated:
//   k_settle_zero     demand counts, bucket cursors, dirty flags and the two global counters to 0;
//   k_settle_count    one global integer atomic per list entry: cnt[i] = d_i;
//   k_settle_alloc    per item: fill = min(d, capacity); an over-demanded item (d > capacity) takes a place in the list
//                     of over-demanded items and a bucket of d keys (two returning atomics on global cursors);
//   k_settle_scatter  every entry of an over-demanded item drops its item-side key into the item's bucket;
//   k_settle_select   a workgroup per over-demanded item: the capacity-th largest of the bucket's d keys by a radix select
//                     (eight passes of 8 bits from the top, a 256-bin LDS histogram each) becomes the item's floor;
//   k_settle_dirty    a row holding an entry whose key is below its item's floor is flagged.
// Integer atomics only: the counts are sums, the places in the over list and in the buckets depend on arrival order but
// are read as sets (the select does not depend on the order of its keys), so floors, dirty flags, fill and n_over are
// the same on every run.
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

constexpr int PC_WIDE = topk::ROWS_WIDE;
constexpr int PC_NARROW = topk::ROWS_NARROW;

__device__ __forceinline__ int readlane_i(int v, int src_lane) { return __builtin_amdgcn_readlane(v, src_lane); }

// CAP keys per user: list [0, L) + survivor buffer [L, CAP)
template <int KB, int NW, int CAP, bool MASKED>
__global__ __launch_bounds__(NW * 64)
void k_priced(int ld, int64_t nusers, const int32_t* __restrict__ users, const int32_t* __restrict__ row_ids, int64_t n,
              int64_t slice, const float* __restrict__ U, const float* __restrict__ Z, const float* __restrict__ b_u,
              const float* __restrict__ b_i, const double* __restrict__ mu_p, const int64_t* __restrict__ seen_ptr,
              const int32_t* __restrict__ seen_idx, int topn, float* __restrict__ top_val,
              int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt, unsigned long long* __restrict__ part,
              const uint32_t* __restrict__ allow, const unsigned long long* __restrict__ floor_key) {
    constexpr int E = 4 * KB, LD = 16 * KB, ZS = walk::lds_row_stride(KB);
    constexpr int L = CAP == 256 ? 128 : 32, BUF = CAP - L;
    constexpr int NT = NW * 64, NV = walk::CHUNK * LD / 4, PF = (NV + NT - 1) / NT;
    static_assert(L >= 32 && BUF >= 64, "a chunk appends up to 32 keys per row");
    __shared__ unsigned long long keys[NW * 16][CAP];
    __shared__ __attribute__((aligned(16))) float zs[walk::CHUNK][ZS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const float mu = (float)(*mu_p);
    const int64_t b0 = ((int64_t)blockIdx.x * NW + wave) * 16;            // first launched row of this wave
    const int64_t lo = (int64_t)blockIdx.y * slice, hi = min(n, lo + slice);
    unsigned long long (*kw)[CAP] = keys + wave * 16;

    float ua[E];
    load_frow<E>(U + (size_t)users[min(b0 + c, nusers - 1)] * ld + E * q, ua);
    float bu[4];
    bool valid[4];
    int64_t cur[4], end[4];
    int nxt[4];                                                          // next seen item of rows 4q + r
    unsigned rid[4];                                                     // batch row of rows 4q + r: the item-side index
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t rb = b0 + 4 * q + r;
        valid[r] = rb < nusers;
        const int u = users[min(rb, nusers - 1)];
        bu[r] = b_u[u];
        rid[r] = (unsigned)row_ids[min(rb, nusers - 1)];
#include "walk_seen_cursor.inc"
    }
#include "walk_row_lists.inc"

    unsigned deny = 0u;     // MASKED: bit c set = item cb + c of the block `select` is called for is not allowed
    // one 16-item block [cb, cb + 16): scores from the accumulator, seen mask, threshold and floor test, append;
    // fl: the floor of item cb + c
    auto select = [&](const f32x4& acc, int64_t cb, unsigned long long fl) {
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
            const bool pass = col < hi && valid[r] && !((msk[r] >> c) & 1u) && score == score && key > thr[r] &&
                              make_key(score, rid[r]) >= fl;
            const unsigned long long m = __ballot(pass);
            const unsigned sub = (unsigned)(m >> (16 * q)) & 0xFFFFu;
            if (pass) kw[4 * q + r][L + cnt[r] + __popc(sub & ((1u << c) - 1u))] = key;
            cnt[r] += __popc(sub);
        }
    };

    f32x4 pf[PF];
    unsigned long long pfl[2] = {0ull, 0ull}, fl[2] = {0ull, 0ull};      // floors of items c and 16 + c: prefetched, current
    auto fetch = [&](int64_t it0) {
#include "walk_z_fetch.inc"
        pfl[0] = floor_key[min(it0 + c, n - 1)];
        pfl[1] = floor_key[min(it0 + 16 + c, n - 1)];
    };
    auto stage = [&]() {
#include "walk_z_stage.inc"
        fl[0] = pfl[0];
        fl[1] = pfl[1];
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
        const unsigned long long f0 = fl[0], f1 = fl[1];  // this chunk's floors, before the prefetch's are taken over
        if constexpr (MASKED) deny = ~word & 0xFFFFu;
        select(acc0, it0, f0);
        if constexpr (MASKED) deny = ~word >> 16;
        select(acc1, it0 + 16, f1);
#include "walk_row_overflow.inc"
    }
#include "walk_row_write.inc"
}

template <int KB>
int launch_priced(int ld, int64_t nusers, const int32_t* users, const int32_t* row_ids, int64_t n, int nsl,
                  const float* U, const float* Z, const float* b_u, const float* b_i, const double* mu,
                  const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow,
                  const unsigned long long* floor_key, int topn, float* tv, int32_t* ti, int32_t* tc,
                  unsigned long long* part, hipStream_t st) {
    constexpr int NN = PC_NARROW / 16, NWD = PC_WIDE / 16;
    const auto narrow = allow ? k_priced<KB, NN, 128, true> : k_priced<KB, NN, 128, false>;
    const auto wide = allow ? k_priced<KB, NWD, 256, true> : k_priced<KB, NWD, 256, false>;
    return topk::launch_by_width(narrow, wide, topn, nusers, nsl, st, ld, nusers, users, row_ids, n,
                                 walk::slice_items(n, nsl), U, Z, b_u, b_i, mu, seen_ptr, seen_idx, topn, tv, ti, tc,
                                 part, allow, floor_key);
}

// ------------------------------------------------------------------------------------------------------ settle
constexpr int ST_THREADS = 256;
constexpr int ST_SELECT_GRID = 2048;       // workgroups of k_settle_select: they stride over the over-demanded items

// the workspace: four int32 [n] arrays, the two counters' word, the buckets [nrows * topn] keys
struct SettleWs {
    int32_t *cnt, *cursor, *off, *over;
    int32_t* alloc;
    unsigned long long* bucket;
};
inline size_t settle_ints(int64_t n) { return ((size_t)4 * (size_t)n + 4 + 1) / 2 * 2; }     // even: the keys stay 8-byte aligned
inline SettleWs settle_ws(void* workspace, int64_t n) {
    int32_t* w = (int32_t*)workspace;
    return SettleWs{w, w + n, w + 2 * n, w + 3 * n, w + 4 * n, (unsigned long long*)(w + settle_ints(n))};
}

__global__ __launch_bounds__(ST_THREADS)
void k_settle_zero(int64_t n, int64_t nrows, int32_t* __restrict__ cnt, int32_t* __restrict__ cursor,
                   int32_t* __restrict__ alloc, int32_t* __restrict__ dirty, int32_t* __restrict__ n_over) {
    const int64_t t = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (t < n) { cnt[t] = 0; cursor[t] = 0; }
    if (t < nrows) dirty[t] = 0;
    if (t == 0) { *alloc = 0; *n_over = 0; }
}

// an entry of the lists that names an item: anything else (-1, or an id outside [0, n)) is an empty slot
__device__ __forceinline__ bool settle_entry(int32_t i, int64_t n) { return i >= 0 && i < n; }

__global__ __launch_bounds__(ST_THREADS)
void k_settle_count(int64_t pairs, int64_t n, const int32_t* __restrict__ top_idx, int32_t* __restrict__ cnt) {
    const int64_t p = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (p >= pairs) return;
    const int32_t i = top_idx[p];
    if (settle_entry(i, n)) atomicAdd(&cnt[i], 1);
}

__global__ __launch_bounds__(ST_THREADS)
void k_settle_alloc(int64_t n, const int32_t* __restrict__ capacity, const int32_t* __restrict__ cnt,
                    int32_t* __restrict__ fill, int32_t* __restrict__ off, int32_t* __restrict__ over,
                    int32_t* __restrict__ alloc, int32_t* __restrict__ n_over) {
    const int64_t i = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n) return;
    const int32_t d = cnt[i], c = max(capacity[i], 0);
    fill[i] = min(d, c);
    if (d > c) {
        over[atomicAdd(n_over, 1)] = (int32_t)i;          // at most n places
        off[i] = atomicAdd(alloc, d);                     // the demands add up to at most nrows * topn
    }
}

__global__ __launch_bounds__(ST_THREADS)
void k_settle_scatter(int64_t pairs, int topn, int64_t n, const int32_t* __restrict__ top_idx,
                      const float* __restrict__ top_val, const int32_t* __restrict__ capacity,
                      const int32_t* __restrict__ cnt, const int32_t* __restrict__ off, int32_t* __restrict__ cursor,
                      unsigned long long* __restrict__ bucket) {
    const int64_t p = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (p >= pairs) return;
    const int32_t i = top_idx[p];
    if (!settle_entry(i, n) || cnt[i] <= max(capacity[i], 0)) return;
    const int32_t slot = atomicAdd(&cursor[i], 1);        // < cnt[i]: the same entries were counted
    bucket[(int64_t)off[i] + slot] = make_key(top_val[p], (unsigned)(p / topn));
}

// floor of every over-demanded item = the c-th largest of its d bucket keys (c = capacity < d; c = 0: ~0, nothing
// passes).  MSB-first radix select: `prefix` holds the bytes decided so far, `rank` what is left of c among the keys
// that share them.  Per pass the bin b with  sum(hist[b' > b]) < rank <= sum(hist[b' >= b])  is the next byte.
__global__ __launch_bounds__(ST_THREADS)
void k_settle_select(const int32_t* __restrict__ n_over, const int32_t* __restrict__ over,
                     const int32_t* __restrict__ capacity, const int32_t* __restrict__ cnt,
                     const int32_t* __restrict__ off, const unsigned long long* __restrict__ bucket,
                     unsigned long long* __restrict__ floor_key) {
    __shared__ unsigned hist[256];
    __shared__ unsigned wtot[ST_THREADS / 64];
    __shared__ unsigned pick[2];                          // the chosen bin, the rank inside it
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nov = *n_over;
    for (int j = blockIdx.x; j < nov; j += gridDim.x) {   // workgroup-uniform
        const int32_t i = over[j];
        const int32_t d = cnt[i], c = max(capacity[i], 0);
        if (c == 0) {
            if (tid == 0) floor_key[i] = ~0ull;
            continue;
        }
        const unsigned long long* keys = bucket + off[i];
        unsigned long long prefix = 0ull;
        unsigned rank = (unsigned)c;
        for (int shift = 56; shift >= 0; shift -= 8) {
            const unsigned long long himask = shift == 56 ? 0ull : ~0ull << (shift + 8);
            hist[tid] = 0u;
            __syncthreads();
            for (int t = tid; t < d; t += ST_THREADS) {
                const unsigned long long key = keys[t];
                if ((key & himask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            // suffix sums over the 256 bins: within the wave by shuffles, across the four waves through wtot
            const unsigned h = hist[tid];
            unsigned s = h;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_down(s, o, 64);
                if (lane + o < 64) s += up;
            }
            if (lane == 0) wtot[wave] = s;
            __syncthreads();
            for (int w = wave + 1; w < ST_THREADS / 64; ++w) s += wtot[w];
            if (s >= rank && s - h < rank) { pick[0] = (unsigned)tid; pick[1] = rank - (s - h); }
            __syncthreads();
            prefix |= (unsigned long long)pick[0] << shift;
            rank = pick[1];
        }
        if (tid == 0) floor_key[i] = prefix;
    }
}

__global__ __launch_bounds__(ST_THREADS)
void k_settle_dirty(int64_t pairs, int topn, int64_t n, const int32_t* __restrict__ top_idx,
                    const float* __restrict__ top_val, const unsigned long long* __restrict__ floor_key,
                    int32_t* __restrict__ dirty) {
    const int64_t p = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (p >= pairs) return;
    const int32_t i = top_idx[p];
    if (!settle_entry(i, n)) return;
    const int64_t b = p / topn;
    if (make_key(top_val[p], (unsigned)b) < floor_key[i]) dirty[b] = 1;      // every writer stores the same value
}

}  // namespace

extern "C" int als_recommend_topk_priced(int k, int ld, int64_t nusers, const int32_t* users, int64_t n,
                                         const float* U, const float* Z, const float* b_u, const float* b_i,
                                         const double* mu, const int64_t* seen_ptr, const int32_t* seen_idx,
                                         const uint32_t* allow, const int32_t* row_ids,
                                         const unsigned long long* floor_key, int topn, int nslices, float* top_val,
                                         int32_t* top_idx, int32_t* top_cnt, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    const int bad = topk::check_shape(k, ld, nusers, n, topn, ALS_TOPK_MAX, nslices);
    if (bad) return bad;
    if (nusers == 0) return 0;
    if (!users || !row_ids || !U || !Z || !b_u || !b_i || !mu || !floor_key || !top_val || !top_idx || !top_cnt ||
        (!seen_ptr != !seen_idx))
        return ALS_E_BADARG;
    const topk::SlicePlan p = topk::plan(nusers, topk::rows_per_wg(topn), n, nslices, nusers * topn,
                                         sizeof(unsigned long long), workspace, workspace_bytes);
    if (!p.nsl) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    ALS_DISPATCH_KB(ld / 16, rc = launch_priced<KB>(ld, nusers, users, row_ids, n, p.nsl, U, Z, b_u, b_i, mu, seen_ptr,
                                                    seen_idx, allow, floor_key, topn, top_val, top_idx, top_cnt,
                                                    p.keys(), st));
    return rc != 0 ? rc : topk::merge_slices(p.nsl, p.keys(), nusers, topn, top_val, top_idx, top_cnt, st);
}

extern "C" size_t als_capacity_settle_workspace_bytes(int64_t nrows, int64_t n, int topn) {
    if (nrows < 0 || nrows >= ((int64_t)1 << 31) || n <= 0 || n >= ((int64_t)1 << 31) || topn < 1 ||
        nrows * topn >= ((int64_t)1 << 31))
        return 0;
    return settle_ints(n) * sizeof(int32_t) + (size_t)nrows * (size_t)topn * sizeof(unsigned long long);
}

extern "C" int als_capacity_settle(int64_t nrows, int topn, int64_t n, const int32_t* top_idx, const float* top_val,
                                   const int32_t* capacity, unsigned long long* floor_key, int32_t* fill,
                                   int32_t* dirty, int32_t* n_over, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    if (nrows < 0 || n < 1 || n >= ((int64_t)1 << 31) || topn < 1 || nrows >= ((int64_t)1 << 31) ||
        nrows * topn >= ((int64_t)1 << 31))
        return ALS_E_BADARG;
    if (!capacity || !floor_key || !fill || !n_over || (nrows > 0 && (!top_idx || !top_val || !dirty))) return ALS_E_BADARG;
    const size_t need = als_capacity_settle_workspace_bytes(nrows, n, topn);
    if (!workspace || workspace_bytes < need) return ALS_E_BADARG;
    const SettleWs w = settle_ws(workspace, n);
    hipStream_t st = (hipStream_t)stream;
    const int64_t pairs = nrows * topn;
    const auto blocks = [](int64_t work) { return dim3((unsigned)((work + ST_THREADS - 1) / ST_THREADS)); };
    const dim3 th(ST_THREADS);
    hipLaunchKernelGGL(k_settle_zero, blocks(max(n, nrows)), th, 0, st, n, nrows, w.cnt, w.cursor, w.alloc, dirty, n_over);
    if (pairs > 0) hipLaunchKernelGGL(k_settle_count, blocks(pairs), th, 0, st, pairs, n, top_idx, w.cnt);
    hipLaunchKernelGGL(k_settle_alloc, blocks(n), th, 0, st, n, capacity, w.cnt, fill, w.off, w.over, w.alloc, n_over);
    if (pairs > 0) {
        hipLaunchKernelGGL(k_settle_scatter, blocks(pairs), th, 0, st, pairs, topn, n, top_idx, top_val, capacity, w.cnt,
                           w.off, w.cursor, w.bucket);
        hipLaunchKernelGGL(k_settle_select, dim3((unsigned)min((int64_t)ST_SELECT_GRID, n)), th, 0, st, n_over, w.over,
                           capacity, w.cnt, w.off, w.bucket, floor_key);
        hipLaunchKernelGGL(k_settle_dirty, blocks(pairs), th, 0, st, pairs, topn, n, top_idx, top_val, floor_key, dirty);
    }
    return topk::launch_status();
}
