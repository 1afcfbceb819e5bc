// K8: top-N recommendation - score(u, i) = U_u.Z_i + mu + b_u + b_i over all items, the user's seen items left
// out, the N best kept per user - without forming the m x n completion.
//
// k_recommend: one workgroup serves NW * 16 users (one 16-user tile per wave) over the items [lo, hi) of one slice.
// The items are walked in chunks of 32: the workgroup stages the chunk's Z rows in LDS once (global loads of the
// next chunk are in flight while the current one is scored), and every wave forms its two 16 x 16 score tiles with
// the SAME v_mfma_f32_16x16x4_f32 chain and epilogue as k_predict_dense (lane (c, q) holds k = 4KB q + e of user
// row c and item row c in step e; ((acc + mu) + b_u) + b_i), so every score is bitwise the value
// als_predict_dense writes.  Z is therefore read from L2 / MALL once per NW * 16 users.
//
// Selection is k_topk_sim's (topk_common.hpp): each candidate is a 64-bit key ordered by (score desc, item asc);
// a candidate above its row's threshold (the current N-th key) is appended - ballot + prefix popcount - to the
// row's survivor buffer in LDS, and a row whose buffer could overflow is compacted by a bitonic sort of
// (list + buffer).  Seen items never reach a buffer: each row keeps a cursor into its ascending seen list and the
// next seen item; only a chunk that reaches that item builds a 16-bit seen mask for the block (one coalesced load
// of the next 16 seen entries by the row's 16 lanes and an OR-reduction).
//
// Item split: with few users (a batch of 1 ... 1000 fills a fraction of the CUs) the item range is cut into
// nslices slices (grid.y); each workgroup writes its per-(slice, user) list as raw keys to the workspace, and
// topk::k_merge_slices (topk_rows.hpp) merges the lists of every user with the same 256-key sort.  The order is
// total, so the result does not depend on the slice count.  The host side of the entry points - argument checks,
// slice plan, workspace, merge launch - is topk_launch.hpp's.
//
// Allow bitmap (als_recommend_topk_masked; the MASKED instantiations): slices start at multiples of 32, so chunk ch
// of a slice is word lo / 32 + ch of the bitmap - one wave-uniform word per chunk.  Its low half joins block 0's
// pass test, its high half block 1's.  A chunk whose word is 0 is never fetched, staged or scored: every wave finds
// the next chunk with a set bit by the same scan (64 words per step: one per lane, ballot, count trailing zeros),
// so the workgroup's barriers stay matched and the prefetch goes to the chunk that is scored next.  The seen cursors
// catch up on their own: the exclusion walk consumes every entry below the block it is asked about.  The unmasked
// instantiations contain none of this: they are the code they were before the bitmap existed.
//
// Ceilings (als_recommend_deep, recommend_deep.hip; the DEEP instantiations): every (slice, user) has a ceiling key in
// ceil[slice * nusers + b], and a candidate passes only when its key is BELOW it as well as above the threshold - ~0
// is no ceiling, 0 closes the slice for the user.  A workgroup none of whose 64 users is open for its slice returns
// before the first barrier (every wave reads the same 64 ceilings, one per lane, so the decision is the workgroup's),
// as does every workgroup of a round whose predecessor raised no flag (*go == 0).  The lists always go to the workspace
// as raw keys, 128 per (slice, user).  The walk itself is untouched, and so is k_rank_count's: the ceiling is one
// more term of the candidate test, which k_rank_count does not have.  The instantiations without DEEP contain none of
// this: their instruction streams are those of the kernel without the parameter.
//
// Eligibility table (als_recommend_topk_segmented; the SEG instantiations): `allow` is then nseg rows of the bitmap,
// seg_stride words apart, and batch row b reads row row_seg[b] - the deny word is per row, not per wave.  A lane (c, q)
// keeps the int64 offsets of its rows 4q + r and loads their four words of the next chunk behind the Z prefetch (word
// lo / 32 + ch of each row; 0 for a row past the batch or with a segment id outside [0, nseg)).  The low halves join
// msk[r] for block 0, the high halves for block 1.  No chunk is skipped by the workgroup - its rows disagree about
// which are empty -, but a wave none of whose 16 rows has a set bit in the chunk forms no scores and selects nothing:
// it stages its share and passes both barriers, so they stay matched.  The seen cursors catch up as under MASKED.
// SEG is combined with neither MASKED nor DEEP, and the other instantiations contain none of it.
//
// The walk has one text: the walk_*.inc fragments included below at their points of use - cursor
// set-up, exclusion walk, Z fetch / stage, bitmap scan, score tiles, and the row state with its compaction and
// write-out - are the same files k_rank_count (rank_eval.hip), k_priced (capacity.hip) and k_quota (quota.hip) include,
// so an edit to a fragment is an edit to all of them.  What is this kernel's own stays here: the DEEP / SEG lines, the
// candidate test, the chunk loop.  catalogue_walk.hpp says why the pieces are included text and not functions.
#include "als_device.hpp"
#include "als_hip.h"
#include "catalogue_walk.hpp"
#include "recommend_deep.hpp"
#include "topk_common.hpp"
#include "topk_launch.hpp"
#include "topk_rows.hpp"

namespace {

using topk::key_index;
using topk::key_score;
using topk::make_key;

constexpr int RC_WIDE = topk::ROWS_WIDE;         // users per workgroup, topn > 32: 4 waves, 256 keys per user
constexpr int RC_NARROW = topk::ROWS_NARROW;     // users per workgroup, topn <= 32: 8 waves, 128 keys per user

__device__ __forceinline__ int readlane_i(int v, int src_lane) { return __builtin_amdgcn_readlane(v, src_lane); }

// CAP keys per user: list [0, L) + survivor buffer [L, CAP)
template <int KB, int NW, int CAP, bool MASKED, bool DEEP = false, bool SEG = false>
__global__ __launch_bounds__(NW * 64)
void k_recommend(int ld, int64_t nusers, const int32_t* __restrict__ users, int64_t n, int64_t slice,
                 const float* __restrict__ U, const float* __restrict__ Z, const float* __restrict__ b_u,
                 const float* __restrict__ b_i, const double* __restrict__ mu_p,
                 const int64_t* __restrict__ seen_ptr, const int32_t* __restrict__ seen_idx, int topn,
                 float* __restrict__ top_val, int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt,
                 unsigned long long* __restrict__ part, const uint32_t* __restrict__ allow,
                 const unsigned long long* __restrict__ ceil, const int32_t* __restrict__ go, int64_t nseg,
                 int64_t seg_stride, const int32_t* __restrict__ row_seg) {
    static_assert(!SEG || (!MASKED && !DEEP), "the eligibility table replaces the bitmap; deep lists do not take one");
    constexpr int E = 4 * KB, LD = 16 * KB, ZS = walk::lds_row_stride(KB);
    constexpr int L = CAP == 256 ? 128 : 32, BUF = CAP - L;
    constexpr int NT = NW * 64, NV = walk::CHUNK * LD / 4, PF = (NV + NT - 1) / NT;
    static_assert(L >= 32 && BUF >= 64, "a chunk appends up to 32 keys per row");
    __shared__ unsigned long long keys[NW * 16][CAP];
    __shared__ __attribute__((aligned(16))) float zs[walk::CHUNK][ZS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const float mu = (float)(*mu_p);
    const int64_t b0 = ((int64_t)blockIdx.x * NW + wave) * 16;            // first batch row of this wave
    const int64_t lo = (int64_t)blockIdx.y * slice, hi = min(n, lo + slice);
    unsigned long long (*kw)[CAP] = keys + wave * 16;
    if constexpr (DEEP) {
        static_assert(NW * 16 == 64, "one ceiling per lane covers the workgroup's users");
        if (go && *go == 0) return;                                      // the round before left no slice open
        const int64_t ub = (int64_t)blockIdx.x * 64 + lane;
        const bool open = ub < nusers && ceil[(int64_t)blockIdx.y * nusers + ub] != 0ull;
        if (!__ballot(open)) return;                                     // the same in every wave of the workgroup
    }

    float ua[E];
    load_frow<E>(U + (size_t)users[min(b0 + c, nusers - 1)] * ld + E * q, ua);
    float bu[4];
    bool valid[4];
    int64_t cur[4], end[4];
    int nxt[4];                                                          // next seen item of rows 4q + r
    unsigned long long cl[4] = {0ull, 0ull, 0ull, 0ull};                 // DEEP: ceiling keys of rows 4q + r
    int64_t so[4] = {0, 0, 0, 0};                                        // SEG: word of chunk 0 in the segment row of rows 4q + r
    bool sv[4] = {false, false, false, false};                           // SEG: the row is valid and its segment id in range
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t rb = b0 + 4 * q + r;
        valid[r] = rb < nusers;
        const int u = users[min(rb, nusers - 1)];
        bu[r] = b_u[u];
        if constexpr (DEEP) cl[r] = valid[r] ? ceil[(int64_t)blockIdx.y * nusers + rb] : 0ull;
        if constexpr (SEG) {
            const int64_t sg = row_seg[min(rb, nusers - 1)];
            sv[r] = valid[r] && sg >= 0 && sg < nseg;
            so[r] = (sv[r] ? sg : 0) * seg_stride + lo / walk::CHUNK;    // lo is a multiple of 32
        }
#include "walk_seen_cursor.inc"
    }
#include "walk_row_lists.inc"

    unsigned deny = 0u;     // MASKED: bit c set = item cb + c of the block `select` is called for is not allowed
    unsigned dn[4] = {0u, 0u, 0u, 0u};                                   // SEG: the same, one word per row 4q + r
    // one 16-item block [cb, cb + 16): scores from the accumulator, seen mask, threshold test, append
    auto select = [&](const f32x4& acc, int64_t cb) {
#include "walk_seen_masks.inc"
        if constexpr (MASKED) {
#pragma unroll
            for (int r = 0; r < 4; ++r) msk[r] |= deny;
        }
        if constexpr (SEG) {
#pragma unroll
            for (int r = 0; r < 4; ++r) msk[r] |= dn[r];
        }
        const int64_t col = cb + c;
        const float bi = b_i[min(col, n - 1)];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float score = walk::score(acc[r], mu, bu[r], bi);
            const unsigned long long key = make_key(score, (unsigned)col);
            bool pass = col < hi && valid[r] && !((msk[r] >> c) & 1u) && score == score && key > thr[r];
            if constexpr (DEEP) pass = pass && key < cl[r];
            const unsigned long long m = __ballot(pass);
            const unsigned sub = (unsigned)(m >> (16 * q)) & 0xFFFFu;
            if (pass) kw[4 * q + r][L + cnt[r] + __popc(sub & ((1u << c) - 1u))] = key;
            cnt[r] += __popc(sub);
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
    // SEG: the words of chunk `ch` in the segment rows of this lane's rows 4q + r, 0 for a row that takes no part;
    // ch < nch keeps the word inside the table row (lo / 32 + ch < ceil(n / 32) <= seg_stride)
    unsigned sp[4] = {0u, 0u, 0u, 0u};
    auto seg_fetch = [&](int64_t ch) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sp[r] = sv[r] ? allow[so[r] + ch] : 0u;
    };
    int64_t nx = 0;                                      // MASKED: the chunk after ch that is scored
    if constexpr (MASKED) {
        nx = next_chunk(0);
        if (nx < nch) { fetch(lo + nx * walk::CHUNK); window(nx + 1); }
    } else if (nch > 0) {
        fetch(lo);
        if constexpr (SEG) seg_fetch(0);
    }
    for (int64_t ch = nx; ch < nch; ch = MASKED ? nx : ch + 1) {
        const int64_t it0 = lo + ch * walk::CHUNK;
        unsigned word = 0u;
        if constexpr (MASKED) word = __builtin_amdgcn_readfirstlane(aw[ch]);
        unsigned sw[4] = {0u, 0u, 0u, 0u};               // SEG: this chunk's words, before the prefetch reuses sp
        if constexpr (SEG) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sw[r] = sp[r];
        }
        __syncthreads();                                 // every wave is done with the previous chunk
        stage();
        __syncthreads();
        if constexpr (MASKED) {
            nx = after(ch);
            if (nx < nch) { fetch(lo + nx * walk::CHUNK); window(nx + 1); }      // however far ahead
        } else if (ch + 1 < nch) {
            fetch(it0 + walk::CHUNK);
            if constexpr (SEG) seg_fetch(ch + 1);
        }
        if constexpr (SEG) {
            // none of the wave's 16 rows may take an item of this chunk: no scores, no selection.  The wave has
            // staged its share and passed both barriers; its buffers are as the last chunk left them
            if (!__ballot((sw[0] | sw[1] | sw[2] | sw[3]) != 0u)) continue;
        }
#include "walk_score_tiles.inc"
        if constexpr (MASKED) deny = ~word & 0xFFFFu;
        if constexpr (SEG) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dn[r] = ~sw[r] & 0xFFFFu;
        }
        select(acc0, it0);
        if constexpr (MASKED) deny = ~word >> 16;
        if constexpr (SEG) {
#pragma unroll
            for (int r = 0; r < 4; ++r) dn[r] = ~sw[r] >> 16;
        }
        select(acc1, it0 + 16);
#include "walk_row_overflow.inc"
    }
#include "walk_row_write.inc"
}

// seg: the SEG instantiations (`allow` is then the eligibility table); otherwise MASKED when there is a bitmap
template <int KB>
int launch_recommend(int ld, int64_t nusers, const int32_t* users, int64_t n, int nsl, const float* U, const float* Z,
                     const float* b_u, const float* b_i, const double* mu, const int64_t* seen_ptr,
                     const int32_t* seen_idx, const uint32_t* allow, bool seg, int64_t nseg, int64_t seg_stride,
                     const int32_t* row_seg, int topn, float* tv, int32_t* ti, int32_t* tc, unsigned long long* part,
                     hipStream_t st) {
    constexpr int NN = RC_NARROW / 16, NWD = RC_WIDE / 16;
    const auto narrow = seg     ? k_recommend<KB, NN, 128, false, false, true>
                        : allow ? k_recommend<KB, NN, 128, true>
                                : k_recommend<KB, NN, 128, false>;
    const auto wide = seg     ? k_recommend<KB, NWD, 256, false, false, true>
                      : allow ? k_recommend<KB, NWD, 256, true>
                              : k_recommend<KB, NWD, 256, false>;
    return topk::launch_by_width(narrow, wide, topn, nusers, nsl, st, ld, nusers, users, n, walk::slice_items(n, nsl), U,
                                 Z, b_u, b_i, mu, seen_ptr, seen_idx, topn, tv, ti, tc, part, allow, nullptr, nullptr,
                                 nseg, seg_stride, row_seg);
}

template <int KB>
int launch_recommend_ceil(int ld, int64_t nusers, const int32_t* users, int64_t n, int nsl, const float* U,
                          const float* Z, const float* b_u, const float* b_i, const double* mu,
                          const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow,
                          unsigned long long* part, const unsigned long long* ceil, const int32_t* go, hipStream_t st) {
    const int64_t slice = walk::slice_items(n, nsl);
    const dim3 grid((unsigned)((nusers + RC_WIDE - 1) / RC_WIDE), (unsigned)nsl);
    auto kern = allow ? k_recommend<KB, RC_WIDE / 16, 256, true, true> : k_recommend<KB, RC_WIDE / 16, 256, false, true>;
    hipLaunchKernelGGL(kern, grid, dim3(RC_WIDE * 4), 0, st, ld, nusers, users, n, slice, U, Z, b_u, b_i, mu, seen_ptr,
                       seen_idx, ALS_TOPK_MAX, nullptr, nullptr, nullptr, part, allow, ceil, go, (int64_t)0, (int64_t)0, nullptr);
    return topk::launch_status();
}

// the body of als_recommend_topk_masked (seg false: nseg, seg_stride and row_seg are 0) and _segmented
int recommend_topk(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U, const float* Z,
                   const float* b_u, const float* b_i, const double* mu, const int64_t* seen_ptr,
                   const int32_t* seen_idx, const uint32_t* allow, bool seg, int64_t nseg, int64_t seg_stride,
                   const int32_t* row_seg, int topn, int nslices, float* top_val, int32_t* top_idx, int32_t* top_cnt,
                   void* workspace, size_t workspace_bytes, void* stream) {
    const int bad = topk::check_shape(k, ld, nusers, n, topn, ALS_TOPK_MAX, nslices);
    if (bad) return bad;
    if (seg && (nseg < 1 || seg_stride < (n + 31) / 32)) return ALS_E_BADARG;
    if (nusers == 0) return 0;
    if (!users || !U || !Z || !b_u || !b_i || !mu || !top_val || !top_idx || !top_cnt || (!seen_ptr != !seen_idx) ||
        (seg && (!allow || !row_seg)))
        return ALS_E_BADARG;
    const topk::SlicePlan p = topk::plan(nusers, topk::rows_per_wg(topn), n, nslices, nusers * topn,
                                         sizeof(unsigned long long), workspace, workspace_bytes);
    if (!p.nsl) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    ALS_DISPATCH_KB(ld / 16, rc = launch_recommend<KB>(ld, nusers, users, n, p.nsl, U, Z, b_u, b_i, mu, seen_ptr,
                                                       seen_idx, allow, seg, nseg, seg_stride, row_seg, topn, top_val,
                                                       top_idx, top_cnt, p.keys(), st));
    return rc != 0 ? rc : topk::merge_slices(p.nsl, p.keys(), nusers, topn, top_val, top_idx, top_cnt, st);
}

}  // namespace

// one scoring round of als_recommend_deep (recommend_deep.hpp)
int deep::score_round(int ld, int64_t nusers, const int32_t* users, int64_t n, int nsl, const float* U, const float* Z,
                      const float* b_u, const float* b_i, const double* mu, const int64_t* seen_ptr,
                      const int32_t* seen_idx, const uint32_t* allow, unsigned long long* part,
                      const unsigned long long* ceil, const int32_t* go, hipStream_t st) {
    int rc = ALS_E_BADK;
    ALS_DISPATCH_KB(ld / 16, rc = launch_recommend_ceil<KB>(ld, nusers, users, n, nsl, U, Z, b_u, b_i, mu, seen_ptr,
                                                            seen_idx, allow, part, ceil, go, st));
    return rc;
}
int deep::plan_slices(int64_t nusers, int64_t n, int nslices) { return topk::slices(nusers, RC_WIDE, n, nslices); }

extern "C" size_t als_recommend_workspace_bytes(int64_t nusers, int64_t n, int topn, int nslices) {
    return topk::workspace_bytes(nusers, topk::rows_per_wg(topn), n, topn, nslices);
}

extern "C" int als_recommend_topk_masked(int k, int ld, int64_t nusers, const int32_t* users, int64_t n,
                                         const float* U, const float* Z, const float* b_u, const float* b_i,
                                         const double* mu, const int64_t* seen_ptr, const int32_t* seen_idx,
                                         const uint32_t* allow, int topn, int nslices, float* top_val,
                                         int32_t* top_idx, int32_t* top_cnt, void* workspace, size_t workspace_bytes,
                                         void* stream) {
    return recommend_topk(k, ld, nusers, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow, false, 0, 0, nullptr,
                          topn, nslices, top_val, top_idx, top_cnt, workspace, workspace_bytes, stream);
}

extern "C" int als_recommend_topk_segmented(int k, int ld, int64_t nusers, const int32_t* users, int64_t n,
                                            const float* U, const float* Z, const float* b_u, const float* b_i,
                                            const double* mu, const int64_t* seen_ptr, const int32_t* seen_idx,
                                            const uint32_t* seg_allow, int64_t nseg, int64_t seg_stride_words,
                                            const int32_t* row_seg, int topn, int nslices, float* top_val,
                                            int32_t* top_idx, int32_t* top_cnt, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    return recommend_topk(k, ld, nusers, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, seg_allow, true, nseg,
                          seg_stride_words, row_seg, topn, nslices, top_val, top_idx, top_cnt, workspace,
                          workspace_bytes, stream);
}

extern "C" int als_recommend_topk(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                                  const float* Z, const float* b_u, const float* b_i, const double* mu,
                                  const int64_t* seen_ptr, const int32_t* seen_idx, int topn, int nslices,
                                  float* top_val, int32_t* top_idx, int32_t* top_cnt, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return als_recommend_topk_masked(k, ld, nusers, users, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, nullptr, topn,
                                     nslices, top_val, top_idx, top_cnt, workspace, workspace_bytes, stream);
}
