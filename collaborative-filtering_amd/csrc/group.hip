// K15: top-N for a group of users - ALS.recommend_group: every member j of group b scores item i with
// s_j(i) = U_j.Z_i + mu + b_u[j] + b_i[i], the g member scores are folded into one group score (their minimum, their
// maximum, or their fp64 mean rounded once to fp32), the items of the group's seen row left out, the topn best items
// kept per group - without forming the members' rows of the m x n completion.
//
// k_group: ONE WAVE serves one group, a workgroup of GR_NW waves serves GR_NW consecutive groups over the items
// [lo, hi) of one slice.  The walk is k_recommend's (recommend.hip): items in chunks of 32, the chunk's Z rows staged in
// LDS once per workgroup while the global loads of the next chunk are in flight.  The members sit in tiles of 16: member
// 16t + c is row c of tile t, and the wave forms, per tile, its two 16 x 16 score tiles with the SAME
// v_mfma_f32_16x16x4_f32 chain and epilogue as k_predict_dense (lane (c, q) holds k = 4KB q + e of member row c and of
// item row c in step e; ((acc + mu) + b_u) + b_i), so every member score is bitwise the value als_predict_dense writes.
// A group of <= 16 members keeps its rows in registers for the whole walk; a larger one loops over its tiles inside
// each chunk and re-reads the rows (they stay in L2: at most 64 rows per wave).  A wave past the last group, or of an
// empty group, stages and takes every barrier, and scores nothing.
//
// Aggregation: lane (c, q) holds acc[r] = score of member row 4q + r for item c.  It folds its rows in-lane (rows past
// g contribute nothing), over the tiles, and the four q groups are folded by two xor shuffles (16, 32), after which
// every lane of column c holds the group score of item c.  Minimum and maximum are one path: max(s) = -min(-s), the
// sign a wave-uniform factor (exact).  v_min_f32 drops a NaN operand, so "some member score is NaN" travels next to the
// value as an explicit flag: s != s per member score, OR-ed in-lane, folded over the q groups by a ballot.  The mean
// adds the fp32 scores in fp64: exact - and so independent of lane layout, tiling and member order - while the nonzero
// member scores of an item lie within a factor 2^17 of each other in magnitude (24-bit values, at most 64 of them,
// 53-bit accumulator); outside that band the result is within one fp64 rounding of the exact sum.  The sum is divided
// by g in fp64 and rounded once to fp32.  A mean of +inf and -inf is a NaN without a NaN member: the candidate test
// drops it like any NaN.
//
// Selection: after the fold there is ONE candidate per item and one list per wave, so the state - threshold, buffered
// survivors, list length - is three wave-uniform values and the LDS key array is [GR_NW][CAP], not topk_rows.hpp's
// sixteen rows per wave.  Lane l < 32 owns item it0 + l of the chunk (the lanes of q group 0 take block 0's scores,
// those of q group 1 block 1's); a candidate above the threshold is appended by one ballot + prefix popcount per chunk,
// and the row is compacted with topk::sort_desc when its buffer could overflow in the next chunk.  Keys, order, ties,
// padding and the merge of the slices' lists (topk::k_merge_slices) are als_recommend_topk's.
//
// Exclusion: seen_ptr / seen_idx are indexed by BATCH GROUP (the caller forms the union of the members' rows).  The
// wave keeps one cursor and the next seen item; only a chunk that reaches it loads the next 64 entries (one per lane)
// and OR-reduces a 32-bit mask.  When all 64 lie below the chunk - the cursor is behind because chunks with an
// all-zero bitmap word were skipped - the cursor jumps by a lower-bound search (as k_audience).  Allow bitmap (the
// MASKED instantiations): k_recommend's scan - a chunk whose word is 0 is never fetched, staged or scored, every wave
// finds the next chunk with a set bit by the same ballot, so the workgroup's barriers stay matched.  The scan and the
// Z fetch / stage are k_recommend's text, not copies of it: walk_allow_scan.inc, walk_z_fetch.inc, walk_z_stage.inc
// (DESIGN section 31).
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

constexpr int GR_CHUNK = walk::CHUNK;
constexpr int GR_NW = 8;            // groups (waves) per workgroup
constexpr int GR_MAXM = ALS_GROUP_MAX_MEMBERS;
static_assert(GR_MAXM == 64, "one member-table entry per lane, four tiles of 16");

// the value of the lanes c, c + 16, c + 32, c + 48 folded, in all four
__device__ __forceinline__ float fold_q_min(float v) {
    v = fminf(v, __shfl_xor(v, 16, 64));
    return fminf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ double fold_q_sum(double v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}
// bit c of the result: the flag of one of the lanes c, c + 16, c + 32, c + 48 is set
__device__ __forceinline__ unsigned fold_q_any(bool flag) {
    unsigned long long m = __ballot(flag);
    m |= m >> 32;
    m |= m >> 16;
    return (unsigned)m & 0xFFFFu;
}

// CAP keys per group: list [0, L) + survivor buffer [L, CAP)
template <int KB, int CAP, bool MASKED>
__global__ __launch_bounds__(GR_NW * 64)
void k_group(int ld, int64_t ngroups, const int64_t* __restrict__ g_ptr, const int32_t* __restrict__ g_users,
             int max_members, int64_t n, int64_t slice, const float* __restrict__ U, const float* __restrict__ Z,
             const float* __restrict__ b_u, const float* __restrict__ b_i, const double* __restrict__ mu_p,
             const int64_t* __restrict__ seen_ptr, const int32_t* __restrict__ seen_idx,
             const uint32_t* __restrict__ allow, int aggregate, int topn, float* __restrict__ top_val,
             int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt, unsigned long long* __restrict__ part) {
    constexpr int NW = GR_NW, E = 4 * KB, LD = 16 * KB, ZS = walk::lds_row_stride(KB);
    constexpr int L = CAP == 256 ? 128 : 32, BUF = CAP - L;
    constexpr int NT = NW * 64, NV = GR_CHUNK * LD / 4, PF = (NV + NT - 1) / NT;
    static_assert(L >= 32 && BUF >= 64, "a chunk appends up to 32 keys");
    __shared__ unsigned long long keys[NW][CAP];
    __shared__ __attribute__((aligned(16))) float zs[GR_CHUNK][ZS];
    __shared__ int mem_uid[NW][GR_MAXM];                 // user id and b_u of member l (l >= g: of the last member)
    __shared__ float mem_bu[NW][GR_MAXM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const float mu = (float)(*mu_p);
    const int64_t b = (int64_t)blockIdx.x * NW + wave;                    // batch group of this wave
    const int64_t lo = (int64_t)blockIdx.y * slice, hi = min(n, lo + slice);
    unsigned long long* kw = keys[wave];

    // members: g of them (a longer list is cut at max_members <= 64, the size of the tables), T tiles of 16
    int g = 0;
    if (b < ngroups) {
        const int64_t p0 = g_ptr[b];
        g = (int)min(max(g_ptr[b + 1] - p0, (int64_t)0), (int64_t)max_members);
        if (g > 0) {
            const int u = g_users[p0 + min(lane, g - 1)];
            mem_uid[wave][lane] = u;
            mem_bu[wave][lane] = b_u[u];
        }
    }
    g = __builtin_amdgcn_readfirstlane(g);
    const bool active = g > 0;
    const int T = (g + 15) >> 4;
    wave_lds_sync();
    float ua[E];
    float bu[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {                                        // tile 0: all there is when g <= 16
        load_frow<E>(U + (size_t)mem_uid[wave][c] * ld + E * q, ua);
#pragma unroll
        for (int r = 0; r < 4; ++r) bu[r] = mem_bu[wave][4 * q + r];
    } else {
#pragma unroll
        for (int e = 0; e < E; ++e) ua[e] = 0.f;
    }
    const bool is_mean = aggregate == ALS_GROUP_MEAN;
    const float sign = aggregate == ALS_GROUP_MAX ? -1.f : 1.f;         // max(s) = -min(-s)
    const double den = (double)max(g, 1);

    // the group's seen row: cursor, end, next seen item (wave-uniform)
    int64_t cur = 0, end = 0;
    if (seen_ptr && active) {
        end = seen_ptr[b + 1];
        cur = walk::lower_bound(seen_idx, seen_ptr[b], end, lo);               // first seen item >= lo
    }
    int nxt = cur < end ? seen_idx[cur] : INT32_MAX;

    unsigned long long thr = 0ull;      // key of the current topn-th entry (0: list not full)
    int cnt = 0;                        // buffered survivors
    int nlist = 0;                      // valid entries of the sorted list

    auto compact = [&]() {              // list + buffer -> sorted list, new threshold
        wave_lds_sync();
        unsigned long long k[CAP / 64];
#pragma unroll
        for (int v = 0; v < CAP / 64; ++v) {
            const int i = lane + 64 * v;
            const bool live = (i < nlist) || (i >= L && i < L + cnt);
            k[v] = live ? kw[i] : 0ull;
        }
        topk::sort_desc<CAP / 64>(k, lane);
#pragma unroll
        for (int v = 0; v < CAP / 64; ++v)
            if (lane + 64 * v < L) kw[lane + 64 * v] = k[v];
        wave_lds_sync();
        const int nn = min(topn, nlist + cnt);
        thr = (nn == topn) ? kw[topn - 1] : 0ull;
        cnt = 0;
        nlist = nn;
    };

    // bit l set: item it0 + l of the chunk [it0, it0 + 32) is in the group's seen row
    auto seen_mask = [&](int64_t it0) -> unsigned {
        unsigned msk = 0u;
        if (nxt < it0 + GR_CHUNK) {                                      // wave-uniform
            bool more = true;
            while (more) {
                const int64_t p = cur + lane;
                const int s = p < end ? seen_idx[p] : INT32_MAX;
                const bool below = s < it0 + GR_CHUNK;
                unsigned bit = (below && s >= it0) ? 1u << (int)(s - it0) : 0u;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) bit |= __shfl_xor(bit, o, 64);
                msk |= bit;
                const int adv = __popcll(__ballot(below));
                cur += adv;
                more = adv == 64;                                        // 64 consumed: there may be more in the chunk
                if constexpr (MASKED) {
                    // all 64 below the chunk: the cursor fell behind over skipped chunks - jump, do not walk
                    const int last = __builtin_amdgcn_readlane(s, 63);
                    if (more && last < it0) cur = walk::lower_bound(seen_idx, cur, end, it0);
                }
            }
            nxt = cur < end ? seen_idx[cur] : INT32_MAX;
        }
        return msk;
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
        if (nx < nch) { fetch(lo + nx * GR_CHUNK); window(nx + 1); }
    } else if (nch > 0) fetch(lo);
    for (int64_t ch = nx; ch < nch; ch = MASKED ? nx : ch + 1) {
        const int64_t it0 = lo + ch * GR_CHUNK;
        unsigned word = ~0u;
        if constexpr (MASKED) word = __builtin_amdgcn_readfirstlane(aw[ch]);
        __syncthreads();                                 // every wave is done with the previous chunk
        stage();
        __syncthreads();
        if constexpr (MASKED) {
            nx = after(ch);
            if (nx < nch) { fetch(lo + nx * GR_CHUNK); window(nx + 1); }      // however far ahead
        } else if (ch + 1 < nch) fetch(it0 + GR_CHUNK);
        if (!active) continue;                           // wave-uniform: no group, or an empty one

        float z0[E], z1[E];
        load_frow<E>(&zs[c][E * q], z0);
        load_frow<E>(&zs[16 + c][E * q], z1);
        const float bi0 = b_i[min(it0 + c, n - 1)], bi1 = b_i[min(it0 + 16 + c, n - 1)];
        float m0 = INFINITY, m1 = INFINITY;              // min of sign * score over this lane's member rows
        double d0 = 0.0, d1 = 0.0;                       // their fp64 sum
        bool nan0 = false, nan1 = false;                 // one of them is a NaN
        for (int t = 0; t < T; ++t) {
            if (T > 1) {                                 // the rows of tile t (L2), its biases
                load_frow<E>(U + (size_t)mem_uid[wave][16 * t + c] * ld + E * q, ua);
#pragma unroll
                for (int r = 0; r < 4; ++r) bu[r] = mem_bu[wave][16 * t + 4 * q + r];
            }
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < E; ++e) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[e], z0[e], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[e], z1[e], acc1, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool live = 16 * t + 4 * q + r < g;                // rows past g contribute the identity
                const float s0 = walk::score(acc0[r], mu, bu[r], bi0);
                const float s1 = walk::score(acc1[r], mu, bu[r], bi1);
                nan0 = nan0 || (live && s0 != s0);
                nan1 = nan1 || (live && s1 != s1);
                if (is_mean) {
                    d0 += live ? (double)s0 : 0.0;
                    d1 += live ? (double)s1 : 0.0;
                } else {
                    m0 = fminf(m0, live ? sign * s0 : INFINITY);
                    m1 = fminf(m1, live ? sign * s1 : INFINITY);
                }
            }
        }
        float gs0, gs1;                                  // group score of item it0 + c / it0 + 16 + c, in all four q groups
        if (is_mean) {
            gs0 = (float)(fold_q_sum(d0) / den);
            gs1 = (float)(fold_q_sum(d1) / den);
        } else {
            gs0 = sign * fold_q_min(m0);
            gs1 = sign * fold_q_min(m1);
        }
        unsigned drop = fold_q_any(nan0) | (fold_q_any(nan1) << 16);    // bit l: item it0 + l has a NaN member score
        drop |= seen_mask(it0);
        if constexpr (MASKED) drop |= ~word;

        // one candidate per item: lane l < 32 owns item it0 + l
        const float gs = q == 0 ? gs0 : gs1;
        const int64_t col = it0 + lane;
        const unsigned long long key = make_key(gs, (unsigned)col);
        const bool pass = lane < GR_CHUNK && col < hi && !((drop >> (lane & 31)) & 1u) && gs == gs && key > thr;
        const unsigned long long pm = __ballot(pass);
        if (pass) kw[L + cnt + __popcll(pm & ((1ull << lane) - 1ull))] = key;
        cnt += __popcll(pm);
        if (cnt > BUF - GR_CHUNK) compact();             // the buffer could overflow in the next chunk
    }
    if (cnt > 0) compact();
    wave_lds_sync();
    if (b >= ngroups) return;
    if (part) {                                          // sliced: raw keys of (slice, group), 0 = empty
        unsigned long long* dst = part + ((int64_t)blockIdx.y * ngroups + b) * topn;
        for (int t = lane; t < topn; t += 64) dst[t] = t < nlist ? kw[t] : 0ull;
    } else {
        for (int t = lane; t < topn; t += 64) {
            const bool ok = t < nlist;
            const unsigned long long key = ok ? kw[t] : 0ull;
            top_val[b * topn + t] = ok ? key_score(key) : -INFINITY;
            top_idx[b * topn + t] = ok ? key_index(key) : -1;
        }
        if (lane == 0) top_cnt[b] = nlist;
    }
}

template <int KB>
int launch_group(int ld, int64_t ngroups, const int64_t* g_ptr, const int32_t* g_users, int max_members, int64_t n,
                 int nsl, const float* U, const float* Z, const float* b_u, const float* b_i, const double* mu,
                 const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow, int aggregate, int topn,
                 float* tv, int32_t* ti, int32_t* tc, unsigned long long* part, hipStream_t st) {
    const int64_t slice = walk::slice_items(n, nsl);
    const dim3 grid((unsigned)((ngroups + GR_NW - 1) / GR_NW), (unsigned)nsl);
    auto kern = topn <= 32 ? (allow ? k_group<KB, 128, true> : k_group<KB, 128, false>)
                           : (allow ? k_group<KB, 256, true> : k_group<KB, 256, false>);
    hipLaunchKernelGGL(kern, grid, dim3(GR_NW * 64), 0, st, ld, ngroups, g_ptr, g_users, max_members, n, slice, U, Z,
                       b_u, b_i, mu, seen_ptr, seen_idx, allow, aggregate, topn, tv, ti, tc, part);
    return topk::launch_status();
}

}  // namespace

extern "C" size_t als_group_workspace_bytes(int64_t ngroups, int64_t n, int topn, int nslices) {
    return topk::workspace_bytes(ngroups, GR_NW, n, topn, nslices);
}

extern "C" int als_group_topk(int k, int ld, int64_t ngroups, const int64_t* g_ptr, const int32_t* g_users,
                              int max_members, int64_t n, const float* U, const float* Z, const float* b_u,
                              const float* b_i, const double* mu, const int64_t* seen_ptr, const int32_t* seen_idx,
                              const uint32_t* allow, int aggregate, int topn, int nslices, float* top_val,
                              int32_t* top_idx, int32_t* top_cnt, void* workspace, size_t workspace_bytes,
                              void* stream) {
    const int bad = topk::check_shape(k, ld, ngroups, n, topn, ALS_TOPK_MAX, nslices);
    if (bad) return bad;
    if (max_members < 0 || max_members > ALS_GROUP_MAX_MEMBERS ||
        (aggregate != ALS_GROUP_MEAN && aggregate != ALS_GROUP_MIN && aggregate != ALS_GROUP_MAX))
        return ALS_E_BADARG;
    if (ngroups == 0) return 0;
    if (!g_ptr || !g_users || !U || !Z || !b_u || !b_i || !mu || !top_val || !top_idx || !top_cnt ||
        (!seen_ptr != !seen_idx))
        return ALS_E_BADARG;
    const topk::SlicePlan p = topk::plan(ngroups, GR_NW, n, nslices, ngroups * topn, sizeof(unsigned long long),
                                         workspace, workspace_bytes);
    if (!p.nsl) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    ALS_DISPATCH_KB(ld / 16, rc = launch_group<KB>(ld, ngroups, g_ptr, g_users, max_members, n, p.nsl, U, Z, b_u, b_i,
                                                   mu, seen_ptr, seen_idx, allow, aggregate, topn, top_val, top_idx,
                                                   top_cnt, p.keys(), st));
    return rc != 0 ? rc : topk::merge_slices(p.nsl, p.keys(), ngroups, topn, top_val, top_idx, top_cnt, st);
}
