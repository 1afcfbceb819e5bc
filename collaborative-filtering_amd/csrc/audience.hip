// K14: the audience of an item - ALS.recommend_users: score(b, u) = U_u.Q_i + mu + b_u[u] + q_bias[i] over all users u,
// i = q_ids[b], the item's raters left out, the topn best users kept per batch row - without forming a column of the
// m x n completion.
//
// k_audience has k_similar's structure (similar.hip): one workgroup serves NW * 16 query items (one 16-query tile per
// wave) over the users [lo, hi) of one slice.  The user table is walked in chunks of 32: the workgroup stages the
// chunk's rows of U and its 32 b_u values in LDS once (the global loads of the next chunk are in flight while the
// current one is scored), the query rows are gathered from Q, and every wave forms its two 16 x 16 tiles with the
// v_mfma_f32_16x16x4_f32 chain of k_predict_dense and the epilogue walk::score(dot, mu, b_u[u], q_bias[i]) =
// ((dot + mu) + b_u) + b_i - the association of als_predict_dense, NOT the ((dot + mu) + b_i) + b_u that
// als_recommend_topk gives when it is called with the two sides swapped.
//
// Operand roles: k_predict_dense has the USER row as the matrix instruction's A operand and the item row as B.  Here
// the query (an item) is A and the walked table row (a user) is B, as in k_similar, so the instruction forms the
// transposed product: lane (c, q) holds k = 4KB q + e of query row c and of table row c in step e, and acc[r] is
// (query 4q + r, user cb + c).  Every a * b is commutative and the four products of one step are added to the
// accumulator in an order that does not depend on the output position, so the dot is bitwise k_predict_dense's;
// tests/test_gpu_audience.py compares every score with als_predict_dense's output with ==.  This layout ships because
// it keeps k_similar's epilogue (per-row state in the q group, per-column values in lane c) unchanged.
//
// Exclusion is k_recommend's (recommend.hip), written here a third time - the body of the walk is not shared, only
// its lower-bound search (walk::lower_bound; catalogue_walk.hpp and DESIGN sections 19 and 28 say why): each query
// row keeps a cursor into the ascending rater list of ITS ITEM (seen_ptr is indexed by q_ids[b]) and the next rater;
// only a block that reaches that rater builds a 16-bit mask (one coalesced load of the next 16 entries by the row's
// 16 lanes and an OR-reduction).  A slice starts with a lower-bound search for lo.  One addition: when a whole
// 16-entry load lies below the block - the cursor is behind because chunks with an all-zero bitmap word were not
// scored - the cursor jumps by a lower-bound search instead of walking, so a hub item's 10^5 ... 10^6 raters cost
// log2(list) loads after a gap and nothing per chunk.
//
// Selection is topk_rows.hpp's; with more than one slice (grid.y) every workgroup writes raw keys to the workspace and
// topk::k_merge_slices folds them.  The order (score desc, user asc) is total, so the result does not depend on the
// slice count.  Allow bitmap (the MASKED instantiations): as k_similar - chunk ch of a slice is word lo / 32 + ch, a
// chunk whose word is 0 is staged (barriers and prefetch stay as they are) but not scored.
#include "als_device.hpp"
#include "als_hip.h"
#include "catalogue_walk.hpp"
#include "topk_common.hpp"
#include "topk_launch.hpp"
#include "topk_rows.hpp"

namespace {

using topk::make_key;

constexpr int AU_CHUNK = walk::CHUNK;

// CAP keys per query: list [0, L) + survivor buffer [L, CAP)
template <int KB, int NW, int CAP, bool MASKED>
__global__ __launch_bounds__(NW * 64)
void k_audience(int ld, int64_t nq, const int32_t* __restrict__ q_ids, const float* __restrict__ Q,
                const float* __restrict__ q_bias, int64_t m, int64_t slice, const float* __restrict__ U,
                const float* __restrict__ b_u, const double* __restrict__ mu_p,
                const int64_t* __restrict__ seen_ptr, const int32_t* __restrict__ seen_idx,
                const uint32_t* __restrict__ allow, int topn, float* __restrict__ top_val,
                int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt, unsigned long long* __restrict__ part) {
    constexpr int E = 4 * KB, LD = 16 * KB, ZS = walk::lds_row_stride(KB);
    constexpr int NT = NW * 64, NV = AU_CHUNK * LD / 4, PF = (NV + NT - 1) / NT;
    static_assert(NT >= AU_CHUNK, "one thread per staged user bias");
    __shared__ unsigned long long keys[NW * 16][CAP];
    __shared__ __attribute__((aligned(16))) float zs[AU_CHUNK][ZS];
    __shared__ float bus[AU_CHUNK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const float mu = (float)(*mu_p);
    const int64_t b0 = ((int64_t)blockIdx.x * NW + wave) * 16;            // first batch row of this wave
    const int64_t lo = (int64_t)blockIdx.y * slice, hi = min(m, lo + slice);
    unsigned long long (*kw)[CAP] = keys + wave * 16;

    float ua[E];
    load_frow<E>(Q + (size_t)q_ids[min(b0 + c, nq - 1)] * ld + E * q, ua);
    float qb[4];
    bool valid[4];
    int64_t cur[4], end[4];
    int nxt[4];                                                          // next rater of the items of rows 4q + r
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t rb = b0 + 4 * q + r;
        valid[r] = rb < nq;
        const int i = q_ids[min(rb, nq - 1)];
        qb[r] = q_bias[i];
        cur[r] = end[r] = 0;
        if (seen_ptr && valid[r]) {
            end[r] = seen_ptr[i + 1];
            cur[r] = walk::lower_bound(seen_idx, seen_ptr[i], end[r], lo);     // first rater >= lo
        }
        nxt[r] = cur[r] < end[r] ? seen_idx[cur[r]] : INT32_MAX;
    }
    topk::Rows<CAP> st;

    // one 16-user block [cb, cb + 16): rater mask, scores from the accumulator, candidate test, append
    auto select = [&](const f32x4& acc, int64_t cb, float bu, unsigned deny) {
        unsigned msk[4] = {deny, deny, deny, deny};
        bool near = false;
#pragma unroll
        for (int r = 0; r < 4; ++r) near = near || nxt[r] < cb + 16;
        if (__ballot(near)) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                bool more = nxt[r] < cb + 16;                            // same in the 16 lanes of the q group
                const bool touched = more;
                while (__ballot(more)) {
                    int s = INT32_MAX;
                    if (more) {
                        const int64_t p = cur[r] + c;
                        s = p < end[r] ? seen_idx[p] : INT32_MAX;
                    }
                    const bool below = more && s < cb + 16;
                    unsigned bit = (below && s >= cb) ? 1u << (int)(s - cb) : 0u;
                    bit |= __shfl_xor(bit, 1, 64);
                    bit |= __shfl_xor(bit, 2, 64);
                    bit |= __shfl_xor(bit, 4, 64);
                    bit |= __shfl_xor(bit, 8, 64);
                    msk[r] |= bit;
                    const int adv = __popc((unsigned)(__ballot(below) >> (16 * q)) & 0xFFFFu);
                    cur[r] += adv;
                    more = more && adv == 16;                            // 16 consumed: there may be more in the block
                    if constexpr (MASKED) {
                        // all 16 below the block: the cursor fell behind over unscored chunks - jump, do not walk
                        const int last = __shfl(s, (lane & 48) | 15, 64);
                        if (more && last < cb) cur[r] = walk::lower_bound(seen_idx, cur[r], end[r], cb);
                    }
                }
                if (touched) nxt[r] = cur[r] < end[r] ? seen_idx[cur[r]] : INT32_MAX;
            }
        }
        const int64_t col = cb + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float score = walk::score(acc[r], mu, bu, qb[r]);
            const unsigned long long key = make_key(score, (unsigned)col);
            const bool pass = col < hi && valid[r] && !((msk[r] >> c) & 1u) && score == score && key > st.thr[r];
            topk::append<CAP>(kw, st, r, pass, key, c, q);
        }
    };

    f32x4 pf[PF];
    float pbu = 0.f;
    auto fetch = [&](int64_t it0) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int v = tid + p * NT;
            if (v < NV) {
                const int i = v / (LD / 4), d = v - i * (LD / 4);
                pf[p] = *reinterpret_cast<const f32x4*>(U + (size_t)min(it0 + i, m - 1) * ld + 4 * d);
            }
        }
        if (tid < AU_CHUNK) pbu = b_u[min(it0 + tid, m - 1)];
    };
    auto stage = [&]() {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int v = tid + p * NT;
            if (v < NV) {
                const int i = v / (LD / 4), d = v - i * (LD / 4);
                *reinterpret_cast<f32x4*>(&zs[i][4 * d]) = pf[p];
            }
        }
        if (tid < AU_CHUNK) bus[tid] = pbu;
    };

    const int64_t nch = hi > lo ? (hi - lo + AU_CHUNK - 1) / AU_CHUNK : 0;
    const uint32_t* aw = MASKED ? allow + lo / AU_CHUNK : nullptr;      // word of chunk 0 (lo is a multiple of 32)
    if (nch > 0) fetch(lo);
    for (int64_t ch = 0; ch < nch; ++ch) {
        const int64_t it0 = lo + ch * AU_CHUNK;
        unsigned word = ~0u;
        if constexpr (MASKED) word = __builtin_amdgcn_readfirstlane(aw[ch]);
        __syncthreads();                                 // every wave is done with the previous chunk
        stage();
        __syncthreads();
        if (ch + 1 < nch) fetch(it0 + AU_CHUNK);
        if (MASKED && word == 0u) continue;              // wave-uniform, the same in every wave
        float z0[E], z1[E];
        load_frow<E>(&zs[c][E * q], z0);
        load_frow<E>(&zs[16 + c][E * q], z1);
        const float bu0 = bus[c], bu1 = bus[16 + c];
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < E; ++e) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[e], z0[e], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[e], z1[e], acc1, 0, 0, 0);
        }
        select(acc0, it0, bu0, ~word & 0xFFFFu);
        select(acc1, it0 + 16, bu1, ~word >> 16);
        topk::compact_full_rows<CAP>(kw, st, topn, lane);
    }
    wave_lds_sync();
    for (int R = 0; R < 16; ++R)
        topk::finish_row<CAP>(kw, st, R, topn, lane, b0 + R, nq, (int64_t)blockIdx.y, part, top_val, top_idx, top_cnt);
}

template <int KB>
int launch_audience(int ld, int64_t nq, const int32_t* q_ids, const float* Q, const float* q_bias, int64_t m, int nsl,
                    const float* U, const float* b_u, const double* mu, const int64_t* seen_ptr,
                    const int32_t* seen_idx, const uint32_t* allow, int topn, float* tv, int32_t* ti, int32_t* tc,
                    unsigned long long* part, hipStream_t st) {
    constexpr int NN = topk::ROWS_NARROW / 16, NWD = topk::ROWS_WIDE / 16;
    return topk::launch_by_width(allow ? k_audience<KB, NN, 128, true> : k_audience<KB, NN, 128, false>,
                                 allow ? k_audience<KB, NWD, 256, true> : k_audience<KB, NWD, 256, false>, topn, nq, nsl,
                                 st, ld, nq, q_ids, Q, q_bias, m, walk::slice_items(m, nsl), U, b_u, mu, seen_ptr,
                                 seen_idx, allow, topn, tv, ti, tc, part);
}

}  // namespace

extern "C" size_t als_audience_workspace_bytes(int64_t nq, int64_t m, int topn, int nslices) {
    return topk::workspace_bytes(nq, topk::rows_per_wg(topn), m, topn, nslices);
}

extern "C" int als_audience_topk(int k, int ld, int64_t nq, const int32_t* q_ids, const float* Q, const float* q_bias,
                                 int64_t m, const float* U, const float* b_u, const double* mu,
                                 const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow, int topn,
                                 int nslices, float* top_val, int32_t* top_idx, int32_t* top_cnt, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    const int bad = topk::check_shape(k, ld, nq, m, topn, ALS_TOPK_MAX, nslices);
    if (bad) return bad;
    if (nq == 0) return 0;
    if (!q_ids || !Q || !q_bias || !U || !b_u || !mu || !top_val || !top_idx || !top_cnt || (!seen_ptr != !seen_idx))
        return ALS_E_BADARG;
    const topk::SlicePlan p = topk::plan(nq, topk::rows_per_wg(topn), m, nslices, nq * topn,
                                         sizeof(unsigned long long), workspace, workspace_bytes);
    if (!p.nsl) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    ALS_DISPATCH_KB(ld / 16, rc = launch_audience<KB>(ld, nq, q_ids, Q, q_bias, m, p.nsl, U, b_u, mu, seen_ptr, seen_idx,
                                                      allow, topn, top_val, top_idx, top_cnt, p.keys(), st));
    return rc != 0 ? rc : topk::merge_slices(p.nsl, p.keys(), nq, topn, top_val, top_idx, top_cnt, st);
}
