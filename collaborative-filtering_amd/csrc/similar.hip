// K13: nearest neighbours of rows of a factor table under the cosine - ALS.similar_items / similar_users.
//
//   als_row_inv_norms   inv[r] = 1 / |T_r|, the squares accumulated in fp64 (rows at 1e-20 or 1e19 neither underflow
//                       nor overflow); 0 for a zero row, NaN for a row with a non-finite entry
//   als_similar_topk    sim(b, j) = (Q_q.T_j * q_inv[q]) * t_inv[j] over all rows j of T, the topn best per batch row
//
// k_similar is k_recommend's walk (recommend.hip) without its seen machinery: one workgroup serves NW * 16 queries
// (one 16-query tile per wave) over the rows [lo, hi) of one slice.  The table is walked in chunks of 32: the workgroup
// stages the chunk's rows and its 32 inverse norms in LDS once (the global loads of the next chunk are in flight while
// the current one is scored), and every wave forms its two 16 x 16 tiles with the SAME v_mfma_f32_16x16x4_f32 chain
// as k_predict_dense (lane (c, q) holds k = 4KB q + e of query row c and table row c in step e), so every dot is
// bitwise the value als_predict_dense writes for zero biases and mu = 0.  The query rows are gathered from the table
// they come from; "self" is one compare per candidate where k_recommend keeps a cursor into a seen list.
//
// Selection is topk_rows.hpp's: 64-bit keys ordered by (sim desc, row asc), threshold, survivor buffer, bitonic
// compaction; with more than one slice (grid.y) every workgroup writes its lists as raw keys to the workspace and
// topk::k_merge_slices folds them.  The order is total, so the result does not depend on the slice count.
//
// Allow bitmap (the MASKED instantiations): slices start at multiples of 32, so chunk ch of a slice is word
// lo / 32 + ch of the bitmap - one wave-uniform word per chunk; its bit joins the candidate test.  A chunk whose word
// is 0 is staged like any other (the barriers and the prefetch stay as they are) but not scored.
#include "als_device.hpp"
#include "als_hip.h"
#include "catalogue_walk.hpp"
#include "topk_common.hpp"
#include "topk_launch.hpp"
#include "topk_rows.hpp"

namespace {

using topk::make_key;

constexpr int SM_CHUNK = walk::CHUNK;

// 16 lanes per row: lane c takes the float4 groups c, c + 16, ... of the row (padding columns are zero)
__global__ __launch_bounds__(256)
void k_row_inv_norms(int ld, int64_t nrows, const float* __restrict__ T, float* __restrict__ inv_norm) {
    const int c = threadIdx.x & 15;
    const int64_t r = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
    double s = 0.0;
    if (r < nrows) {
        const f32x4* row = reinterpret_cast<const f32x4*>(T + (size_t)r * ld);
        for (int j = c; j < ld / 4; j += 16) {
            const f32x4 v = row[j];
            s += (double)v.x * (double)v.x;
            s += (double)v.y * (double)v.y;
            s += (double)v.z * (double)v.z;
            s += (double)v.w * (double)v.w;
        }
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    s += __shfl_xor(s, 8, 64);
    if (r < nrows && c == 0) {
        float out = (float)(1.0 / sqrt(s));
        if (s == 0.0) out = 0.f;
        if (!(s < (double)INFINITY)) out = __builtin_nanf("");         // NaN or +inf: a non-finite entry
        inv_norm[r] = out;
    }
}

// CAP keys per query: list [0, L) + survivor buffer [L, CAP)
template <int KB, int NW, int CAP, bool MASKED>
__global__ __launch_bounds__(NW * 64)
void k_similar(int ld, int64_t nq, const int32_t* __restrict__ q_ids, const float* __restrict__ Q,
               const float* __restrict__ q_inv, const int32_t* __restrict__ self_ids, int64_t n, int64_t slice,
               const float* __restrict__ T, const float* __restrict__ t_inv, const uint32_t* __restrict__ allow,
               int topn, float* __restrict__ top_val, int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt,
               unsigned long long* __restrict__ part) {
    constexpr int E = 4 * KB, LD = 16 * KB, ZS = walk::lds_row_stride(KB);
    constexpr int NT = NW * 64, NV = SM_CHUNK * LD / 4, PF = (NV + NT - 1) / NT;
    static_assert(NT >= SM_CHUNK, "one thread per staged inverse norm");
    __shared__ unsigned long long keys[NW * 16][CAP];
    __shared__ __attribute__((aligned(16))) float zs[SM_CHUNK][ZS];
    __shared__ float tis[SM_CHUNK];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const int64_t b0 = ((int64_t)blockIdx.x * NW + wave) * 16;            // first batch row of this wave
    const int64_t lo = (int64_t)blockIdx.y * slice, hi = min(n, lo + slice);
    unsigned long long (*kw)[CAP] = keys + wave * 16;

    float ua[E];
    load_frow<E>(Q + (size_t)q_ids[min(b0 + c, nq - 1)] * ld + E * q, ua);
    float qi[4];
    bool valid[4];
    int self[4];                                                         // the row that rows 4q + r never return
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t rb = min(b0 + 4 * q + r, nq - 1);
        valid[r] = b0 + 4 * q + r < nq;
        qi[r] = q_inv[q_ids[rb]];
        self[r] = self_ids ? self_ids[rb] : -1;
    }
    topk::Rows<CAP> st;

    // one 16-row block [cb, cb + 16) of the table: similarities from the accumulator, candidate test, append
    auto select = [&](const f32x4& acc, int64_t cb, float ti, unsigned deny) {
        const int64_t col = cb + c;
        const bool open = col < hi && !((deny >> c) & 1u);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float sim = (acc[r] * qi[r]) * ti;
            const unsigned long long key = make_key(sim, (unsigned)col);
            const bool pass = open && valid[r] && (int)col != self[r] && sim == sim && key > st.thr[r];
            topk::append<CAP>(kw, st, r, pass, key, c, q);
        }
    };

    f32x4 pf[PF];
    float pti = 0.f;
    auto fetch = [&](int64_t it0) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int v = tid + p * NT;
            if (v < NV) {
                const int i = v / (LD / 4), d = v - i * (LD / 4);
                pf[p] = *reinterpret_cast<const f32x4*>(T + (size_t)min(it0 + i, n - 1) * ld + 4 * d);
            }
        }
        if (tid < SM_CHUNK) pti = t_inv[min(it0 + tid, n - 1)];
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
        if (tid < SM_CHUNK) tis[tid] = pti;
    };

    const int64_t nch = hi > lo ? (hi - lo + SM_CHUNK - 1) / SM_CHUNK : 0;
    const uint32_t* aw = MASKED ? allow + lo / SM_CHUNK : nullptr;      // word of chunk 0 (lo is a multiple of 32)
    if (nch > 0) fetch(lo);
    for (int64_t ch = 0; ch < nch; ++ch) {
        const int64_t it0 = lo + ch * SM_CHUNK;
        unsigned word = ~0u;
        if constexpr (MASKED) word = __builtin_amdgcn_readfirstlane(aw[ch]);
        __syncthreads();                                 // every wave is done with the previous chunk
        stage();
        __syncthreads();
        if (ch + 1 < nch) fetch(it0 + SM_CHUNK);
        if (MASKED && word == 0u) continue;              // wave-uniform, the same in every wave
        float z0[E], z1[E];
        load_frow<E>(&zs[c][E * q], z0);
        load_frow<E>(&zs[16 + c][E * q], z1);
        const float ti0 = tis[c], ti1 = tis[16 + c];
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < E; ++e) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[e], z0[e], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[e], z1[e], acc1, 0, 0, 0);
        }
        select(acc0, it0, ti0, ~word & 0xFFFFu);
        select(acc1, it0 + 16, ti1, ~word >> 16);
        topk::compact_full_rows<CAP>(kw, st, topn, lane);
    }
    wave_lds_sync();
    for (int R = 0; R < 16; ++R)
        topk::finish_row<CAP>(kw, st, R, topn, lane, b0 + R, nq, (int64_t)blockIdx.y, part, top_val, top_idx, top_cnt);
}

template <int KB>
int launch_similar(int ld, int64_t nq, const int32_t* q_ids, const float* Q, const float* q_inv,
                   const int32_t* self_ids, int64_t n, int nsl, const float* T, const float* t_inv,
                   const uint32_t* allow, int topn, float* tv, int32_t* ti, int32_t* tc, unsigned long long* part,
                   hipStream_t st) {
    constexpr int NN = topk::ROWS_NARROW / 16, NWD = topk::ROWS_WIDE / 16;
    return topk::launch_by_width(allow ? k_similar<KB, NN, 128, true> : k_similar<KB, NN, 128, false>,
                                 allow ? k_similar<KB, NWD, 256, true> : k_similar<KB, NWD, 256, false>, topn, nq, nsl,
                                 st, ld, nq, q_ids, Q, q_inv, self_ids, n, walk::slice_items(n, nsl), T, t_inv, allow,
                                 topn, tv, ti, tc, part);
}

}  // namespace

extern "C" int als_row_inv_norms(int k, int ld, int64_t nrows, const float* T, float* inv_norm, void* stream) {
    const int kp = als_padded_k(k);
    if (kp < 0) return ALS_E_BADK;
    if (ld != kp || nrows < 0 || nrows >= ((int64_t)1 << 31)) return ALS_E_BADARG;
    if (nrows == 0) return 0;
    if (!T || !inv_norm) return ALS_E_BADARG;
    hipLaunchKernelGGL(k_row_inv_norms, dim3((unsigned)((nrows + 15) / 16)), dim3(256), 0, (hipStream_t)stream, ld,
                       nrows, T, inv_norm);
    return topk::launch_status();
}

extern "C" size_t als_similar_workspace_bytes(int64_t nq, int64_t n, int topn, int nslices) {
    return topk::workspace_bytes(nq, topk::rows_per_wg(topn), n, topn, nslices);
}

extern "C" int als_similar_topk(int k, int ld, int64_t nq, const int32_t* q_ids, const float* Q, const float* q_inv,
                                const int32_t* self_ids, int64_t n, const float* T, const float* t_inv,
                                const uint32_t* allow, int topn, int nslices, float* top_val, int32_t* top_idx,
                                int32_t* top_cnt, void* workspace, size_t workspace_bytes, void* stream) {
    const int bad = topk::check_shape(k, ld, nq, n, topn, ALS_TOPK_MAX, nslices);
    if (bad) return bad;
    if (nq == 0) return 0;
    if (!q_ids || !Q || !q_inv || !T || !t_inv || !top_val || !top_idx || !top_cnt) return ALS_E_BADARG;
    const topk::SlicePlan p = topk::plan(nq, topk::rows_per_wg(topn), n, nslices, nq * topn,
                                         sizeof(unsigned long long), workspace, workspace_bytes);
    if (!p.nsl) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    ALS_DISPATCH_KB(ld / 16, rc = launch_similar<KB>(ld, nq, q_ids, Q, q_inv, self_ids, n, p.nsl, T, t_inv, allow, topn,
                                                     top_val, top_idx, top_cnt, p.keys(), st));
    return rc != 0 ? rc : topk::merge_slices(p.nsl, p.keys(), nq, topn, top_val, top_idx, top_cnt, st);
}
