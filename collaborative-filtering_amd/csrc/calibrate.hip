// K17: calibrated top-N - the category profile of a row of ratings (als_category_profile), the greedy
// genre-proportional re-ranking of a candidate pool (als_calibrated_rerank) and the miscalibration of id lists
// (als_list_miscalibration).  DESIGN.md section 25 has the definitions.
//
// All three kernels run one wave per batch row in a one-wave workgroup (rows never exchange anything; see KCfg::WPW).
//
// k_category_profile: lane c owns category c.  The wave reads 64 item ids of the row at a time and walks them in CSR
// order; every lane reads C[id][c] - one coalesced row per item - and adds it in fp64.  An id outside [0, n) reads
// row 0 and adds nothing.
//
// pool_rows (shared by the other two): the row's ids go to LDS - the list ends at the first -1 or the first id outside
// [0, n), which is never dereferenced - and the category rows of the list are gathered into an fp32 image
// [MP + 1][ldc + 1] in dynamic LDS, 64 / ldc rows per wave load.  ldc is a multiple of 16, so the stride is ODD: lane
// j's walk over the categories of "its" row lands on bank (j ST + c) % 32, a bijection of the 32 lanes of a half -
// conflict-free.  Row MP is all zero: the "no candidate" row, which makes the KL of a state the KL of that row.
// The row's target lives in LDS as one float4 per category {p_c, log2 p_c, S_c, -}: one broadcast ds_read_b128 per
// category and step.
//
// Greedy phase (k_calibrated_rerank): lane j owns candidates j and j + 64 - relevance, has-a-category flag, open
// flag in registers.  A step is, per owned candidate, a walk over the categories with p_c > 0 (a wave-uniform
// branch: p belongs to the row) - one division, one v_log_f32, three FMAs per category -, the wave maximum of the
// 64-bit key (topk_common.hpp: encoded objective, inverted position - a total order, ties to the lower position)
// and the update of S by the lanes c.  No atomics, no global traffic behind the gather.
//
// The KL of a state is computed by ONE function (cand_kl) with explicit FMAs, so k_list_miscalibration on a list
// that k_calibrated_rerank returned - same rows, same order of the additions into S - gives bitwise its top_kl.
#include "als_device.hpp"
#include "als_hip.h"
#include "topk_common.hpp"

namespace {

constexpr int64_t CB_MAX_GRID = 1 << 20;     // workgroups of a launch; the rows beyond are taken in further rounds
constexpr int CB_MAX_CAT = 64;               // categories: one lane each
constexpr float CB_LN2 = 0.693147180559945309f;

template <int MP>
struct CalLds {
    f32x4 st[CB_MAX_CAT];   // x = p_c, y = log2 p_c (0 where p_c = 0), z = S_c
    int id[MP];             // item of position j (0 behind the end of the list)
    int pick[MP];           // pool position of list position t
};

__host__ __device__ constexpr size_t cal_image_bytes(int mp, int ldc) { return sizeof(float) * (size_t)(mp + 1) * (ldc + 1); }

// how the lanes share a wave load of category rows: lane = (sub, c) with c < ldc, sub < 64 / ldc
struct RowLanes {
    int sub, c, rpi;
    __device__ RowLanes(int lane, int ldc) : sub(lane / ldc), c(lane - (lane / ldc) * ldc), rpi(64 / ldc) {}
};

// ids of one row -> lds.id, their category rows -> cat, the target -> lds.st with S = 0; returns the list's length
template <int MP>
__device__ __forceinline__ int pool_rows(const float* __restrict__ C, int ncat, int ldc, int64_t n,
                                         const float* __restrict__ prow, const int32_t* __restrict__ src, int len,
                                         int lane, const RowLanes& rl, CalLds<MP>& lds, float* __restrict__ cat) {
    constexpr int NR = MP / 64;
    const int ST = ldc + 1;
    int v[NR];
    int cnt = MP;
#pragma unroll
    for (int r = NR - 1; r >= 0; --r) {
        const int j = lane + 64 * r;
        v[r] = j < len ? src[j] : -1;
        const unsigned long long bad = __ballot(!(v[r] >= 0 && (int64_t)v[r] < n));
        if (bad) cnt = 64 * r + __builtin_ctzll(bad);
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) lds.id[lane + 64 * r] = (lane + 64 * r < cnt) ? v[r] : 0;
    const float pc = lane < ncat ? prow[lane] : 0.f;
    f32x4 s = {pc, pc > 0.f ? log2f(pc) : 0.f, 0.f, 0.f};
    lds.st[lane] = s;
    if (lane <= ldc) cat[MP * ST + lane] = 0.f;                          // the "no candidate" row
    wave_lds_sync();
#pragma unroll 4
    for (int j0 = 0; j0 < cnt; j0 += rl.rpi) {
        const int j = j0 + rl.sub;
        if (rl.sub < rl.rpi && j < cnt) cat[j * ST + rl.c] = C[(size_t)lds.id[j] * ldc + rl.c];
    }
    wave_lds_sync();
    return cnt;
}

// KL_j / ln 2 of the state (S + row j[r], cj[r] categorised items) for the NR rows a lane names: the sum over the
// categories with p_c > 0, ascending, of p_c (log2 p_c - log2((1 - alpha) q_c + alpha p_c)), q_c = (S_c + C_jc) / cj
// (0 when cj = 0), times ln 2
template <int MP, int NR>
__device__ __forceinline__ void cand_kl(const CalLds<MP>& lds, const float* __restrict__ cat, int ST, int ncat,
                                        const int (&j)[NR], const float (&cj)[NR], float alpha, float (&kl)[NR]) {
    const float oma = 1.0f - alpha;
    float acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.f;
    for (int c = 0; c < ncat; ++c) {
        const f32x4 s = lds.st[c];
        const float pc = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(s.x)));
        if (pc > 0.f) {                                                  // wave-uniform: p belongs to the row
            const float ap = alpha * pc;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const float q = cj[r] > 0.f ? (s.z + cat[j[r] * ST + c]) / cj[r] : 0.f;
                const float qt = fmaf(oma, q, ap);
                acc[r] = fmaf(pc, s.y - __builtin_amdgcn_logf(qt), acc[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) kl[r] = CB_LN2 * acc[r];
}

// pool position p joins the list: S += its row (lane c adds category c), returns has_p (wave-uniform)
template <int MP>
__device__ __forceinline__ int add_pick(CalLds<MP>& lds, const float* __restrict__ cat, int ST, int ncat, int p,
                                        int lane) {
    const float x = lane < ncat ? cat[p * ST + lane] : 0.f;
    if (lane < ncat) lds.st[lane].z += x;
    const int has = __ballot(x > 0.f) != 0ull;
    wave_lds_sync();
    return has;
}

// KL of the state in lds.st with cntf categorised items (wave-uniform)
template <int MP>
__device__ __forceinline__ float state_kl(const CalLds<MP>& lds, const float* __restrict__ cat, int ST, int ncat,
                                          float cntf, float alpha) {
    const int j[1] = {MP};
    const float cj[1] = {cntf};
    float kl[1];
    cand_kl<MP, 1>(lds, cat, ST, ncat, j, cj, alpha, kl);
    return kl[0];
}

template <int MP>
__global__ __launch_bounds__(64)
void k_calibrated_rerank(int ncat, int ldc, int64_t nrows, int64_t n, const float* __restrict__ C,
                         const float* __restrict__ P, int pool, const float* __restrict__ cand_val,
                         const int32_t* __restrict__ cand_idx, float lambda, float alpha, int topn,
                         float* __restrict__ top_val, int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt,
                         float* __restrict__ top_kl) {
    constexpr int NR = MP / 64;
    __shared__ CalLds<MP> lds;
    extern __shared__ float cat[];                                       // [MP + 1][ldc + 1]
    const int lane = threadIdx.x;
    const int ST = ldc + 1;
    const RowLanes rl(lane, ldc);
    for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {      // (more than CB_MAX_GRID rows)
        const float* cv = cand_val + row * pool;
        const int cnt = pool_rows<MP>(C, ncat, ldc, n, P + row * ldc, cand_idx + row * pool, pool, lane, rl, lds, cat);
        const int nsel = min(topn, cnt);

        float base[NR], has[NR];
        int jr[NR];
        bool open[NR];                                                   // a candidate that has not been chosen
        float lo = INFINITY, hi = -INFINITY;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int j = lane + 64 * r;
            open[r] = j < cnt;
            jr[r] = open[r] ? j : MP;                                    // behind the end: the zero row
            base[r] = open[r] ? cv[j] : 0.f;
            lo = fminf(lo, open[r] ? base[r] : INFINITY);
            hi = fmaxf(hi, open[r] ? base[r] : -INFINITY);
            bool h = false;
            for (int c = 0; c < ncat; ++c) h |= cat[jr[r] * ST + c] > 0.f;
            has[r] = h ? 1.f : 0.f;
        }
        lo = wave_min_f(lo);
        hi = wave_max_f(hi);
        const float range = hi - lo;
        const bool spread = range > 0.f && range < INFINITY;             // false for 0, inf and NaN
#pragma unroll
        for (int r = 0; r < NR; ++r) base[r] = (1.0f - lambda) * (spread ? (base[r] - lo) / range : 0.f);

        float cntf = 0.f;                                                // chosen items with a category
        for (int t = 0; t < nsel; ++t) {
            float cj[NR], kl[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) cj[r] = cntf + has[r];
            cand_kl<MP, NR>(lds, cat, ST, ncat, jr, cj, alpha, kl);
            unsigned long long key = 0ull;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const unsigned long long kr = topk::make_key(fmaf(-lambda, kl[r], base[r]), (unsigned)(lane + 64 * r));
                key = max(key, open[r] ? kr : 0ull);
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const unsigned long long other = topk::shfl_xor_u64(key, o);      // the read first, then the select
                key = max(key, other);
            }
            // nsel <= cnt: an open candidate is left, and every real key is > 0, so p is one of them
            const int p = __builtin_amdgcn_readfirstlane(topk::key_index(key)) & (MP - 1);
            if (lane == 0) lds.pick[t] = p;
            cntf += (float)add_pick<MP>(lds, cat, ST, ncat, p, lane);
#pragma unroll
            for (int r = 0; r < NR; ++r) open[r] = open[r] && lane + 64 * r != p;
        }
        wave_lds_sync();
        for (int t = lane; t < topn; t += 64) {
            const bool ok = t < nsel;
            const int p = ok ? lds.pick[t] : 0;
            top_idx[row * topn + t] = ok ? lds.id[p] : -1;
            top_val[row * topn + t] = ok ? cv[p] : -INFINITY;
        }
        if (lane == 0) top_cnt[row] = nsel;
        if (top_kl) {
            const float kl = state_kl<MP>(lds, cat, ST, ncat, cntf, alpha);
            if (lane == 0) top_kl[row] = kl;
        }
        wave_lds_sync();                                                 // the image goes to the next row
    }
}

template <int MP>
__global__ __launch_bounds__(64)
void k_list_miscalibration(int ncat, int ldc, int64_t nrows, int64_t n, const float* __restrict__ C,
                           const float* __restrict__ P, int len, const int32_t* __restrict__ idx, float alpha,
                           float* __restrict__ kl_out) {
    __shared__ CalLds<MP> lds;
    extern __shared__ float cat[];
    const int lane = threadIdx.x;
    const int ST = ldc + 1;
    const RowLanes rl(lane, ldc);
    for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int cnt = pool_rows<MP>(C, ncat, ldc, n, P + row * ldc, idx + row * len, len, lane, rl, lds, cat);
        float cntf = 0.f;
        for (int t = 0; t < cnt; ++t) cntf += (float)add_pick<MP>(lds, cat, ST, ncat, t, lane);     // identity picks
        const float kl = state_kl<MP>(lds, cat, ST, ncat, cntf, alpha);
        if (lane == 0) kl_out[row] = kl;
        wave_lds_sync();
    }
}

__global__ __launch_bounds__(64)
void k_category_profile(int ncat, int ldc, int64_t nrows, const int32_t* __restrict__ rows,
                        const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n,
                        const float* __restrict__ C, float* __restrict__ P_out) {
    const int lane = threadIdx.x;
    const int c = min(lane, ldc - 1);
    for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int64_t r = rows ? (int64_t)rows[row] : row;
        const int64_t beg = indptr[r], end = indptr[r + 1];
        double acc = 0.0;
        int cnt = 0;                                                     // items of the row with a category
        for (int64_t e0 = beg; e0 < end; e0 += 64) {
            const int m = __builtin_amdgcn_readfirstlane(end - e0 < 64 ? (int)(end - e0) : 64);
            const int idv = lane < m ? indices[e0 + lane] : -1;
#pragma unroll 4
            for (int t = 0; t < m; ++t) {                                // CSR order
                const int id = __builtin_amdgcn_readlane(idv, t);
                const bool ok = id >= 0 && (int64_t)id < n;
                const float v = C[(size_t)(ok ? id : 0) * ldc + c];      // an id outside the table reads row 0 ...
                const float x = (ok && lane < ncat) ? v : 0.f;           // ... and adds nothing
                acc += (double)x;
                cnt += __ballot(x > 0.f) != 0ull;
            }
        }
        if (lane < ldc) P_out[row * ldc + lane] = cnt ? (float)(acc / (double)cnt) : 0.f;
    }
}

int check_cat(int ncat, int ldc) {
    return (ncat < 1 || ncat > CB_MAX_CAT || ldc != 16 * ((ncat + 15) / 16)) ? ALS_E_BADK : 0;
}

}  // namespace

extern "C" int als_category_profile(int ncat, int ldc, int64_t nrows, const int32_t* rows, const int64_t* indptr,
                                    const int32_t* indices, int64_t n, const float* C, float* P_out, void* stream) {
    if (check_cat(ncat, ldc)) return ALS_E_BADK;
    if (nrows < 0 || n < 1 || n >= ((int64_t)1 << 31)) return ALS_E_BADARG;
    if (nrows == 0) return 0;
    if (!indptr || !indices || !C || !P_out) return ALS_E_BADARG;
    hipLaunchKernelGGL(k_category_profile, dim3((unsigned)min(nrows, CB_MAX_GRID)), dim3(64), 0, (hipStream_t)stream,
                       ncat, ldc, nrows, rows, indptr, indices, n, C, P_out);
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}

extern "C" int als_calibrated_rerank(int ncat, int ldc, int64_t nrows, int64_t n, const float* C, const float* P,
                                     int pool, const float* cand_val, const int32_t* cand_idx, float lambda,
                                     float alpha, int topn, float* top_val, int32_t* top_idx, int32_t* top_cnt,
                                     float* top_kl, void* stream) {
    if (check_cat(ncat, ldc)) return ALS_E_BADK;
    if (nrows < 0 || n < 1 || n >= ((int64_t)1 << 31) || pool < 1 || pool > ALS_TOPK_MAX || topn < 1 ||
        topn > pool || !(lambda >= 0.f && lambda <= 1.f) || !(alpha > 0.f && alpha < 1.f))
        return ALS_E_BADARG;
    if (nrows == 0) return 0;
    if (!C || !P || !cand_val || !cand_idx || !top_val || !top_idx || !top_cnt) return ALS_E_BADARG;
    const int mp = pool <= 64 ? 64 : 128;
    auto kern = pool <= 64 ? k_calibrated_rerank<64> : k_calibrated_rerank<128>;
    hipLaunchKernelGGL(kern, dim3((unsigned)min(nrows, CB_MAX_GRID)), dim3(64), cal_image_bytes(mp, ldc),
                       (hipStream_t)stream, ncat, ldc, nrows, n, C, P, pool, cand_val, cand_idx, lambda, alpha, topn,
                       top_val, top_idx, top_cnt, top_kl);
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}

extern "C" int als_list_miscalibration(int ncat, int ldc, int64_t nrows, int64_t n, const float* C, const float* P,
                                       int len, const int32_t* idx, float alpha, float* kl, void* stream) {
    if (check_cat(ncat, ldc)) return ALS_E_BADK;
    if (nrows < 0 || n < 1 || n >= ((int64_t)1 << 31) || len < 1 || len > ALS_TOPK_MAX ||
        !(alpha > 0.f && alpha < 1.f))
        return ALS_E_BADARG;
    if (nrows == 0) return 0;
    if (!C || !P || !idx || !kl) return ALS_E_BADARG;
    const int mp = len <= 64 ? 64 : 128;
    auto kern = len <= 64 ? k_list_miscalibration<64> : k_list_miscalibration<128>;
    hipLaunchKernelGGL(kern, dim3((unsigned)min(nrows, CB_MAX_GRID)), dim3(64), cal_image_bytes(mp, ldc),
                       (hipStream_t)stream, ncat, ldc, nrows, n, C, P, len, idx, alpha, kl);
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}
