// K12: diversified top-N - greedy maximal-marginal-relevance re-ranking of a candidate pool (als_mmr_rerank) and
// the intra-list diversity of id lists (als_list_diversity).  DESIGN.md section 18 has the definitions.
//
// Both kernels run one wave per batch row in a one-wave workgroup (rows never exchange anything; see KCfg::WPW).
//
// pool_gram (shared): the row's ids go to LDS - the list ends at the first -1 or the first id outside [0, n), which
// is never dereferenced; positions behind the end take item 0, their Gram rows are computed and never read - and
// the lower 16 x 16 tiles of the list's Gram G = Z_S Z_S^T are formed with the v_mfma_f32_16x16x4_f32 chain of
// k_recommend / k_predict_dense: lane (c, q) holds k = 4 KB q + e of row c in step e, both operands straight from
// global memory / L2, block row I in registers while J runs 0 ... I.  A product does not depend on which operand a
// row is and the k order is fixed, so G[a][b] is bitwise the same whatever positions a and b have in a list.
// The fp32 image is [MP][MP + 1]: with an ODD stride the greedy step's read of "everything against p" - lane j
// reads [max(j, p)][min(j, p)], a row read for j < p and a column read for j > p - lands on bank (j + p) % 32 either
// way, conflict-free; the tile stores are 2-way (36 x 4 stores per row at most, against up to 128 greedy steps).
// 1 / sqrt(G_jj) is kept per position; sim(a, b) = G[a][b] * (rn[a] * rn[b]) - one stored G per unordered pair and
// a commutative product: symmetric by construction.
//
// Greedy phase (k_mmr_rerank): lane j owns candidates j and j + 64 - relevance, running maximum similarity, chosen
// flag in registers.  A step is the wave maximum of a 64-bit key (topk_common.hpp: encoded objective, inverted
// position - a total order, ties to the lower position) and one LDS read per owned candidate.  No atomics, no
// global traffic.
//
// ILD: lane t owns list positions t and t + 64 and adds 1 - sim(t, s) for s = 0 ... t - 1 in that order, in fp64;
// the lanes are summed by a fixed butterfly.  The order depends on the list alone, so k_list_diversity on a list
// that k_mmr_rerank returned gives bitwise the ILD k_mmr_rerank wrote for it.
#include "als_device.hpp"
#include "als_hip.h"
#include "topk_common.hpp"

namespace {

constexpr int64_t DV_MAX_GRID = 1 << 20;     // workgroups of a launch; the rows beyond are taken in further rounds

template <int MP>
struct PoolLds {
    static constexpr int ST = MP + 1;
    float g[MP * ST];       // lower triangle of the Gram (diagonal tiles whole)
    float rn[MP];           // 1 / sqrt(G_jj), 0 for a zero row
    int id[MP];             // item of position j (0 behind the end of the list)
    int pick[MP];           // pool position of list position t
};

// ids of one row -> lds.id, Gram -> lds.g, inverse root norms -> lds.rn; returns the length of the list
template <int KB, int MP>
__device__ __forceinline__ int pool_gram(const float* __restrict__ Z, int ld, int64_t n,
                                         const int32_t* __restrict__ src, int len, int lane, PoolLds<MP>& lds) {
    constexpr int E = 4 * KB, NR = MP / 64, ST = PoolLds<MP>::ST;
    const int c = lane & 15, q = lane >> 4;
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
    wave_lds_sync();
    const int nba = (cnt + 15) >> 4;
    for (int I = 0; I < nba; ++I) {
        float a[E], b[E];
        load_frow<E>(Z + (size_t)lds.id[16 * I + c] * ld + E * q, a);
        auto tile = [&](const float (&bb)[E], int J) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < E; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], bb[e], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) lds.g[(16 * I + 4 * q + r) * ST + 16 * J + c] = acc[r];
        };
        for (int J = 0; J < I; ++J) {
            load_frow<E>(Z + (size_t)lds.id[16 * J + c] * ld + E * q, b);
            tile(b, J);
        }
        tile(a, I);
    }
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int j = lane + 64 * r;
        const float gjj = j < cnt ? lds.g[j * ST + j] : 0.f;
        lds.rn[j] = gjj > 0.f ? 1.0f / sqrtf(gjj) : 0.f;
    }
    wave_lds_sync();
    return cnt;
}

template <int MP>
__device__ __forceinline__ float pool_sim(const PoolLds<MP>& lds, int a, float rna, int b, float rnb) {
    return lds.g[max(a, b) * PoolLds<MP>::ST + min(a, b)] * (rna * rnb);
}

// mean of 1 - sim over the unordered pairs of the list lds.pick[0 .. len), NaN for len < 2 (wave-uniform)
template <int MP>
__device__ __forceinline__ float list_ild(const PoolLds<MP>& lds, int len, int lane) {
    constexpr int NR = MP / 64;
    int pt[NR];
    float rt[NR];
    double acc = 0.0;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        pt[r] = lds.pick[min(lane + 64 * r, MP - 1)];
        pt[r] = (lane + 64 * r < len) ? pt[r] : 0;
        rt[r] = lds.rn[pt[r]];
    }
    for (int s = 0; s + 1 < len; ++s) {
        const int ps = lds.pick[s];
        const float rs = lds.rn[ps];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const float sim = pool_sim<MP>(lds, pt[r], rt[r], ps, rs);
            const int t = lane + 64 * r;
            acc += (t > s && t < len) ? 1.0 - (double)sim : 0.0;
        }
    }
    const double tot = wave_sum_d(acc);
    return len < 2 ? __int_as_float(0x7FC00000) : (float)(tot / (0.5 * (double)len * (double)(len - 1)));
}

// one row of als_mmr_rerank
template <int KB, int MP>
__device__ __forceinline__ void mmr_row(PoolLds<MP>& lds, int64_t row, int lane, int ld, int64_t n,
                                        const float* __restrict__ Z, int pool, const float* __restrict__ cand_val,
                                        const int32_t* __restrict__ cand_idx, float lambda, int topn,
                                        float* __restrict__ top_val, int32_t* __restrict__ top_idx,
                                        int32_t* __restrict__ top_cnt, float* __restrict__ top_ild) {
    constexpr int NR = MP / 64;
    const float* cv = cand_val + row * pool;
    const int cnt = pool_gram<KB, MP>(Z, ld, n, cand_idx + row * pool, pool, lane, lds);
    const int nsel = min(topn, cnt);

    float base[NR], rin[NR], msim[NR];
    bool open[NR];                                        // a candidate that has not been chosen
    float lo = INFINITY, hi = -INFINITY;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const int j = lane + 64 * r;
        open[r] = j < cnt;
        base[r] = open[r] ? cv[j] : 0.f;
        lo = fminf(lo, open[r] ? base[r] : INFINITY);
        hi = fmaxf(hi, open[r] ? base[r] : -INFINITY);
        rin[r] = lds.rn[j];
        msim[r] = 0.f;                                    // the maximum over the empty set
    }
    lo = wave_min_f(lo);
    hi = wave_max_f(hi);
    const float range = hi - lo;
    const bool spread = range > 0.f && range < INFINITY;  // false for 0, inf and NaN
#pragma unroll
    for (int r = 0; r < NR; ++r) base[r] = (1.0f - lambda) * (spread ? (base[r] - lo) / range : 0.f);

    for (int t = 0; t < nsel; ++t) {
        unsigned long long key = 0ull;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const unsigned long long kr = topk::make_key(base[r] - lambda * msim[r], (unsigned)(lane + 64 * r));
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
        const float rp = lds.rn[p];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const int j = lane + 64 * r;
            const float sim = pool_sim<MP>(lds, j, rin[r], p, rp);
            msim[r] = t == 0 ? sim : fmaxf(msim[r], sim);
            open[r] = open[r] && j != p;
        }
    }
    wave_lds_sync();
    for (int t = lane; t < topn; t += 64) {
        const bool ok = t < nsel;
        const int p = ok ? lds.pick[t] : 0;
        top_idx[row * topn + t] = ok ? lds.id[p] : -1;
        top_val[row * topn + t] = ok ? cv[p] : -INFINITY;
    }
    if (lane == 0) top_cnt[row] = nsel;
    if (top_ild) {
        const float ild = list_ild<MP>(lds, nsel, lane);
        if (lane == 0) top_ild[row] = ild;
    }
}

template <int KB, int MP>
__global__ __launch_bounds__(64)
void k_mmr_rerank(int ld, int64_t nrows, int64_t n, const float* __restrict__ Z, int pool,
                  const float* __restrict__ cand_val, const int32_t* __restrict__ cand_idx, float lambda, int topn,
                  float* __restrict__ top_val, int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt,
                  float* __restrict__ top_ild) {
    __shared__ PoolLds<MP> lds;
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {      // (more than DV_MAX_GRID rows)
        mmr_row<KB, MP>(lds, row, lane, ld, n, Z, pool, cand_val, cand_idx, lambda, topn, top_val, top_idx, top_cnt,
                        top_ild);
        wave_lds_sync();                                                 // the image goes to the next row
    }
}

template <int KB, int MP>
__global__ __launch_bounds__(64)
void k_list_diversity(int ld, int64_t nrows, int64_t n, const float* __restrict__ Z, int len,
                      const int32_t* __restrict__ idx, float* __restrict__ ild_out) {
    constexpr int NR = MP / 64;
    __shared__ PoolLds<MP> lds;
    const int lane = threadIdx.x;
    for (int64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
        const int cnt = pool_gram<KB, MP>(Z, ld, n, idx + row * len, len, lane, lds);
#pragma unroll
        for (int r = 0; r < NR; ++r) lds.pick[lane + 64 * r] = lane + 64 * r;
        wave_lds_sync();
        const float ild = list_ild<MP>(lds, cnt, lane);
        if (lane == 0) ild_out[row] = ild;
        wave_lds_sync();
    }
}

template <int KB>
int launch_mmr(int ld, int64_t nrows, int64_t n, const float* Z, int pool, const float* cv, const int32_t* ci,
               float lambda, int topn, float* tv, int32_t* ti, int32_t* tc, float* ild, hipStream_t st) {
    auto kern = pool <= 64 ? k_mmr_rerank<KB, 64> : k_mmr_rerank<KB, 128>;
    hipLaunchKernelGGL(kern, dim3((unsigned)min(nrows, DV_MAX_GRID)), dim3(64), 0, st, ld, nrows, n, Z, pool, cv, ci,
                       lambda, topn, tv, ti, tc, ild);
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}

template <int KB>
int launch_ild(int ld, int64_t nrows, int64_t n, const float* Z, int len, const int32_t* idx, float* ild,
               hipStream_t st) {
    auto kern = len <= 64 ? k_list_diversity<KB, 64> : k_list_diversity<KB, 128>;
    hipLaunchKernelGGL(kern, dim3((unsigned)min(nrows, DV_MAX_GRID)), dim3(64), 0, st, ld, nrows, n, Z, len, idx,
                       ild);
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}

}  // namespace

extern "C" int als_mmr_rerank(int k, int ld, int64_t nrows, int64_t n, const float* Z, int pool,
                              const float* cand_val, const int32_t* cand_idx, float lambda, int topn, float* top_val,
                              int32_t* top_idx, int32_t* top_cnt, float* top_ild, void* stream) {
    const int kp = als_padded_k(k);
    if (kp < 0) return ALS_E_BADK;
    if (ld != kp || nrows < 0 || n < 1 || n >= ((int64_t)1 << 31) || pool < 1 ||
        pool > ALS_TOPK_MAX || topn < 1 || topn > pool || !(lambda >= 0.f && lambda <= 1.f))
        return ALS_E_BADARG;
    if (nrows == 0) return 0;
    if (!Z || !cand_val || !cand_idx || !top_val || !top_idx || !top_cnt) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    ALS_DISPATCH_KB(ld / 16, return launch_mmr<KB>(ld, nrows, n, Z, pool, cand_val, cand_idx, lambda, topn, top_val, top_idx,
                                                   top_cnt, top_ild, st));
}

extern "C" int als_list_diversity(int k, int ld, int64_t nrows, int64_t n, const float* Z, int len,
                                  const int32_t* idx, float* ild, void* stream) {
    const int kp = als_padded_k(k);
    if (kp < 0) return ALS_E_BADK;
    if (ld != kp || nrows < 0 || n < 1 || n >= ((int64_t)1 << 31) || len < 1 ||
        len > ALS_TOPK_MAX)
        return ALS_E_BADARG;
    if (nrows == 0) return 0;
    if (!Z || !idx || !ild) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    ALS_DISPATCH_KB(ld / 16, return launch_ild<KB>(ld, nrows, n, Z, len, idx, ild, st));
}
