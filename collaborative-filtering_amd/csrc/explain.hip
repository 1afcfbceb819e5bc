// K11: explanation of a score - for one row of ratings (items S, the item side Z, b_i, mu held fixed) and a target
// item i, the split of the latent score u.z_i over the rated items, and the leverage of the target.
//
// The half-step user of fold-in (fold_in.hip) is linear in the ratings: with A = Z_S^T Z_S + lambda I and
// rho_j = r_j - mu - b_i[j] - bprev (bprev: the bias u was solved with), u = A^-1 sum_j z_j rho_j, so
//     u.z_i = sum_j (z_i^T A^-1 z_j) rho_j = sum_j weight[j] rho_j,      leverage = z_i^T A^-1 z_i.
//
// k_explain: one wave per work row, whatever its length.  The first half is k_fold_in's, statement by statement
// (fp64 Gram passes, panel Cholesky with g and h riding along, p, q, h.p, h.q, b_u / bprev), so b_u is the value
// fold-in rounds to fp32.  Then, for blocks of EX_TB targets: z_i to rows form, L y = z_i (leverage = |y|^2),
// L^T w = y, w to LDS in column order; one second pass over the row - lane t of a chunk of 64 ratings reads the row
// z_j and forms w.z_j for the EX_TB targets in fp64 (w is an LDS broadcast), contribution = weight * rho_j, a
// per-lane running sum for `latent`, and the selection: key = (float32(+-contribution), position in the row) under
// topk_common.hpp's total order - the positions of a row ascend with its item ids, so this is (contribution
// descending, item ascending) - kept as a sorted LDS list of <= 128 keys that is merged with the chunk's 64
// candidates by one bitonic sort, and only when a candidate beats the current topm-th key.  The kept entries are
// written from a recomputation of weight and contribution in fp64 (the same FMA chain as the pass, so float32 of
// what is written is the key that ordered it), never from the decoded key.
//
// Every reduction has a fixed order that depends on the row alone (lane t sums the ratings t, t + 64, ...; the
// butterfly adds the lanes), so a (row, target) result does not depend on the batch or on the other targets.
#include "als_device.hpp"
#include "als_hip.h"
#include "row_f64_common.hpp"
#include "topk_common.hpp"

namespace {

using namespace f64row;

constexpr int EX_TB = 4;            // targets that share one pass over the row
constexpr int EX_L = ALS_TOPK_MAX;  // keys of one target's list

// the gather source of the Gram passes (as fold_in.hip): Z with b_i as the "other" bias, tail lanes masked
struct ExplainSrc {
    const float* F;
    int ld;
    const int32_t* indices;
    const float* vals;
    const float* bias_other;
    int F_zero_row;
};

// d[t] = sum over columns of z[col] * w[t][col], columns ascending, one FMA chain per t (fp32 row, fp64 w in LDS)
template <int KB, int NT>
__device__ __forceinline__ void row_dots(const float* __restrict__ z, const double* w, double (&d)[NT]) {
    constexpr int KP = 16 * KB;
#pragma unroll
    for (int t = 0; t < NT; ++t) d[t] = 0.0;
#pragma unroll 2
    for (int j = 0; j < KP; j += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(z + j);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const double* wt = w + t * KP + j;
            d[t] = fma((double)v.x, wt[0], d[t]);
            d[t] = fma((double)v.y, wt[1], d[t]);
            d[t] = fma((double)v.z, wt[2], d[t]);
            d[t] = fma((double)v.w, wt[3], d[t]);
        }
    }
}

// list (sorted descending, 0 = no entry) <- the best EX_L of list + the 64 candidates `cand` (one per lane, 0 = none);
// V = 2 sorts list[0, 64) + candidates (enough for topm <= 64), V = 4 the whole list
template <int V>
__device__ __forceinline__ void merge_keys(unsigned long long* list, unsigned long long cand, int lane) {
    unsigned long long k[V];
#pragma unroll
    for (int v = 0; v < V; ++v) k[v] = 0ull;
    k[0] = list[lane];
    if constexpr (V == 4) k[1] = list[lane + 64];
    k[V / 2] = cand;
    topk::sort_desc<V>(k, lane);
    list[lane] = k[0];
    if constexpr (V == 4) list[lane + 64] = k[1];
}

template <int KB>
__global__ __launch_bounds__(64)
void k_explain(const als_explain_params P) {
    using C = F64Cfg<KB>;
    constexpr int KP = C::KP, NR = C::NR;
    __shared__ __attribute__((aligned(16))) double img[C::IMG];
    __shared__ __attribute__((aligned(16))) double wl[EX_TB * KP];
    __shared__ unsigned long long keys[EX_TB][EX_L];
    const int lane = threadIdx.x;
    const int c = lane & 15, q = lane >> 4;
    const int64_t wr = blockIdx.x;
    const int64_t row = P.rows ? (int64_t)P.rows[wr] : wr;
    const int64_t beg = P.indptr[row];
    const int len = (int)(P.indptr[row + 1] - beg);
    const ExplainSrc S{P.Z, P.ld, P.indices, P.vals, P.b_i, 0};
    const double mu = *P.mu;

    // ---- k_fold_in's factorisation and biases -----------------------------------------------------------
    double g[KB], h[KB], s = 0.0, s2 = 0.0;
#pragma unroll
    for (int b = 0; b < KB; ++b) { g[b] = 0.0; h[b] = 0.0; }
    gram_passes_f64<KB, 0, true, true>(S, beg, len, mu, 0.0, img, g, h, s, s2, lane);
    double g_p[NR], h_p[NR];
    to_rows_f64<KB>(g, h, g_p, h_p, lane);
    s = wave_sum_f64(s);
    wave_lds_sync();

    const double lam = (double)P.lambda_u + 1e-10;
    if (q == 0) {
        for (int J = 0; J < KB; ++J)
            img[blk64(J, J) * 256 + c * 16 + c] += (perm_to_col<KB>(16 * J + c) < P.k) ? lam : 1.0;
    }
    wave_lds_sync();

    double dinv[NR];
    double bu, bprev;                                                // b_T and the b_{T-1} that u_T is solved with
    {
        double b[2][NR], y[2][NR];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            b[0][rr] = g_p[rr]; b[1][rr] = h_p[rr];
            y[0][rr] = 0.0; y[1][rr] = 0.0; dinv[rr] = 0.0;
        }
        bool bad = false;
        cholesky_f64<KB, 2>(img, b, y, dinv, bad, lane);
        if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicMax(P.status, (int)(wr + 1));
        solve_lt_f64<KB>(img, y[0], dinv, lane);                // p = A^-1 g
        solve_lt_f64<KB>(img, y[1], dinv, lane);                // q = A^-1 h

        double hp = 0.0, hq = 0.0;
#pragma unroll
        for (int rr = 0; rr < NR; ++rr)
            if (lane + 64 * rr < KP) { hp = fma(h_p[rr], y[0][rr], hp); hq = fma(h_p[rr], y[1][rr], hq); }
        hp = wave_sum_f64(hp);
        hq = wave_sum_f64(hq);
        const double d = (double)len + (double)P.lambda_bu + 1e-10;
        if (P.n_sweeps == 0) {
            bu = (s - hp) / (d - hq);
            bprev = bu;
        } else {
            bu = 0.0; bprev = 0.0;
            for (int t = 0; t < P.n_sweeps; ++t) { bprev = bu; bu = (s - hp + bu * hq) / d; }
        }
    }
    if (lane == 0) P.b_u_out[wr] = bu;

    // ---- the targets, EX_TB at a time ----------------------------------------------------------------------
    const int64_t t_beg = P.t_ptr[wr], t_end = P.t_ptr[wr + 1];
    const int topm = P.topm;
    const double sign = P.largest ? 1.0 : -1.0;
    for (int64_t tg0 = t_beg; tg0 < t_end; tg0 += EX_TB) {
        const int nb = (int)min((int64_t)EX_TB, t_end - tg0);
        wave_lds_sync();                                        // the previous block is done with wl / keys
#pragma unroll 1
        for (int tb = 0; tb < EX_TB; ++tb) {
            double x[NR];
            if (tb < nb) {                                      // wave-uniform
                const int64_t it = min(max((int64_t)P.t_items[tg0 + tb], (int64_t)0), P.n - 1);
#pragma unroll
                for (int rr = 0; rr < NR; ++rr) {
                    const int i = lane + 64 * rr;
                    x[rr] = i < KP ? (double)P.Z[it * P.ld + perm_to_col<KB>(i)] : 0.0;
                }
                solve_l_f64<KB>(img, x, dinv, lane);            // y = L^-1 z_i
                double lev = 0.0;
#pragma unroll
                for (int rr = 0; rr < NR; ++rr)
                    if (lane + 64 * rr < KP) lev = fma(x[rr], x[rr], lev);
                lev = wave_sum_f64(lev);
                if (lane == 0) P.leverage[tg0 + tb] = lev;
                solve_lt_f64<KB>(img, x, dinv, lane);           // w = A^-1 z_i
            } else {
#pragma unroll
                for (int rr = 0; rr < NR; ++rr) x[rr] = 0.0;
            }
#pragma unroll
            for (int rr = 0; rr < NR; ++rr) {
                const int i = lane + 64 * rr;
                if (i < KP) wl[tb * KP + perm_to_col<KB>(i)] = x[rr];
            }
            keys[tb][lane] = 0ull;
            keys[tb][lane + 64] = 0ull;
        }
        wave_lds_sync();

        double lat[EX_TB];
        unsigned long long thr[EX_TB];                          // the current topm-th key (0: list not full)
#pragma unroll
        for (int tb = 0; tb < EX_TB; ++tb) { lat[tb] = 0.0; thr[tb] = 0ull; }
        for (int base = 0; base < len; base += 64) {
            const int t = base + lane;
            const bool ok = t < len;
            const int idx = ok ? P.indices[beg + t] : 0;
            const float v = ok ? P.vals[beg + t] : 0.f;
            const float bo = ok ? P.b_i[idx] : 0.f;
            const double rho = ((double)v - mu - (double)bo) - bprev;
            double wgt[EX_TB];
            row_dots<KB, EX_TB>(P.Z + (size_t)idx * P.ld, wl, wgt);
            unsigned long long key[EX_TB];
#pragma unroll
            for (int tb = 0; tb < EX_TB; ++tb) {
                const double ctr = wgt[tb] * rho;
                lat[tb] += ok ? ctr : 0.0;
                const float c32 = (float)(sign * ctr);
                const unsigned long long kk = topk::make_key(c32, (unsigned)t);
                key[tb] = (ok && c32 == c32 && kk > thr[tb]) ? kk : 0ull;
            }
#pragma unroll 1
            for (int tb = 0; tb < nb; ++tb) {
                unsigned long long kc = key[0];
#pragma unroll
                for (int e = 1; e < EX_TB; ++e) kc = (tb == e) ? key[e] : kc;
                if (__builtin_amdgcn_ballot_w64(kc != 0ull) == 0) continue;
                if (topm <= 64) merge_keys<2>(keys[tb], kc, lane);
                else merge_keys<4>(keys[tb], kc, lane);
                wave_lds_sync();
                const unsigned long long tk = keys[tb][topm - 1];
#pragma unroll
                for (int e = 0; e < EX_TB; ++e) thr[e] = (tb == e) ? tk : thr[e];
            }
        }
#pragma unroll
        for (int tb = 0; tb < EX_TB; ++tb) lat[tb] = wave_sum_f64(lat[tb]);

        // outputs of the block
#pragma unroll 1
        for (int tb = 0; tb < nb; ++tb) {
            const int64_t tg = tg0 + tb;
            double latent = lat[0];
#pragma unroll
            for (int e = 1; e < EX_TB; ++e) latent = (tb == e) ? lat[e] : latent;
            if (lane == 0) {
                const int64_t it = min(max((int64_t)P.t_items[tg], (int64_t)0), P.n - 1);
                P.latent[tg] = latent;
                P.score[tg] = mu + bu + (double)P.b_i[it] + latent;
            }
            int cnt = 0;
            for (int s0 = 0; s0 < topm; s0 += 64) {
                const int sl = s0 + lane;
                const unsigned long long kk = sl < topm ? keys[tb][sl] : 0ull;
                const bool kept = kk != 0ull;
                cnt += __popcll(__builtin_amdgcn_ballot_w64(kept));
                const int pos = kept ? topk::key_index(kk) : 0;
                const int idx = kept ? P.indices[beg + pos] : 0;
                const float v = kept ? P.vals[beg + pos] : 0.f;
                const float bo = kept ? P.b_i[idx] : 0.f;
                const double rho = ((double)v - mu - (double)bo) - bprev;
                double wgt[1];
                row_dots<KB, 1>(P.Z + (size_t)idx * P.ld, wl + tb * KP, wgt);
                if (sl < topm) {
                    P.top_item[tg * topm + sl] = kept ? idx : -1;
                    P.top_contrib[tg * topm + sl] = kept ? wgt[0] * rho : 0.0;
                    P.top_weight[tg * topm + sl] = kept ? wgt[0] : 0.0;
                }
            }
            if (lane == 0) P.top_cnt[tg] = cnt;
        }
    }
}

}  // namespace

extern "C" int als_explain(const als_explain_params* p, void* stream) {
    if (!p) return ALS_E_BADARG;
    const int kp = als_padded_k(p->k);
    if (kp < 0) return ALS_E_BADK;
    if (p->ld != kp || p->nrows < 0 || p->nrows >= INT32_MAX || p->n_sweeps < 0 || p->n < 1 ||
        p->n * (int64_t)kp >= ((int64_t)1 << 31) || !(p->lambda_u >= 0.f) || !(p->lambda_bu >= 0.f) ||
        p->topm < 1 || p->topm > ALS_TOPK_MAX)
        return ALS_E_BADARG;
    if (p->nrows == 0) return 0;
    if (!p->indptr || !p->indices || !p->vals || !p->Z || !p->b_i || !p->mu || !p->t_ptr || !p->t_items ||
        !p->score || !p->latent || !p->leverage || !p->top_item || !p->top_contrib || !p->top_weight ||
        !p->top_cnt || !p->b_u_out || !p->status)
        return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p->nrows);
    ALS_DISPATCH_KB(kp / 16, hipLaunchKernelGGL(k_explain<KB>, grid, dim3(64), 0, st, *p));
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}
