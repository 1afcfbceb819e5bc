// K9b: item fold-in - factors and biases of items outside the fit, the user side (U, b_u, mu) and the fitted items'
// V held fixed: the fit's item half-step (scripts/als.py:436-466) for new columns.
//
// For one item with raters S (n = |S|), ratings r and graph row N (fitted items j, weights s_j, D = sum_j s_j):
//     A = U_S^T U_S + lambda I,  g = U_S^T (r - mu - b_u[S]) + alpha sum_j s_j V_j,  h = U_S^T 1,
//     s = sum (r - mu - b_u[S]),  d = n + lambda_bi + 1e-10,
//     lambda = (lambda_v or lambda_v / sqrt(n + 1) under pop_reg) + 1e-10 + alpha D,
// then the scalar recurrence / bordered fixed point of fold_in.hip.  As in the fit, the residual ignores the feature
// part of Z (scripts/als.py:447) and the graph term reads V, not Z (:458).
//
// k_fold_in_items: one wave per item, whatever its rater count, fp64 throughout, on row_f64_common.hpp like
// k_fold_in: the fp64 Gram passes gather U rows by rater id (tail lanes masked); the neighbour sum and D run in fp64
// over the graph row in storage order, eight V rows in flight, each lane for its own perm positions, and are added
// to g and the diagonal before the factorisation.  An item without ratings is solved too (A = lambda I, h = 0):
// v = alpha sum_j s_j V_j / lambda, b = 0.  A sibling of k_fold_in in a translation unit of its own: sharing
// fold_in.hip changed k_fold_in's instruction schedule, which must stay as it was.
#include <math.h>

#include "als_device.hpp"
#include "als_hip.h"
#include "row_f64_common.hpp"

namespace {

using namespace f64row;

// the gather source of the Gram passes: U with b_u as the "other" bias; tail lanes gather row 0 and are masked
struct FoldItemSrc {
    const float* F;
    int ld;
    const int32_t* indices;
    const float* vals;
    const float* bias_other;
    int F_zero_row;
};

template <int KB>
__global__ __launch_bounds__(64)
void k_fold_in_items(const als_fold_in_items_params P) {
    using C = F64Cfg<KB>;
    constexpr int KP = C::KP, NR = C::NR;
    constexpr int NG = 8;                                   // neighbour rows whose V loads are in flight together
    __shared__ __attribute__((aligned(16))) double img[C::IMG];
    const int lane = threadIdx.x;
    const int c = lane & 15, q = lane >> 4;
    const int64_t row = blockIdx.x;
    const int64_t beg = P.indptr[row];
    const int len = (int)(P.indptr[row + 1] - beg);
    const FoldItemSrc S{P.U, P.ld, P.indices, P.vals, P.b_u, 0};
    const double mu = *P.mu;

    double g[KB], h[KB], s = 0.0, s2 = 0.0;
#pragma unroll
    for (int b = 0; b < KB; ++b) { g[b] = 0.0; h[b] = 0.0; }
    gram_passes_f64<KB, 0, true, true>(S, beg, len, mu, 0.0, img, g, h, s, s2, lane);
    double g_p[NR], h_p[NR];
    to_rows_f64<KB>(g, h, g_p, h_p, lane);
    s = wave_sum_f64(s);

    // graph term: nb = sum_j s_ij V_j and D = sum_j s_ij in fp64, neighbours in storage order (every lane runs the
    // same chain for its own perm positions)
    double deg = 0.0;
    if (P.S_ptr) {
        int col[NR];                                        // storage column of the lane's perm positions
        bool live[NR];                                      // ... and whether it is one of the k real ones
        double nb[NR];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int i = lane + 64 * rr;
            col[rr] = perm_to_col<KB>(min(i, KP - 1));
            live[rr] = i < KP && col[rr] < P.k;
            nb[rr] = 0.0;
        }
        const int64_t sbeg = P.S_ptr[row];
        const int slen = (int)(P.S_ptr[row + 1] - sbeg);
#pragma unroll 1
        for (int base = 0; base < slen; base += 64) {
            const bool ok = base + lane < slen;
            const int j_l = ok ? P.S_idx[sbeg + base + lane] : 0;
            const float w_l = ok ? P.S_val[sbeg + base + lane] : 0.f;
            const int cnt = min(64, slen - base);
#pragma unroll 1
            for (int u0 = 0; u0 < cnt; u0 += NG) {
                float v[NG][NR];
                double w[NG];
#pragma unroll
                for (int e = 0; e < NG; ++e) {
                    const int uu = min(u0 + e, cnt - 1);
                    const int j = __builtin_amdgcn_readlane(j_l, uu);
                    w[e] = (u0 + e < cnt) ? (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(w_l), uu))
                                          : 0.0;
                    const float* Vj = P.V + (int64_t)j * P.ld;
#pragma unroll
                    for (int rr = 0; rr < NR; ++rr) v[e][rr] = Vj[col[rr]];
                }
#pragma unroll
                for (int e = 0; e < NG; ++e) {
                    if (u0 + e < cnt) {
                        deg += w[e];
#pragma unroll
                        for (int rr = 0; rr < NR; ++rr)
                            nb[rr] = live[rr] ? fma(w[e], (double)v[e][rr], nb[rr]) : 0.0;
                    }
                }
            }
        }
        const double alpha = (double)P.alpha;
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) g_p[rr] = fma(alpha, nb[rr], g_p[rr]);
    }
    wave_lds_sync();

    // per-row regulariser on the diagonal (scripts/als.py:450-455), 1 on the padded columns
    const double lv = P.pop_reg ? (double)P.lambda_v / __builtin_sqrt((double)len + 1.0) : (double)P.lambda_v;
    const double lam = lv + 1e-10 + (double)P.alpha * deg;
    if (q == 0) {
        for (int J = 0; J < KB; ++J)
            img[blk64(J, J) * 256 + c * 16 + c] += (perm_to_col<KB>(16 * J + c) < P.k) ? lam : 1.0;
    }
    wave_lds_sync();

    double b[2][NR], y[2][NR], dinv[NR];
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) {
        b[0][rr] = g_p[rr]; b[1][rr] = h_p[rr];
        y[0][rr] = 0.0; y[1][rr] = 0.0; dinv[rr] = 0.0;
    }
    bool bad = false;
    cholesky_f64<KB, 2>(img, b, y, dinv, bad, lane);
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicMax(P.status, (int)(row + 1));
    solve_lt_f64<KB>(img, y[0], dinv, lane);                // p = A^-1 g
    solve_lt_f64<KB>(img, y[1], dinv, lane);                // q = A^-1 h

    double hp = 0.0, hq = 0.0;
#pragma unroll
    for (int rr = 0; rr < NR; ++rr)
        if (lane + 64 * rr < KP) { hp = fma(h_p[rr], y[0][rr], hp); hq = fma(h_p[rr], y[1][rr], hq); }
    hp = wave_sum_f64(hp);
    hq = wave_sum_f64(hq);
    const double d = (double)len + (double)P.lambda_bi + 1e-10;     // scripts/als.py:464
    double bi, bprev;
    if (P.n_sweeps == 0) {
        bi = (s - hp) / (d - hq);
        bprev = bi;
    } else {
        bi = 0.0; bprev = 0.0;
        for (int t = 0; t < P.n_sweeps; ++t) { bprev = bi; bi = (s - hp + bi * hq) / d; }
    }
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) {
        const int i = lane + 64 * rr;
        if (i < KP) P.V_out[row * P.ld + perm_to_col<KB>(i)] = (float)fma(-bprev, y[1][rr], y[0][rr]);
    }
    if (lane == 0) P.b_i_out[row] = (float)bi;
}

}  // namespace

extern "C" int als_fold_in_items(const als_fold_in_items_params* p, void* stream) {
    if (!p) return ALS_E_BADARG;
    const int kp = als_padded_k(p->k);
    if (kp < 0) return ALS_E_BADK;
    if (p->ld != kp || p->nrows < 0 || p->nrows >= INT32_MAX || p->n_sweeps < 0 || (p->pop_reg != 0 && p->pop_reg != 1)
        || p->m < 1 || p->m * (int64_t)kp >= ((int64_t)1 << 31) || p->n < 0 || p->n * (int64_t)kp >= ((int64_t)1 << 31)
        || !(p->lambda_v >= 0.f) || !(p->lambda_bi >= 0.f) || !(p->alpha >= 0.f) || !(p->lambda_v < INFINITY)
        || !(p->lambda_bi < INFINITY) || !(p->alpha < INFINITY))
        return ALS_E_BADARG;
    if (p->nrows == 0) return 0;
    if (!p->indptr || !p->indices || !p->vals || !p->U || !p->b_u || !p->mu || !p->V_out || !p->b_i_out ||
        !p->status)
        return ALS_E_BADARG;
    const bool graph = p->S_ptr || p->S_idx || p->S_val;
    if (graph && (!p->S_ptr || !p->S_idx || !p->S_val || !p->V || p->n < 1)) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p->nrows);
    ALS_DISPATCH_KB(kp / 16, hipLaunchKernelGGL(k_fold_in_items<KB>, grid, dim3(64), 0, st, *p));
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}
