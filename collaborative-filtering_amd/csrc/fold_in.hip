// K9: fold-in - user factors and biases for rows outside the fit, the item side (Z, b_i, mu) held fixed.
//
// For one row with rated items S (n = |S|) and ratings r, the user half-step of the fit (scripts/als.py:411-433)
// needs
//     A = Z_S^T Z_S + lambda I,  g = Z_S^T (r - mu - b_i[S]),  h = Z_S^T 1,  s = sum (r - mu - b_i[S]),
//     d = n + lambda_bu + 1e-10,  lambda = lambda_u + 1e-10,
// and alternates u_t = A^-1 (g - b_{t-1} h), b_t = (s - h.u_t) / d from b_0 = 0.  With p = A^-1 g, q = A^-1 h every
// sweep is the scalar recurrence b_t = (s - h.p + b_{t-1} h.q) / d (u_T = p - b_{T-1} q), and its fixed point - the
// solution of the bordered system [[A, h], [h^T, d]] [u; b] = [g; s] - is b* = (s - h.p) / (d - h.q), u* = p - b* q.
// So one factorisation serves any number of sweeps.
//
// k_fold_in: one wave per row, whatever its length, in fp64 like k_row_tasks_f64 (row_f64_common.hpp): the fp64
// Gram passes (tail lanes masked: Z has no zero row) accumulate A, g, h and s; the panel Cholesky carries g and h
// along its forward substitution; two transposed solves give p and q; two wave sums give h.p and h.q.  The result of
// a row depends on that row's ratings alone (no cross-row state, fixed reduction orders).
#include "als_device.hpp"
#include "als_hip.h"
#include "row_f64_common.hpp"

namespace {

using namespace f64row;

// the gather source of the Gram passes: Z with b_i as the "other" bias; tail lanes gather row 0 and are masked
struct FoldSrc {
    const float* F;
    int ld;
    const int32_t* indices;
    const float* vals;
    const float* bias_other;
    int F_zero_row;
};

template <int KB>
__global__ __launch_bounds__(64)
void k_fold_in(const als_fold_in_params P) {
    using C = F64Cfg<KB>;
    constexpr int KP = C::KP, NR = C::NR;
    __shared__ __attribute__((aligned(16))) double img[C::IMG];
    const int lane = threadIdx.x;
    const int c = lane & 15, q = lane >> 4;
    const int64_t row = blockIdx.x;
    const int64_t beg = P.indptr[row];
    const int len = (int)(P.indptr[row + 1] - beg);
    const FoldSrc S{P.Z, P.ld, P.indices, P.vals, P.b_i, 0};
    const double mu = *P.mu;

    double g[KB], h[KB], s = 0.0, s2 = 0.0;
#pragma unroll
    for (int b = 0; b < KB; ++b) { g[b] = 0.0; h[b] = 0.0; }
    gram_passes_f64<KB, 0, true, true>(S, beg, len, mu, 0.0, img, g, h, s, s2, lane);
    double g_p[NR], h_p[NR];
    to_rows_f64<KB>(g, h, g_p, h_p, lane);
    s = wave_sum_f64(s);
    wave_lds_sync();

    // regulariser on the diagonal, 1 on the padded columns (as finish_row_f64)
    const double lam = (double)P.lambda_u + 1e-10;
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
    const double d = (double)len + (double)P.lambda_bu + 1e-10;     // scripts/als.py:431
    double bu, bprev;                                                // b_T and the b_{T-1} that u_T is solved with
    if (P.n_sweeps == 0) {
        bu = (s - hp) / (d - hq);
        bprev = bu;
    } else {
        bu = 0.0; bprev = 0.0;
        for (int t = 0; t < P.n_sweeps; ++t) { bprev = bu; bu = (s - hp + bu * hq) / d; }
    }
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) {
        const int i = lane + 64 * rr;
        if (i < KP) P.U_out[row * P.ld + perm_to_col<KB>(i)] = (float)fma(-bprev, y[1][rr], y[0][rr]);
    }
    if (lane == 0) P.b_u_out[row] = (float)bu;
}

}  // namespace

extern "C" int als_fold_in(const als_fold_in_params* p, void* stream) {
    if (!p) return ALS_E_BADARG;
    const int kp = als_padded_k(p->k);
    if (kp < 0) return ALS_E_BADK;
    if (p->ld != kp || p->nrows < 0 || p->nrows >= INT32_MAX || p->n_sweeps < 0 || p->n < 1 ||
        p->n * (int64_t)kp >= ((int64_t)1 << 31) || !(p->lambda_u >= 0.f) || !(p->lambda_bu >= 0.f))
        return ALS_E_BADARG;
    if (p->nrows == 0) return 0;
    if (!p->indptr || !p->indices || !p->vals || !p->Z || !p->b_i || !p->mu || !p->U_out || !p->b_u_out || !p->status)
        return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)p->nrows);
    ALS_DISPATCH_KB(kp / 16, hipLaunchKernelGGL(k_fold_in<KB>, grid, dim3(64), 0, st, *p));
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}
