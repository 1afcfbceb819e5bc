// fp64 row-solve building blocks shared by K1's fp64 kernels (row_solve_f64.hip) and the fold-in kernel
// (fold_in.hip): the Gram passes on the fp64 matrix cores, and - used by fold_in.hip; finish_row_f64 keeps its own
// one-right-hand-side copy inline - the right-looking panel Cholesky of the LDS image with NRHS right-hand sides
// riding along the forward substitution, and the transposed solve; for explain.hip also the forward substitution on
// its own (solve_l_f64: a right-hand side that arrives after the factorisation).
//
// The image: lower 16x16 blocks of the KP x KP matrix in perm space (perm_to_col), fp64, row-major inside a block,
// block (I, K) at blk64(I, K) * 256.  Vectors in "rows" form: lane (+ 64 rr) holds perm position lane + 64 rr.
#pragma once
#include "als_device.hpp"

namespace f64row {

typedef double f64x4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int blk64(int I, int K) { return I * (I + 1) / 2 + K; }

template <int KB>
struct F64Cfg {
    static constexpr int KP = 16 * KB;
    static constexpr int NACC = KB * (KB + 1) / 2;
    static constexpr int NR = (KP + 63) / 64;
    static constexpr int IMG = NACC * 256;                 // doubles: lower 16x16 blocks, row-major inside a block
    static constexpr int SLOT = IMG + 2 * KP + 2;          // doubles of one partial slot: image, rhs, colsum, sumr, sumr2
    static constexpr int MAXB = 28;                        // accumulator blocks per Gram pass (8 registers each)
    // last block row (exclusive) of the pass that starts at block row I0
    static constexpr int pass_end(int I0) {
        int n = 0, I = I0;
        while (I < KB && (n + I + 1 <= MAXB || I == I0)) { n += I + 1; ++I; }
        return I;
    }
};

__device__ __forceinline__ double readlane_d(double v, int src) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double bperm_d(double v, int src) {
    const int lo = __builtin_amdgcn_ds_bpermute(src << 2, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(src << 2, __double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------------------
// one Gram pass: block rows [I0, I1) of the lower triangle, all ratings [beg, beg + len) of the task.
// Src: anything with the members F, ld, indices, vals, bias_other and F_zero_row of als_row_solve_params.
// MASK = false: lanes past the end gather row F_zero_row, which must be a zero row of F (K1's tables have one).
// MASK = true: they gather F_zero_row (any valid row) and zero what they loaded (tables without a zero row).
// ---------------------------------------------------------------------------------------------------------
template <int KB, int I0, int I1, bool FIRST, bool MASK = false, class Src>
__device__ __forceinline__ void gram_pass_f64(const Src& P, int64_t beg, int len, double mu,
                                              double bself, double* __restrict__ img, double (&rhs)[KB],
                                              double (&cs)[KB], double& sumr, double& sumr2, int lane) {
    constexpr int NB = blk64(I1, 0) - blk64(I0, 0);
    constexpr int GS = 4;                                    // rating steps whose gathers are in flight together
    const int c = lane & 15, q = lane >> 4;
    const float* Fc = P.F + KB * c;
    f64x4 acc[NB];
#pragma unroll
    for (int a = 0; a < NB; ++a) acc[a] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int base = 0; base < len; base += 64) {
        const int t = base + lane;
        const bool ok = t < len;
        const int idx = ok ? P.indices[beg + t] : P.F_zero_row;
        double r_l = 0.0;
        if (FIRST) {            // r = R - (mu + b_self + b_other) in fp64 (scripts/als.py:425, 447)
            const float v = ok ? P.vals[beg + t] : 0.f;
            const float bo = ok ? P.bias_other[idx] : 0.f;
            const double rb = ok ? ((double)v - mu - (double)bo) : 0.0;
            sumr += rb;
            sumr2 = fma(rb, rb, sumr2);
            r_l = ok ? rb - bself : 0.0;
        }
        const int off_l = idx * P.ld;
        const int nvalid = min(64, len - base);
#pragma unroll 1
        for (int g0 = 0; g0 < 16; g0 += GS) {
            if (4 * g0 >= nvalid) break;
            float f[GS][KB];
            double r_t[GS];
#pragma unroll
            for (int s = 0; s < GS; ++s) {
                const int off = bperm_i(off_l, 4 * (g0 + s) + q);
                if (FIRST) r_t[s] = bperm_d(r_l, 4 * (g0 + s) + q);
                load_frow<KB>(Fc + (uint32_t)off, f[s]);
            }
            if constexpr (MASK) {
#pragma unroll
                for (int s = 0; s < GS; ++s) {
                    const bool live = 4 * (g0 + s) + q < nvalid;
#pragma unroll
                    for (int b = 0; b < KB; ++b) f[s][b] = live ? f[s][b] : 0.f;
                }
            }
#pragma unroll
            for (int s = 0; s < GS; ++s) {
                double fd[KB];
#pragma unroll
                for (int b = 0; b < KB; ++b) fd[b] = (double)f[s][b];
                if (FIRST) {
#pragma unroll
                    for (int b = 0; b < KB; ++b) { rhs[b] = fma(fd[b], r_t[s], rhs[b]); cs[b] += fd[b]; }
                }
#pragma unroll
                for (int I = I0; I < I1; ++I)
#pragma unroll
                    for (int K = 0; K <= I; ++K)
                        acc[blk64(I, K) - blk64(I0, 0)] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                            fd[I], fd[K], acc[blk64(I, K) - blk64(I0, 0)], 0, 0, 0);
            }
        }
    }
    // accumulator register i of lane (c, q) is element (row q + 4 i, col c) of its block
#pragma unroll
    for (int I = I0; I < I1; ++I)
#pragma unroll
        for (int K = 0; K <= I; ++K)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                img[blk64(I, K) * 256 + (q + 4 * i) * 16 + c] = acc[blk64(I, K) - blk64(I0, 0)][i];
}

template <int KB, int I0, bool FIRST, bool MASK = false, class Src>
__device__ __forceinline__ void gram_passes_f64(const Src& P, int64_t beg, int len, double mu,
                                                double bself, double* __restrict__ img, double (&rhs)[KB],
                                                double (&cs)[KB], double& sumr, double& sumr2, int lane) {
    if constexpr (I0 < KB) {
        constexpr int I1 = F64Cfg<KB>::pass_end(I0);
        gram_pass_f64<KB, I0, I1, FIRST, MASK>(P, beg, len, mu, bself, img, rhs, cs, sumr, sumr2, lane);
        gram_passes_f64<KB, I1, false, MASK>(P, beg, len, mu, bself, img, rhs, cs, sumr, sumr2, lane);
    }
}

// rhs / colsum from "block b, position c, partial over q" to "perm position i = lane + 64 rr"
template <int KB>
__device__ __forceinline__ void to_rows_f64(double (&rhs)[KB], double (&cs)[KB], double (&rhs_p)[F64Cfg<KB>::NR],
                                            double (&cs_p)[F64Cfg<KB>::NR], int lane) {
    const int q = lane >> 4;
#pragma unroll
    for (int b = 0; b < KB; ++b) {
        rhs[b] += __shfl_xor(rhs[b], 16, 64); rhs[b] += __shfl_xor(rhs[b], 32, 64);
        cs[b] += __shfl_xor(cs[b], 16, 64);   cs[b] += __shfl_xor(cs[b], 32, 64);
    }
#pragma unroll
    for (int rr = 0; rr < F64Cfg<KB>::NR; ++rr) {
        double bsel = 0.0, csel = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * rr + e < KB) {
                bsel = (q == e) ? rhs[4 * rr + e] : bsel;
                csel = (q == e) ? cs[4 * rr + e] : csel;
            }
        rhs_p[rr] = bsel;
        cs_p[rr] = csel;
    }
}

// ---------------------------------------------------------------------------------------------------------
// Right-looking blocked Cholesky of the (regularised) image in place, 16-column panels: per panel every lane takes
// the panel part of its matrix rows into registers, the panel is eliminated on the VALU (readlane broadcasts),
// written back, and the rank-16 trailing update runs on the fp64 matrix cores with LDS operands.  The forward
// substitution of the NRHS right-hand sides b rides along: y[j] = L^-1 b[j] (b is consumed).  dinv: 1 / L_ii of
// the lane's rows.  bad: a pivot was not positive (or NaN).
// ---------------------------------------------------------------------------------------------------------
template <int KB, int NRHS>
__device__ __forceinline__ void cholesky_f64(double* img, double (&b)[NRHS][F64Cfg<KB>::NR],
                                             double (&y)[NRHS][F64Cfg<KB>::NR], double (&dinv)[F64Cfg<KB>::NR],
                                             bool& bad, int lane) {
    using C = F64Cfg<KB>;
    constexpr int KP = C::KP, NR = C::NR;
    const int c = lane & 15, q = lane >> 4;
#pragma unroll 1
    for (int J = 0; J < KB; ++J) {
        // the panel part of the lane's matrix rows: p[rr][t] = A[i][16 J + t], i = lane + 64 rr >= 16 J
        double p[NR][16];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int i = min(max(lane + 64 * rr, 16 * J), KP - 1);        // lanes above the panel: dummy row
            const double* src = img + blk64(i >> 4, J) * 256 + (i & 15) * 16;
#pragma unroll
            for (int t = 0; t < 16; ++t) p[rr][t] = src[t];
        }
#pragma unroll
        for (int T = 0; T < 16; ++T) {
            const int piv = 16 * J + T, RP = piv >> 6, LP = piv & 63;
            double dsel = p[0][T], bsel[NRHS];
#pragma unroll
            for (int j = 0; j < NRHS; ++j) bsel[j] = b[j][0];
#pragma unroll
            for (int rr = 1; rr < NR; ++rr) {
                dsel = (RP == rr) ? p[rr][T] : dsel;
#pragma unroll
                for (int j = 0; j < NRHS; ++j) bsel[j] = (RP == rr) ? b[j][rr] : bsel[j];
            }
            const double d = readlane_d(dsel, LP);
            bad = bad || !(d > 0.0);                                         // not positive definite (or NaN)
            const double inv = 1.0 / __builtin_sqrt(d);
            double l[NR];
#pragma unroll
            for (int rr = 0; rr < NR; ++rr) { l[rr] = p[rr][T] * inv; p[rr][T] = l[rr]; }
            double yt[NRHS];
#pragma unroll
            for (int j = 0; j < NRHS; ++j) yt[j] = readlane_d(bsel[j], LP) * inv;
#pragma unroll
            for (int rr = 0; rr < NR; ++rr) {
#pragma unroll
                for (int j = 0; j < NRHS; ++j) b[j][rr] = fma(-l[rr], yt[j], b[j][rr]);
                const bool own = (RP == rr) && (lane == LP);
#pragma unroll
                for (int j = 0; j < NRHS; ++j) y[j][rr] = own ? yt[j] : y[j][rr];
                dinv[rr] = own ? inv : dinv[rr];
            }
#pragma unroll
            for (int t2 = T + 1; t2 < 16; ++t2) {
                const int pr = 16 * J + t2, R2 = pr >> 6, L2 = pr & 63;
                double lsel = l[0];
#pragma unroll
                for (int rr = 1; rr < NR; ++rr) lsel = (R2 == rr) ? l[rr] : lsel;
                const double mlt = readlane_d(lsel, L2);                     // L[16 J + t2][16 J + T]
#pragma unroll
                for (int rr = 0; rr < NR; ++rr) p[rr][t2] = fma(-l[rr], mlt, p[rr][t2]);
            }
        }
        // L block column J back to the image (rows at or below the panel; the diagonal block's upper part is
        // never read)
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int i = lane + 64 * rr;
            if (i >= 16 * J && i < KP) {
                double* dst = img + blk64(i >> 4, J) * 256 + (i & 15) * 16;
#pragma unroll
                for (int t = 0; t < 16; ++t) dst[t] = p[rr][t];
            }
        }
        wave_lds_sync();
        // trailing update on the fp64 matrix cores: block (I, K) -= L_IJ L_KJ^T for J < K <= I.
        // operands: A[row = c][k = q + 4 s] = L_IJ[c][4 s + q], B[k][col = c] = L_KJ[c][4 s + q]
        for (int I = J + 1; I < KB; ++I) {
            double aop[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) aop[s] = img[blk64(I, J) * 256 + c * 16 + 4 * s + q];
            for (int K = J + 1; K <= I; ++K) {
                double* Cb = img + blk64(I, K) * 256;
                f64x4 acc;
                double bop[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = Cb[(q + 4 * i) * 16 + c];
#pragma unroll
                for (int s = 0; s < 4; ++s) bop[s] = -img[blk64(K, J) * 256 + c * 16 + 4 * s + q];
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[s], bop[s], acc, 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i) Cb[(q + 4 * i) * 16 + c] = acc[i];
            }
        }
        wave_lds_sync();
    }
}

// L^T x = y in place (xs holds y on entry, x on exit): lane (+64 rr) owns unknown i and reads its column
// L[p][i], p > i, from the factorised image
template <int KB>
__device__ __forceinline__ void solve_lt_f64(const double* img, double (&xs)[F64Cfg<KB>::NR],
                                             const double (&dinv)[F64Cfg<KB>::NR], int lane) {
    constexpr int KP = F64Cfg<KB>::KP, NR = F64Cfg<KB>::NR;
#pragma unroll 1
    for (int p = KP - 1; p >= 0; --p) {
        const int RP = p >> 6, LP = p & 63;
        double xsel = xs[0] * dinv[0];
#pragma unroll
        for (int rr = 1; rr < NR; ++rr) xsel = (RP == rr) ? xs[rr] * dinv[rr] : xsel;
        const double xp = readlane_d(xsel, LP);
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int i = lane + 64 * rr;
            const bool below = i < p;
            const int ic = below ? i : 0;
            const double lpi = img[blk64(p >> 4, ic >> 4) * 256 + (p & 15) * 16 + (ic & 15)];
            xs[rr] = below ? fma(-lpi, xp, xs[rr]) : ((i == p) ? xp : xs[rr]);
        }
    }
}

// L x = b in place (xs holds b on entry, x on exit), the stand-alone form of the forward substitution that rides
// along cholesky_f64: per 16-column panel every lane takes the panel part of its rows from the factorised image
// (rows above the panel: a dummy row, never applied), the panel's unknowns are broadcast one by one
template <int KB>
__device__ __forceinline__ void solve_l_f64(const double* img, double (&xs)[F64Cfg<KB>::NR],
                                            const double (&dinv)[F64Cfg<KB>::NR], int lane) {
    constexpr int KP = F64Cfg<KB>::KP, NR = F64Cfg<KB>::NR;
#pragma unroll 1
    for (int J = 0; J < KB; ++J) {
        double p[NR][16];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int i = min(max(lane + 64 * rr, 16 * J), KP - 1);
            const double* src = img + blk64(i >> 4, J) * 256 + (i & 15) * 16;
#pragma unroll
            for (int t = 0; t < 16; ++t) p[rr][t] = src[t];
        }
#pragma unroll
        for (int T = 0; T < 16; ++T) {
            const int piv = 16 * J + T, RP = piv >> 6, LP = piv & 63;
            double xsel = xs[0] * dinv[0];
#pragma unroll
            for (int rr = 1; rr < NR; ++rr) xsel = (RP == rr) ? xs[rr] * dinv[rr] : xsel;
            const double xp = readlane_d(xsel, LP);
#pragma unroll
            for (int rr = 0; rr < NR; ++rr) {
                const int i = lane + 64 * rr;
                xs[rr] = (i > piv) ? fma(-p[rr][T], xp, xs[rr]) : ((i == piv) ? xp : xs[rr]);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// The Gram alone in NATURAL column order (explore.hip: a factor that is triangular in the columns as numbered):
// gram_pass_f64's loop with block b, position c = column 16 b + c of F - one dword per block and lane instead of
// the lane's contiguous KB floats - no right-hand side, and the tail lanes masked (they gather row 0).
// ---------------------------------------------------------------------------------------------------------
template <int KB, int I0, int I1>
__device__ __forceinline__ void gram_pass_nat_f64(const float* __restrict__ F, int ld,
                                                  const int32_t* __restrict__ indices, int64_t beg, int len,
                                                  double* __restrict__ img, int lane) {
    constexpr int NB = blk64(I1, 0) - blk64(I0, 0);
    constexpr int GS = 4;
    const int c = lane & 15, q = lane >> 4;
    const float* Fc = F + c;
    f64x4 acc[NB];
#pragma unroll
    for (int a = 0; a < NB; ++a) acc[a] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int base = 0; base < len; base += 64) {
        const int t = base + lane;
        const int idx = t < len ? indices[beg + t] : 0;
        const int off_l = idx * ld;
        const int nvalid = min(64, len - base);
#pragma unroll 1
        for (int g0 = 0; g0 < 16; g0 += GS) {
            if (4 * g0 >= nvalid) break;
            float f[GS][KB];
#pragma unroll
            for (int s = 0; s < GS; ++s) {
                const int off = bperm_i(off_l, 4 * (g0 + s) + q);
#pragma unroll
                for (int b = 0; b < KB; ++b) f[s][b] = Fc[(uint32_t)off + 16 * b];
            }
#pragma unroll
            for (int s = 0; s < GS; ++s) {
                const bool live = 4 * (g0 + s) + q < nvalid;
                double fd[KB];
#pragma unroll
                for (int b = 0; b < KB; ++b) fd[b] = live ? (double)f[s][b] : 0.0;
#pragma unroll
                for (int I = I0; I < I1; ++I)
#pragma unroll
                    for (int K = 0; K <= I; ++K)
                        acc[blk64(I, K) - blk64(I0, 0)] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                            fd[I], fd[K], acc[blk64(I, K) - blk64(I0, 0)], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int I = I0; I < I1; ++I)
#pragma unroll
        for (int K = 0; K <= I; ++K)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                img[blk64(I, K) * 256 + (q + 4 * i) * 16 + c] = acc[blk64(I, K) - blk64(I0, 0)][i];
}

template <int KB, int I0>
__device__ __forceinline__ void gram_passes_nat_f64(const float* __restrict__ F, int ld,
                                                    const int32_t* __restrict__ indices, int64_t beg, int len,
                                                    double* __restrict__ img, int lane) {
    if constexpr (I0 < KB) {
        constexpr int I1 = F64Cfg<KB>::pass_end(I0);
        gram_pass_nat_f64<KB, I0, I1>(F, ld, indices, beg, len, img, lane);
        gram_passes_nat_f64<KB, I1>(F, ld, indices, beg, len, img, lane);
    }
}

}  // namespace f64row
