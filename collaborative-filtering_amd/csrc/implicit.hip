// K18: the confidence-weighted fit for implicit feedback (Hu, Koren, Volinsky, ICDM 2008) - DESIGN.md section 32.
//
// A half-step of that model solves, per row with entries t (other side's rows f_t, weights a_t >= 0, t_t),
//     A = G + sum_t a_t f_t f_t^T + (lambda + 1e-10) I,   b = sum_t t_t f_t,   x = A^-1 b,
// with G = a0 F^T F over ALL rows of the other side's table F - the term that stands for the unobserved entries and
// is the same for every row of the half-step.  Two entry points:
//
// als_table_gram_f64: G = F^T F of an fp32 table in fp64 on v_mfma_f64_16x16x4_f64.  A fixed grid of
//   als_table_gram_partials() = 512 one-wave workgroups, workgroup p accumulating the contiguous rows
//   [p ceil(nrows / P), (p + 1) ceil(nrows / P)) into its partial image; a second launch adds the partials in index
//   order.  Nothing depends on timing: the result is a function of (F, nrows, k) alone, bit for bit.  The output is
//   the lower-block perm-space image of row_f64_common.hpp, the form the row kernel adds to its own image with one
//   pass of "img[e] += G[e]" (natural order would cost it a permuted read per element).
//   als_table_gram_weighted_f64 is the same grid, ranges and fold with G = F^T diag(w) F: the
//   second instantiation of table_gram_pass, whose A operand is f w_r; als_table_gram_f64 launches the first one.
//
// als_implicit_row_solve: one wave per task as k_row_tasks_f64 (same als_task / als_long_row lists, same fp64 slot
//   layout, slots folded in slot order by slot_fold.hpp), the Gram pass being gram_pass_f64 with the A operand scaled
//   by a_t and rhs += t_t f_t.  Lanes past the end of a row gather a valid row of F with a = t = 0, which removes
//   them exactly (F is finite), so F needs no zero row.  After the image is complete: + G, the regulariser on the
//   real diagonal and 1 on the padded one, cholesky_f64<KB, 1>, solve_lt_f64; only x is rounded to fp32.
//   G enters as G_scale G, or as (G_scale g_scale_row[row]) G where a per-row scale is given (section 33).
//   A row's result depends on its entries, F, G and its scale alone (fixed reduction orders, no cross-row state).
#include "als_device.hpp"
#include "als_hip.h"
#include "row_f64_common.hpp"
#include "slot_fold.hpp"

namespace {

using namespace f64row;

constexpr int TABLE_GRAM_PARTIALS = 512;

// ---------------------------------------------------------------------------------------------------------
// table Gram: block rows [I0, I1) of the lower triangle over the table rows [beg, end).  Lane (c, q) holds the KB
// contiguous floats F[row 4 s + q][KB c ...] = position c of every block (perm space), as in gram_pass_f64; columns
// >= k and rows >= end are zeroed after the load.  WEIGHTED: G = sum_r w_r f_r f_r^T - the A operand of every MFMA
// is (double)f * (double)w_r, exact in fp64 (24 + 24 significand bits), the B operand is unscaled; rows >= end take
// weight 0 and read w at `beg`, so nothing past nrows is read.  With every w_r = 1 the operands, and so the bits, are
// the unweighted pass's.
// ---------------------------------------------------------------------------------------------------------
template <int KB, int I0, int I1, bool WEIGHTED>
__device__ __forceinline__ void table_gram_pass(const float* __restrict__ F, const float* __restrict__ w, int k,
                                                int64_t beg, int64_t end, double* __restrict__ out, int lane) {
    constexpr int NB = blk64(I1, 0) - blk64(I0, 0);
    constexpr int GS = 4;                                    // 4-row steps whose loads are in flight together
    constexpr int LD = 16 * KB;
    const int c = lane & 15, q = lane >> 4;
    const float* Fc = F + KB * c;
    f64x4 acc[NB];
#pragma unroll
    for (int a = 0; a < NB; ++a) acc[a] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t r0 = beg; r0 < end; r0 += 4 * GS) {
        float f[GS][KB];
        float wr[GS];
        bool live[GS];
#pragma unroll
        for (int s = 0; s < GS; ++s) {
            const int64_t r = r0 + 4 * s + q;
            live[s] = r < end;
            load_frow<KB>(Fc + (live[s] ? r : beg) * LD, f[s]);
            if constexpr (WEIGHTED) wr[s] = w[live[s] ? r : beg];
        }
#pragma unroll
        for (int s = 0; s < GS; ++s) {
            double fd[KB];
#pragma unroll
            for (int b = 0; b < KB; ++b) fd[b] = (live[s] && KB * c + b < k) ? (double)f[s][b] : 0.0;
            if constexpr (WEIGHTED) {
                const double wd = live[s] ? (double)wr[s] : 0.0;
                double fw[KB];
#pragma unroll
                for (int b = 0; b < KB; ++b) fw[b] = fd[b] * wd;
#pragma unroll
                for (int I = I0; I < I1; ++I)
#pragma unroll
                    for (int K = 0; K <= I; ++K)
                        acc[blk64(I, K) - blk64(I0, 0)] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                            fw[I], fd[K], acc[blk64(I, K) - blk64(I0, 0)], 0, 0, 0);
            } else {
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
                out[blk64(I, K) * 256 + (q + 4 * i) * 16 + c] = acc[blk64(I, K) - blk64(I0, 0)][i];
}

template <int KB, int I0, bool WEIGHTED>
__device__ __forceinline__ void table_gram_passes(const float* __restrict__ F, const float* __restrict__ w, int k,
                                                  int64_t beg, int64_t end, double* __restrict__ out, int lane) {
    if constexpr (I0 < KB) {
        constexpr int I1 = F64Cfg<KB>::pass_end(I0);
        table_gram_pass<KB, I0, I1, WEIGHTED>(F, w, k, beg, end, out, lane);
        table_gram_passes<KB, I1, WEIGHTED>(F, w, k, beg, end, out, lane);
    }
}

template <int KB>
__global__ __launch_bounds__(64)
void k_table_gram(const float* __restrict__ F, int k, int64_t nrows, double* __restrict__ partials) {
    const int64_t chunk = (nrows + TABLE_GRAM_PARTIALS - 1) / TABLE_GRAM_PARTIALS;
    const int64_t beg = min(nrows, (int64_t)blockIdx.x * chunk), end = min(nrows, beg + chunk);
    table_gram_passes<KB, 0, false>(F, nullptr, k, beg, end, partials + (size_t)blockIdx.x * F64Cfg<KB>::IMG,
                                    threadIdx.x);
}

// the same grid and row ranges with the row weights w [nrows]
template <int KB>
__global__ __launch_bounds__(64)
void k_table_gram_weighted(const float* __restrict__ F, const float* __restrict__ w, int k, int64_t nrows,
                           double* __restrict__ partials) {
    const int64_t chunk = (nrows + TABLE_GRAM_PARTIALS - 1) / TABLE_GRAM_PARTIALS;
    const int64_t beg = min(nrows, (int64_t)blockIdx.x * chunk), end = min(nrows, beg + chunk);
    // (a workgroup with an empty range runs no step: it reads neither F nor w)
    table_gram_passes<KB, 0, true>(F, w, k, beg, end, partials + (size_t)blockIdx.x * F64Cfg<KB>::IMG, threadIdx.x);
}

// G[e] = partial 0 + partial 1 + ... in index order, one thread per element
__global__ __launch_bounds__(256)
void k_table_gram_fold(const double* __restrict__ partials, int img, double* __restrict__ G) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= img) return;
    double acc = partials[e];
    for (int p = 1; p < TABLE_GRAM_PARTIALS; ++p) acc += partials[(size_t)p * img + e];
    G[e] = acc;
}

// ---------------------------------------------------------------------------------------------------------
// weighted Gram pass of one task: gram_pass_f64's loop with the A operand of every rating scaled by its weight a_t
// and (FIRST) rhs += t_t f_t.  Lanes past the end hold a = t = 0 and gather row P.F_zero_row (or row 0).
// ---------------------------------------------------------------------------------------------------------
template <int KB, int I0, int I1, bool FIRST>
__device__ __forceinline__ void wgram_pass(const als_implicit_params& P, int64_t beg, int len,
                                           double* __restrict__ img, double (&rhs)[KB], int lane) {
    constexpr int NB = blk64(I1, 0) - blk64(I0, 0);
    constexpr int GS = 4;                                    // rating steps whose gathers are in flight together
    const int c = lane & 15, q = lane >> 4;
    const float* Fc = P.F + KB * c;
    const int pad_row = P.F_zero_row >= 0 ? P.F_zero_row : 0;
    f64x4 acc[NB];
#pragma unroll
    for (int a = 0; a < NB; ++a) acc[a] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int base = 0; base < len; base += 64) {
        const int t = base + lane;
        const bool ok = t < len;
        const int idx = ok ? P.indices[beg + t] : pad_row;
        const double a_l = ok ? (double)P.gram_w[beg + t] : 0.0;
        double t_l = 0.0;
        if (FIRST) t_l = ok ? (P.rhs_w ? (double)P.rhs_w[beg + t] : 1.0 + a_l) : 0.0;
        const int off_l = idx * P.ld;
        const int nvalid = min(64, len - base);
#pragma unroll 1
        for (int g0 = 0; g0 < 16; g0 += GS) {
            if (4 * g0 >= nvalid) break;
            float f[GS][KB];
            double a_t[GS], t_t[GS];
#pragma unroll
            for (int s = 0; s < GS; ++s) {
                const int off = bperm_i(off_l, 4 * (g0 + s) + q);
                a_t[s] = bperm_d(a_l, 4 * (g0 + s) + q);
                if (FIRST) t_t[s] = bperm_d(t_l, 4 * (g0 + s) + q);
                load_frow<KB>(Fc + (uint32_t)off, f[s]);
            }
#pragma unroll
            for (int s = 0; s < GS; ++s) {
                double fd[KB], fa[KB];
#pragma unroll
                for (int b = 0; b < KB; ++b) { fd[b] = (double)f[s][b]; fa[b] = fd[b] * a_t[s]; }
                if (FIRST) {
#pragma unroll
                    for (int b = 0; b < KB; ++b) rhs[b] = fma(fd[b], t_t[s], rhs[b]);
                }
#pragma unroll
                for (int I = I0; I < I1; ++I)
#pragma unroll
                    for (int K = 0; K <= I; ++K)
                        acc[blk64(I, K) - blk64(I0, 0)] = __builtin_amdgcn_mfma_f64_16x16x4f64(
                            fa[I], fd[K], acc[blk64(I, K) - blk64(I0, 0)], 0, 0, 0);
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

template <int KB, int I0, bool FIRST>
__device__ __forceinline__ void wgram_passes(const als_implicit_params& P, int64_t beg, int len,
                                             double* __restrict__ img, double (&rhs)[KB], int lane) {
    if constexpr (I0 < KB) {
        constexpr int I1 = F64Cfg<KB>::pass_end(I0);
        wgram_pass<KB, I0, I1, FIRST>(P, beg, len, img, rhs, lane);
        wgram_passes<KB, I1, false>(P, beg, len, img, rhs, lane);
    }
}

// rhs from "block b, position c, partial over q" to "perm position i = lane + 64 rr" (to_rows_f64 for one vector)
template <int KB>
__device__ __forceinline__ void rhs_to_rows(double (&rhs)[KB], double (&rhs_p)[F64Cfg<KB>::NR], int lane) {
    const int q = lane >> 4;
#pragma unroll
    for (int b = 0; b < KB; ++b) { rhs[b] += __shfl_xor(rhs[b], 16, 64); rhs[b] += __shfl_xor(rhs[b], 32, 64); }
#pragma unroll
    for (int rr = 0; rr < F64Cfg<KB>::NR; ++rr) {
        double bsel = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * rr + e < KB) bsel = (q == e) ? rhs[4 * rr + e] : bsel;
        rhs_p[rr] = bsel;
    }
}

// img: lower blocks of sum a f f^T; rhs_p: lane = perm row.  + a0 G (times the row's own scale, when one is given),
// regularise, factorise, solve, store.
template <int KB>
__device__ __forceinline__ void finish_implicit(const als_implicit_params& P, int row, double* __restrict__ img,
                                                double (&rhs_p)[F64Cfg<KB>::NR], int lane) {
    using C = F64Cfg<KB>;
    constexpr int KP = C::KP, NR = C::NR;
    const int c = lane & 15, q = lane >> 4;
    const double g_scale = P.g_scale_row ? P.G_scale * (double)P.g_scale_row[row] : P.G_scale;
    for (int e = lane; e < C::IMG; e += 64) img[e] += g_scale * P.G[e];
    wave_lds_sync();
    // regulariser on the real diagonal, 1 on the padded one (as finish_row_f64)
    const double lam = (double)(P.lambda_row ? P.lambda_row[row] : P.lambda_scalar) + 1e-10;
    if (q == 0) {
        for (int J = 0; J < KB; ++J)
            img[blk64(J, J) * 256 + c * 16 + c] += (perm_to_col<KB>(16 * J + c) < P.k) ? lam : 1.0;
    }
    wave_lds_sync();

    double b[1][NR], y[1][NR], dinv[NR];
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) { b[0][rr] = rhs_p[rr]; y[0][rr] = 0.0; dinv[rr] = 0.0; }
    bool bad = false;
    cholesky_f64<KB, 1>(img, b, y, dinv, bad, lane);
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicMax(P.status, row + 1);
    solve_lt_f64<KB>(img, y[0], dinv, lane);

    double xb = 0.0;
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) {
        const int i = lane + 64 * rr;
        if (i < KP) {
            const int col = perm_to_col<KB>(i);
            P.X_out[(int64_t)row * P.ld + col] = col < P.k ? (float)y[0][rr] : 0.f;
            xb = fma(y[0][rr], rhs_p[rr], xb);
        }
    }
    if (P.xb_out) {
        xb = wave_sum_f64(xb);
        if (lane == 0) P.xb_out[row] = xb;
    }
}

template <int KB>
__global__ __launch_bounds__(64)
void k_implicit_tasks(const als_implicit_params P) {
    using C = F64Cfg<KB>;
    __shared__ __attribute__((aligned(16))) double img[C::IMG];
    const int lane = threadIdx.x;
    const int64_t tid = blockIdx.x;
    if (tid >= P.ntasks) return;
    const als_task t = P.tasks[tid];
    const int row = t.row;
    const int64_t rbeg = P.indptr[row], rend = P.indptr[row + 1];
    const int64_t beg = rbeg + (int64_t)t.seg * ALS_SPLIT_CHUNK;
    const int len = (int)min((int64_t)ALS_SPLIT_CHUNK, rend - beg);
    double rhs[KB];
#pragma unroll
    for (int b = 0; b < KB; ++b) rhs[b] = 0.0;
    wgram_passes<KB, 0, true>(P, beg, len, img, rhs, lane);
    double rhs_p[C::NR];
    rhs_to_rows<KB>(rhs, rhs_p, lane);
    wave_lds_sync();
    if (t.slot >= 0) {          // segment of a split row: image + right-hand side to the workspace slot (fp64 layout;
        double* ws = (double*)P.workspace + (size_t)t.slot * C::SLOT;      // the rest of the slot is written as zero)
        for (int e = lane; e < C::IMG; e += 64) ws[e] = img[e];
#pragma unroll
        for (int rr = 0; rr < C::NR; ++rr)
            if (lane + 64 * rr < C::KP) {
                ws[C::IMG + lane + 64 * rr] = rhs_p[rr];
                ws[C::IMG + C::KP + lane + 64 * rr] = 0.0;
            }
        if (lane == 0) { ws[C::IMG + 2 * C::KP] = 0.0; ws[C::IMG + 2 * C::KP + 1] = 0.0; }
        return;
    }
    finish_implicit<KB>(P, row, img, rhs_p, lane);
}

// partial slots of a split row summed into its first slot, slots in ascending order (k_sum_slots_f64's launch shape)
template <int KB>
struct ImplicitSlots {
    static_assert(F64Cfg<KB>::SLOT % 2 == 0, "a slot is a whole number of f64x2");
    static constexpr int NV = F64Cfg<KB>::SLOT / 2;
    static constexpr int GROUPS = (NV + 63) / 64;
};

template <int KB>
__global__ __launch_bounds__(64)
void k_implicit_sum_slots(const als_long_row* __restrict__ long_rows, double* __restrict__ workspace) {
    using slot_fold::f64x2;
    constexpr int NV = ImplicitSlots<KB>::NV, G = ImplicitSlots<KB>::GROUPS;
    const als_long_row lr = long_rows[blockIdx.x / G];
    const int e = (blockIdx.x % G) * 64 + threadIdx.x;
    if (e >= NV || lr.nslots < 2) return;
    f64x2* w0 = reinterpret_cast<f64x2*>(workspace) + (size_t)lr.slot0 * NV + e;
    w0[0] = slot_fold::fold<false>(w0, (size_t)NV, lr.nslots);
}

template <int KB>
__global__ __launch_bounds__(64)
void k_implicit_long(const als_implicit_params P) {
    using C = F64Cfg<KB>;
    __shared__ __attribute__((aligned(16))) double img[C::IMG];
    const int lane = threadIdx.x;
    if ((int64_t)blockIdx.x >= P.nlong) return;
    const als_long_row lr = P.long_rows[blockIdx.x];
    const double* ws = (const double*)P.workspace + (size_t)lr.slot0 * C::SLOT;
    for (int e = lane; e < C::IMG; e += 64) img[e] = ws[e];
    double rhs_p[C::NR];
#pragma unroll
    for (int rr = 0; rr < C::NR; ++rr) rhs_p[rr] = ws[C::IMG + min(lane + 64 * rr, C::KP - 1)];
    wave_lds_sync();
    finish_implicit<KB>(P, lr.row, img, rhs_p, lane);
}

// rows without entries are in no task list: x = 0 (x.b = 0)
__global__ __launch_bounds__(256)
void k_implicit_empty_rows(const als_implicit_params P) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= P.nrows || P.indptr[row + 1] != P.indptr[row]) return;
    for (int j = 0; j < P.ld; ++j) P.X_out[row * P.ld + j] = 0.f;
    if (P.xb_out) P.xb_out[row] = 0.0;
}

template <int KB>
int launch_table_gram(int k, int64_t nrows, const float* F, const float* w, double* partials, double* G,
                      hipStream_t st) {
    constexpr int IMG = F64Cfg<KB>::IMG;
    if (w)
        hipLaunchKernelGGL(k_table_gram_weighted<KB>, dim3(TABLE_GRAM_PARTIALS), dim3(64), 0, st, F, w, k, nrows,
                           partials);
    else
        hipLaunchKernelGGL(k_table_gram<KB>, dim3(TABLE_GRAM_PARTIALS), dim3(64), 0, st, F, k, nrows, partials);
    hipLaunchKernelGGL(k_table_gram_fold, dim3((IMG + 255) / 256), dim3(256), 0, st, partials, IMG, G);
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}

template <int KB>
int launch_implicit(const als_implicit_params* p, hipStream_t st) {
    hipLaunchKernelGGL(k_implicit_empty_rows, dim3((unsigned)((p->nrows + 255) / 256)), dim3(256), 0, st, *p);
    if (p->ntasks > 0)
        hipLaunchKernelGGL(k_implicit_tasks<KB>, dim3((unsigned)p->ntasks), dim3(64), 0, st, *p);
    if (p->nlong > 0) {
        hipLaunchKernelGGL(k_implicit_sum_slots<KB>, dim3((unsigned)(p->nlong * ImplicitSlots<KB>::GROUPS)), dim3(64),
                           0, st, p->long_rows, (double*)p->workspace);
        hipLaunchKernelGGL(k_implicit_long<KB>, dim3((unsigned)p->nlong), dim3(64), 0, st, *p);
    }
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}

}  // namespace

extern "C" int als_table_gram_partials(void) { return TABLE_GRAM_PARTIALS; }

extern "C" int als_table_gram_weighted_f64(int k, int ld, int64_t nrows, const float* F, const float* w,
                                           double* partials, double* G_out, void* stream) {
    const int kp = als_padded_k(k);
    if (kp < 0) return ALS_E_BADK;
    if (ld != kp || nrows < 0 || (nrows > 0 && !F) || !partials || !G_out || ((uintptr_t)F & 15) != 0)
        return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    ALS_DISPATCH_KB(kp / 16, return launch_table_gram<KB>(k, nrows, F, w, partials, G_out, st));
    return 0;
}

extern "C" int als_table_gram_f64(int k, int ld, int64_t nrows, const float* F, double* partials, double* G_out,
                                  void* stream) {
    return als_table_gram_weighted_f64(k, ld, nrows, F, nullptr, partials, G_out, stream);
}

extern "C" int als_implicit_row_solve(const als_implicit_params* p, void* stream) {
    if (!p) return ALS_E_BADARG;
    const int kp = als_padded_k(p->k);
    if (kp < 0) return ALS_E_BADK;
    if (p->ld != kp || p->nrows < 0 || p->nrows >= INT32_MAX || p->ncols < 1 ||
        p->ncols * (int64_t)kp >= ((int64_t)1 << 31) || p->F_zero_row < -1 || p->F_zero_row >= p->ncols ||
        p->ntasks < 0 || p->ntasks > (int64_t)0x7FFFFFFF || p->nlong < 0 ||
        (!p->lambda_row && !(p->lambda_scalar >= 0.f)))
        return ALS_E_BADARG;
    if (p->nrows == 0) return 0;
    if (!p->indptr || !p->indices || !p->gram_w || !p->F || !p->G || !p->X_out || !p->status ||
        ((uintptr_t)p->F & 15) != 0 || (p->ntasks > 0 && !p->tasks) ||
        (p->nlong > 0 && (!p->long_rows || !p->workspace || ((uintptr_t)p->workspace & 15) != 0)))
        return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    ALS_DISPATCH_KB(kp / 16,
                    if (p->nlong * ImplicitSlots<KB>::GROUPS > (int64_t)0x7FFFFFFF) return ALS_E_BADARG;
                    return launch_implicit<KB>(p, st));
    return 0;
}
