/*
 * als_hip.h - C ABI of the MI355X (gfx950) ALS hot path.
 *
 * The reference (zhukovanadezhda/collaborative-filtering) has no FFI: its hot
 * path is the Python method `ALS.fit` (scripts/als.py:300-529) and
 * `ALS.predict` (scripts/als.py:532-574).  This header is the boundary the
 * build's Python mirror of that class (collaborative-filtering_amd/als.py)
 * calls through ctypes; every entry point names the reference lines it
 * replaces.  See INTEGRATION.md for the binding a maintainer would add.
 *
 * Conventions
 *   - plain C: pointers, sizes, scalars; no C++/torch types.
 *   - every pointer is a DEVICE pointer (HBM) unless it says "host".
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*);
 *     nothing synchronises, allocates or frees.
 *   - return value: 0 ok, negative = argument error (ALS_E_*).
 *   - factor matrices are row-major fp32 with leading dimension
 *     ld = als_padded_k(k) (k rounded up to a multiple of 16); the padding
 *     columns must be zero on input and are written as zero.
 *   - rating matrices are CSR-like: int64 row pointers, int32 indices, fp32
 *     values.  The same entry point serves the user step (CSR) and the item
 *     step (CSC); "row" below means a row of whichever orientation is passed.
 *   - "perm space": inside the solver a factor column c lives at position
 *     perm(c) = 16*(c % KB) + c / KB, KB = ld/16.  Outputs documented as
 *     perm-space use that order; als_perm_index() gives the map.
 */
#ifndef ALS_HIP_H
#define ALS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALS_HIP_VERSION 103
#define ALS_NXCD 8             /* XCDs (private L2s) of the MI355X: als_host_row_tasks deals equal-length tasks over them */

#define ALS_E_BADARG   (-1)
#define ALS_E_BADK     (-2)   /* k outside 1..ALS_MAX_K */
#define ALS_E_LAUNCH   (-3)   /* hipGetLastError() != hipSuccess after a launch */

#define ALS_GRAM_F32    0
#define ALS_GRAM_F16X2  1     /* 2-way fp16 split of the scaled floats, three cross products on v_mfma_f32_16x16x32_f16,
                                 fp32 accumulate: fp32-equivalent (default) */
#define ALS_GRAM_F64    2     /* fp64 Gram (v_mfma_f64_16x16x4_f64), fp64 Cholesky and substitutions: the
                                 reference's arithmetic type; x and the bias are rounded to fp32 on store */

#define ALS_MAX_K 160
#define ALS_SPLIT_CHUNK 4096  /* ratings per task segment (see als_task) */

/* One unit of row-solve work: ratings [seg*ALS_SPLIT_CHUNK, +len) of `row`.
 * slot < 0 : the row fits one segment and is solved in place.
 * slot >= 0: partial normal equations go to workspace slot `slot`; the row is
 *            completed by the matching als_long_row entry.                  */
typedef struct als_task {
    int32_t row;
    int32_t seg;
    int32_t slot;
    int32_t reserved;
} als_task;

/* A row split over `nslots` consecutive workspace slots starting at `slot0`. */
typedef struct als_long_row {
    int32_t row;
    int32_t slot0;
    int32_t nslots;
    int32_t reserved;
} als_long_row;

int als_version(void);
int als_padded_k(int k);                       /* ld for k factors            */
int als_perm_index(int k, int c);              /* perm-space position of col c */
/* bytes of one partial slot / of the whole workspace for `nslots` slots */
int64_t als_partial_slot_bytes(int k);
int64_t als_partial_slot_bytes_f64(int k);     /* slot size when gram_mode == ALS_GRAM_F64 */

/* ---------------------------------------------------------------------------
 * als_row_solve - normal-equation build and solve for a set of rows.
 * Replaces the bodies of the user loop (scripts/als.py:414-433) and the item
 * loop (scripts/als.py:436-466) incl. cholesky_solve (scripts/helpers.py:5-20).
 *
 * For every task row with nnz > 0:
 *     F_t   = F[indices[t]]                       (gathered factor rows)
 *     r_t   = vals[t] - (mu + bias_self[row] + bias_other[indices[t]])
 *     A     = F^T F + (lambda(row) + 1e-10 + diag_extra[row]) I
 *     b     = F^T r + rhs_extra[row]              (rhs_extra: actual col order)
 *     x     = A^{-1} b          (Cholesky; x -> X_out[row])
 *     bias  = sum_t(vals[t] - F_t.x - mu - bias_other[indices[t]])
 *             / (nnz + lambda_bias(row) + 1e-10)  (-> bias_out[row])
 * lambda(row) = lambda_row ? lambda_row[row] : lambda_scalar (same for bias).
 * Rows with nnz == 0 must not appear in the task list (they keep their
 * previous X/bias, as in the reference).
 *
 * Optional outputs
 *   gram_out   [nrows][ld][ld]  F^T F (no lambda), perm space, lower 16x16
 *                               blocks (block row >= block col) written; the
 *                               upper blocks are left untouched.
 *   rhs_out    [nrows][ld]    F^T r (perm space, without rhs_extra),
 *   colsum_out [nrows][ld]    sum_t F_t (perm space),
 *   sumr_out   [nrows]        sum_t(vals[t] - mu - bias_other[indices[t]])
 *   sumr2_out  [nrows]        sum_t(vals[t] - mu - bias_other[indices[t]])^2
 *                             (each written when its pointer is non-NULL)
 *   stat_out   [nrows][2]     solve mode only: (sum d, sum d^2) of the row's residuals after the update
 *   factor-only mode (factor_out != NULL): nothing is solved; instead
 *     factor_out [nrows][ld][ld] symmetric completion of the Cholesky factor
 *                               L (perm space) with 1/L_ii on the diagonal
 *   is written for als_gs_sweep, which also needs rhs_out/colsum_out/sumr_out.
 * status: int32[1], must be 0 on entry (host zeroes it); on a non-SPD pivot
 *   - or a row whose new bias is not finite, which is what a residual beyond
 *   the range of R_scale on the F_planes path leads to - the kernel stores
 *   (row + 1) with atomicMax.
 * workspace: als_partial_slot_bytes(k) * (number of slots referenced by
 *   tasks) bytes; may be NULL when no task has slot >= 0.
 * ------------------------------------------------------------------------- */
typedef struct als_row_solve_params {
    int32_t k;
    int32_t ld;                 /* = als_padded_k(k); ld of F, X_out, rhs_extra */
    int64_t nrows;              /* rows in this orientation (bounds checks only) */
    int32_t F_zero_row;         /* index of an all-zero row of F (ratings past the end of a
                                   row are pointed at it instead of being masked); F_zero_row*ld
                                   and every indices[t]*ld must be < 2^31 */
    int32_t reserved0;          /* 0 (profiling builds: phase-ablation flags) */
    int32_t gram_mode;          /* ALS_GRAM_F32: v_mfma_f32_16x16x4_f32 on the gathered floats;
                                   ALS_GRAM_F16X2: every float times S (a power of two, als_factor_scale) is split
                                   into two fp16 terms by rounding to nearest (error <= 2^-23), three cross
                                   products on v_mfma_f32_16x16x32_f16, fp32 accumulate (same accuracy
                                   class, the 16-bit matrix cores run beside the VALU); needs F_scale;
                                   ALS_GRAM_F64: everything in fp64 (row_solve_f64.hip) - for lambda << 1 with
                                   rank-deficient rows, where cond(A) ~ 1/lambda amplifies the fp32 rounding of
                                   the Gram; workspace slots are als_partial_slot_bytes_f64(k) bytes; the
                                   dual-form classes are ignored */
    int32_t ndual_tail;         /* number of TRAILING tasks that are whole rows (slot < 0) of at most 64 ratings
                                   to be solved in the dual form (n x n instead of k x k system, same
                                   solution); honoured in plain solve calls (no by-product outputs, no
                                   rhs_extra / diag_extra, f16x2 Gram).  Pays when the n x n system is much
                                   the smaller one (k > 64: 5x per row at k = 128; at k = 64, n <= 48 it measured
                                   equal to the primal kernel); 0 = never */
    int32_t ndual_mid;          /* number of tasks just BEFORE that tail that are whole rows of 65 ... 96 ratings,
                                   for the dual form at k > 96 (an 80- or 96-size system); 0 = never */
    int32_t F_scale_ready;      /* != 0: F_scale[0 .. 1] already hold als_factor_scale(F) (several calls on one F) */
    const int64_t* indptr;
    const int32_t* indices;
    const float*   vals;
    const float*   F;           /* gathered side factors [ncols][ld] */
    const float*   bias_self;   /* [nrows], values before this step */
    const float*   bias_other;  /* [ncols] */
    const double*  mu;          /* device scalar */
    float          lambda_scalar;
    const float*   lambda_row;          /* nullable */
    float          lambda_bias_scalar;
    const float*   lambda_bias_row;     /* nullable */
    const float*   rhs_extra;           /* nullable [nrows][ld] */
    const float*   diag_extra;          /* nullable [nrows] */
    float*         X_out;               /* [nrows][ld] */
    float*         bias_out;            /* [nrows] (may alias bias_self) */
    float*         gram_out;            /* nullable */
    float*         factor_out;          /* nullable -> factor-only mode */
    float*         rhs_out;
    float*         colsum_out;
    float*         sumr_out;
    float*         sumr2_out;           /* nullable [nrows]: sum_t (vals[t]-mu-bias_other)^2 (factor-only mode) */
    float*         stat_out;            /* nullable [nrows][2]: (sum d, sum d^2) of the row with the NEW x and
                                           bias, d = vals - F_t.x - mu - bias_other - bias_new; lets the caller
                                           skip als_residual_stats when Z == F-side of the other step */
    int32_t*       status;
    const als_task*     tasks;      int64_t ntasks;
    const als_long_row* long_rows;  int64_t nlong;
    void*          workspace;
    /* Conditioning-driven precision (solve_dtype "auto"): with cond_limit > 0 every row's condition estimate is taken
     * from what the fp32 factorisation leaves in registers - kappa = max( (max_i L_ii / min_i L_ii)^2,
     * (trace(G) / rank + lambda) / min_i L_ii^2, and for rows of fewer than 4 k ratings (mean eigenvalue) / lambda ),
     * three lower bounds of cond_2(A).  A row with kappa > cond_limit (or whose fp32 factorisation breaks down, or
     * whose closed-form statistics would cancel) writes none of its results - its row id is appended to redo_rows
     * (order irrelevant) and the call then redoes exactly those rows in fp64 (Gram, factorisation, substitutions:
     * the kernel of ALS_GRAM_F64 on the whole row).  The relative error of an fp32 row is then bounded by about
     * cond_limit * 3e-7 (the fp32 rounding of its Gram).  f32 / f16x2 modes only.
     * The fp64 redo costs about 20 fp32 rows per row: over a long fit at small lambda most user rows end up flagged and
     * the U-step grows 20-fold (profiles/r03_auto_redo_over_a_long_fit.txt).  als_row_solve_refine (solve_dtype
     * "refine") takes the same flagged rows through fp64 iterative refinement on their fp32 factor instead and leaves
     * only those that do not converge to the fp64 kernel. */
    float          cond_limit;          /* 0 = off */
    int32_t        byproducts_f64;      /* ALS_GRAM_F64 only, != 0: gram_out, rhs_out, colsum_out, sumr_out, sumr2_out are
                                           arrays of DOUBLE (same shapes) - for the W-step / item statistics in fp64
                                           (als_w_params::f64, als_item_stats_f64) - and factor_out an array of double
                                           (als_gs_sweep_params::factor_f64) */
    int32_t*       redo_count;          /* device int32[1]; the call resets it; afterwards: number of rows redone */
    int32_t*       redo_rows;           /* device int32[rows of this orientation] (only the first redo_count are used) */
    float*         cond_out;            /* nullable [nrows]: kappa of every row solved in fp32 (diagnostics) */
    float*         F_scale;             /* ALS_GRAM_F16X2: ALS_FSCALE_FLOATS floats of device memory, zero before the FIRST
                                           use (later calls leave words 2, 3 zero); the call writes {S, 1 / S^2} of F to
                                           words 0, 1 unless F_scale_ready; must not be shared by concurrent calls */
    void*          F_planes;            /* nullable; ALS_GRAM_F16X2 at k = 49 ... 64 or 113 ... 128: scratch of (F_zero_row + 1) * ld 32-bit
                                           words (F_zero_row must be the LAST row of F).  When given, the call first
                                           writes the two fp16 terms of every element of F into it (same layout as F)
                                           and the Gram is built from those pre-split operands, right-hand side and
                                           column sums on the matrix cores too - same Gram bit for bit, far fewer
                                           vector instructions per rating.  Pays where F is small and the launch is
                                           bound by vector issue (the U-step); costs one pass over F.  Must not be
                                           shared by concurrent calls */
    float          R_scale;             /* F_planes path only: scale of the residuals vals - mu - bias_other - bias_self,
                                           which that path hands to the matrix cores as two fp16 terms each.  The
                                           CALLER supplies it: the power of two that puts the largest |vals| of the
                                           call in [2^9, 2^10) (a per-fit constant; the bindings' residual_scale()).
                                           A residual of up to 64 times the largest rating then stays inside the fp16
                                           range and one down to 2^-13 of it keeps full precision (2^-21 relative);
                                           the results are the same bits, times 2^p, when vals, mu and the biases are
                                           multiplied by 2^p and R_scale by 2^-p.  A residual beyond the range
                                           (|r| R_scale >= 65520) makes the row's sums inf / NaN: status receives
                                           (row + 1) as for a non-SPD pivot.  0 = 1.0 (no scale: accurate for ratings
                                           of order 1 ... 10^3 only); anything else that is not a normal power of
                                           two: ALS_E_BADARG */
} als_row_solve_params;

int als_row_solve(const als_row_solve_params* p, void* stream);

/* ---------------------------------------------------------------------------
 * als_row_solve_refine - als_row_solve with cond_limit > 0 (solve_dtype "refine"), the flagged rows by fp64
 * ITERATIVE REFINEMENT on their fp32 factor instead of an fp64 factorisation.
 *
 * The fp32 launches and the list of flagged rows (redo_rows / redo_count) are those of als_row_solve.  A PLAIN solve
 * call (X_out and bias_out; gram_out, factor_out, rhs_out, colsum_out, sumr_out, sumr2_out, rhs_extra and diag_extra
 * all NULL; reserved0 == 0) then hands the list to k_row_refine: per row the fp32 Gram (f32 or f16x2 as the call
 * says, always the primal k x k form) and its Cholesky factor L, x0 from the fp32 substitutions, and at most
 * max_steps times
 *     r = F^T (rho - F x) - lambda x      fp64, from the ratings (rho = vals - mu - bias_other - bias_self)
 *     d = (L L^T)^-1 r                    fp32, r scaled by a power of two
 *     x += d                              fp64
 * until the predicted remaining error |d_t|^2 / |d_t-1| (max norms; |d_1| at the first step) is at most
 * 2^-29 |x|.  Bias and stat_out of an accepted row are evaluated in fp64 from the ratings with the final x; x and
 * the bias are rounded to fp32 once.  A row that does not contract (|d_t| > |d_t-1| / 4), that runs out of steps,
 * whose fp32 factorisation breaks down or that has more than ALS_SPLIT_CHUNK ratings is appended to fallback_rows
 * and redone by the fp64 kernel of als_row_solve, as every flagged row of any other call is (fallback_count ==
 * redo_count then).  *p->redo_count keeps its meaning: the number of rows flagged.
 * Needs cond_limit > 0 and gram_mode ALS_GRAM_F32 or ALS_GRAM_F16X2 (ALS_E_BADARG otherwise).
 * ------------------------------------------------------------------------- */
typedef struct als_refine_params {
    int32_t  max_steps;         /* 1 ... 8 */
    int32_t* fallback_count;    /* device int32[1]; the call resets it; afterwards: rows redone by the fp64 kernel */
    int32_t* fallback_rows;     /* device int32[rows of this orientation] (only the first fallback_count are used) */
    int32_t* step_hist;         /* nullable device int32[9]: rows accepted after s steps, reset by the call */
} als_refine_params;

int als_row_solve_refine(const als_row_solve_params* p, const als_refine_params* r, void* stream);

/* Operand scale of the f16x2 Gram for a factor matrix F of `nfloats` floats (a multiple of 4, F 16-byte aligned):
 * scale[0] = S = 2^j with S max|F| in [2^14, 2^15) (clamped to 2^-60 ... 2^60), scale[1] = 1 / S^2; scale[2 .. 3]
 * are working words, zero on entry and on exit.  als_row_solve calls this itself unless F_scale_ready. */
#define ALS_FSCALE_FLOATS 4
int als_factor_scale(const float* F, int64_t nfloats, float* scale, void* stream);

/* ---------------------------------------------------------------------------
 * als_gs_sweep - one level of the Gauss-Seidel Laplacian sweep.
 * Replaces the graph part of the item loop (scripts/als.py:453-461,464-466):
 * for each listed item i (all items of one dependency level):
 *     b = rhs[i] + alpha * sum_j S_ij V[j]        (V read live)
 *     V[i] = (L L^T)^{-1} b ;  b_i[i] = (sumr[i] - colsum[i].V[i]) / denom
 * factor/rhs/colsum/sumr come from als_row_solve in factor-only mode.
 * ------------------------------------------------------------------------- */
typedef struct als_gs_sweep_params {
    int32_t k, ld;
    const int32_t* items;  int64_t nitems;   /* items of this level */
    const int64_t* S_ptr;  const int32_t* S_idx;  const float* S_val;
    float alpha;
    const float* factor;  const float* rhs;  const float* colsum;
    const float* sumr;
    const int64_t* indptr;               /* CSC pointers (nnz per item) */
    float lambda_bias_scalar;  const float* lambda_bias_row;
    float* V;                            /* [n][ld], updated in place */
    float* bias;                         /* [n] */
    /* optional fused statistics (all three or none): */
    const float* sumr2;                  /* [n] from als_row_solve (sumr2_out) */
    const float* lambda_eff;             /* [n] total diagonal shift used in the factor (lambda+1e-10+diag_extra) */
    float* stat_out;                     /* [n][2]: (sum d, sum d^2) with the new V[i], bias[i] */
    int32_t f64;                         /* != 0: factor, rhs, colsum, sumr, sumr2 are arrays of DOUBLE (als_row_solve with
                                            ALS_GRAM_F64 and byproducts_f64); neighbour sums, substitutions, bias and
                                            statistics then run in fp64 (als_gs_sweep / als_gs_sweep_levels only) */
    int32_t reserved;
} als_gs_sweep_params;

int als_gs_sweep(const als_gs_sweep_params* p, void* stream);

/* Whole sweep as ONE persistent launch without level barriers.  p->items lists ALL swept
 * items in (level, id) order (p->nitems of them).  S_idx_wait is p->S_idx with the sign bit set on
 * every edge (i -> j) that item i must wait for (j < i and j swept in this call).  publish: scratch
 * [nrows][ld] floats (nrows = rows of p->V); the call resets it and the kernel hands solved rows from
 * producer to consumer through it (each word doubles as its own "ready" flag).  nondep: optional scratch
 * [nrows][ld]: when given, the neighbour sums that do not depend on the sweep (edges without the wait flag) are
 * formed for all items by one parallel launch before the persistent one - same sums, same order, off the
 * dependency chain.  err: int32[1], the caller
 * zeroes it once; set to 1 when a dependency wait exceeded its bound (2^27 shader-clock ticks, ~60 ms: the launch was not resident as a
 * whole because something else held compute units).  Results are then invalid and the caller should redo the
 * sweep - from the state before it - with als_gs_sweep_levels, which has no residency requirement. */
int als_gs_sweep_dataflow(const als_gs_sweep_params* p, const int32_t* S_idx_wait, float* publish,
                          int64_t nrows, float* nondep, int32_t* err, void* stream);

/* Whole sweep in one call: level l covers p->items[level_offsets[l] .. level_offsets[l+1]) (host
 * array of nlevels+1 offsets into the device array p->items; p->nitems is ignored).  One launch per
 * level on `stream`; levels are dependent, so stream order is the synchronisation. */
int als_gs_sweep_levels(const als_gs_sweep_params* p, const int64_t* level_offsets /* host */,
                        int64_t nlevels, void* stream);

/* ---------------------------------------------------------------------------
 * als_residual_stats - replaces scripts/als.py:503-512: one pass over the
 * ratings (CSR) computing sum(d) and sum(d^2), d = r - (U_u.Z_i + b_u + b_i
 * + mu_old), in fp64.  out[0]=sum d, out[1]=sum d^2 (device doubles).
 * partials: scratch of 2*ceil(ntasks/4) doubles.
 * ------------------------------------------------------------------------- */
int als_residual_stats(int k, int ld, const int64_t* indptr, const int32_t* indices,
                       const float* vals, const float* U, const float* Z,
                       const float* b_u, const float* b_i, const double* mu,
                       const als_task* tasks, int64_t ntasks,
                       double* partials, double* out, void* stream);

/* ---------------------------------------------------------------------------
 * als_w_normal_equations - normal equations of the feature-projection step,
 * replaces scripts/als.py:469-499 (the N_obs x (d k) design matrix is never formed).
 *   phase 0: per-item vectors h_{f,i} = g_i + G_i xw_{f,i} for all features (H, perm space),
 *            from the V-step by-products gram/rhs/colsum (als_row_solve), the new and old item
 *            bias, V and the OLD projections W (Jacobi across features, as the reference).
 *   phase 1: for ONE feature (columns feat_col0 .. +feat_d of X): A_out [(d*k)^2] =
 *            sum_i (x_i x_i^T) (x) G_i and B_out [d*k] = sum_i x_i (x) h_{f,i}, fp64, index
 *            a*k + c with c the factor column in storage order (the reference's vec layout,
 *            scripts/als.py:494); A_out is bitwise symmetric; the caller adds lambda.
 * Items [item_begin, item_end) only (a rank's shard); A/B are then all-reduced by the caller.
 * ------------------------------------------------------------------------- */
typedef struct als_w_params {
    int32_t k, ld;
    int32_t phase;                 /* 0: item vectors, 1: accumulate one feature */
    int32_t nfeat;                 /* phase 0: number of features (<= 8) */
    int64_t item_begin, item_end;
    const float* gram;             /* [n][ld][ld] lower blocks (als_row_solve gram_out) */
    const float* rhs;              /* [n][ld] perm  (rhs_out)    */
    const float* colsum;           /* [n][ld] perm  (colsum_out) */
    const float* V;                /* [n][ld] */
    const float* b_new;            /* [n] item bias after the V-step  */
    const float* b_old;            /* [n] item bias before the V-step */
    int32_t D;                     /* total feature columns of X */
    int32_t f64;                   /* != 0: gram, rhs, colsum, H are arrays of double (als_row_solve byproducts_f64) and W
                                      is the fp64 projection matrix [D][k] (row stride k, storage column order) */
    const float* X;                /* [n][D] all features side by side */
    const int32_t* feat_off;       /* device int32 [nfeat+1] column offsets (phase 0) */
    const float* W;                /* [D][ld] old projections, storage column order (phase 0) */
    float* H;                      /* [nfeat][nrows_h][ld] (phase 0 writes, phase 1 reads) */
    int64_t nrows_h;
    int32_t feat_index, feat_col0, feat_d, nchunks;   /* phase 1 */
    double* partA;                 /* scratch: d(d+1)/2 * nchunks * (ld/16)(ld/16+1)/2 * 256 doubles */
    double* partB;                 /* scratch: d * nchunks * ld doubles */
    double* A_out;                 /* [(d*k)][(d*k)] */
    double* B_out;                 /* [d*k] */
} als_w_params;

int als_w_normal_equations(const als_w_params* p, void* stream);

/* -------------------------------------------------------------------------
 * als_spd_solve_f64: x = (A + diag_add I)^-1 b by a dense fp64 Cholesky factorisation -
 * the reference's `cholesky_solve(A, b)` on the W-step's (d k) x (d k) normal equations
 * (scripts/als.py:497-500; scripts/helpers.py cholesky_solve).
 * A: [N][lda] row-major fp64, lda >= N (columns N .. lda-1 are never read), symmetric (both triangles
 * valid), not modified.  b, x: [N] (may alias).  1 <= N <= ALS_SPD_MAX_N.
 * workspace: als_spd_solve_workspace_bytes(N) bytes of device memory (0 = N out of range); its contents
 * on entry do not matter, a call writes everything it reads.
 * status (device int32): any value on entry, every call resets it.  0 ok; p > 0: pivot p-1 is the first
 * that was not positive; a NaN pivot counts, so a NaN entry A[r][c], r >= c, reports r + 1.  x is then
 * meaningless (the pivot is replaced by 1 and the call runs to its end).
 * Backward stable at LAPACK's level for cond_2 up to 1e12 and under A 2^p, |p| <= 400 (tests/test_gpu_spd_solve.py).
 * Enqueues at most 2 ceil(N/64) + 2 small kernels on `stream`; the last one takes (ceil(N/64) + 1) 512 bytes
 * of dynamic LDS, 64 KB at ALS_SPD_MAX_N.
 * ------------------------------------------------------------------------- */
#define ALS_SPD_MAX_N 8128
size_t als_spd_solve_workspace_bytes(int64_t N);
int als_spd_solve_f64(int64_t N, const double* A, int64_t lda, const double* b, double diag_add,
                      double* x, void* workspace, int32_t* status, void* stream);

/* Closed-form residual sums per item when Z != V (fits with features), replacing the pass over the
 * ratings of scripts/als.py:505-511: stat_out[i] = (sum d, sum d^2), d = r - mu - b_u - b_new[i] - u.Z[i],
 * from the als_row_solve by-products of this iteration's V-step (gram_out, rhs_out, colsum_out, sumr_out,
 * sumr2_out - rhs formed with b_old) over items [item_begin, item_end).  Z: [n][ld] storage order. */
int als_item_stats(int k, int ld, int64_t item_begin, int64_t item_end, const float* gram,
                   const float* rhs, const float* colsum, const float* sumr, const float* sumr2,
                   const int64_t* indptr, const float* Z, const float* b_new, const float* b_old,
                   float* stat_out, void* stream);

/* The same from fp64 by-products (als_row_solve with gram_mode ALS_GRAM_F64 and byproducts_f64). */
int als_item_stats_f64(int k, int ld, int64_t item_begin, int64_t item_end, const double* gram,
                       const double* rhs, const double* colsum, const double* sumr, const double* sumr2,
                       const int64_t* indptr, const float* Z, const float* b_new, const float* b_old,
                       float* stat_out, void* stream);

/* out[0] = sum_i x[2i], out[1] = sum_i x[2i+1] in fp64 (reduction of stat_out).
 * partials: scratch of 2*als_sumsq_partials() doubles. */
int als_sum_pairs(const float* x, int64_t npairs, double* partials, double* out, void* stream);

/* sum of squares of a float array in fp64 (scripts/als.py:514-517 norms).
 * partials: scratch of als_sumsq_partials() doubles. out: device double. */
int als_sumsq_partials(void);
int als_sumsq(const float* x, int64_t n, double* partials, double* out, void* stream);

/* The history row of an iteration in two launches (scripts/als.py:505-517): stats = (sum d, sum d^2) of the residuals
 * before the mu update (als_sum_pairs / als_residual_stats), nnz ratings.  mu (device double) += sum d / nnz;
 * row[6] = {train RMSE with the new mu, |U|_F, |V|_F, |b_u|, |b_i|, mu}.  The arrays must be 16-byte aligned.
 * partials: scratch of 4 * als_sumsq_partials() doubles. */
int als_history_row(const float* U, int64_t nU, const float* V, int64_t nV, const float* b_u, int64_t nbu,
                    const float* b_i, int64_t nbi, const double* stats, int64_t nnz, double* mu,
                    double* partials, double* row, void* stream);

/* Z = V + X W  (scripts/als.py:262-281); X [n][D] fp32 (all features
 * concatenated column-wise), W [D][ld] fp32.  D == 0 copies V. */
int als_compose_z(int64_t n, int ld, int D, const float* V, const float* X,
                  const float* W, float* Z, void* stream);

/* predictions at (u,i) pairs: out[t] = U_u.Z_i + mu + b_u + b_i
 * (the only way callers read predict(): scripts/tune_params.py:165-166) */
int als_predict_at(int k, int ld, int64_t npairs, const int32_t* us, const int32_t* is,
                   const float* U, const float* Z, const float* b_u, const float* b_i,
                   const double* mu, float* out, void* stream);

/* dense completion R_hat[m][n] = U Z^T + mu + b_u + b_i (scripts/als.py:574) */
int als_predict_dense(int k, int ld, int64_t m, int64_t n, const float* U,
                      const float* Z, const float* b_u, const float* b_i,
                      const double* mu, float* out, void* stream);

/* ---------------------------------------------------------------------------
 * Item-item similarity graph on the device (scripts/als.py:224-240 without the n x n matrix).
 * als_topk_similarity: XT is the row-normalised feature matrix Xn [n][d] (fp32) re-laid as [nsteps][n_pad][4]
 *   (feature dims in groups of 4, zero padded: nsteps in {1, 2, 4, 5, 8, 16}, i.e. d <= 64; n_pad a multiple of
 *   16, padding rows zero).  For every row i the topk (<= ALS_TOPK_MAX) largest entries of row i of Xn Xn^T with
 *   its diagonal set to 0 (the diagonal entry competes like any other, as in the reference; zeros are never
 *   edges), ordered by (similarity descending, j ascending) - among equal similarities the LOWEST column indices win (the
 *   reference's argpartition keeps an implementation-defined subset of such ties):
 *   top_val / top_idx [n][topk] (unused slots 0 / -1), top_cnt [n] = min(topk, n).
 * als_graph_classify: S = max(S, S^T) on those lists: own[i][t] = 1 when entry t of row i is an edge of the
 *   symmetric graph, mirror[i][t] = 1 when its transpose (j, i, s) must be added because j's list does not
 *   contain i (one-sided positive entries; one-sided negative ones and zeros are not edges).
 * ------------------------------------------------------------------------- */
#define ALS_TOPK_MAX 128
int als_topk_similarity(int64_t n, int64_t n_pad, int nsteps, const float* XT, int topk, float* top_val,
                        int32_t* top_idx, int32_t* top_cnt, void* stream);
int als_graph_classify(int64_t n, int topk, const float* top_val, const int32_t* top_idx,
                       const int32_t* top_cnt, uint8_t* own, uint8_t* mirror, void* stream);

/* ---------------------------------------------------------------------------
 * Top-N recommendation.  For every batch row b (user u = users[b], in [0, m); duplicates allowed):
 *   score(u, i) = U_u.Z_i + mu + b_u + b_i - bitwise the fp32 value als_predict_dense writes at (u, i) -
 *   over all items i < n that are not in u's seen row (seen_ptr [m+1] / seen_idx: a CSR indexed by USER ID,
 *   column indices ascending within each row; both NULL = exclude nothing).  NaN scores are never returned.
 *   top_val / top_idx [nusers][topn], ordered by (score descending, item ascending) - among equal scores the
 *   LOWEST item indices win; unused slots: top_idx -1, top_val -inf; top_cnt [nusers] = number of valid slots.
 *   1 <= topn <= ALS_TOPK_MAX, n < 2^31; nusers == 0 is a no-op.
 * nslices: 0 = automatic, otherwise the number of item slices (<= ALS_RECOMMEND_MAX_SLICES, at most one per 32
 *   items) the item range is cut into, each slice's lists merged by a second launch; the result does not depend on
 *   it (an override for tests and measurements).
 * workspace: als_recommend_workspace_bytes(nusers, n, topn, nslices) bytes of device memory (0: may be NULL);
 *   the call allocates nothing.
 * ------------------------------------------------------------------------- */
#define ALS_RECOMMEND_MAX_SLICES 64
size_t als_recommend_workspace_bytes(int64_t nusers, int64_t n, int topn, int nslices);
int als_recommend_topk(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                       const float* Z, const float* b_u, const float* b_i, const double* mu,
                       const int64_t* seen_ptr, const int32_t* seen_idx, int topn, int nslices,
                       float* top_val, int32_t* top_idx, int32_t* top_cnt, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Top-N recommendation over a restricted catalogue: als_recommend_topk with the items limited to an allow bitmap.
 *   allow: device bitmap of ceil(n / 32) words; item i is allowed iff bit (i & 31) of word (i >> 5) is set; bits at
 *   positions >= n are ignored.  A disallowed item is never returned, exactly like a seen one; everything else -
 *   scores, order, ties, unused slots, top_cnt, nslices, the workspace (als_recommend_workspace_bytes) - is
 *   als_recommend_topk's, and the result does not depend on the slice count.  An all-zero bitmap gives empty lists
 *   (top_cnt 0).  allow == NULL allows every item: the call is then als_recommend_topk (which forwards here).
 * The items are walked in chunks of 32; a chunk whose word is 0 is neither loaded nor scored, only scanned past.
 * ------------------------------------------------------------------------- */
int als_recommend_topk_masked(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                              const float* Z, const float* b_u, const float* b_i, const double* mu,
                              const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow, int topn,
                              int nslices, float* top_val, int32_t* top_idx, int32_t* top_cnt, void* workspace,
                              size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Deep top-N with a paging cursor: als_recommend_topk_masked for 1 <= topn <= ALS_TOPK_DEEP_MAX, exactly.
 *   Model arguments, seen rows, allow (NULL = every item), scores, order, ties, unused slots (top_idx -1, top_val
 *   -inf) and top_cnt are als_recommend_topk_masked's; for topn <= ALS_TOPK_MAX and after_key == NULL the outputs
 *   equal that call's, element for element.  n < 2^31; nusers == 0 is a no-op.
 * after_key: NULL, or [nusers] cursor keys.  A candidate is the 64-bit key (enc(score) << 32) | (0xFFFFFFFF - item),
 *   enc(s) = the bits of s + 0.0f with the sign bit set when s >= 0 and all bits inverted otherwise, so that the
 *   integer order of the keys is (score descending, item ascending).  Row b then lists the topn best candidates whose
 *   key is STRICTLY BELOW after_key[b]: with the key of the last entry of a page, the next page.  after_key[b] == 0
 *   (no candidate is below it) gives an empty row, ~0 is no cursor.
 * rounds: NULL, or one device int that receives the number of scoring rounds that did work, 1 ... ceil(topn / 128).
 *   The call enqueues ceil(topn / 128) rounds of (scoring below a per-slice ceiling, merge) without synchronising with
 *   the host; the kernels of a round return at once when the round before left no slice open, which is the rule when
 *   the best topn items are spread over the slices.  The result is exact and does not depend on the slice count.
 * nslices: as als_recommend_topk; 0 = automatic: that call's count, but at least ALS_DEEP_SLICE_FACTOR ceil(topn / 128)
 *   (capped by ALS_RECOMMEND_MAX_SLICES and one slice per 32 items).
 * workspace: als_recommend_deep_workspace_bytes(nusers, n, topn, nslices) bytes of device memory, always > 0:
 *   8 nusers (128 S + NL + S) + 64 with S the slice count and NL = 128, 256, 512 or 1024, the least that holds topn
 *   (the slice lists, the running list, the ceilings, the round flags).  The call allocates nothing.
 * ------------------------------------------------------------------------- */
#define ALS_TOPK_DEEP_MAX 1024
#define ALS_DEEP_SLICE_FACTOR 4
size_t als_recommend_deep_workspace_bytes(int64_t nusers, int64_t n, int topn, int nslices);
int als_recommend_deep(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                       const float* Z, const float* b_u, const float* b_i, const double* mu,
                       const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow,
                       const unsigned long long* after_key, int topn, int nslices, float* top_val, int32_t* top_idx,
                       int32_t* top_cnt, int32_t* rounds, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Exact full-catalogue ranks (evaluation).  Model arguments as als_recommend_topk: score(u, j) is bitwise the fp32
 * value als_predict_dense writes; seen_ptr / seen_idx a CSR by USER ID, ascending (both NULL = exclude nothing).
 * For user u the candidates are C(u) = { j < n : j not in u's seen row, score(u, j) is not NaN }.
 * Queries: nq batch rows; row b has user q_users[b] (in [0, m), duplicates allowed) and the targets
 *   q_items[q_ptr[b] .. q_ptr[b+1]) (q_ptr [nq+1] int64, q_ptr[0] = 0, q_ptr[nq] = nt; items in [0, n), any order,
 *   duplicates allowed, any number per row: a row with more than 16 targets is served by further passes over
 *   the catalogue inside the kernel).
 * Outputs, per target t of row b (position p in q_items), u = q_users[b]:
 *   t_score[p] = score(u, t);
 *   above[p]   = |{ j in C(u) : score(u, j) > score(u, t), or score(u, j) == score(u, t) and j < t }| - the number
 *                of candidates that precede t in als_recommend_topk's order (score descending, item ascending;
 *                -0.0 == +0.0).  Defined whether or not t is seen (t never precedes itself); -1 if score(u, t) is NaN.
 *   n_cand[b]  = |C(u)|.
 * n < 2^31; nq == 0 is a no-op.  nslices as als_recommend_topk (0 = automatic; the counts of the item slices are
 *   added by a second launch, so the result does not depend on it).
 * workspace: als_rank_count_workspace_bytes(k, nq, nt, n, nslices) bytes of device memory (0: may be NULL); the
 *   call allocates nothing.
 * ------------------------------------------------------------------------- */
size_t als_rank_count_workspace_bytes(int k, int64_t nq, int64_t nt, int64_t n, int nslices);
int als_rank_count(int k, int ld, int64_t n, const float* U, const float* Z, const float* b_u, const float* b_i,
                   const double* mu, const int64_t* seen_ptr, const int32_t* seen_idx, int64_t nq,
                   const int32_t* q_users, const int64_t* q_ptr, const int32_t* q_items, int64_t nt, int nslices,
                   float* t_score, int32_t* above, int32_t* n_cand, void* workspace, size_t workspace_bytes,
                   void* stream);

/* ---------------------------------------------------------------------------
 * Exact ranks within a restricted catalogue: als_rank_count with the candidates limited to an allow bitmap (the
 * bitmap of als_recommend_topk_masked: ceil(n / 32) words, bit (i & 31) of word (i >> 5), bits >= n ignored):
 *   C(u) = { j < n : j allowed, j not in u's seen row, score(u, j) is not NaN };
 *   above[p] and n_cand[b] count within this C(u); t_score[p] is unchanged.  As for a seen target, above[p] is
 *   defined whether or not t itself is allowed (the position t would take), so an item that
 *   als_recommend_topk_masked returns at position j has above == j under the same bitmap and seen rows.
 * allow == NULL allows every item: the call is then als_rank_count (which forwards here).  Workspace:
 *   als_rank_count_workspace_bytes.
 * ------------------------------------------------------------------------- */
int als_rank_count_masked(int k, int ld, int64_t n, const float* U, const float* Z, const float* b_u,
                          const float* b_i, const double* mu, const int64_t* seen_ptr, const int32_t* seen_idx,
                          const uint32_t* allow, int64_t nq, const int32_t* q_users, const int64_t* q_ptr,
                          const int32_t* q_items, int64_t nt, int nslices, float* t_score, int32_t* above,
                          int32_t* n_cand, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Per-row eligibility: als_recommend_topk_masked / als_rank_count_masked with one allow bitmap PER BATCH ROW, picked
 * from a table of segments ("this user's country / tier / age rating / language").
 *   seg_allow: device table of nseg >= 1 bitmap rows, seg_stride_words (>= ceil(n / 32)) words apart; row s is an
 *   allow bitmap as als_recommend_topk_masked reads it (item i = bit (i & 31) of word (i >> 5), bits >= n ignored).
 *   row_seg [nusers] (als_rank_count_segmented: [nq]): the segment of every batch row - per row, not per user id, so a
 *   user may appear under several segments in one call.  A row whose id is outside [0, nseg) has no candidates
 *   (top_cnt 0 / n_cand 0); nothing is read for it.
 *   Row b of the outputs equals, element for element, row b of als_recommend_topk_masked (als_rank_count_masked)
 *   called with allow = seg_allow + row_seg[b] * seg_stride_words; every other argument, the slices and the
 *   workspace (als_recommend_workspace_bytes / als_rank_count_workspace_bytes) are that call's.
 * The whole catalogue is walked for every workgroup (its rows disagree about which chunks are empty); a wave none of
 * whose 16 rows is allowed an item of a chunk of 32 skips the chunk's scores and selection.
 * ------------------------------------------------------------------------- */
int als_recommend_topk_segmented(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                                 const float* Z, const float* b_u, const float* b_i, const double* mu,
                                 const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* seg_allow,
                                 int64_t nseg, int64_t seg_stride_words, const int32_t* row_seg, int topn, int nslices,
                                 float* top_val, int32_t* top_idx, int32_t* top_cnt, void* workspace,
                                 size_t workspace_bytes, void* stream);
int als_rank_count_segmented(int k, int ld, int64_t n, const float* U, const float* Z, const float* b_u,
                             const float* b_i, const double* mu, const int64_t* seen_ptr, const int32_t* seen_idx,
                             const uint32_t* seg_allow, int64_t nseg, int64_t seg_stride_words, const int32_t* row_seg,
                             int64_t nq, const int32_t* q_users, const int64_t* q_ptr, const int32_t* q_items,
                             int64_t nt, int nslices, float* t_score, int32_t* above, int32_t* n_cand,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * The eligibility table from item attributes: out [nseg][W], W = ceil(n / 32), dense rows (seg_stride_words = W).
 *   item_tags [n][tw]: 1 <= tw <= ALS_ELIGIBILITY_MAX_TAG_WORDS words of attribute bits per item; need_all, need_any,
 *   forbid [nseg][tw]: the rule of every segment (NULL = all zero); base_allow: an allow bitmap over the n items ANDed
 *   into every segment, or NULL.  With t = item_tags[i] and the rule words of segment s:
 *     eligible(s, i) = (t & forbid) == 0 in every word  &&  (t & need_all) == need_all in every word
 *                      &&  (need_any is all zero  ||  (t & need_any) != 0 in some word)  &&  bit i of base_allow.
 *   Bit (i & 31) of out[s][i >> 5] = eligible(s, i); the bits >= n of the last word are written 0.
 * item_tags is read once (one lane per item keeps its words and loops over the segments).  n < 2^31; nseg == 0 is a
 * no-op; tw outside its range: ALS_E_BADARG.
 * ------------------------------------------------------------------------- */
#define ALS_ELIGIBILITY_MAX_TAG_WORDS 8
int als_eligibility_bitmaps(int64_t n, int tw, const uint32_t* item_tags, int64_t nseg, const uint32_t* need_all,
                            const uint32_t* need_any, const uint32_t* forbid, const uint32_t* base_allow,
                            uint32_t* out, void* stream);

/* ---------------------------------------------------------------------------
 * Top-N under per-item exposure caps (ALS.recommend_capacity): the two device pieces of its threshold rounds.
 *
 * Item-side keys: the pair (batch row b, item i) with score s has the key (enc(s) << 32) | (0xFFFFFFFF - b) - the key
 *   of als_recommend_deep with the BATCH ROW in the index word -, so the demanders of one item are ordered by (score
 *   descending, row ascending) and their keys are distinct.  floor_key [n]: one such key per item, 0 = no floor.
 *
 * als_recommend_topk_priced: als_recommend_topk_masked (allow == NULL: every item) with one more term in the candidate
 *   test - launched row b takes item i only if key(score(users[b], i), row_ids[b]) >= floor_key[i].  row_ids [nusers]:
 *   the batch row of every launched row (in [0, 2^31)), used in that key and nowhere else, so a compacted work list
 *   keeps its rows' priorities.  Everything else - scores, order, ties, unused slots, top_cnt, nslices, the workspace
 *   (als_recommend_workspace_bytes) - is that call's; with floor_key all 0 the outputs equal its outputs, element for
 *   element, whatever row_ids holds.
 *
 * als_capacity_settle: from the lists of the WHOLE batch (top_idx / top_val [nrows][topn], list row = batch row; a
 *   slot whose id is outside [0, n) is empty) and capacity [n] (negative counts as 0):
 *     d_i        = the number of list entries naming item i (an item is named at most once per row);
 *     fill[i]    = min(d_i, capacity[i]);
 *     floor_key[i] for every item with d_i > capacity[i] (over-demanded) = the capacity[i]-th largest item-side key
 *                  among its entries (capacity 0: ~0, which nothing passes); the other floors are left as they are;
 *     dirty[b]   = 1 if row b holds an entry whose item-side key is below the (new) floor of its item, else 0;
 *     *n_over    = the number of over-demanded items.
 *   The results do not depend on the order in which the integer atomics inside arrive.  nrows * topn < 2^31, n < 2^31.
 * workspace: als_capacity_settle_workspace_bytes(nrows, n, topn) bytes of device memory, always > 0 (four int32 [n]
 *   arrays, the counters, 8 nrows topn bytes of key buckets); the call allocates nothing, enqueues its launches on
 *   `stream` and does not synchronise with the host.
 * ------------------------------------------------------------------------- */
int als_recommend_topk_priced(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                              const float* Z, const float* b_u, const float* b_i, const double* mu,
                              const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow,
                              const int32_t* row_ids, const unsigned long long* floor_key, int topn, int nslices, float* top_val,
                              int32_t* top_idx, int32_t* top_cnt, void* workspace, size_t workspace_bytes,
                              void* stream);
size_t als_capacity_settle_workspace_bytes(int64_t nrows, int64_t n, int topn);
int als_capacity_settle(int64_t nrows, int topn, int64_t n, const int32_t* top_idx, const float* top_val,
                        const int32_t* capacity, unsigned long long* floor_key, int32_t* fill, int32_t* dirty,
                        int32_t* n_over, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Top-N with per-group caps inside each list (ALS.recommend_quota): "at most group_cap[g] items of group g in a list".
 *
 * als_recommend_topk_quota: als_recommend_topk_masked (allow == NULL: every item) with a group label per item and a
 *   cap per group.  item_group [n]: the label of every item, in [0, ngroups); any other value (-1 by convention) means
 *   the item belongs to no group and is never capped.  group_cap [ngroups]: at most this many items of the group in a
 *   list (<= 0: none; may be NULL when ngroups == 0).  Row b's list is one scan of the masked call's candidates in its
 *   order (score descending, item ascending): a candidate is taken iff fewer than group_cap[g] taken items share its
 *   group g, and the scan stops after topn taken items.  Scores, ties, unused slots (-1 / -inf), top_cnt, nslices and
 *   the workspace (als_recommend_workspace_bytes) are that call's; with every label outside [0, ngroups), or every
 *   cap >= topn, the outputs equal its outputs, element for element, and a group of cap 0 equals clearing its items
 *   from the bitmap.  The result does not depend on nslices.  A list that the caps keep from filling (fewer than topn
 *   takeable candidates) is exact as well but slow: its threshold never rises; callers clamp topn to the number of
 *   takeable items first (serving._Serving._quota_chunks does).
 * ------------------------------------------------------------------------- */
int als_recommend_topk_quota(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                             const float* Z, const float* b_u, const float* b_i, const double* mu,
                             const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow,
                             const int32_t* item_group, const int32_t* group_cap, int64_t ngroups, int topn,
                             int nslices, float* top_val, int32_t* top_idx, int32_t* top_cnt, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Fold-in: factors and biases of users outside the fit, the item side (Z, b_i, mu) held fixed - the fit's user
 * half-step (scripts/als.py:411-433) for new rows.  For every row r < nrows of the CSR (indptr [nrows+1] /
 * indices / vals: device, column indices in [0, n), unique and ascending within a row), with S its items, n_r = |S|:
 *   A = Z_S^T Z_S + (lambda_u + 1e-10) I,  g = Z_S^T (r - mu - b_i[S]),  h = Z_S^T 1,  s = sum (r - mu - b_i[S]),
 *   d = n_r + lambda_bu + 1e-10;
 *   n_sweeps = T >= 1: T alternations from b = 0, u_t = A^-1 (g - b_{t-1} h), b_t = (s - h.u_t) / d -> (u_T, b_T);
 *   n_sweeps = 0: their fixed point, the solution of [[A, h], [h^T, d]] [u; b] = [g; s].
 * One fp64 factorisation per row (Gram on the fp64 matrix cores from the fp32 Z, Cholesky and substitutions in
 * fp64); U_out [nrows][ld] (fp32, laid out as als_row_solve's X_out: columns >= k written 0) and b_u_out [nrows].
 * A row without ratings gets u = 0, b = 0.  A row's result depends only on its own ratings.
 * Z [n][ld] with zero padding columns (k .. ld-1), b_i [n], mu: device double.  ld = als_padded_k(k), n * ld < 2^31,
 * nrows < 2^31 - 1; nrows == 0 is a no-op.  status (device int32): a non-positive or NaN pivot (only a non-finite Z
 * makes one) sets it to max(status, row + 1).
 * ------------------------------------------------------------------------- */
typedef struct als_fold_in_params {
    int k, ld;
    int64_t nrows;
    int n_sweeps;                                   /* 0 = fixed point */
    const int64_t* indptr;
    const int32_t* indices;
    const float* vals;
    int64_t n;
    const float* Z;
    const float* b_i;
    const double* mu;
    float lambda_u, lambda_bu;
    float* U_out;
    float* b_u_out;
    int32_t* status;
} als_fold_in_params;
int als_fold_in(const als_fold_in_params* p, void* stream);

/* ---------------------------------------------------------------------------
 * Item fold-in: factors and biases of items outside the fit, the user side (U, b_u, mu) and the fitted items' V
 * held fixed - the fit's item half-step (scripts/als.py:436-466) for new columns.  For every row r < nrows of the
 * ratings CSR (indptr [nrows+1] / indices / vals: device, rater ids in [0, m), unique within a row), with S its
 * raters, n_r = |S|, and its graph row N_r (S_ptr [nrows+1] / S_idx / S_val: fitted item ids j in [0, n) with
 * weights s_rj, in any order; all three NULL = no graph), D_r = sum_j s_rj:
 *   lambda_r = (pop_reg ? lambda_v / sqrt(n_r + 1) : lambda_v) + 1e-10 + alpha D_r,
 *   A = U_S^T U_S + lambda_r I,  g = U_S^T (r - mu - b_u[S]) + alpha sum_j s_rj V_j,  h = U_S^T 1,
 *   s = sum (r - mu - b_u[S]),  d = n_r + lambda_bi + 1e-10;
 * then the recurrence / fixed point of als_fold_in (n_sweeps = T >= 1 or 0).  D_r and the neighbour sum run in
 * fp64 in the row's storage order.  A row without ratings is solved too: v = alpha sum_j s_rj V_j / lambda_r,
 * b = 0.  V_out [nrows][ld] (columns >= k written 0), b_i_out [nrows].  U [m][ld] and V [n][ld] with zero padding
 * columns, mu: device double.  ld = als_padded_k(k), m * ld < 2^31 and n * ld < 2^31, nrows < 2^31 - 1; nrows == 0
 * is a no-op.  status as in als_fold_in.
 * ------------------------------------------------------------------------- */
typedef struct als_fold_in_items_params {
    int k, ld;
    int64_t nrows;
    int n_sweeps;                                   /* 0 = fixed point */
    int pop_reg;                                    /* 1: lambda_v / sqrt(n_r + 1) */
    const int64_t* indptr;
    const int32_t* indices;
    const float* vals;
    int64_t m;
    const float* U;
    const float* b_u;
    const double* mu;
    const int64_t* S_ptr;
    const int32_t* S_idx;
    const float* S_val;
    int64_t n;
    const float* V;
    float lambda_v, lambda_bi, alpha, reserved;
    float* V_out;
    float* b_i_out;
    int32_t* status;
} als_fold_in_items_params;
int als_fold_in_items(const als_fold_in_items_params* p, void* stream);

/* ---------------------------------------------------------------------------
 * Explanation of a score: how the ratings of a row make up the score of a target item, and the leverage of the
 * target.  Work row w < nrows reads row rows[w] of the ratings CSR (rows NULL: row w; indptr / indices / vals:
 * device, column indices in [0, n), unique and ascending within a row); S its items, n_w = |S|.  With als_fold_in's
 *   A = Z_S^T Z_S + (lambda_u + 1e-10) I, g, h, s, d and n_sweeps: (u, b_u) as als_fold_in, and bprev the bias u was
 *   solved with (n_sweeps = 0: b_u = bprev = the fixed point; T >= 1: b_u = b_T, bprev = b_{T-1}),
 * every target i in t_items[t_ptr[w] .. t_ptr[w+1]) (t_ptr [nrows+1] int64, t_ptr[0] = 0; items in [0, n), any
 * order, repeats allowed, a target may be in S) gets, all in fp64 from the fp32 tables (position p in t_items):
 *   rho_j = r_j - mu - b_i[j] - bprev,  w = A^-1 z_i,  weight[j] = w.z_j,  contribution[j] = weight[j] rho_j (j in S);
 *   latent[p] = sum_j contribution[j] (= u.z_i up to rounding),  leverage[p] = z_i^T A^-1 z_i = |L^-1 z_i|^2,
 *   score[p] = mu + b_u + b_i[i] + latent[p];
 *   the topm (1 .. ALS_TOPK_MAX) strongest rated items: top_item / top_contrib / top_weight [nt][topm], ordered by
 *   (float32(contribution) descending, item ascending) for largest != 0 and by (float32(-contribution) descending,
 *   item ascending) for largest == 0; the values written are the fp64 ones, only the ordering key is rounded.
 *   Unused slots: item -1, contribution and weight 0.  top_cnt[p] = min(topm, n_w).
 * b_u_out [nrows] (double): b_u of the work row.  A row without ratings: u = 0, b_u = 0, latent = 0,
 * leverage = |z_i|^2 / (lambda_u + 1e-10), score = mu + b_i[i].  A (row, target) result depends only on that row's
 * ratings and the target.  Sizes and status as als_fold_in (status: max(status, w + 1), the WORK row); nrows == 0
 * is a no-op.  Every pointer but rows must be valid (device).
 * ------------------------------------------------------------------------- */
typedef struct als_explain_params {
    int k, ld;
    int64_t nrows;                                  /* work rows */
    int n_sweeps;                                   /* 0 = fixed point */
    int topm;
    int largest;
    int reserved;
    const int64_t* indptr;
    const int32_t* indices;
    const float* vals;
    const int32_t* rows;                            /* [nrows] CSR row of each work row, or NULL */
    int64_t n;
    const float* Z;
    const float* b_i;
    const double* mu;
    float lambda_u, lambda_bu;
    const int64_t* t_ptr;
    const int32_t* t_items;
    double* score;
    double* latent;
    double* leverage;
    int32_t* top_item;
    double* top_contrib;
    double* top_weight;
    int32_t* top_cnt;
    double* b_u_out;
    int32_t* status;
} als_explain_params;
int als_explain(const als_explain_params* p, void* stream);

/* ---------------------------------------------------------------------------
 * Diversified top-N.  A list is a row of item ids; it ends at the first -1 or at the first
 * id outside [0, n) (never dereferenced) or at its full width.  For two positions of a list, in fp32 from Z [n][ld]:
 *   G_jl = z_j . z_l (the matrix-core chain of als_predict_dense),  sim(j, l) = G_jl / sqrt(G_jj G_ll), 0 when either
 *   norm is 0; one value per unordered pair, so sim(j, l) == sim(l, j) bitwise;
 *   ILD = mean over the unordered pairs of the list of 1 - sim (fp64 sum in list order), NaN for fewer than 2 items.
 *
 * als_mmr_rerank: greedy maximal marginal relevance over a candidate pool per row.  cand_idx / cand_val
 *   [nrows][pool]: the pool in als_recommend_topk's output form (its top_idx / top_val with topn = pool).  With
 *   rel_j = (s_j - s_min) / (s_max - s_min) over the pool's entries (every rel_j = 0 when s_max - s_min is 0 or
 *   not finite), step t = 0 .. topn-1 picks, among the candidates not yet chosen, the one maximising
 *   (1 - lambda) rel_j - lambda max_{l chosen} sim(j, l)   (the maximum over the empty set is 0),
 *   ties to the lower pool position.  top_idx / top_val [nrows][topn]: the picks in pick order with their cand_val
 *   (copied), unused slots -1 / -inf; top_cnt [nrows] = min(topn, entries of the pool); top_ild [nrows] (nullable):
 *   the ILD of the returned list.  lambda = 0 returns the first topn pool entries of a pool ordered by score.
 * als_list_diversity: ild [nrows] = the ILD of the lists idx [nrows][len]; on a list als_mmr_rerank returned it is
 *   bitwise that call's top_ild.
 * Both: 1 <= pool, len <= ALS_TOPK_MAX, 1 <= topn <= pool, 0 <= lambda <= 1, n < 2^31, ld = als_padded_k(k);
 * asynchronous on the stream, no workspace; nrows == 0 is a no-op.
 * ------------------------------------------------------------------------- */
int als_mmr_rerank(int k, int ld, int64_t nrows, int64_t n, const float* Z, int pool, const float* cand_val,
                   const int32_t* cand_idx, float lambda, int topn, float* top_val, int32_t* top_idx,
                   int32_t* top_cnt, float* top_ild, void* stream);
int als_list_diversity(int k, int ld, int64_t nrows, int64_t n, const float* Z, int len, const int32_t* idx,
                       float* ild, void* stream);

/* ---------------------------------------------------------------------------
 * Nearest neighbours under the cosine: the rows of a factor table most similar to query rows.
 *
 * als_row_inv_norms: one pass over T [nrows][ld] (fp32, padding columns zero):
 *   inv_norm[r] = (float)(1 / sqrt(s)),  s = sum_c (double)T[r][c]^2 accumulated in fp64 - rows at 1e-20 or 1e19
 *   neither underflow nor overflow;  exactly 0 when s == 0;  NaN when s is NaN or +inf (a non-finite entry).
 *   nrows < 2^31; nrows == 0 is a no-op.
 *
 * als_similar_topk: for every batch row b, with q = q_ids[b] a row of Q (duplicates allowed, order kept):
 *   sim(b, j) = (Q_q.T_j * q_inv[q]) * t_inv[j] in fp32, in exactly this association; Q_q.T_j is bitwise the fp32
 *   value als_predict_dense writes for (U = Q, Z = T, zero biases, mu = 0); q_inv / t_inv are the als_row_inv_norms
 *   of Q / T.  A zero-norm row (inv 0) has similarity 0 to everything and competes like any other candidate; a row
 *   with inv NaN is never returned, and as a query it gets an empty list (top_cnt 0).
 *   The candidates are the rows j < n of T with j != self_ids[b] (self_ids NULL, or an entry of -1: no exclusion),
 *   the bit of j set in allow (the bitmap of als_recommend_topk_masked: ceil(n / 32) words, bit (j & 31) of word
 *   (j >> 5), bits >= n ignored; NULL allows every row), and a similarity that is not NaN.
 *   top_val / top_idx [nq][topn], ordered by (sim descending, j ascending), -0.0 == +0.0; unused slots: top_idx -1,
 *   top_val -inf; top_cnt [nq] = number of valid slots.  1 <= topn <= ALS_TOPK_MAX, n < 2^31; nq == 0 is a no-op.
 *   Q and T may be the same table (the neighbours of its own rows, self_ids = q_ids) or different ones of the same
 *   width (e.g. folded-in rows against the fitted table).
 * nslices: as als_recommend_topk - 0 = automatic, otherwise the number of slices (<= ALS_RECOMMEND_MAX_SLICES, at
 *   most one per 32 rows) the range of T is cut into, the slices' lists merged by a second launch; the result does
 *   not depend on it.
 * workspace: als_similar_workspace_bytes(nq, n, topn, nslices) bytes of device memory (0: may be NULL); the call
 *   allocates nothing.
 * ------------------------------------------------------------------------- */
int als_row_inv_norms(int k, int ld, int64_t nrows, const float* T, float* inv_norm, void* stream);
size_t als_similar_workspace_bytes(int64_t nq, int64_t n, int topn, int nslices);
int als_similar_topk(int k, int ld, int64_t nq, const int32_t* q_ids, const float* Q, const float* q_inv,
                     const int32_t* self_ids, int64_t n, const float* T, const float* t_inv, const uint32_t* allow,
                     int topn, int nslices, float* top_val, int32_t* top_idx, int32_t* top_cnt, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Audience of an item: als_recommend_topk in the other direction - the users to show an item
 * to.  For every batch row b, with i = q_ids[b] a row of Q (an item; duplicates allowed, order kept):
 *   score(b, u) = U_u.Q_i + mu + b_u[u] + q_bias[i] = ((dot + mu) + b_u[u]) + q_bias[i] in fp32 - bitwise the value
 *   als_predict_dense writes at (u, i) for Z = Q, b_i = q_bias (als_recommend_topk called with the two sides swapped
 *   adds the biases in the other order and differs in the last bit) -
 *   over all users u < m that are not in row i of the rater CSR (seen_ptr [rows(Q) + 1] / seen_idx: indexed by the
 *   QUERY'S ROW ID q_ids[b], user ids ascending within each row - the training CSC; both NULL = exclude nothing) and
 *   whose bit is set in allow (the bitmap of als_recommend_topk_masked over USERS: ceil(m / 32) words, bit (u & 31) of
 *   word (u >> 5), bits >= m ignored; NULL allows every user).  NaN scores are never returned.
 *   top_val / top_idx [nq][topn], ordered by (score descending, user ascending), -0.0 == +0.0 - among equal scores the
 *   LOWEST user ids win; unused slots: top_idx -1, top_val -inf; top_cnt [nq] = number of valid slots.
 *   1 <= topn <= ALS_TOPK_MAX, m < 2^31; nq == 0 is a no-op.  Q [rows][ld] and U [m][ld] with zero padding columns,
 *   ld = als_padded_k(k); q_bias [rows(Q)], b_u [m], mu: device double.
 * nslices: as als_recommend_topk - 0 = automatic, otherwise the number of slices (<= ALS_RECOMMEND_MAX_SLICES, at
 *   most one per 32 users) the user range is cut into, the slices' lists merged by a second launch; the result does
 *   not depend on it.
 * The users are walked in chunks of 32; a chunk whose bitmap word is 0 is not scored.  A rater list of any length
 *   costs one 16-entry load per block that holds a rater and a binary search per slice or skipped range.
 * workspace: als_audience_workspace_bytes(nq, m, topn, nslices) bytes of device memory (0: may be NULL); the call
 *   allocates nothing.
 * ------------------------------------------------------------------------- */
size_t als_audience_workspace_bytes(int64_t nq, int64_t m, int topn, int nslices);
int als_audience_topk(int k, int ld, int64_t nq, const int32_t* q_ids, const float* Q, const float* q_bias,
                      int64_t m, const float* U, const float* b_u, const double* mu,
                      const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow,
                      int topn, int nslices, float* top_val, int32_t* top_idx, int32_t* top_cnt,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Top-N for a group of users: one list for a household, a table, a room.  Batch group b has the
 * members g_users[g_ptr[b] .. g_ptr[b+1]) (g_ptr [ngroups+1] int64, device; rows of U and b_u, distinct within a group;
 * groups may repeat, order kept), 0 ... ALS_GROUP_MAX_MEMBERS of them.  Member j scores item i with
 *   s_j(i) = U_j.Z_i + mu + b_u[j] + b_i[i] - bitwise the fp32 value als_predict_dense writes at (j, i) -
 * and the group score of item i over the g members is, by aggregate,
 *   ALS_GROUP_MIN   the smallest s_j(i) (least misery),
 *   ALS_GROUP_MAX   the largest s_j(i),
 *   ALS_GROUP_MEAN  the fp64 sum of the fp32 s_j(i), divided by g in fp64, rounded once to fp32.  The order of the
 *                   sum is not specified: it is exact, and so independent of order, tiling and lane layout, when the
 *                   nonzero member scores of an item lie within a factor 2^17 of each other in magnitude (24-bit
 *                   values, at most 64 of them, 53-bit accumulator); outside that band the result is within one fp64
 *                   rounding of the exact sum.
 * Candidates of group b: the items i < n that are not in row b of the seen CSR (seen_ptr [ngroups+1] / seen_idx:
 *   indexed by BATCH GROUP, not by user - the caller forms the union of the members' rows; item ids ascending and
 *   distinct within a row; both NULL = exclude nothing), whose bit is set in allow (the item bitmap of
 *   als_recommend_topk_masked; NULL allows every item), for which NO member score is NaN (a minimum or maximum that
 *   skipped a NaN member is never returned) and whose group score is not NaN (a mean of +inf and -inf).
 *   top_val / top_idx [ngroups][topn], ordered by (group score descending, item ascending), -0.0 == +0.0 - among equal
 *   scores the LOWEST item ids win; unused slots: top_idx -1, top_val -inf; top_cnt [ngroups] = number of valid slots.
 *   A group without members gets an empty list (top_cnt 0).  A group of one gets als_recommend_topk's list for that
 *   user, bit for bit, under every aggregate.
 *   1 <= topn <= ALS_TOPK_MAX, n < 2^31; ngroups == 0 is a no-op.
 * max_members: the host cannot read the device g_ptr without a copy, so the caller states an upper bound of the group
 *   sizes, 0 ... ALS_GROUP_MAX_MEMBERS (anything else, like an unknown aggregate, is ALS_E_BADARG).  The kernel sizes
 *   nothing by g_ptr alone: a group longer than max_members is cut to its first max_members members.
 * nslices, workspace: as als_recommend_topk - 0 = automatic, the slices' lists merged by a second launch, the result
 *   does not depend on it; als_group_workspace_bytes(ngroups, n, topn, nslices) bytes of device memory (0: may be
 *   NULL); the call allocates nothing.
 * One wave serves one group: a group of <= 16 members costs one 16-row score tile per 16 items whatever its size, a
 *   larger one ceil(g / 16) tiles.  A chunk of 32 items whose bitmap word is 0 is neither loaded nor scored.
 * ------------------------------------------------------------------------- */
#define ALS_GROUP_MAX_MEMBERS 64
#define ALS_GROUP_MEAN 0
#define ALS_GROUP_MIN  1
#define ALS_GROUP_MAX  2
size_t als_group_workspace_bytes(int64_t ngroups, int64_t n, int topn, int nslices);
int als_group_topk(int k, int ld, int64_t ngroups, const int64_t* g_ptr, const int32_t* g_users, int max_members,
                   int64_t n, const float* U, const float* Z, const float* b_u, const float* b_i, const double* mu,
                   const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow, int aggregate,
                   int topn, int nslices, float* top_val, int32_t* top_idx, int32_t* top_cnt,
                   void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Uncertainty-aware top-N.  For a row of ratings with items S, A = Z_S^T Z_S +
 * (lambda_u + 1e-10) I is als_fold_in's / als_explain's ridge system, L its lower Cholesky factor (columns in their
 * natural order), and the leverage z_i^T A^-1 z_i = |L^-1 z_i|^2 of als_explain is, up to the noise variance, the
 * posterior variance of the latent score of item i.
 *
 * als_row_whitener: W_out [nrows][ld][ld] (fp32, row-major) = float32(L^-1) of every work row w < nrows - CSR row
 *   rows[w], or row w when rows == NULL (indptr / indices as als_explain; no ratings are read, any row length).  W
 *   is lower triangular: the upper triangle and the padding rows / columns k .. ld-1 are written 0.  fp64 Gram on
 *   the matrix cores, Cholesky and the inversion (forward substitution on the identity) in fp64, rounded once.  A
 *   row without ratings gets I / sqrt(lambda_u + 1e-10).  Sizes and status as als_fold_in (status: max(status,
 *   w + 1), the WORK row); nrows == 0 is a no-op.
 *
 * als_explore_topk: als_recommend_topk_masked with every item i of batch row b (user users[b]) keyed by
 *   key(i) = base(i) + beta * sqrt(lev(i)),   lev(i) = |W_b z_i|^2   (W [nusers][ld][ld], indexed by BATCH ROW),
 *   base(i) bitwise the fp32 value als_predict_dense writes at (users[b], i); lev(i) is formed in fp32 on the matrix
 *   cores over the lower 16 x 16 blocks of W_b and depends on (W_b, z_i) alone - not on the slice, the position in the
 *   batch or the neighbouring items; the key is sqrt, product and sum in fp32, each correctly rounded, never
 *   contracted: top_val == base + beta * sqrtf(top_lev) evaluated in float32.  beta: finite, either sign; beta == 0
 *   gives als_recommend_topk_masked's lists for finite leverages.
 *   Candidates: the items allowed (allow == NULL: all), not in the user's seen row (CSR by USER ID), whose base and
 *   key are not NaN.  top_val [nusers][topn] = the keys, top_idx, top_cnt, the order (key descending, item
 *   ascending), ties, unused slots (-inf / -1) and the slice independence as als_recommend_topk; top_lev
 *   [nusers][topn] = lev of every returned item (recomputed by the same instruction chain), 0 in unused slots.
 *   nslices / workspace: as als_recommend_topk, als_explore_workspace_bytes(k, nusers, n, topn, nslices) bytes.
 *   One wave serves one batch row; as many rows per workgroup as their W images leave room in the LDS share one
 *   staged chunk of Z (8 at k <= 80 ... 2 at k = 160).
 * ------------------------------------------------------------------------- */
int als_row_whitener(int k, int ld, int64_t nrows, const int64_t* indptr, const int32_t* indices,
                     const int32_t* rows, int64_t n, const float* Z, float lambda_u, float* W_out,
                     int32_t* status, void* stream);
size_t als_explore_workspace_bytes(int k, int64_t nusers, int64_t n, int topn, int nslices);
int als_explore_topk(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                     const float* Z, const float* b_u, const float* b_i, const double* mu, const float* W,
                     float beta, const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow,
                     int topn, int nslices, float* top_val, int32_t* top_idx, int32_t* top_cnt,
                     float* top_lev, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Calibrated top-N (Steck, RecSys 2018): a list whose categories follow the proportions of a
 * target distribution.
 *
 * Category table C [n][ldc], fp32: ncat (1 .. 64) real columns, ldc = ncat rounded up to a multiple of 16, padding
 *   columns zero.  Row i is p(c | i): non-negative, summing to 1, or all zero (an item without a category);
 *   has_i = 1 when any entry of row i is > 0.
 * Target P [nrows][ldc], fp32, same shape rules: row b is p(c | b), or all zero when nothing is known of the row.
 *   P entries and alpha * P entries are expected to be zero or normal fp32 numbers (the hardware log2 does not take
 *   subnormals).
 *
 * als_category_profile: P_out[b] = (sum_{i in H_b} C_i) / #{i in H_b : has_i}, H_b the CSR row rows[b] (rows == NULL:
 *   row b) of indptr (int64) / indices (int32): the sum in fp64 in CSR order, rounded once to fp32; all zero when
 *   the count is 0.  An index outside [0, n) is skipped.  rows may name a row more than once.
 *
 * als_calibrated_rerank: per row a pool cand_idx / cand_val [nrows][pool] in als_recommend_topk's output form (as
 *   als_mmr_rerank: a list ends at the first -1 or at the first id outside [0, n), never dereferenced, or at its full
 *   width; rel_j is als_mmr_rerank's min-max relevance).  State: S_c = fp32 sum of the chosen items' rows in pick
 *   order, cnt = chosen items with has = 1.  For an open candidate j, in fp32:
 *     cnt_j = cnt + has_j,  q_c = (S_c + C_jc) / cnt_j (0 when cnt_j = 0),  q~_c = (1 - alpha) q_c + alpha p_c,
 *     KL_j = ln 2 * sum_{c : p_c > 0} p_c (log2 p_c - log2 q~_c)   (c ascending, v_log_f32),
 *     obj_j = (1 - lambda) rel_j - lambda KL_j;
 *   step t = 0 .. topn-1 picks the open candidate with the largest objective, ties to the lower pool position.
 *   top_idx / top_val [nrows][topn]: the picks in pick order with their cand_val (copied), unused slots -1 / -inf;
 *   top_cnt [nrows] = min(topn, entries of the pool); top_kl [nrows] (nullable): the KL of the final state (q from S
 *   and cnt alone).  lambda = 0, or an all-zero target row at any lambda, returns the first topn pool entries of a
 *   pool ordered by score; items without a category leave q unchanged.
 * als_list_miscalibration: kl [nrows] = the KL of the state reached by adding the items of the list idx [nrows][len]
 *   in list order; on a list als_calibrated_rerank returned it is bitwise that call's top_kl.
 *
 * ncat outside 1 .. 64 or ldc != 16 ceil(ncat / 16): ALS_E_BADK.  1 <= pool, len <= ALS_TOPK_MAX, 1 <= topn <= pool,
 * 0 <= lambda <= 1, 0 < alpha < 1, n < 2^31 (ALS_E_BADARG otherwise, as for a NULL required pointer); asynchronous
 * on the stream, no workspace; nrows == 0 is a no-op.
 * ------------------------------------------------------------------------- */
int als_category_profile(int ncat, int ldc, int64_t nrows, const int32_t* rows, const int64_t* indptr,
                         const int32_t* indices, int64_t n, const float* C, float* P_out, void* stream);
int als_calibrated_rerank(int ncat, int ldc, int64_t nrows, int64_t n, const float* C, const float* P, int pool,
                          const float* cand_val, const int32_t* cand_idx, float lambda, float alpha, int topn,
                          float* top_val, int32_t* top_idx, int32_t* top_cnt, float* top_kl, void* stream);
int als_list_miscalibration(int ncat, int ldc, int64_t nrows, int64_t n, const float* C, const float* P, int len,
                            const int32_t* idx, float alpha, float* kl, void* stream);

/* ---------------------------------------------------------------------------
 * Implicit feedback: the confidence-weighted fit of Hu, Koren and Volinsky (ICDM 2008), the model behind
 * ImplicitALS.  A half-step solves, for every row with entries t (rows f_t of the other side's table F):
 *     A = G + sum_t a_t f_t f_t^T + (lambda(row) + 1e-10) I,   b = sum_t t_t f_t,   x = A^-1 b,
 * where G = a0 F^T F over ALL rows of F stands for the unobserved entries and is the same for every row.
 *
 * als_table_gram_f64: G_out = F^T F over the nrows rows of the fp32 table F [nrows][ld] (16-byte aligned), accumulated
 *   in fp64 on the fp64 matrix cores.  A fixed grid of als_table_gram_partials() workgroups, each summing a contiguous
 *   row range into its partial, and a second launch that adds the partials in index order: the result is bitwise
 *   reproducible and a function of (F, nrows, k) alone.  Columns k .. ld-1 of F contribute zero whatever they hold;
 *   nrows == 0 gives G = 0.
 *   G_out: the LOWER-BLOCK PERM-SPACE IMAGE the fp64 row kernels factorise - (ld/16)(ld/16 + 1)/2 blocks of 16 x 16
 *   doubles, block (I, K), K <= I, at offset 256 (I (I + 1) / 2 + K), row-major inside a block, element (r, c) of it
 *   being G[col(16 I + r)][col(16 K + c)] with col(p) the factor column at perm position p (als_perm_index) - chosen
 *   over natural order because als_implicit_row_solve then adds G to a row's image with one linear pass.  Diagonal
 *   blocks are full and symmetric; positions of padding columns are exactly zero.
 *   partials: scratch of als_table_gram_partials() images (256 (ld/16)(ld/16 + 1)/2 doubles each).
 *
 * als_implicit_row_solve: the per-row solve above, one wave per task, fp64 throughout on the fp32-stored F; only x
 *   is rounded to fp32.  tasks / long_rows / workspace as als_row_solve takes them (als_host_row_tasks; slots are
 *   als_partial_slot_bytes_f64(k) bytes, summed in slot order; no wave takes more than ALS_SPLIT_CHUNK entries).
 *   A row's result depends on its own entries, F and G alone.  Rows with entries that no task names are left
 *   untouched; rows WITHOUT entries (of all nrows) get x = 0, x.b = 0.  nrows == 0 is a no-op.
 * ------------------------------------------------------------------------- */
typedef struct als_implicit_params {
    int32_t k, ld;                  /* ld = als_padded_k(k) */
    int64_t nrows;                  /* rows of this orientation, < 2^31 - 1 */
    int64_t ncols;                  /* rows of F, >= 1; ncols * ld < 2^31 */
    int32_t F_zero_row;             /* the row of F that lanes past the end of a row gather: any row in [0, ncols), or
                                       -1 = F has no spare row (row 0 is read).  Those lanes carry a = t = 0, which
                                       removes them exactly, so the row need not be zero - only finite */
    int32_t reserved;
    const int64_t* indptr;          /* [nrows + 1] */
    const int32_t* indices;         /* [nnz], in [0, ncols) */
    const float*   gram_w;          /* [nnz] a_t; >= 0 by contract (A is then positive definite for lambda >= 0) */
    const float*   rhs_w;           /* nullable [nnz] t_t; NULL: t_t = 1 + a_t (preference 1 with confidence 1 + a) */
    const float*   F;               /* [ncols][ld], padding columns zero, 16-byte aligned */
    const double*  G;               /* als_table_gram_f64 image of F (or any symmetric image in that layout) */
    double         G_scale;         /* a0, the weight of the unobserved entries: A = G_scale G + ... (see g_scale_row) */
    float          lambda_scalar;   /* >= 0 */
    const float*   lambda_row;      /* nullable [nrows] */
    float*         X_out;           /* [nrows][ld], padding columns written as zero */
    double*        xb_out;          /* nullable [nrows]: x.b with the unrounded x (the closed-form loss) */
    int32_t*       status;          /* as als_row_solve: 0 on entry; a non-positive (or NaN) pivot stores row + 1 by
                                       atomicMax */
    const als_task*     tasks;      int64_t ntasks;
    const als_long_row* long_rows;  int64_t nlong;
    void*          workspace;       /* 16-byte aligned; may be NULL when nlong == 0 */
    const float*   g_scale_row;     /* nullable [nrows], >= 0 by contract: A = (G_scale g_scale_row[row]) G + ..., the
                                       product formed in fp64.  NULL: G_scale for every row (the same bits as a
                                       g_scale_row of ones).  Appended last: every earlier offset stands */
} als_implicit_params;

int als_table_gram_partials(void);
int als_table_gram_f64(int k, int ld, int64_t nrows, const float* F, double* partials, double* G_out, void* stream);
/* G_out = sum_r w[r] f_r f_r^T = F^T diag(w) F: als_table_gram_f64 (same grid, partials, fold order, output image and
 * argument checks) with the row weights w [nrows] (device, fp32, >= 0 by contract; nothing past nrows is read).  The
 * A operand of every matrix-core step is (double)f * (double)w[r] - exact in fp64 - and the B operand is unscaled, so
 * with every w[r] = 1.0f, or w = NULL, the result is bitwise als_table_gram_f64's; it is a function of
 * (F, w, nrows, k) alone.  For general w a diagonal block is symmetric to rounding, not bitwise; the row kernels read
 * its lower triangle. */
int als_table_gram_weighted_f64(int k, int ld, int64_t nrows, const float* F, const float* w, double* partials,
                                double* G_out, void* stream);
int als_implicit_row_solve(const als_implicit_params* p, void* stream);

/* ---------------------------------------------------------------------------
 * Item-feature normalisation (scripts/prepare_features.py:95-124, 131-201) of a float64 [n][d] matrix X (device):
 * method 0 none (cast), 1 row_l1, 2 row_l2, 3 col_zscore, 4 col_minmax; out: float32 [n][d].  Sums run in numpy's
 * order, so out is bitwise the reference's result.  colwork: 2*d doubles (methods 3, 4).  status (device int32,
 * zeroed by the caller): bit 0 set when X holds a NaN / inf (the reference raises ValueError; impute first).
 * ------------------------------------------------------------------------- */
int als_normalize_features(int64_t n, int d, const double* X, int method, double eps, float* out,
                           double* colwork, int32_t* status, void* stream);
/* Median imputation in place (scripts/prepare_features.py:82-92): every NaN / +-inf of X [n][d] (device, float64)
 * becomes the median of its column's finite entries (mean of the two middle ones for an even count, 0 for a column
 * without finite entries).  Exact order statistics by radix select; work: 3*d doubles. */
int als_impute_col_median(int64_t n, int d, double* X, double* work, void* stream);

/* ---------------------------------------------------------------------------
 * Host-side set-up passes (HOST pointers, synchronous, no GPU involved).  They replace the reference's
 * per-fit index-list construction (scripts/als.py:332-340) and prepare the inputs of the entry points above;
 * the named caller times fit + predict together (scripts/evaluate_models.py:245-255), so this is inside its
 * measured region.
 * ------------------------------------------------------------------------- */
/* COO ratings -> CSR by user (uptr [m+1], uidx / uval [N]) and CSC by item (iptr [n+1], iidx / ival [N]),
 * indices ascending inside every row / column.  Returns -10 for an index outside the m x n shape, -11 for a
 * duplicate (user, item) pair. */
int als_host_coo_to_sides(int64_t m, int64_t n, int64_t N, const int64_t* rows, const int64_t* cols,
                          const float* vals, int64_t* uptr, int32_t* uidx, float* uval,
                          int64_t* iptr, int32_t* iidx, float* ival);

/* Task list of als_row_solve for rows [row_begin, row_end) with at least one rating: rows longer than `chunk`
 * (= ALS_SPLIT_CHUNK) are split, tasks are ordered longest first, whole rows of at most `mid_len` / `dual_len`
 * ratings go last (ndual_mid / ndual_tail of als_row_solve_params).  counts[6] = {ntasks, nlong, nslots,
 * ratings covered, ndual, nmid}; call once with tasks == NULL to size the arrays. */
int als_host_row_tasks(const int64_t* indptr, int64_t row_begin, int64_t row_end, int32_t chunk,
                       int32_t dual_len, int32_t mid_len, als_task* tasks, als_long_row* long_rows,
                       int64_t* counts);

/* Dependency levels of the index-ordered Gauss-Seidel sweep over the active items of [begin, end):
 * level[n] (-1 = not swept), items in (level, id) order, offsets[nlevels + 1] (n + 1 entries provided),
 * wait (nullable, [nnz(S)]) = the S_idx_wait input of als_gs_sweep_dataflow.  out[2] = {nitems, nlevels}. */
int als_host_level_schedule(int64_t n, const int64_t* S_ptr, const int32_t* S_idx, const uint8_t* active,
                            int64_t begin, int64_t end, int64_t* level, int32_t* items,
                            int64_t* offsets, int32_t* wait, int64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ALS_HIP_H */
