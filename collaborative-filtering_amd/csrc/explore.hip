// K16: uncertainty-aware top-N - ALS.recommend_explore: every item i of the catalogue is ranked for batch row b by
//     key(i) = base(i) + beta * sqrt(leverage(i)),   leverage(i) = |W z_i|^2,   W = float32(L^-1),  L L^T = A,
// A = Z_S^T Z_S + (lambda_u + 1e-10) I the row's ridge system (als_fold_in's / als_explain's A), base(i) bitwise the
// fp32 score als_predict_dense writes - LinUCB on the user's own ridge posterior (beta > 0), or its cautious mirror
// (beta < 0) - without forming a row of the m x n completion or the k x n matrix W Z^T.
//
// k_row_whitener: one wave per work row, whatever its length.  The Gram passes are row_f64_common.hpp's
// (gram_passes_nat_f64: the image in NATURAL column order - block b, position c is column 16 b + c - so that the
// factor is the lower Cholesky factor of A as written, not of a column permutation of it), the regulariser and
// cholesky_f64 as in k_fold_in.  Then L X = I by forward substitution IN PLACE, one column per lane: step p forms row
// p of X - lane j (+ 64 rr) its entry X[p][j] = (e_j[p] - sum_{j <= t < p} L[p][t] X[t][j]) / L[p][p], L[p][t] an LDS
// broadcast, X[t][j] the lane's own column, which already overwrote L[t][j] (row t < p of L is dead after step t).
// fp64 throughout; W_out is the fp32 rounding, the upper triangle and the padding rows / columns written 0.
//
// k_explore: ONE WAVE serves one batch row, a workgroup of NW waves serves NW consecutive rows over the items [lo, hi)
// of one slice - k_group's organisation (group.hip): catalogue_walk.hpp's walk in chunks of 32 items, the chunk's Z
// rows staged in LDS once per workgroup under the next chunk's global loads.  Each wave keeps the lower 16 x 16 blocks
// of its W in LDS in OPERAND ORDER (block (I, K): float 4 lane + s = W[16 I + c][16 K + 4 q + s], one conflict-free
// ds_read_b128 per lane and block), which decides NW: as many waves as 160 KiB hold (ex_nw).  Per chunk:
//   base:     one v_mfma_f32_16x16x4_f32 chain per 16-item tile with the user's row as row 0 of the 16-row operand
//             (the other rows 0), k_predict_dense's lane mapping, order over k and epilogue (walk::score) - bitwise
//             als_predict_dense's value; the rows 1 ... 15 of the result are never read.
//   leverage: Y = W Z_tile^T over the lower blocks only (tiles_lev): per block row I one accumulator per tile, the
//             chain over K <= I and the 4 steps of a block, the W operand read once for the chunk's two tiles; the
//             squares of the four rows a lane holds are added in-lane (fmaf, I ascending), and the four q groups are
//             folded by two xor shuffles (16, 32) - every lane of column c then holds |W z_c|^2.
//   key:      three correctly rounded fp32 operations, no contraction (explore_key).
// A leverage depends on (W, z_i) alone: an MFMA column does not see its neighbours, the additions have one order.
// Selection (one candidate per item and one list per wave), seen cursor, slices and their merge (topk::k_merge_slices)
// are k_group's, character for character; Z fetch / stage, the allow-bitmap scan and the base-score tiles are the
// walk_*.inc fragments of k_recommend's walk.
//
// k_explore_lev: top_lev.  After the lists are final (merged), one wave per batch row recomputes the leverages of
// the returned items with the same tiles_lev - so sqrt / multiply / add of top_lev in fp32 gives top_val back
// bitwise - and writes 0 into the unused slots.
#include "als_device.hpp"
#include "als_hip.h"
#include "catalogue_walk.hpp"
#include "row_f64_common.hpp"
#include "topk_common.hpp"
#include "topk_launch.hpp"
#include "topk_rows.hpp"

namespace {

using namespace f64row;
using topk::key_index;
using topk::key_score;
using topk::make_key;

constexpr int EX_CHUNK = walk::CHUNK;
constexpr int EX_LDS = 156 * 1024;      // of the CU's 160 KiB

constexpr int ex_nblk(int KB) { return KB * (KB + 1) / 2; }
// rows (waves) per workgroup: what the W images (1 KiB per lower block) and the key arrays leave of the LDS
constexpr int ex_nw(int KB) {
    const int per_wave = ex_nblk(KB) * 1024 + 256 * 8;
    const int nw = (EX_LDS - EX_CHUNK * walk::lds_row_stride(KB) * 4) / per_wave;
    return nw > 8 ? 8 : nw;
}
static_assert(ex_nw(10) >= 2 && ex_nw(4) == 8, "k = 160 shares a chunk between two rows at least");

// ---------------------------------------------------------------------------------------------------------------
// the whitener
// ---------------------------------------------------------------------------------------------------------------
template <int KB>
__global__ __launch_bounds__(64)
void k_row_whitener(int k, int ld, const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                    const int32_t* __restrict__ rows, const float* __restrict__ Z, float lambda_u,
                    float* __restrict__ W_out, int32_t* __restrict__ status) {
    using C = F64Cfg<KB>;
    constexpr int KP = C::KP, NR = C::NR;
    __shared__ __attribute__((aligned(16))) double img[C::IMG];
    const int lane = threadIdx.x;
    const int c = lane & 15, q = lane >> 4;
    const int64_t wr = blockIdx.x;
    const int64_t row = rows ? (int64_t)rows[wr] : wr;
    const int64_t beg = indptr[row];
    const int len = (int)(indptr[row + 1] - beg);

    gram_passes_nat_f64<KB, 0>(Z, ld, indices, beg, len, img, lane);
    wave_lds_sync();
    // regulariser on the diagonal, 1 on the padded columns (as k_fold_in; natural order: column 16 J + c)
    const double lam = (double)lambda_u + 1e-10;
    if (q == 0) {
        for (int J = 0; J < KB; ++J) img[blk64(J, J) * 256 + c * 16 + c] += (16 * J + c < k) ? lam : 1.0;
    }
    wave_lds_sync();

    double b[1][NR], y[1][NR], dinv[NR];
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) { b[0][rr] = 0.0; y[0][rr] = 0.0; dinv[rr] = 0.0; }
    bool bad = false;
    cholesky_f64<KB, 1>(img, b, y, dinv, bad, lane);
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicMax(status, (int)(wr + 1));

    // L X = I in place, one column per lane
    int jc[NR];
#pragma unroll
    for (int rr = 0; rr < NR; ++rr) jc[rr] = min(lane + 64 * rr, KP - 1);
#pragma unroll 1
    for (int p = 0; p < KP; ++p) {
        double dsel = dinv[0];
#pragma unroll
        for (int rr = 1; rr < NR; ++rr) dsel = ((p >> 6) == rr) ? dinv[rr] : dsel;
        const double dp = readlane_d(dsel, p & 63);                         // 1 / L[p][p]
        const double* lrow = img + (p & 15) * 16;                            // L[p][t] = lrow[blk64(p >> 4, t >> 4) * 256 + (t & 15)]
        const int pb = blk64(p >> 4, 0) * 256;
        double x[NR];
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int j = lane + 64 * rr;
            double acc = (j == p) ? 1.0 : 0.0;
            if (64 * rr <= p) {                                              // wave-uniform: some column of the group is <= p
                const int jj = jc[rr];
#pragma unroll 4
                for (int t = 64 * rr; t < p; ++t) {
                    const double lpt = lrow[pb + (t >> 4) * 256 + (t & 15)];
                    const int tt = max(t, jj);                               // t < j: a valid address, the value masked
                    const double xtj = img[blk64(tt >> 4, jj >> 4) * 256 + (tt & 15) * 16 + (jj & 15)];
                    acc = fma(-lpt, (t >= j) ? xtj : 0.0, acc);
                }
            }
            x[rr] = acc * dp;
        }
        wave_lds_sync();                                                     // row p of L has been read by every lane
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int j = lane + 64 * rr;
            if (j <= p) img[blk64(p >> 4, j >> 4) * 256 + (p & 15) * 16 + (j & 15)] = x[rr];
        }
        wave_lds_sync();
    }

    float* dst = W_out + (size_t)wr * KP * KP;
    for (int i = 0; i < KP; ++i) {
#pragma unroll
        for (int rr = 0; rr < NR; ++rr) {
            const int j = lane + 64 * rr;
            if (j < KP) {
                const bool nz = j <= i && i < k;
                const int jj = min(j, i);
                const double v = img[blk64(i >> 4, jj >> 4) * 256 + (i & 15) * 16 + (jj & 15)];
                dst[(size_t)i * KP + j] = nz ? (float)v : 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// leverages of two 16-item tiles: wl the wave's W image in operand order, z0 / z1 the items' rows in the leverage
// layout (lane (c, q), entry 4 K + s = z[item c][16 K + 4 q + s]).  Every lane of column c gets |W z_c|^2.
// ---------------------------------------------------------------------------------------------------------------
template <int KB>
__device__ __forceinline__ void tiles_lev(const float* wl, const float (&z0)[4 * KB], const float (&z1)[4 * KB],
                                          int lane, float& lev0, float& lev1) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int I = 0; I < KB; ++I) {
        f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int K = 0; K <= I; ++K) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(wl + (I * (I + 1) / 2 + K) * 256 + 4 * lane);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], z0[4 * K + s], a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[s], z1[4 * K + s], a1, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s0 = fmaf(a0[r], a0[r], s0);
            s1 = fmaf(a1[r], a1[r], s1);
        }
    }
    s0 += __shfl_xor(s0, 16, 64);
    s1 += __shfl_xor(s1, 16, 64);
    lev0 = s0 + __shfl_xor(s0, 32, 64);
    lev1 = s1 + __shfl_xor(s1, 32, 64);
}

// the wave's W image: the lower blocks of W [LD][LD] (row-major, global) to LDS in operand order
template <int KB>
__device__ __forceinline__ void load_w_image(const float* __restrict__ W, float* wl, int lane) {
    constexpr int LD = 16 * KB;
    const int c = lane & 15, q = lane >> 4;
#pragma unroll 1
    for (int I = 0; I < KB; ++I)
        for (int K = 0; K <= I; ++K)
            *reinterpret_cast<f32x4*>(wl + (I * (I + 1) / 2 + K) * 256 + 4 * lane) =
                *reinterpret_cast<const f32x4*>(W + (size_t)(16 * I + c) * LD + 16 * K + 4 * q);
}

// base + beta * sqrt(lev): a correctly rounded square root, product and sum, never contracted
__device__ __forceinline__ float explore_key(float base, float beta, float lev) {
#pragma clang fp contract(off)
    const float sig = __builtin_sqrtf(lev);
    const float t = beta * sig;
    return base + t;
}

// CAP keys per row: list [0, L) + survivor buffer [L, CAP)
template <int KB, int CAP, bool MASKED>
__global__ __launch_bounds__(ex_nw(KB) * 64)
void k_explore(int ld, int64_t nusers, const int32_t* __restrict__ users, int64_t n, int64_t slice,
               const float* __restrict__ U, const float* __restrict__ Z, const float* __restrict__ b_u,
               const float* __restrict__ b_i, const double* __restrict__ mu_p, const float* __restrict__ W,
               float beta, const int64_t* __restrict__ seen_ptr, const int32_t* __restrict__ seen_idx,
               const uint32_t* __restrict__ allow, int topn, float* __restrict__ top_val,
               int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt, unsigned long long* __restrict__ part) {
    constexpr int NW = ex_nw(KB), E = 4 * KB, LD = 16 * KB, ZS = walk::lds_row_stride(KB), NBLK = ex_nblk(KB);
    constexpr int L = CAP == 256 ? 128 : 32, BUF = CAP - L;
    constexpr int NT = NW * 64, NV = EX_CHUNK * LD / 4, PF = (NV + NT - 1) / NT;
    static_assert(L >= 32 && BUF >= 64, "a chunk appends up to 32 keys");
    __shared__ unsigned long long keys[NW][CAP];
    __shared__ __attribute__((aligned(16))) float zs[EX_CHUNK][ZS];
    __shared__ __attribute__((aligned(16))) float wimg[NW][NBLK * 256];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const float mu = (float)(*mu_p);
    const int64_t b = (int64_t)blockIdx.x * NW + wave;                    // batch row of this wave
    const int64_t lo = (int64_t)blockIdx.y * slice, hi = min(n, lo + slice);
    unsigned long long* kw = keys[wave];
    const float* wl = wimg[wave];
    const bool active = b < nusers;                                       // wave-uniform

    // the user's row as row 0 of the 16-row operand (k_predict_dense's layout: lane (0, q) holds k = 4 KB q + e)
    int u = 0;
    float ua[E], bu = 0.f;
#pragma unroll
    for (int e = 0; e < E; ++e) ua[e] = 0.f;
    if (active) {
        u = users[b];
        bu = b_u[u];
        float t[E];
        load_frow<E>(U + (size_t)u * ld + E * q, t);
#pragma unroll
        for (int e = 0; e < E; ++e) ua[e] = c == 0 ? t[e] : 0.f;
        load_w_image<KB>(W + (size_t)b * LD * LD, wimg[wave], lane);
    }
    wave_lds_sync();

    // the user's seen row: cursor, end, next seen item (wave-uniform)
    int64_t cur = 0, end = 0;
    if (seen_ptr && active) {
        end = seen_ptr[u + 1];
        cur = walk::lower_bound(seen_idx, seen_ptr[u], end, lo);                // first seen item >= lo
    }
    int nxt = cur < end ? seen_idx[cur] : INT32_MAX;

    unsigned long long thr = 0ull;      // key of the current topn-th entry (0: list not full)
    int cnt = 0;                        // buffered survivors
    int nlist = 0;                      // valid entries of the sorted list

    auto compact = [&]() {              // list + buffer -> sorted list, new threshold
        wave_lds_sync();
        unsigned long long k[CAP / 64];
#pragma unroll
        for (int v = 0; v < CAP / 64; ++v) {
            const int i = lane + 64 * v;
            const bool live = (i < nlist) || (i >= L && i < L + cnt);
            k[v] = live ? kw[i] : 0ull;
        }
        topk::sort_desc<CAP / 64>(k, lane);
#pragma unroll
        for (int v = 0; v < CAP / 64; ++v)
            if (lane + 64 * v < L) kw[lane + 64 * v] = k[v];
        wave_lds_sync();
        const int nn = min(topn, nlist + cnt);
        thr = (nn == topn) ? kw[topn - 1] : 0ull;
        cnt = 0;
        nlist = nn;
    };

    // bit l set: item it0 + l of the chunk [it0, it0 + 32) is in the user's seen row
    auto seen_mask = [&](int64_t it0) -> unsigned {
        unsigned msk = 0u;
        if (nxt < it0 + EX_CHUNK) {                                      // wave-uniform
            bool more = true;
            while (more) {
                const int64_t p = cur + lane;
                const int s = p < end ? seen_idx[p] : INT32_MAX;
                const bool below = s < it0 + EX_CHUNK;
                unsigned bit = (below && s >= it0) ? 1u << (int)(s - it0) : 0u;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) bit |= __shfl_xor(bit, o, 64);
                msk |= bit;
                const int adv = __popcll(__ballot(below));
                cur += adv;
                more = adv == 64;                                        // 64 consumed: there may be more in the chunk
                if constexpr (MASKED) {
                    // all 64 below the chunk: the cursor fell behind over skipped chunks - jump, do not walk
                    const int last = __builtin_amdgcn_readlane(s, 63);
                    if (more && last < it0) cur = walk::lower_bound(seen_idx, cur, end, it0);
                }
            }
            nxt = cur < end ? seen_idx[cur] : INT32_MAX;
        }
        return msk;
    };

    f32x4 pf[PF];
    auto fetch = [&](int64_t it0) {
#include "walk_z_fetch.inc"
    };
    auto stage = [&]() {
#include "walk_z_stage.inc"
    };

#include "walk_allow_scan.inc"
    int64_t nx = 0;                                      // MASKED: the chunk after ch that is scored
    if constexpr (MASKED) {
        nx = next_chunk(0);
        if (nx < nch) { fetch(lo + nx * EX_CHUNK); window(nx + 1); }
    } else if (nch > 0) fetch(lo);
    for (int64_t ch = nx; ch < nch; ch = MASKED ? nx : ch + 1) {
        const int64_t it0 = lo + ch * EX_CHUNK;
        unsigned word = ~0u;
        if constexpr (MASKED) word = __builtin_amdgcn_readfirstlane(aw[ch]);
        __syncthreads();                                 // every wave is done with the previous chunk
        stage();
        __syncthreads();
        if constexpr (MASKED) {
            nx = after(ch);
            if (nx < nch) { fetch(lo + nx * EX_CHUNK); window(nx + 1); }      // however far ahead
        } else if (ch + 1 < nch) fetch(it0 + EX_CHUNK);
        if (!active) continue;                           // wave-uniform: no row

        // base scores: lane (c, 0) gets item it0 + c (tile 0) and it0 + 16 + c (tile 1)
        float sc0, sc1;
        {
#include "walk_score_tiles.inc"
            const float bi0 = b_i[min(it0 + c, n - 1)], bi1 = b_i[min(it0 + 16 + c, n - 1)];
            sc0 = walk::score(acc0[0], mu, bu, bi0);
            sc1 = walk::score(acc1[0], mu, bu, bi1);
        }
        // leverages: every lane of column c
        float lev0, lev1;
        {
            float y0[E], y1[E];
#pragma unroll
            for (int K = 0; K < KB; ++K) {
                const f32x4 v0 = *reinterpret_cast<const f32x4*>(&zs[c][16 * K + 4 * q]);
                const f32x4 v1 = *reinterpret_cast<const f32x4*>(&zs[16 + c][16 * K + 4 * q]);
#pragma unroll
                for (int s = 0; s < 4; ++s) { y0[4 * K + s] = v0[s]; y1[4 * K + s] = v1[s]; }
            }
            tiles_lev<KB>(wl, y0, y1, lane, lev0, lev1);
        }
        unsigned drop = seen_mask(it0);
        if constexpr (MASKED) drop |= ~word;

        // one candidate per item: lane l < 32 owns item it0 + l (its base from lane l & 15)
        const float sc1q = __shfl(sc1, c, 64);
        const float base = q == 0 ? sc0 : sc1q;
        const float kf = explore_key(base, beta, q == 0 ? lev0 : lev1);
        const int64_t col = it0 + lane;
        const unsigned long long key = make_key(kf, (unsigned)col);
        const bool pass = lane < EX_CHUNK && col < hi && !((drop >> (lane & 31)) & 1u) && base == base && kf == kf &&
                          key > thr;
        const unsigned long long pm = __ballot(pass);
        if (pass) kw[L + cnt + __popcll(pm & ((1ull << lane) - 1ull))] = key;
        cnt += __popcll(pm);
        if (cnt > BUF - EX_CHUNK) compact();             // the buffer could overflow in the next chunk
    }
    if (cnt > 0) compact();
    wave_lds_sync();
    if (!active) return;
    if (part) {                                          // sliced: raw keys of (slice, row), 0 = empty
        unsigned long long* dst = part + ((int64_t)blockIdx.y * nusers + b) * topn;
        for (int t = lane; t < topn; t += 64) dst[t] = t < nlist ? kw[t] : 0ull;
    } else {
        for (int t = lane; t < topn; t += 64) {
            const bool ok = t < nlist;
            const unsigned long long key = ok ? kw[t] : 0ull;
            top_val[b * topn + t] = ok ? key_score(key) : -INFINITY;
            top_idx[b * topn + t] = ok ? key_index(key) : -1;
        }
        if (lane == 0) top_cnt[b] = nlist;
    }
}

// top_lev of the final lists: one wave per batch row, 32 returned items per step
template <int KB>
__global__ __launch_bounds__(64)
void k_explore_lev(int64_t n, const float* __restrict__ Z, const float* __restrict__ W, int topn,
                   const int32_t* __restrict__ top_idx, float* __restrict__ top_lev) {
    constexpr int E = 4 * KB, LD = 16 * KB, NBLK = ex_nblk(KB);
    __shared__ __attribute__((aligned(16))) float wimg[NBLK * 256];
    const int lane = threadIdx.x, c = lane & 15, q = lane >> 4;
    const int64_t b = blockIdx.x;
    load_w_image<KB>(W + (size_t)b * LD * LD, wimg, lane);
    wave_lds_sync();
    for (int t0 = 0; t0 < topn; t0 += 32) {
        const int p0 = t0 + c, p1 = t0 + 16 + c;
        const int i0 = p0 < topn ? top_idx[b * topn + p0] : -1;
        const int i1 = p1 < topn ? top_idx[b * topn + p1] : -1;
        const float* r0 = Z + (size_t)min(max((int64_t)i0, (int64_t)0), n - 1) * LD + 4 * q;
        const float* r1 = Z + (size_t)min(max((int64_t)i1, (int64_t)0), n - 1) * LD + 4 * q;
        float y0[E], y1[E];
#pragma unroll
        for (int K = 0; K < KB; ++K) {
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(r0 + 16 * K);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(r1 + 16 * K);
#pragma unroll
            for (int s = 0; s < 4; ++s) { y0[4 * K + s] = v0[s]; y1[4 * K + s] = v1[s]; }
        }
        float lev0, lev1;
        tiles_lev<KB>(wimg, y0, y1, lane, lev0, lev1);
        if (q == 0) {
            if (p0 < topn) top_lev[b * topn + p0] = i0 >= 0 ? lev0 : 0.f;
            if (p1 < topn) top_lev[b * topn + p1] = i1 >= 0 ? lev1 : 0.f;
        }
    }
}

int ex_rows_per_wg(int kb) {            // one wave per batch row; kb = als_padded_k(k) / 16
    static constexpr int nw[11] = {0,        ex_nw(1), ex_nw(2), ex_nw(3), ex_nw(4), ex_nw(5),
                                   ex_nw(6), ex_nw(7), ex_nw(8), ex_nw(9), ex_nw(10)};
    return nw[kb];
}

template <int KB>
int launch_explore(int ld, int64_t nusers, const int32_t* users, int64_t n, int nsl, const float* U, const float* Z,
                   const float* b_u, const float* b_i, const double* mu, const float* W, float beta,
                   const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow, int topn, float* tv,
                   int32_t* ti, int32_t* tc, unsigned long long* part, hipStream_t st) {
    constexpr int NW = ex_nw(KB);
    const int64_t slice = walk::slice_items(n, nsl);
    const dim3 grid((unsigned)((nusers + NW - 1) / NW), (unsigned)nsl);
    auto kern = topn <= 32 ? (allow ? k_explore<KB, 128, true> : k_explore<KB, 128, false>)
                           : (allow ? k_explore<KB, 256, true> : k_explore<KB, 256, false>);
    hipLaunchKernelGGL(kern, grid, dim3(NW * 64), 0, st, ld, nusers, users, n, slice, U, Z, b_u, b_i, mu, W, beta,
                       seen_ptr, seen_idx, allow, topn, tv, ti, tc, part);
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}

}  // namespace

extern "C" int als_row_whitener(int k, int ld, int64_t nrows, const int64_t* indptr, const int32_t* indices,
                                const int32_t* rows, int64_t n, const float* Z, float lambda_u, float* W_out,
                                int32_t* status, void* stream) {
    const int kp = als_padded_k(k);
    if (kp < 0) return ALS_E_BADK;
    if (ld != kp || nrows < 0 || nrows >= INT32_MAX || n < 1 || n * (int64_t)kp >= ((int64_t)1 << 31) ||
        !(lambda_u >= 0.f))
        return ALS_E_BADARG;
    if (nrows == 0) return 0;
    if (!indptr || !indices || !Z || !W_out || !status) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)nrows);
    ALS_DISPATCH_KB(kp / 16, hipLaunchKernelGGL(k_row_whitener<KB>, grid, dim3(64), 0, st, k, ld, indptr, indices, rows,
                                                Z, lambda_u, W_out, status));
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}

extern "C" size_t als_explore_workspace_bytes(int k, int64_t nusers, int64_t n, int topn, int nslices) {
    const int kp = als_padded_k(k);
    return kp < 0 ? 0 : topk::workspace_bytes(nusers, ex_rows_per_wg(kp / 16), n, topn, nslices);
}

extern "C" int als_explore_topk(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                                const float* Z, const float* b_u, const float* b_i, const double* mu, const float* W,
                                float beta, const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow,
                                int topn, int nslices, float* top_val, int32_t* top_idx, int32_t* top_cnt,
                                float* top_lev, void* workspace, size_t workspace_bytes, void* stream) {
    const int bad = topk::check_shape(k, ld, nusers, n, topn, ALS_TOPK_MAX, nslices);
    if (bad) return bad;
    if (!(beta == beta) || beta - beta != 0.f) return ALS_E_BADARG;
    if (nusers == 0) return 0;
    if (!users || !U || !Z || !b_u || !b_i || !mu || !W || !top_val || !top_idx || !top_cnt || !top_lev ||
        (!seen_ptr != !seen_idx))
        return ALS_E_BADARG;
    const topk::SlicePlan p = topk::plan(nusers, ex_rows_per_wg(ld / 16), n, nslices, nusers * topn,
                                         sizeof(unsigned long long), workspace, workspace_bytes);
    if (!p.nsl) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    ALS_DISPATCH_KB(ld / 16, rc = launch_explore<KB>(ld, nusers, users, n, p.nsl, U, Z, b_u, b_i, mu, W, beta, seen_ptr,
                                                     seen_idx, allow, topn, top_val, top_idx, top_cnt, p.keys(), st));
    if (rc == 0) rc = topk::merge_slices(p.nsl, p.keys(), nusers, topn, top_val, top_idx, top_cnt, st);
    if (rc != 0) return rc;
    ALS_DISPATCH_KB(ld / 16, hipLaunchKernelGGL(k_explore_lev<KB>, dim3((unsigned)nusers), dim3(64), 0, st, n, Z, W,
                                                topn, top_idx, top_lev));
    return topk::launch_status();
}
