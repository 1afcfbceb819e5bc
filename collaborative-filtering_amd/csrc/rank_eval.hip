// K11: exact full-catalogue ranks - for a (user, target item) pair, the number of unseen items the model scores
// above the target: k_recommend's scoring with the selection replaced by counting.  Nothing m x n is formed and
// there is no list, so no length limit.
//
// k_rank_count: one workgroup serves NW * 16 batch rows (one 16-row tile per wave) over the items [lo, hi) of one
// slice, in passes of RK_TP targets per row (one pass when no row of the workgroup has more).
//   pass start  every wave scores its rows' targets with the SAME v_mfma_f32_16x16x4_f32 chain and epilogue as the
//               catalogue (lane (c, q) gathers the Z row of row c's t-th target; the diagonal of the 16 x 16 tile is
//               score(row c, target of row c)) and keeps them as 64-bit keys (topk_common.hpp) in LDS.  A target
//               therefore ties with itself bitwise, and a key compare is exactly k_recommend's total order
//               (score descending, item ascending).
//   walk        k_recommend's: chunks of 32 items staged in LDS once per workgroup (the next chunk's global loads in
//               flight), two 16 x 16 score tiles per wave, the same exclusion walk over the ascending seen row.
//               A score that is seen, NaN or out of range becomes key 0, below every target key.  Each lane keeps
//               a private counter per (row of its q group, target): counter += (key > target key) for its 8 scores
//               of the chunk; the target key is read from LDS once per chunk (a broadcast read), groups of 8 targets
//               are skipped when no row of the wave has that many.
//   pass end    the 16 lanes of a q group add their counters; lane c stores target c of the pass.
//
// Item split as k_recommend (grid.y): a sliced call writes its counts to workspace [slice][nt + nq] and
// k_rank_reduce adds them - integers, so the result cannot depend on the slice count.
//
// Allow bitmap (als_rank_count_masked; the MASKED instantiations) as k_recommend's: one wave-uniform word per chunk,
// ANDed into the candidate test - so into `above` and `n_cand` alike -, chunks whose word is 0 skipped by the whole
// workgroup, the prefetch aimed at the next chunk with a set bit.  Target scores are formed whether or not the
// target is allowed.  The unmasked instantiations contain none of this.
//
// Eligibility table (als_rank_count_segmented; the SEG instantiations) as k_recommend's: one word per row 4q + r and
// chunk, prefetched behind the Z loads, ANDed into the candidate test; a wave none of whose rows has a set bit in the
// chunk counts nothing but still stages and passes both barriers.  Not combined with MASKED.
//
// "k_recommend's" above means the same text, not a copy of it: Z fetch / stage, the bitmap scan, the
// cursor set-up (with `u` naming su[r]), the exclusion walk and the score tiles are the walk_*.inc fragments that
// recommend.hip includes too, next to the chunk and slice arithmetic and the score epilogue of catalogue_walk.hpp, which
// says why the fragments are included text and not functions.  The candidate test and the chunk loop are this kernel's.
#include "als_device.hpp"
#include "als_hip.h"
#include "catalogue_walk.hpp"
#include "topk_common.hpp"
#include "topk_launch.hpp"

namespace {

using topk::make_key;

constexpr int RK_TP = 16;           // targets per row and pass (4 * RK_TP counters per lane)
constexpr int RK_TG = 8;            // targets per skip group
constexpr unsigned long long RK_NONE = ~0ull;   // target key of a NaN score / an unused slot: nothing is above it

template <int KB, int NW, bool MASKED, bool SEG = false>
__global__ __launch_bounds__(NW * 64)
void k_rank_count(int ld, int64_t nq, const int32_t* __restrict__ users, const int64_t* __restrict__ q_ptr,
                  const int32_t* __restrict__ q_items, int64_t n, int64_t slice, const float* __restrict__ U,
                  const float* __restrict__ Z, const float* __restrict__ b_u, const float* __restrict__ b_i,
                  const double* __restrict__ mu_p, const int64_t* __restrict__ seen_ptr,
                  const int32_t* __restrict__ seen_idx, float* __restrict__ t_score, int32_t* __restrict__ above,
                  int32_t* __restrict__ n_cand, int64_t slice_stride, const uint32_t* __restrict__ allow, int64_t nseg,
                  int64_t seg_stride, const int32_t* __restrict__ row_seg) {
    static_assert(!SEG || !MASKED, "the eligibility table replaces the bitmap");
    constexpr int E = 4 * KB, LD = 16 * KB, ZS = walk::lds_row_stride(KB);
    constexpr int NT = NW * 64, NV = walk::CHUNK * LD / 4, PF = (NV + NT - 1) / NT;
    __shared__ unsigned long long tks[NW * 16][RK_TP];
    __shared__ __attribute__((aligned(16))) float zs[walk::CHUNK][ZS];
    __shared__ int wg_tmax;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 15, q = lane >> 4;
    const float mu = (float)(*mu_p);
    const int64_t b0 = ((int64_t)blockIdx.x * NW + wave) * 16;            // first batch row of this wave
    const int64_t lo = (int64_t)blockIdx.y * slice, hi = min(n, lo + slice);
    unsigned long long (*tw)[RK_TP] = tks + wave * 16;

    float ua[E];
    load_frow<E>(U + (size_t)users[min(b0 + c, nq - 1)] * ld + E * q, ua);
    float bu[4];
    bool valid[4];
    int su[4];                                                           // user ids of rows 4q + r
    int64_t so[4] = {0, 0, 0, 0};                                        // SEG: word of chunk 0 in the segment row of rows 4q + r
    bool sv[4] = {false, false, false, false};                           // SEG: the row is valid and its segment id in range
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t rb = b0 + 4 * q + r;
        valid[r] = rb < nq;
        su[r] = users[min(rb, nq - 1)];
        bu[r] = b_u[su[r]];
        if constexpr (SEG) {
            const int64_t sg = row_seg[min(rb, nq - 1)];
            sv[r] = valid[r] && sg >= 0 && sg < nseg;
            so[r] = (sv[r] ? sg : 0) * seg_stride + lo / walk::CHUNK;       // lo is a multiple of 32
        }
    }
    // target range of row c (the row whose targets this lane gathers) and the largest count of the wave's rows
    const int64_t ctp = q_ptr[min(b0 + c, nq - 1)];
    const int64_t ctn = b0 + c < nq ? max(q_ptr[min(b0 + c, nq - 1) + 1] - ctp, (int64_t)0) : 0;
    int64_t wtn = ctn;
#pragma unroll
    for (int s = 1; s < 16; s <<= 1) {
        const int lo32 = __shfl_xor((int)(unsigned)wtn, s, 64), hi32 = __shfl_xor((int)(wtn >> 32), s, 64);
        const int64_t o = ((int64_t)hi32 << 32) | (unsigned)lo32;
        wtn = max(wtn, o);
    }
    const int wpass = (int)min((wtn + RK_TP - 1) / RK_TP, (int64_t)INT32_MAX);   // passes this wave needs
    if (tid == 0) wg_tmax = 1;
    __syncthreads();
    if (lane == 0) atomicMax(&wg_tmax, wpass);
    __syncthreads();
    const int npass = wg_tmax;

    f32x4 pf[PF];
    auto fetch = [&](int64_t it0) {
#include "walk_z_fetch.inc"
    };
    auto stage = [&]() {
#include "walk_z_stage.inc"
    };

#include "walk_allow_scan.inc"
    // SEG: the words of chunk `ch` in the segment rows of this lane's rows 4q + r, 0 for a row that takes no part;
    // ch < nch keeps the word inside the table row (lo / 32 + ch < ceil(n / 32) <= seg_stride)
    unsigned sp[4] = {0u, 0u, 0u, 0u};
    auto seg_fetch = [&](int64_t ch) {
#pragma unroll
        for (int r = 0; r < 4; ++r) sp[r] = sv[r] ? allow[so[r] + ch] : 0u;
    };
    for (int pass = 0; pass < npass; ++pass) {
        const int64_t t0 = (int64_t)pass * RK_TP;                        // first target of this pass
        const int wt = (int)max(min(wtn - t0, (int64_t)RK_TP), (int64_t)0);      // targets of the wave's fullest row
        const bool active = wt > 0 || pass == 0;                         // pass 0 counts the candidates of every row

        // ---- target scores of this pass: tile t pairs row c with its target t0 + t; the diagonal is wanted
        for (int t = 0; t < wt; ++t) {
            const bool has = t0 + t < ctn;
            int item = has ? q_items[ctp + t0 + t] : 0;
            item = min(max(item, 0), (int)(n - 1));
            float zt[E];
            load_frow<E>(Z + (size_t)item * ld + E * q, zt);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < E; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ua[e], zt[e], acc, 0, 0, 0);
            float a = 0.f, bur = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) { a = ((c & 3) == r) ? acc[r] : a; bur = ((c & 3) == r) ? bu[r] : bur; }
            const float score = walk::score(a, mu, bur, b_i[item]);
            if ((c >> 2) == q) {                                         // lane (c, c / 4) holds row c, column c
                tw[c][t] = (has && score == score) ? make_key(score, (unsigned)item) : RK_NONE;
                if (has && blockIdx.y == 0) t_score[ctp + t0 + t] = score;
            }
        }
        if (active) {                                                    // unused slots of the groups that are walked
            const int wtg = (wt + RK_TG - 1) / RK_TG * RK_TG;
            for (int t = wt + q; t < wtg; t += 4) tw[c][t] = RK_NONE;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();

        int cnt[4][RK_TP];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int t = 0; t < RK_TP; ++t) cnt[r][t] = 0;
        int ncand[4] = {0, 0, 0, 0};
        int64_t cur[4], end[4];
        int nxt[4];                                                      // next seen item of rows 4q + r
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int u = su[r];                                         // the name the fragment reads
#include "walk_seen_cursor.inc"
        }

        unsigned deny = 0u; // MASKED: bit c set = item cb + c of the block `keys_of` is called for is not allowed
        unsigned dn[4] = {0u, 0u, 0u, 0u};                               // SEG: the same, one word per row 4q + r
        // one 16-item block [cb, cb + 16): keys of the lane's four scores, 0 where the score is no candidate
        auto keys_of = [&](const f32x4& acc, int64_t cb, unsigned long long (&key)[4]) {
#include "walk_seen_masks.inc"
            if constexpr (MASKED) {
#pragma unroll
                for (int r = 0; r < 4; ++r) msk[r] |= deny;
            }
            if constexpr (SEG) {
#pragma unroll
                for (int r = 0; r < 4; ++r) msk[r] |= dn[r];
            }
            const int64_t col = cb + c;
            const float bi = b_i[min(col, n - 1)];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float score = walk::score(acc[r], mu, bu[r], bi);
                const bool cand = col < hi && valid[r] && !((msk[r] >> c) & 1u) && score == score;
                key[r] = cand ? make_key(score, (unsigned)col) : 0ull;
                ncand[r] += cand ? 1 : 0;
            }
        };

        int64_t nx = 0;                                  // MASKED: the chunk after ch that is counted
        if constexpr (MASKED) {
            nx = next_chunk(0);
            if (nx < nch) { fetch(lo + nx * walk::CHUNK); window(nx + 1); }
        } else if (nch > 0) {
            fetch(lo);
            if constexpr (SEG) seg_fetch(0);
        }
        for (int64_t ch = nx; ch < nch; ch = MASKED ? nx : ch + 1) {
            const int64_t it0 = lo + ch * walk::CHUNK;
            unsigned word = 0u;
            if constexpr (MASKED) word = __builtin_amdgcn_readfirstlane(aw[ch]);
            unsigned sw[4] = {0u, 0u, 0u, 0u};           // SEG: this chunk's words, before the prefetch reuses sp
            if constexpr (SEG) {
#pragma unroll
                for (int r = 0; r < 4; ++r) sw[r] = sp[r];
            }
            __syncthreads();                             // every wave is done with the previous chunk
            stage();
            __syncthreads();
            if constexpr (MASKED) {
                nx = after(ch);
                if (nx < nch) { fetch(lo + nx * walk::CHUNK); window(nx + 1); }      // however far ahead
            } else if (ch + 1 < nch) {
                fetch(it0 + walk::CHUNK);
                if constexpr (SEG) seg_fetch(ch + 1);
            }
            if (!active) continue;                       // wave-uniform: this wave's rows have no targets left
            if constexpr (SEG) {
                // none of the wave's 16 rows may take an item of this chunk: no scores, nothing to count.  The wave
                // has staged its share and passed both barriers; its counters are as the last chunk left them
                if (!__ballot((sw[0] | sw[1] | sw[2] | sw[3]) != 0u)) continue;
            }
#include "walk_score_tiles.inc"
            unsigned long long k0[4], k1[4];
            if constexpr (MASKED) deny = ~word & 0xFFFFu;
            if constexpr (SEG) {
#pragma unroll
                for (int r = 0; r < 4; ++r) dn[r] = ~sw[r] & 0xFFFFu;
            }
            keys_of(acc0, it0, k0);
            if constexpr (MASKED) deny = ~word >> 16;
            if constexpr (SEG) {
#pragma unroll
                for (int r = 0; r < 4; ++r) dn[r] = ~sw[r] >> 16;
            }
            keys_of(acc1, it0 + 16, k1);
#pragma unroll
            for (int g = 0; g < RK_TP / RK_TG; ++g) {
                if (g * RK_TG < wt) {                    // wave-uniform
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
#pragma unroll
                        for (int t = g * RK_TG; t < (g + 1) * RK_TG; ++t) {
                            const unsigned long long tk = tw[4 * q + r][t];
                            cnt[r][t] += (k0[r] > tk ? 1 : 0) + (k1[r] > tk ? 1 : 0);
                        }
                    }
                }
            }
        }

        // ---- pass end: add the 16 lanes of each q group; lane c keeps target c of its four rows
        int32_t* out_above = above + (int64_t)blockIdx.y * slice_stride;        // sliced: this slice's partial counts
        int32_t* out_cand = n_cand + (int64_t)blockIdx.y * slice_stride;
#pragma unroll
        for (int g = 0; g < RK_TP / RK_TG; ++g) {
            if (g * RK_TG < wt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t rbc = min(b0 + 4 * q + r, nq - 1);
                    const int64_t tp0 = q_ptr[rbc], tn = valid[r] ? q_ptr[rbc + 1] - tp0 : 0;
#pragma unroll
                    for (int t = g * RK_TG; t < (g + 1) * RK_TG; ++t) {
                        int v = cnt[r][t];
                        v += __shfl_xor(v, 1, 64);
                        v += __shfl_xor(v, 2, 64);
                        v += __shfl_xor(v, 4, 64);
                        v += __shfl_xor(v, 8, 64);
                        if (c == (t & 15) && t0 + t < tn) {
                            const bool none = tw[4 * q + r][t] == RK_NONE;       // NaN target: -1 (slice 0), else 0
                            out_above[tp0 + t0 + t] = none ? (blockIdx.y == 0 ? -1 : 0) : v;
                        }
                    }
                }
            }
        }
        if (pass == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                int v = ncand[r];
                v += __shfl_xor(v, 1, 64);
                v += __shfl_xor(v, 2, 64);
                v += __shfl_xor(v, 4, 64);
                v += __shfl_xor(v, 8, 64);
                if (c == 0 && valid[r]) out_cand[b0 + 4 * q + r] = v;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");          // the next pass rewrites this wave's target keys
        __builtin_amdgcn_wave_barrier();
    }
}

// out[i] = sum over slices of part[s][i], i < total (the `above` entries, then the n_cand entries)
__global__ __launch_bounds__(256)
void k_rank_reduce(int64_t nt, int64_t nq, int nslices, const int32_t* __restrict__ part, int32_t* __restrict__ above,
                   int32_t* __restrict__ n_cand) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, total = nt + nq;
    if (i >= total) return;
    int v = 0;
    for (int s = 0; s < nslices; ++s) v += part[(int64_t)s * total + i];
    if (i < nt) above[i] = v; else n_cand[i - nt] = v;
}

constexpr int rk_waves(int KB) { return KB <= 4 ? 8 : 4; }      // 16-row tiles per workgroup (VGPR budget: DESIGN 15)

// seg: the SEG instantiations (`allow` is then the eligibility table); otherwise MASKED when there is a bitmap
template <int KB>
int launch_rank(int ld, int64_t nq, const int32_t* users, const int64_t* q_ptr, const int32_t* q_items, int64_t n,
                int nsl, const float* U, const float* Z, const float* b_u, const float* b_i, const double* mu,
                const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow, bool seg, int64_t nseg,
                int64_t seg_stride, const int32_t* row_seg, float* t_score, int32_t* above, int32_t* n_cand,
                int64_t slice_stride, hipStream_t st) {
    constexpr int NW = rk_waves(KB);
    const int64_t slice = walk::slice_items(n, nsl);
    const dim3 grid((unsigned)((nq + NW * 16 - 1) / (NW * 16)), (unsigned)nsl);
    const auto kern = seg     ? k_rank_count<KB, NW, false, true>
                      : allow ? k_rank_count<KB, NW, true>
                              : k_rank_count<KB, NW, false>;
    hipLaunchKernelGGL(kern, grid, dim3(NW * 64), 0, st, ld, nq, users, q_ptr, q_items, n, slice, U, Z, b_u, b_i, mu,
                       seen_ptr, seen_idx, t_score, above, n_cand, slice_stride, allow, nseg, seg_stride, row_seg);
    return topk::launch_status();
}

// the body of als_rank_count_masked (seg false: nseg, seg_stride and row_seg are 0) and _segmented
int rank_count(int k, int ld, int64_t n, const float* U, const float* Z, const float* b_u, const float* b_i,
               const double* mu, const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow, bool seg,
               int64_t nseg, int64_t seg_stride, const int32_t* row_seg, int64_t nq, const int32_t* q_users,
               const int64_t* q_ptr, const int32_t* q_items, int64_t nt, int nslices, float* t_score, int32_t* above,
               int32_t* n_cand, void* workspace, size_t workspace_bytes, void* stream) {
    const int bad = topk::check_shape(k, ld, nq, n, 1, 1, nslices);
    if (bad) return bad;
    if (nt < 0 || (seg && (nseg < 1 || seg_stride < (n + 31) / 32))) return ALS_E_BADARG;
    if (nq == 0) return 0;
    if (!q_users || !q_ptr || !U || !Z || !b_u || !b_i || !mu || !n_cand || (!seen_ptr != !seen_idx) ||
        (nt > 0 && (!q_items || !t_score || !above)) || (seg && (!allow || !row_seg)))
        return ALS_E_BADARG;
    // sliced: slice s writes its counts to part[s][0 .. nt) and part[s][nt .. nt + nq)
    const topk::SlicePlan p = topk::plan(nq, rk_waves(ld / 16) * 16, n, nslices, nt + nq, sizeof(int32_t), workspace,
                                         workspace_bytes);
    if (!p.nsl) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    int32_t* part = (int32_t*)p.part;
    int rc;
    ALS_DISPATCH_KB(ld / 16, rc = launch_rank<KB>(ld, nq, q_users, q_ptr, q_items, n, p.nsl, U, Z, b_u, b_i, mu, seen_ptr,
                                                  seen_idx, allow, seg, nseg, seg_stride, row_seg, t_score,
                                                  part ? part : above, part ? part + nt : n_cand, part ? nt + nq : 0,
                                                  st));
    if (rc != 0 || p.nsl == 1) return rc;
    hipLaunchKernelGGL(k_rank_reduce, dim3((unsigned)((nt + nq + 255) / 256)), dim3(256), 0, st, nt, nq, p.nsl, part,
                       above, n_cand);
    return topk::launch_status();
}

}  // namespace

extern "C" size_t als_rank_count_workspace_bytes(int k, int64_t nq, int64_t nt, int64_t n, int nslices) {
    const int kp = als_padded_k(k);
    if (kp < 0 || nq <= 0 || nt < 0 || n <= 0 || nslices < 0) return 0;
    return topk::slice_bytes(topk::slices(nq, rk_waves(kp / 16) * 16, n, nslices), nt + nq, sizeof(int32_t));
}

extern "C" int als_rank_count_masked(int k, int ld, int64_t n, const float* U, const float* Z, const float* b_u,
                                     const float* b_i, const double* mu, const int64_t* seen_ptr,
                                     const int32_t* seen_idx, const uint32_t* allow, int64_t nq,
                                     const int32_t* q_users, const int64_t* q_ptr, const int32_t* q_items, int64_t nt,
                                     int nslices, float* t_score, int32_t* above, int32_t* n_cand, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    return rank_count(k, ld, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow, false, 0, 0, nullptr, nq, q_users, q_ptr,
                      q_items, nt, nslices, t_score, above, n_cand, workspace, workspace_bytes, stream);
}

extern "C" int als_rank_count_segmented(int k, int ld, int64_t n, const float* U, const float* Z, const float* b_u,
                                        const float* b_i, const double* mu, const int64_t* seen_ptr,
                                        const int32_t* seen_idx, const uint32_t* seg_allow, int64_t nseg,
                                        int64_t seg_stride_words, const int32_t* row_seg, int64_t nq,
                                        const int32_t* q_users, const int64_t* q_ptr, const int32_t* q_items,
                                        int64_t nt, int nslices, float* t_score, int32_t* above, int32_t* n_cand,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    return rank_count(k, ld, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, seg_allow, true, nseg, seg_stride_words,
                      row_seg, nq, q_users, q_ptr, q_items, nt, nslices, t_score, above, n_cand, workspace,
                      workspace_bytes, stream);
}

extern "C" int als_rank_count(int k, int ld, int64_t n, const float* U, const float* Z, const float* b_u,
                              const float* b_i, const double* mu, const int64_t* seen_ptr, const int32_t* seen_idx,
                              int64_t nq, const int32_t* q_users, const int64_t* q_ptr, const int32_t* q_items,
                              int64_t nt, int nslices, float* t_score, int32_t* above, int32_t* n_cand,
                              void* workspace, size_t workspace_bytes, void* stream) {
    return als_rank_count_masked(k, ld, n, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, nullptr, nq, q_users, q_ptr, q_items,
                                 nt, nslices, t_score, above, n_cand, workspace, workspace_bytes, stream);
}
