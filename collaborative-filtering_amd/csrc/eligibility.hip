// K20: the eligibility table of als_recommend_topk_segmented / als_rank_count_segmented from item attributes and
// per-segment rules - nseg rows of the allow bitmap, built where they are used, so that 10^6 items x 10^3 segments
// never exist as a dense boolean array on the host.
//
// k_eligibility: one lane per item, 256 items per workgroup.  The lane keeps its item's TW attribute words (and its
// bit of base_allow) in registers and loops over the segments, so item_tags is read once; a segment's 3 TW rule words
// are wave-uniform loads.  eligible(s, i) = no forbidden bit && every need_all bit && (need_any empty || one of its
// bits) && base bit; __ballot packs the wave's 64 answers into two words of out[s], which lanes 0 and 1 store.  Lanes
// past n answer 0, so the bits >= n of the last word are 0.
#include "als_device.hpp"
#include "als_hip.h"

namespace {

constexpr int EL_THREADS = 256;

template <int TW>
__global__ __launch_bounds__(EL_THREADS)
void k_eligibility(int64_t n, const uint32_t* __restrict__ tags, int64_t nseg, const uint32_t* __restrict__ need_all,
                   const uint32_t* __restrict__ need_any, const uint32_t* __restrict__ forbid,
                   const uint32_t* __restrict__ base, uint32_t* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * EL_THREADS + threadIdx.x;
    const int64_t W = (n + 31) / 32, w0 = (i - lane) >> 5;              // the wave's first word (i - lane: multiple of 64)
    const bool in = i < n;
    unsigned t[TW];
#pragma unroll
    for (int w = 0; w < TW; ++w) t[w] = in ? tags[i * TW + w] : 0u;
    const bool keep = in && (!base || ((base[i >> 5] >> (unsigned)(i & 31)) & 1u));
    for (int64_t s = 0; s < nseg; ++s) {
        unsigned bad = 0u, hit = 0u, want = 0u;
#pragma unroll
        for (int w = 0; w < TW; ++w) {
            const unsigned fb = forbid ? forbid[s * TW + w] : 0u;
            const unsigned na = need_all ? need_all[s * TW + w] : 0u;
            const unsigned ny = need_any ? need_any[s * TW + w] : 0u;
            bad |= (t[w] & fb) | (~t[w] & na);
            hit |= t[w] & ny;
            want |= ny;
        }
        const unsigned long long m = __ballot(keep && bad == 0u && (want == 0u || hit != 0u));
        if (lane < 2 && w0 + lane < W) out[s * W + w0 + lane] = (uint32_t)(m >> (32 * lane));
    }
}

}  // namespace

extern "C" int als_eligibility_bitmaps(int64_t n, int tw, const uint32_t* item_tags, int64_t nseg,
                                       const uint32_t* need_all, const uint32_t* need_any, const uint32_t* forbid,
                                       const uint32_t* base_allow, uint32_t* out, void* stream) {
    if (n < 1 || n >= ((int64_t)1 << 31) || tw < 1 || tw > ALS_ELIGIBILITY_MAX_TAG_WORDS || nseg < 0)
        return ALS_E_BADARG;
    if (nseg == 0) return 0;
    if (!item_tags || !out) return ALS_E_BADARG;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + EL_THREADS - 1) / EL_THREADS));
#define ALS_EL_CASE(T)                                                                                             \
    case T:                                                                                                        \
        hipLaunchKernelGGL(k_eligibility<T>, grid, dim3(EL_THREADS), 0, st, n, item_tags, nseg, need_all, need_any, \
                           forbid, base_allow, out);                                                               \
        break;
    switch (tw) {
        ALS_EL_CASE(1) ALS_EL_CASE(2) ALS_EL_CASE(3) ALS_EL_CASE(4)
        ALS_EL_CASE(5) ALS_EL_CASE(6) ALS_EL_CASE(7) ALS_EL_CASE(8)
    }
#undef ALS_EL_CASE
    return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH;
}
