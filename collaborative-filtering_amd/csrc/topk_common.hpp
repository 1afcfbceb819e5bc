// Keys and sorts for per-row top-k selection under a total order: the 64-bit keys for k_recommend (recommend.hip),
// topk::k_merge_slices (topk_rows.hpp), k_rank_count (rank_eval.hip: it compares keys and never sorts), explain.hip and
// diversify.hip; the float encoding and the bitonic sorts also for k_topk_sim (graph_build.hip).
//
// A candidate is one 64-bit key: the high word is enc_f32(score) - an unsigned encoding whose integer order is the
// float order, with -0.0 folded onto +0.0 - and the low word is 0xFFFFFFFF - index, so that among equal scores the
// LOWER index has the larger key.  Sorting keys descending therefore orders by (score descending, index ascending):
// a total order, so a selection does not depend on the order in which candidates arrive.  Every real key is > 0
// (index < 2^31 makes the low word >= 2^31), which leaves 0 free as "no entry".  NaN scores must be filtered by the
// caller (a NaN would encode above +inf).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace topk {

__device__ __forceinline__ unsigned enc_f32(float s) {
    const unsigned b = __float_as_uint(s + 0.0f);                 // -0.0 -> +0.0
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec_f32(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
__device__ __forceinline__ unsigned long long make_key(float s, unsigned idx) {
    return ((unsigned long long)enc_f32(s) << 32) | (0xFFFFFFFFu - idx);
}
__device__ __forceinline__ int32_t key_index(unsigned long long key) {
    return (int32_t)(0xFFFFFFFFu - (unsigned)key);
}
__device__ __forceinline__ float key_score(unsigned long long key) {
    return dec_f32((unsigned)(key >> 32));
}
__device__ __forceinline__ unsigned long long shfl_xor_u64(unsigned long long v, int m) {
    const unsigned lo = __shfl_xor((unsigned)v, m, 64), hi = __shfl_xor((unsigned)(v >> 32), m, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// 64 V keys, V per lane (element i = lane + 64 v), sorted DESCENDING by a bitonic network (V a power of two)
template <int V>
__device__ __forceinline__ void sort_desc(unsigned long long (&k)[V], int lane) {
#pragma unroll
    for (int size = 2; size <= 64 * V; size <<= 1) {
#pragma unroll
        for (int j = size >> 1; j >= 1; j >>= 1) {
            if (j >= 64) {
                const int dv = j >> 6;
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    if ((v & dv) == 0) {
                        const int i = lane + 64 * v;
                        const bool desc = (i & size) == 0;
                        const unsigned long long a = k[v], b = k[v | dv];
                        const bool sw = desc ? (a < b) : (a > b);
                        k[v] = sw ? b : a;
                        k[v | dv] = sw ? a : b;
                    }
                }
            } else {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const int i = lane + 64 * v;
                    const bool desc = (i & size) == 0;
                    const bool lower = (i & j) == 0;                       // this element is the lower index of the pair
                    const unsigned long long o = shfl_xor_u64(k[v], j);
                    const bool take_max = (lower == desc);
                    k[v] = take_max ? (k[v] > o ? k[v] : o) : (k[v] < o ? k[v] : o);
                }
            }
        }
    }
}

// 256 keys, 4 per lane
__device__ __forceinline__ void sort256_desc(unsigned long long (&k)[4], int lane) { sort_desc<4>(k, lane); }

}  // namespace topk
