// K8 deep: the exact top-N of als_recommend_topk_masked for N up to ALS_TOPK_DEEP_MAX = 1024, optionally below a
// cursor key - k_recommend's 128-key lists, asked for again below a ceiling until the answer is exact.
//
// A call is R = ceil(topn / 128) rounds of (scoring, merge), all enqueued at once; nothing waits on the host.
//
// Scoring (recommend.hip, the DEEP instantiations of k_recommend): every slice writes, per user, the best 128 keys
// that are BELOW the (slice, user) ceiling.  Round 0's ceilings are the cursor keys (k_deep_init), or ~0.
//
// Merge (k_deep_merge, one wave per user): the user's running list (sorted, in the workspace) and the new lists of the
// slices that are open for the user are folded into the best NL = 64 V keys, of which the first topn are kept.  Every
// input is sorted, so no full sort is run: V / 2 slice lists at a time are loaded in the directions a bitonic network
// leaves its 128-blocks in and finished by the network's last stages (sizes 256 ... NL); then, with A the list and B
// the sorted batch, max(A[i], B[NL - 1 - i]) is a bitonic sequence that holds the best NL of both, and the last stage
// alone sorts it.  With T the topn-th key of the new list (0: not full), a slice that delivered 128 keys of which the
// last is above T (or T = 0) may hold more keys above T: it stays OPEN, and its ceiling becomes that last key.  Every
// other slice is closed (ceiling 0): what it has not delivered lies below T, and T only rises.  A user with an open
// slice stores the list and raises the round's flag; a user without one is final and is decoded into the outputs.
//
// Termination: a slice open after r rounds has delivered 128 r keys, all above T and therefore all in the list; at most
// topn - 1 keys are above T, so 128 r < topn and no slice is open after R rounds.  The kernels of round r > 0 return
// at once when round r - 1 raised no flag, and a user or a workgroup with nothing open returns before it works.
// Exactness: at the end every slice is exhausted below its ceiling or holds only keys below T, so the list is the best
// topn of all candidates under the total order of the keys - whatever the slice count.
#include "als_device.hpp"
#include "als_hip.h"
#include "recommend_deep.hpp"
#include "topk_common.hpp"
#include "topk_launch.hpp"

namespace {

using topk::key_index;
using topk::key_score;

static_assert(ALS_RECOMMEND_MAX_SLICES <= 64, "k_deep_merge keeps one slice per lane");
static_assert(ALS_TOPK_DEEP_MAX == 8 * ALS_TOPK_MAX, "the list is at most 16 keys per lane");
constexpr int DEEP_FLAG_BYTES = 64;     // the per-round "any open" words at the end of the workspace

__device__ __forceinline__ unsigned long long shfl_u64(unsigned long long v, int src) {
    const unsigned lo = __shfl((unsigned)v, src, 64), hi = __shfl((unsigned)(v >> 32), src, 64);
    return ((unsigned long long)hi << 32) | lo;
}

// The stages size = FROM ... 64 V of topk::sort_desc<V>: sorts k descending when every block of FROM / 2 elements is
// sorted already, descending where (i & FROM / 2) == 0 and ascending elsewhere (element i = lane + 64 v); with
// FROM = 64 V, when k is a descending run followed by an ascending one (or any other bitonic sequence).
template <int V, int FROM>
__device__ __forceinline__ void bitonic_tail(unsigned long long (&k)[V], int lane) {
#pragma unroll
    for (int size = FROM; size <= 64 * V; size <<= 1) {
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
                    const bool lower = (i & j) == 0;
                    const unsigned long long o = topk::shfl_xor_u64(k[v], j);
                    const bool take_max = (lower == desc);
                    k[v] = take_max ? (k[v] > o ? k[v] : o) : (k[v] < o ? k[v] : o);
                }
            }
        }
    }
}

// round 0's ceilings: the cursor key of the user for every slice, or no ceiling; the flags of every round cleared
__global__ __launch_bounds__(256)
void k_deep_init(int64_t nusers, int nslices, const unsigned long long* __restrict__ after_key,
                 unsigned long long* __restrict__ ceil, int32_t* __restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < DEEP_FLAG_BYTES / 4) flags[t] = 0;
    if (t < nusers * nslices) ceil[t] = after_key ? after_key[t % nusers] : ~0ull;
}

// one wave per user; V keys per lane: the list holds NL = 64 V >= topn keys
template <int V>
__global__ __launch_bounds__(256)
void k_deep_merge(int64_t nusers, int nslices, int topn, int round, int nrounds,
                  const unsigned long long* __restrict__ part, unsigned long long* __restrict__ list,
                  unsigned long long* __restrict__ ceil, int32_t* __restrict__ flags, int32_t* __restrict__ rounds,
                  float* __restrict__ top_val, int32_t* __restrict__ top_idx, int32_t* __restrict__ top_cnt) {
    constexpr int NL = 64 * V, G = V > 2 ? V / 2 : 1;        // G slice lists make one batch of NL keys
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (round > 0 && flags[round - 1] == 0) return;          // the round before left no slice open
    if (rounds && blockIdx.x == 0 && threadIdx.x == 0) *rounds = round + 1;
    if (b >= nusers) return;                                 // wave-uniform
    // lane s: slice s.  A slice delivered keys in this round iff its ceiling was not 0.
    const unsigned long long c_in = lane < nslices ? ceil[(int64_t)lane * nusers + b] : 0ull;
    const unsigned long long live = __ballot(c_in != 0ull);
    if (round > 0 && !live) return;                          // final, and decoded, since an earlier round

    unsigned long long A[V];
#pragma unroll
    for (int v = 0; v < V; ++v) A[v] = round > 0 ? list[b * NL + lane + 64 * v] : 0ull;
    for (int s0 = 0; s0 < nslices; s0 += G) {
        if (!((live >> s0) & ((1ull << G) - 1ull))) continue;
        unsigned long long B[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int i = lane + 64 * v, blk = i >> 7, s = s0 + blk;
            const int p = (blk & 1) ? 127 - (i & 127) : (i & 127);       // odd blocks ascending
            const bool ok = s < nslices && ((live >> s) & 1ull);
            B[v] = ok ? part[((int64_t)s * nusers + b) * ALS_TOPK_MAX + p] : 0ull;
        }
        bitonic_tail<V, 256>(B, lane);
#pragma unroll
        for (int v = 0; v < V; ++v) {                        // element NL - 1 - i is register V - 1 - v of lane 63 - lane
            const unsigned long long o = shfl_u64(B[V - 1 - v], 63 - lane);
            A[v] = A[v] > o ? A[v] : o;
        }
        bitonic_tail<V, NL>(A, lane);
    }
    unsigned long long t = 0ull;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        if (lane + 64 * v >= topn) A[v] = 0ull;
        if (v == ((topn - 1) >> 6)) t = A[v];
    }
    const unsigned long long T = shfl_u64(t, (topn - 1) & 63);           // the topn-th key, 0: the list is not full

    bool open = false;
    if (lane < nslices) {
        const unsigned long long last =
            c_in != 0ull ? part[((int64_t)lane * nusers + b) * ALS_TOPK_MAX + ALS_TOPK_MAX - 1] : 0ull;
        open = last != 0ull && (T == 0ull || last > T);
        ceil[(int64_t)lane * nusers + b] = open ? last : 0ull;
    }
    if (__ballot(open) && round + 1 < nrounds) {
#pragma unroll
        for (int v = 0; v < V; ++v) list[b * NL + lane + 64 * v] = A[v];
        if (lane == 0) flags[round] = 1;
        return;
    }
    int cnt = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int i = lane + 64 * v;
        const bool ok = i < topn && A[v] != 0ull;
        cnt += __popcll(__ballot(ok));
        if (i < topn) {
            top_val[b * topn + i] = ok ? key_score(A[v]) : -INFINITY;
            top_idx[b * topn + i] = ok ? key_index(A[v]) : -1;
        }
    }
    if (lane == 0) top_cnt[b] = cnt;
}

int deep_rounds(int topn) { return (topn + ALS_TOPK_MAX - 1) / ALS_TOPK_MAX; }
int deep_list_keys(int topn) {          // 128 R rounded up to a power of two: 128, 256, 512, 1024
    int nl = ALS_TOPK_MAX;
    while (nl < topn) nl *= 2;
    return nl;
}
// nslices == 0: the automatic count of als_recommend_topk, but at least ALS_DEEP_SLICE_FACTOR per round, so that a
// catalogue whose scores do not follow the item id expects topn / slices <= 32 of its top topn in a slice
int deep_slices(int64_t nusers, int64_t n, int topn, int nslices) {
    if (nslices == 0) {
        nslices = deep::plan_slices(nusers, n, 0);
        if (nslices < ALS_DEEP_SLICE_FACTOR * deep_rounds(topn)) nslices = ALS_DEEP_SLICE_FACTOR * deep_rounds(topn);
        if (nslices > ALS_RECOMMEND_MAX_SLICES) nslices = ALS_RECOMMEND_MAX_SLICES;
    }
    return deep::plan_slices(nusers, n, nslices);            // at most one slice per 32-item chunk
}

template <int V>
int launch_merge(int64_t nusers, int nsl, int topn, int round, int nrounds, const unsigned long long* part,
                 unsigned long long* list, unsigned long long* ceil, int32_t* flags, int32_t* rounds, float* tv,
                 int32_t* ti, int32_t* tc, hipStream_t st) {
    hipLaunchKernelGGL(k_deep_merge<V>, dim3((unsigned)((nusers + 3) / 4)), dim3(256), 0, st, nusers, nsl, topn, round,
                       nrounds, part, list, ceil, flags, rounds, tv, ti, tc);
    return topk::launch_status();
}

}  // namespace

extern "C" size_t als_recommend_deep_workspace_bytes(int64_t nusers, int64_t n, int topn, int nslices) {
    if (nusers <= 0 || n <= 0 || topn < 1 || topn > ALS_TOPK_DEEP_MAX || nslices < 0) return 0;
    const size_t s = (size_t)deep_slices(nusers, n, topn, nslices);
    return 8 * (size_t)nusers * (ALS_TOPK_MAX * s + (size_t)deep_list_keys(topn) + s) + DEEP_FLAG_BYTES;
}

extern "C" int als_recommend_deep(int k, int ld, int64_t nusers, const int32_t* users, int64_t n, const float* U,
                                  const float* Z, const float* b_u, const float* b_i, const double* mu,
                                  const int64_t* seen_ptr, const int32_t* seen_idx, const uint32_t* allow,
                                  const unsigned long long* after_key, int topn, int nslices, float* top_val,
                                  int32_t* top_idx, int32_t* top_cnt, int32_t* rounds, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    const int bad = topk::check_shape(k, ld, nusers, n, topn, ALS_TOPK_DEEP_MAX, nslices);
    if (bad) return bad;
    if (nusers == 0) return 0;
    if (!users || !U || !Z || !b_u || !b_i || !mu || !top_val || !top_idx || !top_cnt || (!seen_ptr != !seen_idx))
        return ALS_E_BADARG;
    const int nsl = deep_slices(nusers, n, topn, nslices), nr = deep_rounds(topn), nl = deep_list_keys(topn);
    if (!workspace || workspace_bytes < als_recommend_deep_workspace_bytes(nusers, n, topn, nslices)) return ALS_E_BADARG;
    unsigned long long* part = (unsigned long long*)workspace;
    unsigned long long* list = part + (size_t)nsl * nusers * ALS_TOPK_MAX;
    unsigned long long* ceil = list + (size_t)nusers * nl;
    int32_t* flags = (int32_t*)(ceil + (size_t)nsl * nusers);
    hipStream_t st = (hipStream_t)stream;
    const auto merge = nl == 128 ? launch_merge<2> : nl == 256 ? launch_merge<4> : nl == 512 ? launch_merge<8>
                                                                                             : launch_merge<16>;
    hipLaunchKernelGGL(k_deep_init, dim3((unsigned)(((int64_t)nsl * nusers + 255) / 256)), dim3(256), 0, st, nusers, nsl,
                       after_key, ceil, flags);
    if (hipGetLastError() != hipSuccess) return ALS_E_LAUNCH;
    for (int r = 0; r < nr; ++r) {
        int rc = deep::score_round(ld, nusers, users, n, nsl, U, Z, b_u, b_i, mu, seen_ptr, seen_idx, allow, part, ceil,
                                   r > 0 ? flags + r - 1 : nullptr, st);
        if (rc != 0) return rc;
        rc = merge(nusers, nsl, topn, r, nr, part, list, ceil, flags, rounds, top_val, top_idx, top_cnt, st);
        if (rc != 0) return rc;
    }
    return 0;
}
