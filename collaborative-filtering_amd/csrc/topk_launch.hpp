// Host side of the sliced catalogue walks - als_recommend_topk*, als_recommend_deep, als_rank_count*, als_similar_topk,
// als_audience_topk, als_group_topk, als_explore_topk: what their entry points do around the launch of their own
// kernel, written once.  The order of the checks is the one include/als_hip.h documents: ALS_E_BADK, then the shape
// (ALS_E_BADARG), then "an empty batch is a no-op", then the entry point's pointers, and the workspace last.
//
//   const int bad = topk::check_shape(k, ld, nrows, n, topn, ALS_TOPK_MAX, nslices);
//   if (bad || <a condition of this entry point alone>) return bad ? bad : ALS_E_BADARG;
//   if (nrows == 0) return 0;
//   if (<a required pointer is NULL>) return ALS_E_BADARG;
//   const topk::SlicePlan p = topk::plan(nrows, rows per workgroup, n, nslices, entries, bytes, workspace, bytes);
//   if (!p.nsl) return ALS_E_BADARG;
//   ALS_DISPATCH_KB(ld / 16, rc = launch<KB>(..., p.nsl, ..., p.keys(), st));
//   return rc != 0 ? rc : topk::merge_slices(p.nsl, p.keys(), nrows, topn, top_val, top_idx, top_cnt, st);
//
// Nothing here is device code, and no kernel's text depends on it; the merge kernel and its launch are topk_rows.hpp's.
#pragma once
#include "als_hip.h"
#include "catalogue_walk.hpp"

namespace topk {

inline int launch_status() { return hipGetLastError() == hipSuccess ? 0 : ALS_E_LAUNCH; }

// batch rows per workgroup of the kernels that keep one list per row (k_recommend, k_similar, k_audience):
// topn <= 32: 8 waves, 128 keys per row (list 32); above: 4 waves, 256 keys per row (list 128)
constexpr int ROWS_NARROW = 128, ROWS_WIDE = 64;
inline int rows_per_wg(int topn) { return topn <= 32 ? ROWS_NARROW : ROWS_WIDE; }

// k, ld and the shape every entry point takes: 0, ALS_E_BADK or ALS_E_BADARG (a call without topn passes 1, 1)
inline int check_shape(int k, int ld, int64_t nrows, int64_t n, int topn, int topn_max, int nslices) {
    const int kp = als_padded_k(k);
    if (kp < 0) return ALS_E_BADK;
    if (ld != kp || nrows < 0 || n < 1 || n >= ((int64_t)1 << 31) || topn < 1 || topn > topn_max || nslices < 0 ||
        nslices > ALS_RECOMMEND_MAX_SLICES)
        return ALS_E_BADARG;
    return 0;
}

inline int slices(int64_t nrows, int64_t rows_per_wg, int64_t n, int nslices) {
    return walk::plan_slices(nrows, rows_per_wg, n, nslices, ALS_RECOMMEND_MAX_SLICES);
}

// bytes the slices' partial results take: `entries` values of `entry_bytes` per slice; one slice writes the outputs
inline size_t slice_bytes(int nsl, int64_t entries, size_t entry_bytes) {
    return nsl > 1 ? (size_t)nsl * (size_t)entries * entry_bytes : 0;
}

// the *_workspace_bytes queries of the top-N calls: 0 for a shape the call refuses, or that takes one slice
inline size_t workspace_bytes(int64_t nrows, int64_t rows_per_wg, int64_t n, int topn, int nslices) {
    if (nrows <= 0 || n <= 0 || topn < 1 || topn > ALS_TOPK_MAX || nslices < 0) return 0;
    return slice_bytes(slices(nrows, rows_per_wg, n, nslices), nrows * topn, sizeof(unsigned long long));
}

struct SlicePlan {
    int nsl = 0;                        // 0: the workspace is missing or too small
    void* part = nullptr;               // the slices' partial results; NULL with one slice
    unsigned long long* keys() const { return (unsigned long long*)part; }
};
inline SlicePlan plan(int64_t nrows, int64_t rows_per_wg, int64_t n, int nslices, int64_t entries, size_t entry_bytes,
                      void* workspace, size_t workspace_bytes) {
    SlicePlan p;
    const int nsl = slices(nrows, rows_per_wg, n, nslices);
    const size_t need = slice_bytes(nsl, entries, entry_bytes);
    if (need > 0 && (!workspace || workspace_bytes < need)) return p;
    p.nsl = nsl;
    p.part = nsl > 1 ? workspace : nullptr;
    return p;
}

// one launch of a kernel with a narrow and a wide instantiation (rows_per_wg), grid.y = the slices
template <class Kernel, class... Args>
int launch_by_width(Kernel narrow, Kernel wide, int topn, int64_t nrows, int nsl, hipStream_t st, Args... args) {
    const int rows = rows_per_wg(topn);
    const Kernel kern = rows == ROWS_NARROW ? narrow : wide;
    const dim3 grid((unsigned)((nrows + rows - 1) / rows), (unsigned)nsl);
    hipLaunchKernelGGL(kern, grid, dim3(rows * 4), 0, st, args...);
    return launch_status();
}

}  // namespace topk
